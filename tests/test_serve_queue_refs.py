"""A prompt queue served through a fixed batch whose finished rows are refilled
(runtime/decode.py ``Decoder.admit`` / ``Decoder.serve``, ``GPT.generate_batch(batch_size=)``,
``sample.py --serve_batch``) on the CPU: the fp32 torch paths against the recompute loop."""

import pytest
import torch

from nanosandbox_amd import ops
from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime.decode import Decoder

V = 97
LENS = (3, 7, 12, 1, 5, 9, 2)
BUDGETS = (6, 1, 12, 3, 9, 2, 7)
ARGS = dict(block_size=48, vocab_size=V, n_layer=2, n_head=4, n_embd=64, dropout=0.0, bias=True)


def _model():
    torch.manual_seed(0)
    return GPT(GPTConfig(**ARGS)).eval()


@pytest.fixture(scope="module")
def greedy():
    """The reference: every prompt on its own through the recompute loop, its own budget of greedy
    tokens, with the smallest top-1 / top-2 logit gap met on the way."""
    m = _model()
    g = torch.Generator().manual_seed(1)  # a seed whose continuations offer a stop token (test_queue_stop_token)
    prompts = [torch.randint(0, V, (n,), generator=g) for n in LENS]
    refs, gaps = [], []
    with torch.no_grad():
        for p, n in zip(prompts, BUDGETS):
            y = m.generate(p[None], n, top_k=1)[0]
            top2 = torch.topk(m.forward_logits(y[None, :-1])[0, p.numel() - 1:], 2, dim=-1).values
            refs.append(y)
            gaps.append(float((top2[:, 0] - top2[:, 1]).min()))
    return m, prompts, refs, gaps


@pytest.mark.parametrize("batch_size", [3, 1, 7])
def test_greedy_queue_matches_recompute(greedy, batch_size):
    m, prompts, refs, gaps = greedy
    # the comparison is only meaningful where the argmax is stable under the fp32 path differences
    assert min(gaps) >= 1e-3, gaps
    outs = m.generate_batch(prompts, list(BUDGETS), top_k=1, batch_size=batch_size)
    assert len(outs) == len(refs)
    for o, r, p, n in zip(outs, refs, prompts, BUDGETS):
        assert o.numel() == p.numel() + n
        assert torch.equal(o, r)


def test_queue_stop_token(greedy):
    m, prompts, refs, _ = greedy
    new = [r[n:].tolist() for r, n in zip(refs, LENS)]
    # some request's k-th new token, k >= 2, that another request never emits
    stop = next((x[k] for x in new for k in range(1, len(x))
                 if x.index(x[k]) >= 1 and any(x[k] not in y for y in new)), None)
    assert stop is not None, new
    outs = m.generate_batch(prompts, list(BUDGETS), top_k=1, stop_token=stop, batch_size=3)
    early = full = 0
    for o, r, x, n in zip(outs, refs, new, LENS):
        want = r if stop not in x else r[:n + x.index(stop) + 1]
        assert torch.equal(o, want)
        early += stop in x and x.index(stop) + 1 < len(x)
        full += stop not in x
    assert early >= 1 and full >= 1


def test_queue_schedule(monkeypatch):
    """One long request and five short ones through 2 rows: the short ones follow each other in
    the second row while the long one runs, so the steps are the long request's own."""
    m = _model()
    monkeypatch.setattr(Decoder, "DONE_POLL", 1)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, V, (4,), generator=g) for _ in range(6)]
    budgets = [30, 3, 3, 3, 3, 3]
    dec = Decoder(m, 2, use_graph=False, per_row=True)
    outs = m.generate_batch(prompts, budgets, top_k=1, batch_size=2, decoder=dec)
    assert [o.numel() - 4 for o in outs] == budgets
    assert dec.queue_stats["steps"] <= 30  # chunks of 2 would need 29 + 2 + 2 = 33
    assert dec.queue_stats["admitted"] == 6
    assert 2 <= dec.queue_stats["admissions"] <= 5
    for p, n, o in zip(prompts, budgets, outs):
        assert torch.equal(o, m.generate(p[None], n, top_k=1)[0])


def test_admit_into_the_middle_of_a_run():
    m = _model()
    g = torch.Generator().manual_seed(3)
    lens = (5, 9, 3)
    idx = torch.randint(0, V, (3, 9), generator=g)
    dec = Decoder(m, 3, use_graph=False, per_row=True)
    with torch.no_grad():
        dec.sample_into(dec.prefill(idx, torch.tensor(lens)), 1.0, 1)
        dec.run(4, 1.0, 1)
        keep = [0, 2]
        before = ([c[keep].clone() for c in dec.kc + dec.vc], dec.pos[keep].clone(), dec.done[keep].clone(),
                  dec.tok[keep].clone(), dec.gen[keep].clone())
        L = 6
        new = torch.randint(0, V, (1, 8), generator=g)  # 6 prompt tokens, right-padded to 8
        lg = dec.admit([1], new, torch.tensor([L]))
        one = Decoder(m, 1, use_graph=False, per_row=True)
        ref = one.prefill(new, torch.tensor([L]))
    assert lg.shape == (1, V) and torch.allclose(lg, ref, atol=1e-5, rtol=1e-5)
    for c, r in zip(dec.kc + dec.vc, one.kc + one.vc):
        assert torch.allclose(c[1, :, :L], r[0, :, :L], atol=1e-5, rtol=1e-5)
    assert dec.pos.tolist()[1] == L and dec.done.tolist()[1] == 0
    after = ([c[keep] for c in dec.kc + dec.vc], dec.pos[keep], dec.done[keep], dec.tok[keep], dec.gen[keep])
    for a, b in zip(before[0], after[0]):
        assert torch.equal(a, b)
    for a, b in zip(before[1:], after[1:]):
        assert torch.equal(a, b)
    # the first token of the admitted row alone: the other rows' tok, gen and done stay
    dec.sample_admitted([1], lg, 1.0, 1)
    assert int(dec.tok[1]) == int(ref.argmax()) == int(dec.gen[1, L])
    assert torch.equal(dec.tok[keep], before[3]) and torch.equal(dec.gen[keep], before[4])
    assert torch.equal(dec.done[keep], before[2])


def test_kv_append_rows_matches_a_per_row_loop():
    torch.manual_seed(4)
    B, H, D, T, S, p0 = 4, 2, 8, 16, 5, 3
    C = H * D
    rows = torch.tensor([3, 0, 2])
    qkv = torch.randn(3, S, 3 * C)
    kc, vc = torch.full((B, H, T, D), 7.0), torch.full((B, H, T, D), 7.0)
    k2, v2 = kc.clone(), vc.clone()
    ops.kv_append(qkv, kc, vc, None, p0, rows=rows)
    for j, r in enumerate(rows.tolist()):
        ops.kv_append(qkv[j:j + 1], k2[r:r + 1], v2[r:r + 1], None, p0)
    assert torch.equal(kc, k2) and torch.equal(vc, v2)
    assert bool((kc[1] == 7.0).all()) and bool((kc[:, :, :p0] == 7.0).all()) and bool((kc[:, :, p0 + S:] == 7.0).all())
    # int8 caches: the stored rows are quantize_cache_rows of the K / V rows, bit for bit
    def cache():
        return ops.QuantCache(torch.full((B, H, T, D), 5, dtype=torch.int8), torch.full((B, H, T), 3.0))
    kq, vq = cache(), cache()
    ops.kv_append(qkv, kq, vq, None, p0, rows=rows)
    k, v = qkv.view(3, S, 3, H, D)[:, :, 1:].permute(2, 0, 3, 1, 4)
    for c, x in ((kq, k), (vq, v)):
        want = ops.quantize_cache_rows(x)
        assert torch.equal(c.q[rows, :, p0:p0 + S], want.q) and torch.equal(c.scale[rows, :, p0:p0 + S], want.scale)
        assert bool((c.q[1] == 5).all()) and bool((c.scale[1] == 3.0).all())
        assert bool((c.q[:, :, :p0] == 5).all()) and bool((c.scale[:, :, p0 + S:] == 3.0).all())


def test_sample_end_flags_exactly_the_rows_at_or_past_their_end():
    torch.manual_seed(5)
    B = 5
    logits = torch.randn(B, V)
    pos = torch.tensor([4, 4, 4, 4, 9])
    end = torch.tensor([5, 4, 3, 0, 9])       # pos < end, == end, > end, (done) > end, == end
    done = torch.tensor([0, 0, 0, 1, 0])
    tok = torch.full((B, 1), 55)
    gen = torch.full((B, 12), -1)
    ops.sample_topk_(logits, 1.0, 1, 7, pos, tok, gen, done=done, row_key=torch.arange(B), end=end)
    assert done.tolist() == [0, 1, 1, 1, 1]
    am = logits.argmax(1)
    for b in (0, 1, 2, 4):
        assert int(tok[b]) == int(am[b]) == int(gen[b, pos[b]])
    assert int(tok[3]) == 55 and bool((gen[3] == -1).all())  # a finished row draws nothing


def _ckpt(tmp_path, monkeypatch):
    from nanosandbox_amd import sample

    args = {k: v for k, v in ARGS.items()}
    torch.save({"model": _model().state_dict(), "model_args": args, "iter_num": 0, "best_val_loss": 0.0,
                "config": {}}, tmp_path / "ckpt.pt")
    (tmp_path / "prompts.txt").write_text("1,2,3\n9,8,7,6,5,4,3\n4,4\n")
    (tmp_path / "prompt.txt").write_text("1,2,3")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    return (sample, [f"--out_dir={tmp_path}", "--device=cpu", "--max_new_tokens=6", "--top_k=1"],
            f"--start=FILE:{tmp_path / 'prompt.txt'}")


def test_cli_serve_batch_prints_what_the_batches_print(tmp_path, monkeypatch):
    sample, base, start = _ckpt(tmp_path, monkeypatch)
    pf = f"--prompts_file={tmp_path / 'prompts.txt'}"
    plain = sample.main(base + ["--num_samples=2", pf])
    served = sample.main(base + ["--num_samples=2", pf, "--serve_batch=2"])
    assert len(plain) == 6 and served == plain
    # copies of start, and a stop token that ends the printed text before it
    one = sample.main(base + [start, "--num_samples=1"])
    assert sample.main(base + [start, "--num_samples=3", "--serve_batch=2"]) == one * 3
    first = int(one[0].split(",")[3])
    assert sample.main(base + [start, "--num_samples=2", "--serve_batch=2", f"--stop_token={first}"]) == \
        ["1,2,3"] * 2
    # shared_prompt composes: the same greedy text
    assert sample.main(base + [start, "--num_samples=3", "--serve_batch=2", "--shared_prompt=True"]) == one * 3


def test_refusals(tmp_path, monkeypatch):
    m = _model()
    p = [torch.tensor([1, 2, 3]), torch.tensor([4, 5])]
    with pytest.raises(ValueError):
        m.generate_batch(p, 4, top_k=1, batch_size=0)
    with pytest.raises(ValueError):
        m.generate_batch(p, [4], top_k=1, batch_size=2)
    with pytest.raises(ValueError):
        m.generate_batch(p, [4, 0], top_k=1, batch_size=2)
    with pytest.raises(ValueError):
        m.generate_batch(p, 4, top_k=1, batch_size=2, shared_prefix=True)
    with pytest.raises(ValueError):  # shared_prompt: every prompt the same
        m.generate_batch(p, 4, top_k=1, batch_size=2, shared_prompt=True)
    long = torch.arange(40) % V
    for kw in (dict(quantize="int8"), dict(kv_quantize="int8")):  # no recompute loop for a request that does not fit
        with pytest.raises(ValueError):
            m.generate_batch([p[0], long], 20, top_k=1, batch_size=2, **kw)
    with pytest.raises(ValueError):
        m.generate_batch([long, long], 20, top_k=1, batch_size=2, shared_prompt=True)
    # without them the request that does not fit goes alone, as in today's batches
    outs = m.generate_batch([p[0], long, p[1]], 20, top_k=1, batch_size=2)
    for o, q in zip(outs, [p[0], long, p[1]]):
        assert torch.equal(o, m.generate(q[None], 20, top_k=1)[0])
    sample, base, start = _ckpt(tmp_path, monkeypatch)
    with pytest.raises(ValueError):
        sample.main(base + [start, "--serve_batch=2", "--kv_cache=False"])
    with pytest.raises(ValueError):
        sample.main(base + [f"--prompts_file={tmp_path / 'prompts.txt'}", "--serve_batch=2", "--shared_prefix=True"])
    with pytest.raises(ValueError):
        sample.main(base + [start, "--serve_batch=-1"])
