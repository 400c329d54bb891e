"""Repetition, presence and frequency penalties without a GPU: ``ops.penalize_logits`` against a
scalar loop, ``ops.token_counts_`` against ``torch.bincount``, the CPU branch of
``ops.sample_topk_(counts=)``, and the front ends (``GPT.generate`` / ``generate_cached`` /
``generate_batch``, ``sample.py``) against a loop written here."""

import math
import struct

import pytest
import torch

V = 512
RP, PP, FP = 1.3, 0.5, 0.2
PEN = dict(repetition_penalty=RP, presence_penalty=PP, frequency_penalty=FP)
N_NEW = 48


def _f32(x):
    """x rounded to fp32, as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def _scalar_rule(l, c, rp, pp, fp):
    """The rule on one logit, every operation rounded to fp32 on its own."""
    rp, pp, fp = _f32(rp), _f32(pp), _f32(fp)
    s = c > 0
    x = (_f32(l / rp) if l > 0 else _f32(l * rp)) if s else l
    y = _f32(x - _f32(fp * float(c)))
    return _f32(y - (pp if s else 0.0))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_penalize_logits_against_a_scalar_loop():
    from nanosandbox_amd import ops

    ls = [1.7, 0.3333, 12.5, -2.25, -0.1, 0.0, -0.0, 3.0e-39, -7.0e-40]
    cs = [0, 1, 7]
    logits = torch.tensor([[l for l in ls for _ in cs]], dtype=torch.float32)
    counts = torch.tensor([[c for _ in ls for c in cs]], dtype=torch.int32)
    for rp, pp, fp in ((RP, PP, FP), (0.7, -0.25, 0.05), (2.0, 0.0, 0.0), (1.0, 1e4, 0.0), (1.0, 0.0, -0.3)):
        got = ops.penalize_logits(logits, counts, rp, pp, fp)
        want = torch.tensor([[_scalar_rule(float(l), int(c), rp, pp, fp) for l, c in zip(logits[0], counts[0])]],
                            dtype=torch.float32)
        assert got.dtype == torch.float32 and torch.equal(_bits(got), _bits(want)), (rp, pp, fp)
    # the identity returns the input's bits, signed zeros and denormals included, with and without counts
    for kw in ({}, dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)):
        assert torch.equal(_bits(ops.penalize_logits(logits, counts, **kw)), _bits(logits))
    # a table wider than the vocabulary: the first V columns are the counts
    wide = torch.cat([counts, torch.full((1, 3), 5, dtype=torch.int32)], dim=1)
    assert torch.equal(ops.penalize_logits(logits, wide, RP, PP, FP), ops.penalize_logits(logits, counts, RP, PP, FP))


def test_token_counts_is_bincount():
    from nanosandbox_amd import ops

    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 40, (3, 37), generator=g)
    hist = lambda ids: torch.bincount(ids, minlength=40).to(torch.int32)  # noqa: E731
    cnt = torch.full((3, 40), 9, dtype=torch.int32)
    ops.token_counts_(cnt, idx)
    assert torch.equal(cnt, torch.stack([hist(r) for r in idx]))
    lengths = torch.tensor([1, 37, 20])
    ops.token_counts_(cnt, idx, lengths)
    assert torch.equal(cnt, torch.stack([hist(r[:n]) for r, n in zip(idx, lengths.tolist())]))
    # rows: the other rows keep what they held; accumulate adds on top
    table = torch.full((4, 40), -7, dtype=torch.int32)
    rows = torch.tensor([3, 0, 2])
    ops.token_counts_(table, idx, lengths, rows)
    want = torch.full((4, 40), -7, dtype=torch.int32)
    for r, ids, n in zip(rows.tolist(), idx, lengths.tolist()):
        want[r] = hist(ids[:n])
    assert torch.equal(table, want)
    ops.token_counts_(table, idx[:1], None, torch.tensor([2]), accumulate=True)
    want[2] += hist(idx[0])
    assert torch.equal(table, want)


def test_cpu_sampler_counts_what_it_draws():
    from nanosandbox_amd import ops

    torch.manual_seed(0)
    B, Vs = 4, 64
    logits = torch.randn(B, Vs) * 3.0
    counts = torch.randint(0, 3, (B, Vs), dtype=torch.int32)
    before = counts.clone()
    done = torch.tensor([0, 1, 0, 0])
    tok = torch.full((B, 1), 777, dtype=torch.int64)
    gen = torch.full((B, 8), -5, dtype=torch.int64)
    ops.sample_topk_(logits, 1.0, 1, 7, torch.tensor([3, 3, 5, 1]), tok, gen, done=done, counts=counts, **PEN)
    want = ops.penalize_logits(logits, before, RP, PP, FP).argmax(1)
    grown = counts - before
    for b in (0, 2, 3):
        assert int(tok[b]) == int(want[b])
        assert int(grown[b].sum()) == 1 and int(grown[b, want[b]]) == 1  # the one-hot of the drawn id
    assert int(tok[1]) == 777 and not grown[1].any() and done.tolist() == [0, 1, 0, 0]
    with pytest.raises(ValueError):  # a penalty without the table
        ops.sample_topk_(logits, 1.0, 1, 7, torch.tensor([3]), tok, gen, repetition_penalty=1.3)


def _model():
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    return GPT(GPTConfig(block_size=256, vocab_size=V, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False)).eval()


def _prompts(lens=(5, 40), seed=6):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, V, (k,), generator=g) for k in lens]


@pytest.fixture(scope="module")
def greedy():
    """The tiny model, its prompts, and per prompt the penalised greedy run of a loop written here
    (forward_logits, bincount, the formula, argmax) with its smallest top-2 margin."""
    m, prompts = _model(), _prompts()
    refs, margins = [], []
    with torch.no_grad():
        for p in prompts:
            y, gap = p.clone(), math.inf
            for _ in range(N_NEW):
                l = m.forward_logits(y[None])[0, -1].float()
                c = torch.bincount(y, minlength=V)
                s = c > 0
                x = torch.where(s, torch.where(l > 0, l / torch.full_like(l, RP), l * torch.full_like(l, RP)), l)
                z = (x - torch.full_like(l, FP) * c.float()) - torch.where(s, torch.full_like(l, PP), torch.zeros_like(l))
                top = torch.topk(z, 2).values
                gap = min(gap, float(top[0] - top[1]))
                y = torch.cat([y, z.argmax()[None]])
            refs.append(y)
            margins.append(gap)
    return m, prompts, refs, margins


def test_generate_is_the_independent_loop(greedy):
    m, prompts, refs, margins = greedy
    assert min(margins) > 1e-4, margins  # no near-tie: arg-max decoding is path independent at this margin
    plain = [m.generate(p[None], N_NEW, top_k=1)[0] for p in prompts]
    for p, ref, base in zip(prompts, refs, plain):
        L = p.numel()
        assert torch.equal(m.generate(p[None], N_NEW, top_k=1, **PEN)[0], ref)
        assert torch.equal(m.generate_cached(p[None], N_NEW, top_k=1, **PEN)[0], ref)
        assert len(set(ref[L:].tolist())) >= 40 and len(set(base[L:].tolist())) <= 5
    outs = m.generate_batch(prompts, N_NEW, top_k=1, **PEN)
    assert all(torch.equal(o, ref) for o, ref in zip(outs, refs))
    # the queue: two requests through one row, the second admitted into the first one's row
    outs = m.generate_batch(prompts, N_NEW, top_k=1, batch_size=1, **PEN)
    assert all(torch.equal(o, ref) for o, ref in zip(outs, refs))
    assert not any(hasattr(prm, "compute") for prm in m.parameters())


def test_penalties_off_is_the_call_without_them(greedy):
    m, prompts, _, _ = greedy
    off = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    p = prompts[0]
    for kw in (dict(top_k=1), dict(temperature=0.8, top_k=20)):
        for fn in (lambda **k: m.generate(p[None], 12, **k)[0], lambda **k: m.generate_cached(p[None], 12, **k)[0],
                   lambda **k: m.generate_batch([p, prompts[1]], 12, **k)[1]):
            torch.manual_seed(4)
            a = fn(**kw)
            torch.manual_seed(4)
            b = fn(**kw, **off)
            assert torch.equal(a, b)


def test_decoder_state_and_refusals():
    from nanosandbox_amd.runtime.decode import Decoder, sampling_penalties, sample_next

    m = _model()
    assert sampling_penalties() is None and sampling_penalties(1.0, 0.0, 0.0) is None
    assert sampling_penalties(RP, None, FP) == (RP, 0.0, FP)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
                dict(presence_penalty=float("inf")), dict(frequency_penalty=float("nan"))):
        with pytest.raises(ValueError):
            sampling_penalties(**bad)
        with pytest.raises(ValueError):
            m.generate(torch.tensor([[1, 2]]), 2, **bad)
        with pytest.raises(ValueError):
            m.generate_cached(torch.tensor([[1, 2]]), 2, **bad)
    with pytest.raises(ValueError):
        Decoder(m, 2, speculate=2, penalize=True)
    with pytest.raises(ValueError):
        m.generate_cached(torch.tensor([[1, 2, 3]]), 4, speculate=2, repetition_penalty=1.3)
    with pytest.raises(ValueError):
        m.generate_batch([torch.tensor([1, 2, 3])], 4, speculate=2, presence_penalty=0.5)
    prompts = _prompts((5, 9), seed=2)
    idx = torch.zeros(2, 9, dtype=torch.int64)
    idx[0, :5], idx[1] = prompts
    hist = lambda ids: torch.bincount(ids, minlength=V).to(torch.int32)  # noqa: E731
    plain = Decoder(m, 2, per_row=True)
    dec = Decoder(m, 2, per_row=True, penalize=True)
    try:
        assert plain.cnt is None and dec.cnt.shape == (2, V) and dec.cnt.dtype == torch.int32
        assert dec.fits(2, per_row=True, penalize=True) and not dec.fits(2, per_row=True)
        assert plain.fits(2, per_row=True) and not plain.fits(2, per_row=True, penalize=True)
        with pytest.raises(ValueError):  # a penalty needs the table
            plain.sample_into(plain.prefill(idx, torch.tensor([5, 9])), 1.0, 1, **PEN)
        dec.sample_into(dec.prefill(idx, torch.tensor([5, 9])), 1.0, 1, **PEN)
        assert torch.equal(dec.cnt, torch.stack([hist(torch.cat([p, dec.gen[b, p.numel()][None]]))
                                                 for b, p in enumerate(prompts)]))
        dec.run(6, 1.0, 1)  # no penalty passed: the identity, and still counted
        texts = [torch.cat([p, dec.gen[b, p.numel():p.numel() + 7]]) for b, p in enumerate(prompts)]
        assert torch.equal(dec.cnt, torch.stack([hist(t) for t in texts]))
        keep = dec.cnt[0].clone()
        dec.admit([1], prompts[0][None])
        assert torch.equal(dec.cnt[0], keep) and torch.equal(dec.cnt[1], hist(prompts[0]))
    finally:
        plain.release()
        dec.release()
    # the eager sampling path
    logits = torch.randn(2, V)
    counts = torch.stack([hist(t) for t in texts])
    from nanosandbox_amd import ops
    assert torch.equal(sample_next(logits, 1.0, 1, counts=counts, **PEN)[:, 0],
                       ops.penalize_logits(logits, counts, RP, PP, FP).argmax(1))


def test_sample_cli_penalties(tmp_path, monkeypatch):
    from nanosandbox_amd import sample

    torch.manual_seed(0)
    from nanosandbox_amd.models import GPT, GPTConfig
    args = dict(block_size=48, vocab_size=97, n_layer=2, n_head=4, n_embd=64, bias=True, dropout=0.0)
    m = GPT(GPTConfig(**args)).eval()
    torch.save({"model": m.state_dict(), "model_args": args, "iter_num": 0, "best_val_loss": 0.0, "config": {}},
               tmp_path / "ckpt.pt")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    (tmp_path / "prompt.txt").write_text("1,2,3")
    base = [f"--out_dir={tmp_path}", "--device=cpu", "--max_new_tokens=8", f"--start=FILE:{tmp_path / 'prompt.txt'}",
            "--num_samples=2", "--top_k=1"]
    want = ",".join(map(str, m.generate(torch.tensor([[1, 2, 3]]), 8, top_k=1, **PEN)[0].tolist()))
    pen = ["--repetition_penalty=1.3", "--presence_penalty=0.5", "--frequency_penalty=0.2"]
    for extra in ([], ["--kv_cache=False"], ["--sample_batch=2"], ["--serve_batch=2"]):
        assert sample.main(base + pen + extra) == [want, want], extra
    assert len(sample.main(base + ["--repetition_penalty=1.3"])) == 2
    for bad in (["--repetition_penalty=0.0"], ["--repetition_penalty=-1.0"], ["--speculate=2", "--presence_penalty=0.5"]):
        with pytest.raises(ValueError):
            sample.main(base + bad)
