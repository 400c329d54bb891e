"""A prompt queue served through a fixed batch on MI355X: the row-mapped K / V append kernels
and the request-keyed sampler against torch and the plain per-row kernels, ``Decoder.admit``
against a prefill of the same shape, and ``GPT.generate_batch(batch_size=)`` under the graph
against the eager steps and the full fused forward (runtime/decode.py ``Decoder.serve``)."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
V = 512
LENS = (5, 40, 33, 9, 17, 2, 26, 12, 1, 21)
BUDGETS = (24, 1, 7, 16, 3, 20, 11, 5, 13, 9)  # spread over 1 .. 24


def _model():
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=V, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval().to(DEV).set_compute_dtype(BF)


def _prompts(lens=LENS, seed=6):
    g = torch.Generator().manual_seed(seed)  # host RNG: the same prompts everywhere
    return [torch.randint(0, V, (k,), generator=g).to(DEV) for k in lens]


def _check_margin(m, y, L):
    """Every new token of y (prompt length L) lies within twice the decoder's 0.03 relative-norm
    logit bound (tests/test_ragged_decode_gpu.py) of the full forward's maximum, and the margin
    is narrow enough to mean something: fewer than V / 8 ids inside it at every position."""
    with torch.no_grad():
        ref = m.forward_logits(y[None, :-1])[0].float()[L - 1:]  # position t predicts y[t + 1]
    chosen = ref.gather(1, y[L:, None])[:, 0]
    floor = ref.max(dim=1).values - 2 * 0.03 * ref.norm(dim=1)
    inside = (ref >= floor[:, None]).sum(dim=1)
    assert bool((chosen >= floor).all()), (chosen - floor).min().item()
    assert int(inside.max()) < V // 8, inside.tolist()


@pytest.mark.parametrize("rows", [[2], [3, 0, 2]])
@pytest.mark.parametrize("S", [1, 37])
@pytest.mark.parametrize("pos0", [0, 20])
def test_append_rows_kernels(kernels, rows, S, pos0):
    from nanosandbox_amd import ops

    torch.manual_seed(0)
    B, H, D, T = 4, 2, 64, 64
    n, C = len(rows), H * D
    qkv = (torch.randn(n, S, 3 * C, device=DEV) * 2).to(BF)
    r = torch.tensor(rows, device=DEV, dtype=torch.int64)
    k, v = qkv.view(n, S, 3, H, D)[:, :, 1:].permute(2, 0, 3, 1, 4)  # [n, H, S, D] each
    # bf16 caches: the written rows bitwise, every other byte the sentinel's
    kc = torch.full((B, H, T, D), -3.0, device=DEV, dtype=BF)
    vc = torch.full((B, H, T, D), -3.0, device=DEV, dtype=BF)
    wk, wv = kc.clone(), vc.clone()
    wk[r, :, pos0:pos0 + S], wv[r, :, pos0:pos0 + S] = k, v
    ops.kv_append(qkv, kc, vc, None, pos0, rows=r)
    assert torch.equal(kc, wk) and torch.equal(vc, wv)
    # int8 caches: q and scale of quantize_cache_rows
    def cache():
        return ops.QuantCache(torch.full((B, H, T, D), 5, device=DEV, dtype=torch.int8),
                              torch.full((B, H, T), 3.0, device=DEV))
    kq, vq = cache(), cache()
    want = []
    for x in (k, v):
        c, ref = cache(), ops.quantize_cache_rows(x)
        c.q[r, :, pos0:pos0 + S], c.scale[r, :, pos0:pos0 + S] = ref.q, ref.scale
        want.append(c)
    ops.kv_append(qkv, kq, vq, None, pos0, rows=r)
    for got, w in zip((kq, vq), want):
        assert torch.equal(got.q, w.q) and torch.equal(got.scale, w.scale)


@pytest.mark.parametrize("Vs", [512, 509])
@pytest.mark.parametrize("kw", [dict(top_k=50), dict(top_k=50, top_p=0.9), dict(top_k=None)])
def test_keyed_sampler_draws_the_requests_stream(kernels, Vs, kw):
    """A row keyed k draws what row k of the plain per-row call draws (same salts, same position)."""
    from nanosandbox_amd import ops

    torch.manual_seed(2)
    kw = dict(kw)
    top_k = kw.pop("top_k")
    keys, positions = [9, 2, 7, 0], [3, 9, 9, 40]
    B, G = 4, 48
    logits = torch.randn(B, Vs, device=DEV) * 3.0
    big = torch.randn(10, Vs, device=DEV)
    big[keys] = logits
    pos = torch.tensor(positions, device=DEV, dtype=torch.int64)
    bpos = torch.zeros(10, device=DEV, dtype=torch.int64)
    bpos[keys] = pos
    key = torch.tensor(keys, device=DEV, dtype=torch.int64)
    salt_dev = torch.tensor([123456789], device=DEV, dtype=torch.int64)

    def plain(stop):
        tok = torch.full((10, 1), 777, device=DEV, dtype=torch.int64)
        gen = torch.full((10, G), -5, device=DEV, dtype=torch.int64)
        done = torch.zeros(10, device=DEV, dtype=torch.int64)
        ops.sample_topk_(big, 0.8, top_k, 99, bpos, tok, gen, salt_dev=salt_dev, stop_token=stop, done=done, **kw)
        return tok, gen, done

    t0, _, _ = plain(None)
    stop = int(t0[2])  # what key 2 draws: that row finishes, the others only if they draw it too
    rt, rg, rd = plain(stop)
    tok = torch.full((B, 1), 777, device=DEV, dtype=torch.int64)
    gen = torch.full((B, G), -5, device=DEV, dtype=torch.int64)
    done = torch.zeros(B, device=DEV, dtype=torch.int64)
    ops.sample_topk_(logits, 0.8, top_k, 99, pos, tok, gen, salt_dev=salt_dev, stop_token=stop, done=done,
                     row_key=key, **kw)
    assert torch.equal(tok, rt[keys]) and torch.equal(gen, rg[keys]) and torch.equal(done, rd[keys])
    assert int(done[1]) == 1 and 0 <= int(tok.min()) and int(tok.max()) < Vs


def test_sampler_end_position(kernels):
    from nanosandbox_amd import ops

    torch.manual_seed(1)
    B = 5
    logits = torch.randn(B, V, device=DEV) * 3.0
    am = logits.argmax(1)
    positions = [4, 4, 4, 4, 9]
    pos = torch.tensor(positions, device=DEV, dtype=torch.int64)
    end = torch.tensor([5, 4, 3, 0, 9], device=DEV, dtype=torch.int64)  # <, ==, >, (done), == and the stop token
    done = torch.tensor([0, 0, 0, 1, 0], device=DEV, dtype=torch.int64)
    tok = torch.full((B, 1), 777, device=DEV, dtype=torch.int64)
    gen = torch.full((B, 12), -5, device=DEV, dtype=torch.int64)
    ops.sample_topk_(logits, 1.0, 1, 99, pos, tok, gen, stop_token=int(am[4]), done=done, end=end)
    want = torch.full((B, 12), -5, device=DEV, dtype=torch.int64)
    for b in (0, 1, 2, 4):
        want[b, positions[b]] = am[b]
        assert int(tok[b]) == int(am[b])
    assert int(tok[3]) == 777 and torch.equal(gen, want)  # the finished row is skipped
    first = 1 if int(am[0]) == int(am[4]) else 0
    assert done.tolist() == [first, 1, 1, 1, 1]  # stop and end together: finished once


@pytest.mark.parametrize("mode,rows", [("bf16", [2]), ("bf16", [3, 0, 2]), ("kv8", [2]), ("kv8", [3, 0, 2]),
                                       ("q8", [3, 0, 2])])
def test_admit_is_the_prefill_of_its_shape(kernels, mode, rows):
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    kw = dict(kv_quantize="int8") if mode == "kv8" else dict(quantize="int8") if mode == "q8" else {}
    n, S = len(rows), 40
    lens = (5, 40, 33) if n == 3 else (40,)
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, V, (n, S), generator=g).to(DEV)
    old = torch.randint(0, V, (4, 23), generator=g).to(DEV)
    lengths = torch.tensor(lens, device=DEV)

    def parts(c, sel, upto):
        return [c.q[sel, :, :upto], c.scale[sel, :, :upto]] if isinstance(c, ops.QuantCache) else [c[sel, :, :upto]]

    with torch.no_grad():
        ref = Decoder(m, n, use_graph=False, per_row=True, **kw)
        try:
            want = ref.prefill(idx, lengths).clone()
            want_kv = [t.clone() for c in ref.kc + ref.vc for t in parts(c, slice(None), S)]
        finally:
            ref.release()
        dec = Decoder(m, 4, use_graph=False, per_row=True, **kw)
        try:
            dec.sample_into(dec.prefill(old), 1.0, 1)
            dec.run(3, 1.0, 1)
            keep = [b for b in range(4) if b not in rows]
            state = lambda: ([t.clone() for c in dec.kc + dec.vc for t in parts(c, keep, dec.T)]  # noqa: E731
                             + [dec.pos[keep].clone(), dec.done[keep].clone(), dec.tok[keep].clone(),
                                dec.gen[keep].clone()])
            before = state()
            got = dec.admit(rows, idx, lengths)
            got_kv = [t for c in dec.kc + dec.vc for t in parts(c, rows, S)]
            assert torch.equal(got, want)
            assert all(torch.equal(a, b) for a, b in zip(got_kv, want_kv))
            assert all(torch.equal(a, b) for a, b in zip(before, state()))
            assert dec.pos[rows].tolist() == list(lens) and dec.done[rows].tolist() == [0] * n
        finally:
            dec.release()


@pytest.mark.parametrize("mode", ["bf16", "kv8", "q8", "one_row"])
def test_queue_greedy_under_the_graph(kernels, mode):
    m = _model()
    kw = dict(kv_quantize="int8") if mode == "kv8" else dict(quantize="int8") if mode == "q8" else {}
    nreq, bs = (6, 1) if mode == "one_row" else (10, 3)  # one row: the fused single-row step
    prompts, budgets = _prompts()[:nreq], list(BUDGETS[:nreq])
    outs = {g: m.generate_batch(prompts, budgets, top_k=1, batch_size=bs, use_graph=g, **kw) for g in (True, False)}
    for a, b, p, n in zip(outs[True], outs[False], prompts, budgets):
        assert torch.equal(a, b)
        assert a.numel() == p.numel() + n and torch.equal(a[:p.numel()], p)
        _check_margin(m, a, p.numel())
    assert not any(hasattr(p, "compute") for p in m.parameters())  # shadows released


def test_queue_stop_token_under_the_graph(kernels):
    m = _model()
    prompts, budgets = _prompts(), list(BUDGETS)
    free = m.generate_batch(prompts, budgets, top_k=1, batch_size=3, use_graph=True)
    new = [f[p.numel():].tolist() for f, p in zip(free, prompts)]
    # a stop token: some request's k-th new token (k >= 2) that another request never emits
    stop = next((x[k] for x in new for k in range(1, len(x))
                 if x.index(x[k]) >= 1 and any(x[k] not in y for y in new)), None)
    assert stop is not None, new
    outs = {g: m.generate_batch(prompts, budgets, top_k=1, batch_size=3, stop_token=stop, use_graph=g)
            for g in (True, False)}
    early = 0
    for a, b, p, n in zip(outs[True], outs[False], prompts, budgets):
        assert torch.equal(a, b)
        x = a[p.numel():].tolist()
        assert 1 <= len(x) <= n and stop not in x[:-1]
        assert x[-1] == stop or len(x) == n
        early += x[-1] == stop and len(x) < n
        _check_margin(m, a, p.numel())
    assert early >= 1


def test_queue_shared_prompt_is_schedule_independent(kernels, monkeypatch):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    p = _prompts((11,), seed=9)[0]
    budgets = [24, 3, 17, 1, 9, 24, 12]
    want = m.generate_batch([p] * 3, 24, top_k=1, shared_prompt=True)[0]
    dec = Decoder(m, 3, per_row=True, shared_prompt=True, max_new=24)
    try:
        outs = m.generate_batch([p] * 7, budgets, top_k=1, shared_prompt=True, batch_size=3, decoder=dec)
        assert dec.prefills == 1 and dec.queue_stats["admitted"] == 7
        outs2 = m.generate_batch([p] * 7, budgets, top_k=1, shared_prompt=True, batch_size=3, decoder=dec)
        assert dec.prefills == 1  # the prompt stays cached between calls
    finally:
        dec.release()
    for o, o2, n in zip(outs, outs2, budgets):
        assert torch.equal(o, want[:11 + n]) and torch.equal(o2, o)

    def sampled(poll, stop=None):
        monkeypatch.setattr(Decoder, "DONE_POLL", poll)
        torch.manual_seed(7)
        return m.generate_batch([p] * 7, budgets, temperature=1.0, top_k=50, shared_prompt=True, batch_size=3,
                                stop_token=stop)

    a, b = sampled(16), sampled(1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))  # another schedule, the same keyed draws
    assert all(x.numel() == 11 + n for x, n in zip(a, budgets))
    long = [x for x, n in zip(a, budgets) if n >= 9]
    assert not all(torch.equal(long[0][:20], x[:20]) for x in long[1:])  # the requests draw independently
    stop = int(a[0][11 + 6])
    for y, f in zip(sampled(16, stop), a):
        fnew = f[11:].tolist()
        cut = fnew[:fnew.index(stop) + 1] if stop in fnew else fnew
        assert y[11:].tolist() == cut
    assert not [n for n, prm in m.named_parameters() if hasattr(prm, "compute")]
