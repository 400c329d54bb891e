"""Speculative decoding on MI355X: the multi-query decode attention kernel bit for bit against
successive single-query calls, the accept / draft kernel against its Python form, and
``Decoder(..., speculate=K)`` under the graph against the eager steps, the full fused forward and
the plain decoder's sampled stream (runtime/decode.py, csrc/kernels/decode_spec.hip, spec.hip)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
V = 512
LENS = (5, 40, 33, 9, 17, 2, 26, 12, 1, 21)


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


# ---------------------------------------------------------------------------------------------
# 1. the attention kernel

H, TMAX, D = 2, 512, 64
SENTINEL = -3.0


def _spec_call(qkv, kc, vc, pos):
    from nanosandbox_amd.ops import _lib

    B, S, _ = qkv.shape
    n_split = -(-TMAX // 256)
    ws = torch.full((B, S, H, n_split, 4 + D), float("nan"), device=DEV)
    out = torch.full((B, S, H * D), float("nan"), device=DEV, dtype=BF)
    _lib.call("nsa_decode_attn_spec", _lib.ptr(qkv), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(pos), _lib.ptr(ws),
              _lib.ptr(out), B, S, H, D, TMAX, 1.0 / math.sqrt(D), _lib.stream())
    return out, ws


def _single_call(qkv1, kc, vc, pos):
    from nanosandbox_amd.ops import _lib

    B = qkv1.shape[0]
    n_split = -(-TMAX // 256)
    ws = torch.full((B, H, n_split, 4 + D), float("nan"), device=DEV)
    out = torch.full((B, H * D), float("nan"), device=DEV, dtype=BF)
    _lib.call("nsa_decode_attn_rows", _lib.ptr(qkv1), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(pos), _lib.ptr(ws),
              _lib.ptr(out), B, H, D, TMAX, 1.0 / math.sqrt(D), 1, _lib.stream())
    return out, ws


# the new rows at 0, inside a chunk, straddling 255 | 256, at Tmax - S, and at Tmax - 2 (dead queries)
def _positions(B, S):
    straddle = 256 - (S + 1) // 2
    assert straddle <= 255 and straddle + S - 1 >= 256
    if B == 1:
        return [[0], [77], [straddle], [TMAX - S], [TMAX - 2], [TMAX - 1]]
    return [[0, 77, straddle], [TMAX - S, 300, 256], [TMAX - 2, TMAX - 1, 255]]


@pytest.mark.parametrize("S", [2, 5, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_attention_kernel_is_successive_single_queries(kernels, B, S):
    torch.manual_seed(3)
    for positions in _positions(B, S):
        assert len(set(positions)) == B  # per-row positions all different
        pos = torch.tensor(positions, device=DEV, dtype=torch.int64)
        qkv = (torch.randn(B, S, 3 * H * D, device=DEV) * 2).to(BF)
        # caches: random rows below every row's position, the sentinel from there on
        kc = torch.full((B, H, TMAX, D), SENTINEL, device=DEV, dtype=BF)
        vc = torch.full((B, H, TMAX, D), SENTINEL, device=DEV, dtype=BF)
        for b, p in enumerate(positions):
            kc[b, :, :p] = torch.randn(H, p, D, device=DEV).to(BF)
            vc[b, :, :p] = torch.randn(H, p, D, device=DEV).to(BF)
        rk, rv = kc.clone(), vc.clone()
        out, ws = _spec_call(qkv, kc, vc, pos)
        for j in range(S):
            live = [b for b, p in enumerate(positions) if p + j < TMAX]
            dead = [b for b in range(B) if b not in live]
            # the reference call runs every row; a dead row is parked on a copy at a position of its own
            pk, pv = rk.clone(), rv.clone()
            pj = torch.tensor([p + j if p + j < TMAX else 0 for p in positions], device=DEV, dtype=torch.int64)
            o1, w1 = _single_call(qkv[:, j].contiguous(), pk, pv, pj)
            for b in live:
                rk[b], rv[b] = pk[b], pv[b]
                assert torch.equal(out[b, j], o1[b]), (positions, j, b)
                assert torch.equal(ws[b, j].view(torch.int32), w1[b].view(torch.int32)), (positions, j, b)
            for b in dead:  # zeros out (finite: it feeds the linears and the sampler), nothing stored
                assert bool((out[b, j] == 0).all()), (positions, j, b)
                assert bool(torch.isfinite(ws[b, j][..., 1:]).all())
        # the written rows bitwise, every other cache byte unchanged (rk / rv: the successive calls' caches)
        assert torch.equal(kc, rk) and torch.equal(vc, rv)
        for b, p in enumerate(positions):
            n = min(S, TMAX - p)
            assert bool((kc[b, :, p + n:] == SENTINEL).all()) and bool((vc[b, :, p + n:] == SENTINEL).all())
            k = qkv[b, :n].view(n, 3, H, D)[:, 1].transpose(0, 1)
            assert torch.equal(kc[b, :, p:p + n], k)


def test_attention_op_refuses_int8_caches(kernels):
    from nanosandbox_amd import ops

    qkv = torch.zeros(1, 2, 3 * H * D, device=DEV, dtype=BF)
    c = ops.QuantCache(torch.zeros(1, H, 64, D, device=DEV, dtype=torch.int8), torch.ones(1, H, 64, device=DEV))
    with pytest.raises(AssertionError):
        ops.decode_attention_spec(qkv, c, c, torch.zeros(1, device=DEV, dtype=torch.int64), H)


# ---------------------------------------------------------------------------------------------
# 2. the accept / draft kernel against its Python form (the cases of tests/test_speculate_refs.py)

def test_bookkeeping_kernel_matches_the_reference(kernels):
    from nanosandbox_amd import ops
    from test_speculate_refs import accept_cases, draft_cases

    for name, (gen, pos, tok, K, N, T, table) in draft_cases().items():
        want = ops.ngram_draft(gen, pos, tok, K, N, T, table)
        got = ops.ngram_draft(gen.to(DEV), pos.to(DEV), tok.to(DEV), K, N, T, None if table is None else table.to(DEV))
        for g, w in zip(got, want):
            assert torch.equal(g.cpu(), w), name
    for name, case in accept_cases().items():
        outs = []
        for dev in ("cpu", DEV):
            st = {k: (v.clone().to(dev) if torch.is_tensor(v) else v) for k, v in case.items()}
            ops.spec_accept_(st["cand"], st["stok"], st["spos"], st["cpos"], st["gen"], st["pos"], st["tok"],
                             st["done"], st["end"], T=st["T"], N=st["N"], stop_token=st["stop"], table=st["table"],
                             stats=st["stats"])
            outs.append(st)
        for k, v in outs[0].items():
            if torch.is_tensor(v):
                assert torch.equal(outs[1][k].cpu(), v), (name, k)


# ---------------------------------------------------------------------------------------------
# 3. greedy, end to end

@pytest.mark.parametrize("K,rows", [(4, 3), (7, 1), (7, 2)])
def test_greedy_under_the_graph(kernels, K, rows):
    from nanosandbox_amd.runtime.decode import batch_decoder

    m = _model()
    prompts, N = _prompts()[:rows], 48
    outs, stats = {}, {}
    for g in (True, False):
        dec = batch_decoder(m, prompts, N, use_graph=g, speculate=K)
        try:
            outs[g] = m.generate_batch(prompts, N, top_k=1, use_graph=g, speculate=K, decoder=dec)
            stats[g] = dec.spec_stats
            assert dec.use_graph == g and (dec.replays > 0) == g
            assert all(key[-3:] == ("spec", K, 3) for key in dec.sgraphs)
        finally:
            dec.release()
    assert stats[True] == stats[False]
    for a, b, p in zip(outs[True], outs[False], prompts):
        assert torch.equal(a, b)
        assert a.numel() == p.numel() + N and torch.equal(a[:p.numel()], p)
        _check_margin(m, a, p.numel())
    st = stats[True]
    for b in range(rows):
        assert st["steps"][b] < N  # more than one token per model pass
        assert st["steps"][b] + st["accepted"][b] == N - 1
        assert st["accepted"][b] <= st["offered"][b] <= K * st["steps"][b]
    assert not any(hasattr(p, "compute") for p in m.parameters())  # shadows released


def test_plain_path_keeps_its_graph_keys(kernels):
    from nanosandbox_amd.runtime.decode import batch_decoder

    m = _model()
    prompts, N = _prompts()[:3], 12
    dec = batch_decoder(m, prompts, N)
    try:
        m.generate_batch(prompts, N, top_k=1, decoder=dec)
        assert list(dec.sgraphs) == [(1.0, 1, None)] and dec.replays == N - 1 and dec.K == 0
    finally:
        dec.release()


def test_gpu_refusals(kernels):
    """What only the GPU refuses: more than 16 step rows, and a model without the fused decode kernels."""
    from nanosandbox_amd.models import GPT, GPTConfig
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    for B, K in ((3, 7), (9, 1), (4, 4)):
        with pytest.raises(ValueError):
            Decoder(m, B, speculate=K)
        with pytest.raises(ValueError):
            m.generate_batch(_prompts()[:B], 4, top_k=1, speculate=K)
    Decoder(m, 8, speculate=1).release()  # 16 step rows: the skinny kernels' last size
    wide = GPT(GPTConfig(block_size=64, vocab_size=V, n_layer=1, n_head=2, n_embd=256, dropout=0.0, bias=False))
    wide = wide.eval().to(DEV).set_compute_dtype(BF)  # head_dim 128
    with pytest.raises(ValueError):
        Decoder(wide, 1, speculate=2)
    assert not any(hasattr(p, "compute") for p in list(m.parameters()) + list(wide.parameters()))


# ---------------------------------------------------------------------------------------------
# 4. schedule independence, sampled: what is drafted changes the steps, never the tokens

@pytest.mark.parametrize("mode", ["bf16", "q8"])
def test_sampled_tokens_do_not_depend_on_the_drafts(kernels, mode):
    from nanosandbox_amd.runtime.decode import batch_decoder

    m = _model()
    kw = dict(quantize="int8") if mode == "q8" else {}
    K, N = 4, 40
    prompts = _prompts()[:3]
    dec = batch_decoder(m, prompts, N, speculate=K, **kw)

    def run(table=None, stop=None):
        torch.manual_seed(7)
        out = m.generate_batch(prompts, N, temperature=1.0, top_k=50, stop_token=stop, speculate=K, decoder=dec,
                               spec_table=table, **kw)
        return out, dec.spec_stats

    try:
        y, _ = run()
        assert all(a.numel() == p.numel() + N for a, p in zip(y, prompts))
        right, st = run(y)
        assert all(torch.equal(a, b) for a, b in zip(right, y))
        assert st["steps"] == [-(-(N - 1) // (K + 1))] * 3 and st["accepted"] == st["offered"]
        wrong, st = run([(a + 1) % V for a in y])
        assert all(torch.equal(a, b) for a, b in zip(wrong, y))
        assert st["steps"] == [N - 1] * 3 and st["accepted"] == [0] * 3
        # a stop token: some row's k-th new token (k >= 2) that another row never emits
        new = [a[p.numel():].tolist() for a, p in zip(y, prompts)]
        stop = next((x[k] for x in new for k in range(1, len(x))
                     if x.index(x[k]) >= 1 and any(x[k] not in z for z in new)), None)
        assert stop is not None, new
        cut = [x[:x.index(stop) + 1] if stop in x else x for x in new]
        for table in (None, y, [(a + 1) % V for a in y]):
            out, st = run(table, stop)
            assert [a[p.numel():].tolist() for a, p in zip(out, prompts)] == cut
            assert [s + a for s, a in zip(st["steps"], st["accepted"])] == [len(x) - 1 for x in cut]
        assert len(dec.sgraphs) == 4  # n-gram and table drafts, with and without the stop token
    finally:
        dec.release()


# ---------------------------------------------------------------------------------------------
# 5. the cache tail: prompt + new tokens == block_size, rows near the end have dead queries

def test_cache_tail(kernels):
    from nanosandbox_amd.runtime.decode import batch_decoder

    m = _model()
    T = m.config.block_size
    prompts, N = _prompts((T - 24, T - 30)), 24  # row 0 ends at the cache's last position
    outs = {}
    for K in (1, 7):
        dec = batch_decoder(m, prompts, N, speculate=K)
        try:
            outs[K] = m.generate_batch(prompts, N, top_k=1, speculate=K, decoder=dec)
            # every row stops at its last token's position, row 0 at the cache's last row
            assert dec.pos.tolist() == [T - 1, T - 7] and dec.done.tolist() == [1, 1]
            assert all(bool(torch.isfinite(c.float()).all()) for c in dec.kc + dec.vc)
            st = dec.spec_stats
            assert [s + a for s, a in zip(st["steps"], st["accepted"])] == [N - 1] * 2
        finally:
            dec.release()
    for a, b, p in zip(outs[1], outs[7], prompts):
        assert torch.equal(a, b) and a.numel() == p.numel() + N
        assert 0 <= int(a.min()) and int(a.max()) < V
