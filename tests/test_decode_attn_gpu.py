"""The decode-side attention kernels per key and per element: ``decode_attn_chunk`` and the
combines (``nsa_decode_attn`` / ``_rows``, ``nsa_gemv_attn``), the shared-prompt kernel
(``nsa_decode_attn_shared`` / ``_rows``), prefix attention (``nsa_prefix_attn``) and the bf16
``nsa_kv_append`` / ``_rows``, against the float64 references and the three pins of
``test_decode_attn_refs.py`` (counting, selecting, peaked: its docstring derives them).

Every entry point is called raw through ``_lib.call``.  ``ws`` and ``out`` are NaN-prefilled,
every cache row the query may not see is NaN (appending, the row at ``pos`` too, in the K and in
the V cache), and every input buffer is compared bit for bit (int16 views: NaN != NaN) before
and after.  One contract for the row at ``pos``: without ``append`` it is the cache's, K and V
alike, and the k | v parts of ``qkv`` are not read (``test_key_at_pos_is_the_cache_row``).

Worst error / bound of the peaked inputs on an MI355X: decode 0.9145, shared prompt 0.8804
(B = 1) and 0.9257, prefix attention 0.9293 (B = 1) and 0.9339.  All of it is the bound's first
term, the bf16 rounding of an output just above a power of two; the fp32 emulation of the
refs file, rounded to bf16, gives the same five figures.
"""

import pytest
import torch

from test_decode_attn_refs import (BF, C, D, DEC_B, DEC_POS, DEC_T, H, INF, PF_BS, PF_PS, PF_SS, PF_TP, SCALE, SH_BS,
                                   SH_PS, SH_R, SH_TP, U16, combine_ref, count_cols, count_partial,
                                   dec_codes, dec_peaked, dec_row_positions, decode_ref, int_values, onehot_v,
                                   peaked_bound, pf_codes, pf_peaked, prefix_ref, sh_codes, sh_configs, sh_peaked,
                                   shared_keys, shared_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
I64 = torch.int64
F32 = torch.float32
U32 = 2.0 ** -24  # one fp32 rounding, relative


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _within(y, ref, bound, tag):
    ratio = float(((y.double() - ref).abs() / bound).max())
    assert ratio <= 1.0, f"{tag}: error / bound {ratio:.4f}"
    return ratio


def _parts(ws):
    """(m, l, pad, pad, o[64]) -> (m, l, o[64])"""
    return torch.cat([ws[..., :2], ws[..., 4:]], dim=-1)


def _empty(parts):
    return bool((parts[..., 0] == -INF).all()) and not bool(parts[..., 1:].any())


def _combine_bound(ref, mag, n):
    """One bf16 rounding of the result, and the combine's own fp32 work on mag = sum_s f_s |o_s| / L
    (>= |ref|): one rounding per partial in the numerator's sum and one in the denominator's (2 n
    at the worst), and 8 for exp2 (2 ulp, in both sums), the scaling by 1 / L or the division."""
    return U16 * ref.abs() + (2 * n + 8) * U32 * mag + 1e-30


def _combined(out, parts, tag):
    """out is the float64 combine of the partials the launch left, within one bf16 rounding."""
    ref, mag = combine_ref(parts)
    _within(out, ref, _combine_bound(ref, mag, parts.shape[-2]), tag + " combine")


def _qkv(q, kn, vn):
    """[B, H, D] each -> [B, 1, 3C] (q | k | v)"""
    return torch.stack([q, kn, vn], dim=1).reshape(q.shape[0], 1, 3 * C).contiguous()


# ------------------------------------------------------------------------------- raw launches
def _launch_decode(qkv, kc, vc, pos, append, rows):
    from nanosandbox_amd.ops import _lib

    B, T = kc.shape[0], kc.shape[2]
    ws = torch.full((B, H, -(-T // 256), 4 + D), NAN, device=DEV, dtype=F32)
    out = torch.full((B, H, D), NAN, device=DEV, dtype=BF)
    _lib.call("nsa_decode_attn_rows" if rows else "nsa_decode_attn", _lib.ptr(qkv), _lib.ptr(kc), _lib.ptr(vc),
              _lib.ptr(pos), _lib.ptr(ws), _lib.ptr(out), B, H, D, T, SCALE, int(append), _lib.stream())
    torch.cuda.synchronize()
    return out, ws


def _launch_shared(qkv, pk, pv, kc, vc, plen, pos, append, rows):
    from nanosandbox_amd.ops import _lib

    B, R, Tp = kc.shape[0], kc.shape[2], pk.shape[1]
    ws = torch.full((B, H, -(-Tp // 128) + -(-R // 256), 4 + D), NAN, device=DEV, dtype=F32)
    out = torch.full((B, H, D), NAN, device=DEV, dtype=BF)
    _lib.call("nsa_decode_attn_shared_rows" if rows else "nsa_decode_attn_shared", _lib.ptr(qkv), _lib.ptr(pk),
              _lib.ptr(pv), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(plen), _lib.ptr(pos), _lib.ptr(ws), _lib.ptr(out),
              B, H, Tp, R, SCALE, int(append), _lib.stream())
    torch.cuda.synchronize()
    return out, ws


def _launch_prefix(qkv, pk, pv, P):
    from nanosandbox_amd.ops import _lib

    B, S = qkv.shape[:2]
    out = torch.full((B, S, C), NAN, device=DEV, dtype=BF)
    _lib.call("nsa_prefix_attn", _lib.ptr(qkv), _lib.ptr(pk), _lib.ptr(pv), _lib.ptr(out), B, S, H, pk.shape[1], P,
              SCALE, _lib.stream())
    torch.cuda.synchronize()
    return out


def _launch_gemv_attn(ws, W, y):
    from nanosandbox_amd.ops import _lib

    _lib.call("nsa_gemv_attn", _lib.ptr(ws), ws.shape[1], _lib.ptr(W), None, _lib.ptr(y), W.shape[0], W.shape[1], 0, 0,
              _lib.stream())
    torch.cuda.synchronize()


def _launch_kv_append(qkv, kc, vc, pos, pos0, T):
    from nanosandbox_amd.ops import _lib

    B, S = qkv.shape[:2]
    _lib.call("nsa_kv_append", _lib.ptr(qkv), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(pos), pos0, B, S, H, D, T,
              _lib.stream())
    torch.cuda.synchronize()


def _launch_kv_append_rows(qkv, kc, vc, rows, pos0, Bc, T):
    from nanosandbox_amd.ops import _lib

    n, S = qkv.shape[:2]
    _lib.call("nsa_kv_append_rows", _lib.ptr(qkv), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(rows), pos0, n, Bc, S, H, D, T,
              _lib.stream())
    torch.cuda.synchronize()


# ======================================================================== the per-row decode kernel
def _run_decode(q, kn, vn, kc, vc, pos, append, rows, finite=True):
    """One launch on the caches given (changed in place).  pos: B positions, all equal unless
    ``rows``.  Asserts: qkv and pos untouched; the caches differ from before only in row pos[b]
    when appending (then bitwise the qkv rows), not at all otherwise; no NaN in ws and out
    -> (out [B, H, D] bf16, partials [B, H, n_split, 66])."""
    qkv = _qkv(q, kn, vn)
    pt = torch.tensor(pos if rows else pos[:1], device=DEV, dtype=I64)
    qkv0, pt0, kc0, vc0 = qkv.clone(), pt.clone(), kc.clone(), vc.clone()
    out, ws = _launch_decode(qkv, kc, vc, pt, append, rows)
    assert _same(qkv, qkv0) and torch.equal(pt, pt0)
    for b, p in enumerate(pos):
        if append and p < kc.shape[2]:
            kc0[b, :, p], vc0[b, :, p] = kn[b], vn[b]
    assert _same(kc, kc0) and _same(vc, vc0), (pos, append, rows)
    parts = _parts(ws)
    assert not bool(parts.isnan().any()), (pos, append, rows)
    if finite:
        assert not bool(out.isnan().any()), (pos, append, rows)
    return out, parts


def _dec_caches(K, V, pos, append):
    """Clones with NaN in every row the query may not see: the rows past pos[b], and appending
    the row at pos[b] too."""
    kc, vc = K.clone(), V.clone()
    for b, p in enumerate(pos):
        kc[b, :, p + (0 if append else 1):] = NAN
        vc[b, :, p + (0 if append else 1):] = NAN
    return kc, vc


def _dec_sweep():
    """(tag, positions, per-row form) of every launch shape: each position shared, and as one of
    three unequal per-row positions."""
    for i, p in enumerate(DEC_POS):
        yield f"pos {p}", [p] * DEC_B, False
        yield f"rows {dec_row_positions(i)}", dec_row_positions(i), True


_COUNTS = {}


def _count_partial(lo, hi, layout, G):
    key = (lo, max(hi, lo), layout, G)
    if key not in _COUNTS:
        _COUNTS[key] = count_partial(lo, hi, layout, G)
    return _COUNTS[key]


@pytest.mark.parametrize("layout", [0, 1], ids=["in-chunk", "by-chunk"])
def test_decode_counting_pin(kernels, layout):
    """q = 0, one-hot V: every partial, live or empty, is exactly (0, live keys, counts) and out
    is count / n within one bf16 rounding.  Without append the k | v parts of qkv hold other
    integers, which a kernel that read them would count."""
    B, T, G = DEC_B, DEC_T, 256
    v1 = onehot_v(torch.arange(T), layout, G).to(DEV)
    V = v1[None, None].expand(B, H, T, D).contiguous()
    K, other = _dev(int_values((B, H, T, D)), int_values((B, H, D)))
    q = torch.zeros(B, H, D, device=DEV, dtype=BF)
    for tag, pos, rows in _dec_sweep():
        for append in (0, 1):
            vn = torch.stack([v1[p] for p in pos])[:, None].expand(B, H, D).contiguous() if append else other
            kc, vc = _dec_caches(K, V, pos, append)
            out, parts = _run_decode(q, other, vn, kc, vc, pos, append, rows)
            want = torch.stack([torch.stack([_count_partial(k0, min(k0 + G, p + 1), layout, G)
                                             for k0 in range(0, T, G)]) for p in pos])          # [B, n_split, 66]
            assert torch.equal(parts.cpu().double(), want[:, None].expand(B, H, -1, -1)), (tag, append)
            ref = torch.stack([count_cols(0, p + 1, layout, G) / (p + 1) for p in pos])[:, None].expand(B, H, D)
            _within(out.cpu(), ref, U16 * ref + 1e-30, f"{tag} append {append}")


def _dec_targets(p):
    """key 0, every chunk's first and last key, pos - 1 and pos itself"""
    return sorted(t for t in {0, 255, 256, 511, 512, p - 1, p} if 0 <= t <= p)


@pytest.mark.parametrize("append", [0, 1])
def test_decode_selecting_pin(kernels, append):
    """Query 8 s_t against keys 8 s_k: out == V[t] bit for bit, the target swept over key 0, every
    chunk's edges, pos - 1 and pos.  Appending, the row at pos comes from qkv (the cache holds NaN
    there); otherwise from the cache, and qkv holds a code that is no key's and other values."""
    B, T = DEC_B, DEC_T
    code = (8 * dec_codes()).to(BF).to(DEV)                       # [H, T + 1, 64], the last one spare
    K = code[None, :, :T].expand(B, H, T, D).contiguous()
    V, other = _dev(int_values((B, H, T, D)), int_values((B, H, D)))
    hs = torch.arange(H, device=DEV)
    for tag, pos, rows in _dec_sweep():
        tgs = [_dec_targets(p) for p in pos]
        for j in range(4):
            t = torch.tensor([[tg[(2 * j + h) % len(tg)] for h in range(H)] for tg in tgs], device=DEV)   # [B, H]
            q = code[hs[None, :], t]
            if append:
                pt = torch.tensor(pos, device=DEV)
                kn, vn = code[hs[None, :], pt[:, None]], V[torch.arange(B, device=DEV), :, pt]
            else:
                kn, vn = code[None, :, T].expand(B, H, D).contiguous(), other
            kc, vc = _dec_caches(K, V, pos, append)
            out, _ = _run_decode(q, kn, vn, kc, vc, pos, append, rows)
            want = V[torch.arange(B, device=DEV)[:, None], hs[None, :], t]
            assert _same(out, want), (tag, append, t.tolist())


def test_key_at_pos_is_the_cache_row(kernels):
    """The ``key == pos`` contract: without append, K[pos] and V[pos] are the cache's, as in the
    fp32 torch path of ``ops.decode_attention`` and in the int8 kernel.  (a) the query selects
    pos, whose cache K row is its code, while qkv's k is a code that is no key's: out is the
    cache's V[pos].  (b) the query selects another key t and qkv's k is that query itself: a
    kernel that scored pos against qkv's k would see two keys tie at the top and return the mean
    of two V rows.  (The kernel before this test took K[pos] from qkv: both failed.)"""
    from nanosandbox_amd import ops

    B, T = DEC_B, DEC_T
    code = (8 * dec_codes()).to(BF).to(DEV)
    K = code[None, :, :T].expand(B, H, T, D).contiguous()
    V, other = _dev(int_values((B, H, T, D)), int_values((B, H, D)))
    for p in (1, 255, 256, 599):
        for rows in (False, True):
            pos = [p, max(p - 1, 1), min(p + 1, T - 1)] if rows else [p] * B
            pt = torch.tensor(pos, device=DEV)
            kc, vc = _dec_caches(K, V, pos, 0)
            q = K[torch.arange(B, device=DEV), :, pt]                                # (a): target pos[b]
            spare = code[None, :, T].expand(B, H, D).contiguous()
            out, _ = _run_decode(q, spare, other, kc, vc, pos, 0, rows)
            want = V[torch.arange(B, device=DEV), :, pt]
            assert _same(out, want), (p, rows, "a")
            cpu = ops.decode_attention(_qkv(q, spare, other).cpu(), kc.cpu(), vc.cpu(), pt.cpu(), H)
            assert _same(cpu.view(B, H, D), want.cpu()), (p, rows, "the fp32 torch path")
            q = K[:, :, 0].contiguous()                                              # (b): target key 0
            out, _ = _run_decode(q, q.clone(), other, kc, vc, pos, 0, rows)
            assert _same(out, V[:, :, 0].contiguous()), (p, rows, "b")


def test_decode_peaked_per_element(kernels):
    """Peaked random inputs: every output element within 2^-8 |ref| + 2^-12 mag of float64, and
    out the float64 combine of the partials within one bf16 rounding."""
    q, kn, vn, K, V = _dev(*dec_peaked())
    worst = 0.0
    for tag, pos, rows in _dec_sweep():
        for append in (0, 1):
            Ke, Ve = K.clone(), V.clone()
            if append:
                for b, p in enumerate(pos):
                    Ke[b, :, p], Ve[b, :, p] = kn[b], vn[b]
            kc, vc = _dec_caches(K, V, pos, append)
            out, parts = _run_decode(q, kn, vn, kc, vc, pos, append, rows)
            ref, mag = decode_ref(q, Ke, Ve, pos)
            worst = max(worst, _within(out, ref, peaked_bound(ref, mag), f"{tag} append {append}"))
            _combined(out, parts, tag)
    print(f"decode, peaked inputs: worst error / bound {worst:.4f}")


def test_decode_append_is_kv_append_then_plain(kernels):
    """append=1 equals nsa_kv_append followed by append=0 bit for bit, in out and in every
    partial, and the shared-position form equals the per-row form at equal positions."""
    q, kn, vn, K, V = _dev(*dec_peaked())
    B, T = DEC_B, DEC_T
    qkv = _qkv(q, kn, vn)
    for i, p in enumerate(DEC_POS):
        kc, vc = _dec_caches(K, V, [p] * B, 1)
        a = _run_decode(q, kn, vn, kc, vc, [p] * B, 1, True)
        kc, vc = _dec_caches(K, V, [p] * B, 1)
        b = _run_decode(q, kn, vn, kc, vc, [p] * B, 1, False)
        kc, vc = _dec_caches(K, V, [p] * B, 1)
        _launch_kv_append(qkv, kc, vc, torch.tensor([p], device=DEV, dtype=I64), 0, T)
        c = _run_decode(q, kn, vn, kc, vc, [p] * B, 0, False)
        d = _run_decode(q, kn, vn, kc, vc, [p] * B, 0, True)
        for x in (b, c, d):
            assert _same(x[0], a[0]) and _same(x[1], a[1]), p
        pos = dec_row_positions(i)  # unequal positions: the append row by row
        kc, vc = _dec_caches(K, V, pos, 1)
        a = _run_decode(q, kn, vn, kc, vc, pos, 1, True)
        kc, vc = _dec_caches(K, V, pos, 1)
        for r, pr in enumerate(pos):
            _launch_kv_append(qkv[r:r + 1], kc[r:r + 1], vc[r:r + 1], None, pr, T)
        c = _run_decode(q, kn, vn, kc, vc, pos, 0, True)
        assert _same(c[0], a[0]) and _same(c[1], a[1]), pos


@pytest.mark.parametrize("p", [600, 700])
def test_decode_position_past_the_cache(kernels, p):
    """pos >= Tmax: no cache byte changes and every partial is the empty partial.  ``out`` is not
    asserted: the combine of empty partials only is 2^(-inf + inf) * 0 / 0, NaN in every element.
    No caller reaches it: ``Decoder`` sizes its caches to at most block_size rows and the front
    ends of ``runtime/decode.py`` (``_cached_mode``, ``_batch_plan``) refuse or reroute a request
    whose prompt + new tokens exceed them, so no step runs at a position past the last cache row
    (the position-embedding table ends there too)."""
    q, kn, vn, K, V = _dev(*dec_peaked())
    for rows in (False, True):
        for append in (0, 1):
            pos = [p, 3, p + 1] if rows else [p] * DEC_B
            kc, vc = K.clone(), V.clone()
            _, parts = _run_decode(q, kn, vn, kc, vc, pos, append, rows, finite=False)  # asserts the caches
            for b, pb in enumerate(pos):
                assert _empty(parts[b]) == (pb >= DEC_T), (pos, b)


# ================================================================================== the combines
def _handmade(ns):
    """Hand-made partial sets [ns, 66] -> (sets [n, ns, 66] float64, twins [n, ns, 66]): a twin is
    its set with the partials that must vanish exactly replaced by empty ones."""
    g = torch.Generator().manual_seed(ns)

    def live(m, big=1.0):
        return torch.cat([torch.tensor([m, 1.5 + 40 * float(torch.rand(1, generator=g))]),
                          big * torch.randn(D, generator=g)]).double()

    empty = count_partial(0, 0, 0, 1)
    sets, twins = [], []
    for slot in (0, ns // 2, ns - 1):  # one live chunk among empty ones
        s = torch.stack([live(5.25) if i == slot else empty for i in range(ns)])
        sets.append(s)
        twins.append(s)
    if ns > 1:
        # maxima 200 log2 units apart: 2^-200 is 0 in fp32, so the lower chunk (large values) vanishes exactly
        lo, hi = (ns - 1) // 3, ns - 1 - (ns - 1) // 3 if ns > 2 else 1
        s = torch.stack([live(100.0) if i == hi else live(-100.0, 1e4) if i == lo else empty for i in range(ns)])
        sets.append(s)
        twins.append(torch.stack([s[i] if i == hi else empty for i in range(ns)]))
        s = torch.stack([live(-3.5) for _ in range(ns)])  # equal maxima
        sets.append(s)
        twins.append(s)
        s = torch.stack([live(float(i % 7) - 2.0) if i % 3 else empty for i in range(ns)])  # mixed
        sets.append(s)
        twins.append(s)
    return torch.stack(sets), torch.stack(twins)


@pytest.mark.parametrize("ns", [1, 2, 5, 67])
def test_combine_in_the_linear_prologue(kernels, ns):
    """Hand-made partials through ``nsa_gemv_attn`` with an identity W (every set one head): the
    float64 combine within one bf16 rounding; a chunk 200 log2 units below vanishes exactly."""
    sets, twins = _handmade(ns)
    n = sets.shape[0]
    W = torch.eye(n * D, device=DEV, dtype=BF)
    ys = []
    for parts in (sets, twins):
        ws = torch.full((n, ns, 4 + D), NAN, device=DEV, dtype=F32)  # the pad words stay NaN: never read
        ws[..., :2], ws[..., 4:] = parts[..., :2].to(DEV), parts[..., 2:].to(DEV)
        ws0, W0 = ws.clone(), W.clone()
        y = torch.full((n * D,), NAN, device=DEV, dtype=BF)
        _launch_gemv_attn(ws, W, y)
        assert _same(ws, ws0) and _same(W, W0) and not bool(y.isnan().any())
        ref, mag = combine_ref(ws0.cpu()[..., [0, 1] + list(range(4, 4 + D))])
        _within(y.cpu().view(n, D), ref, _combine_bound(ref, mag, ns), f"n_split {ns}")
        ys.append(y)
    assert _same(ys[0], ys[1])


def _run_shared(q, kn, vn, pk, pv, kc, vc, P, offs, append):
    """One launch of the shared-prompt entry point on the caches given (row caches changed in
    place).  pk / pv [H, Tp, D]; offs: one row offset pos - P (a shared position) or B.  Asserts:
    qkv, the prompt caches, plen and pos untouched; the row caches differ from before only at
    slot offs[b] when appending (then bitwise the qkv rows); no NaN in ws and out
    -> (out [B, H, D], partials [B, H, npc + nrc, 66])."""
    B = q.shape[0]
    rows = len(offs) > 1
    qkv = _qkv(q, kn, vn)
    plen = torch.tensor([P], device=DEV, dtype=I64)
    pt = torch.tensor([P + o for o in offs], device=DEV, dtype=I64)
    keep = [t.clone() for t in (qkv, pk, pv, plen, pt)]
    kc0, vc0 = kc.clone(), vc.clone()
    out, ws = _launch_shared(qkv, pk, pv, kc, vc, plen, pt, append, rows)
    assert all(_same(a, b) if a.dtype == BF else torch.equal(a, b) for a, b in zip((qkv, pk, pv, plen, pt), keep))
    for b, o in enumerate(offs if rows else offs * B):
        if append and 0 <= o < kc.shape[2]:
            kc0[b, :, o], vc0[b, :, o] = kn[b], vn[b]
    assert _same(kc, kc0) and _same(vc, vc0), (P, offs, append)
    parts = _parts(ws)
    assert not bool(parts.isnan().any()) and not bool(out.isnan().any()), (P, offs, append)
    return out, parts


@pytest.mark.parametrize("Tp", [300, 8320], ids=["wide", "past-64-partials"])
def test_combine_of_the_shared_form(kernels, Tp):
    """``decode_attn_combine_wide_kernel`` (up to 64 partials per row) and the fallback past that,
    reached through ``nsa_decode_attn_shared`` on a grid of mostly empty chunks: one live chunk at
    the first, a middle and the last slot; equal maxima in every chunk; maxima 200 log2 units
    apart.  out is the float64 combine of the partials in ws within one bf16 rounding, and the
    chunk far below vanishes exactly."""
    B, npc = 2, -(-Tp // 128)
    s = dec_codes()[:, 0].to(BF).to(DEV)                                      # one code per head [H, 64]
    pv = int_values((H, Tp, D)).to(DEV)
    V = int_values((B, H, 512, D)).to(DEV)
    q = (8 * s)[None].expand(B, H, D).contiguous()
    other = int_values((B, H, D)).to(DEV)
    nanp = torch.full((H, Tp, D), NAN, device=DEV, dtype=BF)

    def prompt(P, kfun):
        pk, pvc = nanp.clone(), nanp.clone()
        pk[:, :P], pvc[:, :P] = kfun(P), pv[:, :P]
        return pk, pvc

    flat = lambda P: s[:, None].expand(H, P, D)
    # one live chunk: the first slot (P = 5, the row slot negative), a middle one (no prompt, R = 512:
    # the row's chunk 0 of 2) and the last (no prompt, R = 256)
    for P, R, off, slot in ((5, 512, -1, 0), (0, 512, 3, npc), (0, 256, 3, npc)):
        pk, pvc = prompt(P, flat)
        kc = torch.full((B, H, R, D), NAN, device=DEV, dtype=BF)
        vc = kc.clone()
        if off >= 0:
            kc[:, :, :off + 1], vc[:, :, :off + 1] = flat(off + 1)[None], V[:, :, :off + 1]
        out, parts = _run_shared(q, other, other, pk, pvc, kc, vc, P, [off], 0)
        n = parts.shape[2]
        assert slot in (0, n - 1) or 0 < slot < n - 1
        assert all(_empty(parts[:, :, i]) == (i != slot) for i in range(n)), (P, R, off)
        _combined(out, parts, f"one live chunk at slot {slot} of {n}")
        want = (pv[:, :P].double().mean(1)[None].expand(B, H, D) if P else V[:, :, :off + 1].double().mean(2))
        _within(out, want, _combine_bound(want, 127.0, n), f"slot {slot}")
    # equal maxima: every key scores the same, every chunk is live with m = 64 log2(e) * 8 / 8
    R, off = 512, 300
    pk, pvc = prompt(Tp, flat)
    kc = torch.full((B, H, R, D), NAN, device=DEV, dtype=BF)
    vc = kc.clone()
    kc[:, :, :off + 1], vc[:, :, :off + 1] = flat(off + 1)[None], V[:, :, :off + 1]
    out, parts = _run_shared(q, other, other, pk, pvc, kc, vc, Tp, [off], 0)
    assert bool((parts[..., 0] == parts[0, 0, 0, 0]).all()) and bool(parts[..., 0].isfinite().all())
    _combined(out, parts, "equal maxima")
    want = (pv.double().sum(1)[None] + V[:, :, :off + 1].double().sum(2)) / (Tp + off + 1)
    _within(out, want, _combine_bound(want, 127.0, parts.shape[2]), "equal maxima")
    # 200 apart: chunk 0 holds K = s (+92.3 log2 units), every later key K = -1.25 s (-115.4)
    two = lambda P: torch.cat([flat(128), (-1.25 * flat(P - 128).float()).to(BF)], dim=1)
    pk, pvc = prompt(Tp, two)
    kc[:, :, :off + 1] = (-1.25 * flat(off + 1).float()).to(BF)[None]
    out, parts = _run_shared(q, other, other, pk, pvc, kc, vc, Tp, [off], 0)
    assert float((parts[..., 0, 0].min() - parts[..., 1:, 0].max())) >= 200.0
    _combined(out, parts, "maxima 200 apart")
    pk, pvc = prompt(128, flat)  # the same with the far chunks gone: bitwise the same output
    alone, _ = _run_shared(q, other, other, pk, pvc, kc, vc, 128, [-1], 0)
    assert _same(out, alone)


# ========================================================================== the shared-prompt kernel
def _sh_caches(pk, pv, K, V, P, offs, append):
    """Clones with NaN in every row no query may see: prompt rows from P on, row slots past
    offs[b], and appending the slot at offs[b] too."""
    pkc, pvc, kc, vc = pk.clone(), pv.clone(), K.clone(), V.clone()
    pkc[:, P:], pvc[:, P:] = NAN, NAN
    for b, o in enumerate(offs):
        kc[b, :, o + (0 if append else 1):] = NAN
        vc[b, :, o + (0 if append else 1):] = NAN
    return pkc, pvc, kc, vc


def _sh_sweep(B):
    for i, P in enumerate(SH_PS):
        for offs, append in sh_configs(i, B):
            yield P, offs, (offs * B if len(offs) == 1 else offs), append


@pytest.mark.parametrize("B", SH_BS)
@pytest.mark.parametrize("layout", [0, 1], ids=["in-chunk", "by-wave"])
def test_shared_counting_pin(kernels, layout, B):
    """q = 0, one-hot V over the prompt (by key, or by 32-key wave) and over the row slots: every
    partial of every row exactly (0, live keys, counts) or empty, out = count / n."""
    Tp, R = SH_TP, SH_R
    pv1, v1 = onehot_v(torch.arange(Tp), layout, 32).to(DEV), onehot_v(torch.arange(R), layout, 256).to(DEV)
    pv = pv1[None].expand(H, Tp, D).contiguous()
    V = v1[None, None].expand(B, H, R, D).contiguous()
    pk, K, other = _dev(int_values((H, Tp, D)), int_values((B, H, R, D)), int_values((B, H, D)))
    q = torch.zeros(B, H, D, device=DEV, dtype=BF)
    for P, offs, ro, append in _sh_sweep(B):
        vn = torch.stack([v1[o] for o in ro])[:, None].expand(B, H, D).contiguous() if append else other
        pkc, pvc, kc, vc = _sh_caches(pk, pv, K, V, P, ro, append)
        out, parts = _run_shared(q, other, vn, pkc, pvc, kc, vc, P, offs, append)
        pw = torch.stack([_count_partial(k0, min(k0 + 128, P), layout, 32) for k0 in range(0, Tp, 128)])
        want = torch.stack([torch.cat([pw, torch.stack([_count_partial(k0, min(k0 + 256, o + 1), layout, 256)
                                                        for k0 in range(0, R, 256)])]) for o in ro])
        assert torch.equal(parts.cpu().double(), want[:, None].expand(B, H, -1, -1)), (P, offs, append)
        ref = torch.stack([(count_cols(0, P, layout, 32) + count_cols(0, o + 1, layout, 256)) / (P + o + 1)
                           for o in ro])[:, None].expand(B, H, D)
        _within(out.cpu(), ref, U16 * ref + 1e-30, f"P {P} offs {offs[:3]}")


def _sh_targets(P, off):
    """virtual keys: each wave's first and last prompt key, P - 1, the row's slot 0 and its slot pos - P"""
    t = {P - 1, P, P + off}
    for w in range(-(-P // 32)):
        t |= {32 * w, min(32 * w + 31, P - 1)}
    return sorted(t)


@pytest.mark.parametrize("B", SH_BS)
def test_shared_selecting_pin(kernels, B):
    """out == V[t] bit for bit over the virtual key list, the targets swept over every wave's
    edges in the prompt chunks, P - 1, the row's slot 0 and slot pos - P; rows 15, 16 and B - 1
    get different targets, so a lane that reads or stores another row's query shows."""
    Tp, R = SH_TP, SH_R
    code = (8 * sh_codes()).to(BF).to(DEV)                        # [H, Tp + R + 1, 64]
    pk = code[:, :Tp].contiguous()
    K = code[None, :, Tp:Tp + R].expand(B, H, R, D).contiguous()
    pv, V, other = _dev(int_values((H, Tp, D)), int_values((B, H, R, D)), int_values((B, H, D)))
    spare = code[None, :, Tp + R].expand(B, H, D).contiguous()
    hs, bs = torch.arange(H, device=DEV), torch.arange(B, device=DEV)
    for P, offs, ro, append in _sh_sweep(B):
        tgs = [_sh_targets(P, o) for o in ro]
        rt = torch.tensor(ro, device=DEV)
        kn, vn = (code[hs[None, :], Tp + rt[:, None]], V[bs, :, rt]) if append else (spare, other)
        for j in range(-(-max(map(len, tgs)) // (B * H))):
            idx = [[(H * (b + j * B) + h) % len(tgs[b]) for h in range(H)] for b in range(B)]
            for n, b in enumerate(r for r in (15, 16, B - 1) if r < B and B > 15):
                idx[b] = [(n + h + j) % len(tgs[b]) for h in range(H)]
            t = torch.tensor([[tgs[b][i] for i in idx[b]] for b in range(B)], device=DEV)        # [B, H], virtual
            q = code[hs[None, :], torch.where(t < P, t, t - P + Tp)]
            pkc, pvc, kc, vc = _sh_caches(pk, pv, K, V, P, ro, append)
            out, _ = _run_shared(q, kn, vn, pkc, pvc, kc, vc, P, offs, append)
            want = torch.where((t < P)[..., None], pv[hs[None, :], t.clamp(max=Tp - 1)],
                               V[bs[:, None], hs[None, :], (t - P).clamp(min=0)])
            assert _same(out, want), (P, offs, append, t.tolist())


@pytest.mark.parametrize("B", SH_BS)
def test_shared_peaked_per_element(kernels, B):
    """Peaked random inputs against float64 over the concatenated keys, per element; empty
    partials exactly empty, live ones finite; out the float64 combine of the partials."""
    q, kn, vn, pk, pv, K, V = _dev(*sh_peaked(B))
    npc = -(-SH_TP // 128)
    worst = 0.0
    for P, offs, ro, append in _sh_sweep(B):
        Ke, Ve = K.clone(), V.clone()
        if append:
            for b, o in enumerate(ro):
                Ke[b, :, o], Ve[b, :, o] = kn[b], vn[b]
        pkc, pvc, kc, vc = _sh_caches(pk, pv, K, V, P, ro, append)
        out, parts = _run_shared(q, kn, vn, pkc, pvc, kc, vc, P, offs, append)
        live = -(-P // 128)
        assert _empty(parts[:, :, live:npc]) and bool(parts[:, :, :live, 0].isfinite().all())
        for b, o in enumerate(ro):
            lr = o // 256 + 1
            assert _empty(parts[b, :, npc + lr:]) and bool(parts[b, :, npc:npc + lr, 0].isfinite().all())
        ref, mag = shared_ref(q, pk, pv, Ke, Ve, P, [P + o for o in ro])
        worst = max(worst, _within(out, ref, peaked_bound(ref, mag), f"P {P} offs {offs[:3]} append {append}"))
        _combined(out, parts, f"P {P}")
    print(f"shared prompt, B {B}, peaked inputs: worst error / bound {worst:.4f}")


# ================================================================================= prefix attention
def _run_prefix(q, k, v, pk, pv, P, op=False):
    """q, k, v [B, H, S, D], prefix caches [H, Tp, D] (given with NaN from row P on) -> out
    [B, H, S, D] bf16.  Asserts: every out row written, qkv / pk / pv untouched."""
    B, _, S, _ = q.shape
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, S, 3 * C).contiguous()
    keep = [t.clone() for t in (qkv, pk, pv)]
    out = _launch_prefix(qkv, pk, pv, P)
    assert all(_same(a, b) for a, b in zip((qkv, pk, pv), keep)) and not bool(out.isnan().any()), (B, P, S)
    if op:
        from nanosandbox_amd import ops
        assert _same(ops.prefix_attention(qkv, pk[None], pv[None], P, H), out), (B, P, S)  # the op is that launch
    return out.view(B, S, H, D).permute(0, 2, 1, 3)


def _pf_prefix(pk, pv, P):
    pkc, pvc = pk.clone(), pv.clone()
    pkc[:, P:], pvc[:, P:] = NAN, NAN
    return pkc, pvc


@pytest.mark.parametrize("B", PF_BS)
@pytest.mark.parametrize("layout,G", [(0, 32), (1, 32), (1, 128)], ids=["in-round", "by-wave", "by-round"])
def test_prefix_counting_pin(kernels, layout, G, B):
    """q = 0, V one-hot by virtual key index: out[b, i] is the counts over P + i + 1 keys."""
    Smax = max(PF_SS)
    pk, kr = _dev(int_values((H, PF_TP, D)), int_values((B, H, Smax, D)))
    for P in PF_PS:
        hot = onehot_v(torch.arange(P + Smax), layout, G)
        cum = torch.cumsum(hot.double(), 0)                                  # cum[n - 1]: the counts of n keys
        assert torch.equal(cum[P + 5], count_cols(0, P + 6, layout, G))
        hot = hot.to(DEV)
        pv = torch.zeros(H, PF_TP, D, device=DEV, dtype=BF)
        pv[:, :P] = hot[:P]
        pkc, pvc = _pf_prefix(pk, pv, P)
        for S in PF_SS:
            q = torch.zeros(B, H, S, D, device=DEV, dtype=BF)
            v = hot[None, None, P:P + S].expand(B, H, S, D).contiguous()
            out = _run_prefix(q, kr[:, :, :S].contiguous(), v, pkc, pvc, P)
            ref = (cum[P:P + S] / torch.arange(P + 1, P + S + 1)[:, None].double())[None, None].expand(B, H, S, D)
            _within(out.cpu(), ref, U16 * ref + 1e-30, f"P {P} S {S}")


def _pf_targets(P, i):
    """virtual keys query i may be asked for: key 0, the wave and round edges, P - 1, the row's key 0, i - 1 and i"""
    n = P + i + 1
    t = {0, P - 1, P, P + i - 1, P + i}
    for g in (32, 128):
        for j in range(1, n // g + 1):
            t |= {g * j - 1, g * j}
    return sorted(x for x in t if 0 <= x < n)


@pytest.mark.parametrize("B", PF_BS)
def test_prefix_selecting_pin(kernels, B):
    """Every query has its own target, cycling over prefix key 0, the wave-round edges, P - 1, the
    row's key 0, key i - 1 and key i: out[b, i] == V[t] bit for bit.  A query that sees one key
    too many or too few, or a column group with the other group's limit, returns other integers."""
    Tp, Smax = PF_TP, max(PF_SS)
    code = (8 * pf_codes()).to(BF).to(DEV)                        # [H, Tp + Smax + 1, 64]
    pk = code[:, :Tp].contiguous()
    kr = code[None, :, Tp:Tp + Smax].expand(B, H, Smax, D).contiguous()
    pv, vr = _dev(int_values((H, Tp, D)), int_values((B, H, Smax, D)))
    hs, bs = torch.arange(H, device=DEV), torch.arange(B, device=DEV)
    for P in PF_PS:
        pkc, pvc = _pf_prefix(pk, pv, P)
        tg = [_pf_targets(P, i) for i in range(Smax)]
        for S in PF_SS:
            t = torch.tensor([[[tg[i][(i + 3 * b + 5 * h + S) % len(tg[i])] for i in range(S)] for h in range(H)]
                              for b in range(B)], device=DEV)                                     # [B, H, S], virtual
            q = code[hs[None, :, None], torch.where(t < P, t, t - P + Tp)]
            v = vr[:, :, :S].contiguous()
            out = _run_prefix(q, kr[:, :, :S].contiguous(), v, pkc, pvc, P)
            vv = shared_keys(pv, v, P)                                                            # [B, H, P + S, D]
            want = vv[bs[:, None, None], hs[None, :, None], t]
            assert _same(out.contiguous(), want), (P, S, (out.float() != want.float()).any(-1).nonzero()[:4].tolist())


@pytest.mark.parametrize("B", PF_BS)
def test_prefix_peaked_per_element(kernels, B):
    """Peaked random inputs against float64 per element; ``ops.prefix_attention`` is the raw launch."""
    worst = 0.0
    for P in PF_PS:
        for S in PF_SS:
            q, k, v, pk, pv = _dev(*pf_peaked(B, S))
            pkc, pvc = _pf_prefix(pk, pv, P)
            out = _run_prefix(q.contiguous(), k.contiguous(), v.contiguous(), pkc, pvc, P, op=True)
            ref, mag = prefix_ref(q, k, v, pk, pv, P)
            worst = max(worst, _within(out, ref, peaked_bound(ref, mag), f"P {P} S {S}"))
    print(f"prefix attention, B {B}, peaked inputs: worst error / bound {worst:.4f}")


# ======================================================================================== kv_append
def _guarded(B, T):
    """A NaN-filled cache [B, H, T, D] inside a NaN-filled buffer with one guard row on each side."""
    big = torch.full((B + 2, H, T, D), NAN, device=DEV, dtype=BF)
    return big, big[1:-1]


@pytest.mark.parametrize("S", [1, 77])
@pytest.mark.parametrize("device_pos", [False, True], ids=["host-pos", "device-pos"])
def test_kv_append_rows_and_dropped_tail(kernels, device_pos, S):
    """Rows p0 .. p0 + S - 1 of both caches are the qkv rows bitwise and every other byte keeps
    its NaN prefill, guard rows included; rows that would land at or past Tmax are dropped."""
    B, T = 2, 128
    qkv = int_values((B, S, 3 * C)).to(DEV)
    k, v = qkv.view(B, S, 3, H, D)[:, :, 1:].permute(2, 0, 3, 1, 4)                # [B, H, S, D] each
    for p0 in (0, 5, T - S, T - S + 3 if S > 3 else T - 1, T, T + 40):
        (bk, kc), (bv, vc) = _guarded(B, T), _guarded(B, T)
        wk, wv, q0 = bk.clone(), bv.clone(), qkv.clone()
        n = max(0, min(S, T - p0))
        wk[1:-1, :, p0:p0 + n], wv[1:-1, :, p0:p0 + n] = k[:, :, :n], v[:, :, :n]
        pos = torch.tensor([p0], device=DEV, dtype=I64) if device_pos else None
        _launch_kv_append(qkv, kc, vc, pos, 0 if device_pos else p0, T)
        assert _same(bk, wk) and _same(bv, wv) and _same(qkv, q0), (p0, S)


def test_kv_append_row_map(kernels):
    """``nsa_kv_append_rows`` with the indices -1, Bc and a valid one: only the valid cache row changes."""
    Bc, T, S, p0 = 3, 128, 5, 9
    qkv = int_values((3, S, 3 * C)).to(DEV)
    k, v = qkv.view(3, S, 3, H, D)[:, :, 1:].permute(2, 0, 3, 1, 4)
    for rows in ([-1, Bc, 1], [2, -1, Bc], [Bc + 5, 0, -7]):
        (bk, kc), (bv, vc) = _guarded(Bc, T), _guarded(Bc, T)
        wk, wv = bk.clone(), bv.clone()
        for j, r in enumerate(rows):
            if 0 <= r < Bc:
                wk[1 + r, :, p0:p0 + S], wv[1 + r, :, p0:p0 + S] = k[j], v[j]
        rt = torch.tensor(rows, device=DEV, dtype=I64)
        _launch_kv_append_rows(qkv, kc, vc, rt, p0, Bc, T)
        assert _same(bk, wk) and _same(bv, wv) and rt.tolist() == rows, rows
