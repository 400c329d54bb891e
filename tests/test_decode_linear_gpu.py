"""The weight-streaming decode linears bit for bit and per element: ``nsa_gemv``, ``nsa_gemv_ln``,
``nsa_gemv_emb_ln``, ``nsa_skinny_gemm``, ``nsa_skinny_ln_gemm``, their ``_q8`` forms and
``nsa_gemv_attn_q8``, against the float64 references of ``test_decode_linear_refs.py`` (its docstring
derives the two exact devices and every bound).

Every entry point is launched raw through ``_lib.call``.  ``y`` (and ``s_out`` / ``res_out``) is a
view inside a NaN-filled flat buffer with 16 guard elements on each side: after every launch the
view holds no NaN and the guards are untouched; after a refusal, and for an ``s_out`` without a
branch, the whole buffer is.

The random-valued tests print their worst error / bound (``-s``); the figures measured on an MI355X
stand in their docstrings.  All of them sit just under 1 by construction: a bf16 output's own
rounding is up to the whole 2^-8 |ref| term; the fp32 outputs use 0.2 % of their bound.
"""

import math
import os
import subprocess
import sys

import pytest
import torch

from test_decode_attn_gpu import _combine_bound, _handmade, _within
from test_decode_attn_refs import D, combine_ref
from test_decode_linear_refs import (AMBIGUOUS_SHARE, BF, EMB_POS, EMB_ROWS, EMB_TOK, EPS, F32, GEMV1_Q8_K, GEMV_K,
                                     GEMV_N, GEMV_ROWS, GEMV_WIDE, RAND_GEMV, RAND_ROW_LN, RAND_SKINNY,
                                     RAND_SKINNY_LN, RAND_SKINNY_Q8, ROW_LN_K, ROW_LN_N, ROW_LN_WIDE, SKINNY_K,
                                     SKINNY_LN_K, SKINNY_LN_N, SKINNY_LN_ROWS, SKINNY_N, SKINNY_Q8_K, SKINNY_Q8_N,
                                     SKINNY_Q8_ROWS, SKINNY_ROWS, exact_ln_params, exact_ln_rows, exact_ln_x,
                                     int_bias, int_weight, int_x, linear_ref, ln_bound, ln_linear_ref, plain_bound,
                                     rand_linear, rand_ln, rand_tables, split_res_branch, split_tables)
from test_layernorm_gpu import HIP_INVALID_VALUE, _call

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
I64 = torch.int64
GUARD = 16
KINDS = pytest.mark.parametrize("q8", [False, True], ids=["bf16", "int8"])


def _by_kind(ks):
    """(q8, K) over a table of widths per weight kind"""
    return pytest.mark.parametrize("q8,K", [pytest.param(q8, K, id=f"{'int8' if q8 else 'bf16'}-{K}")
                                            for q8 in (False, True) for K in ks[q8]])


class Guarded:
    """A NaN-filled flat buffer; ``view`` is its inside, GUARD elements from either end."""

    def __init__(self, shape, dtype):
        n = math.prod(shape)
        self.flat = torch.full((n + 2 * GUARD,), NAN, device=DEV, dtype=dtype)
        self.view = self.flat[GUARD:GUARD + n].view(shape)

    def written(self):
        nan = self.flat.isnan()
        return bool(nan[:GUARD].all()) and bool(nan[-GUARD:].all()) and not bool(nan[GUARD:-GUARD].any())

    def untouched(self):
        return bool(self.flat.isnan().all())


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _name(kind, q8):
    return "nsa_" + kind + ("_q8" if q8 else "")


def _w(W, scale, q8):
    return [W, scale] if q8 else [W]


# ------------------------------------------------------------------------------- raw launches
def call_plain(kind, q8, x, W, scale, bias, y, rows, N, K, act=0, f32=0):
    _call(_name(kind, q8), x, *_w(W, scale, q8), bias, y, rows, N, K, act, f32)


def call_row_ln(q8, res, branch, res_out, lw, lb, W, scale, bias, y, N, K, act=0, f32=0, pos_inc=None):
    _call(_name("gemv_ln", q8), res, branch, res_out, lw, lb, *_w(W, scale, q8), bias, y, N, K, EPS, act, f32, pos_inc)


def call_emb_ln(q8, tok, pos, wte, wpe, res_out, lw, lb, W, scale, bias, y, N, K, act=0, f32=0):
    _call(_name("gemv_emb_ln", q8), tok, pos, wte, wpe, res_out, lw, lb, *_w(W, scale, q8), bias, y, N, K, EPS, act,
          f32)


def call_skinny_ln(q8, res, branch, s_out, lw, lb, W, scale, bias, y, rows, N, K, act=0, f32=0):
    _call(_name("skinny_ln_gemm", q8), res, branch, s_out, lw, lb, EPS, *_w(W, scale, q8), bias, y, rows, N, K, act,
          f32)


def call_attn(q8, ws, W, scale, bias, y, N, K, act=0, f32=0):
    _call(_name("gemv_attn", q8), ws, ws.shape[1], *_w(W, scale, q8), bias, y, N, K, act, f32)


def _out(rows, N, f32):
    return Guarded((rows, N), F32 if f32 else BF)


def _exact(g, ref, f32, tag):
    """The launch wrote all of y and nothing beside it, and y is the float64 result bit for bit."""
    torch.cuda.synchronize()
    assert g.written(), tag
    assert torch.equal(ref.float().double(), ref), tag  # the premise: ref is an fp32 number
    want = ref.float() if f32 else ref.to(BF)
    assert torch.equal(g.view, want), (tag, (g.view != want).nonzero()[:4].tolist())


_WEIGHTS = {}


def _weights(N, K, q8):
    """The integer weights on the device (the last few shapes stay cached)."""
    key = (N, K, q8)
    if key not in _WEIGHTS:
        while len(_WEIGHTS) > 3:
            _WEIGHTS.pop(next(iter(_WEIGHTS)))
        _WEIGHTS[key] = _dev(*int_weight(N, K, q8))
    return _WEIGHTS[key]


# =================================================================== 1. exact pins, plain linears
def _plain_exact(kind, q8, rows, N, K):
    x, b = _dev(int_x(rows, K), int_bias(N))
    W, scale = _weights(N, K, q8)
    x0 = x.clone()
    for bias in (None, b):
        ref = linear_ref(x, W, scale, bias)[0]
        for f32 in (0, 1):
            g = _out(rows, N, f32)
            call_plain(kind, q8, x, W, scale, bias, g.view, rows, N, K, 0, f32)
            _exact(g, ref, f32, (kind, q8, rows, N, K, bias is not None, f32))
    assert torch.equal(x, x0)


@_by_kind(GEMV_K)
def test_gemv_exact(kernels, q8, K):
    """``nsa_gemv`` / ``_q8`` at 1 .. 8 rows (the templates M = 1, 2, 4, 8 and their zero-padded rows)
    and every clamped tail width of a column block: integer operands, bit for bit."""
    for rows in GEMV_ROWS:
        for N in GEMV_N:
            _plain_exact("gemv", q8, rows, N, K)


@KINDS
def test_gemv_exact_many_column_blocks(kernels, q8):
    """An odd N past 4096 columns at K = 64."""
    for rows in GEMV_ROWS:
        _plain_exact("gemv", q8, rows, *GEMV_WIDE)


@pytest.mark.parametrize("K", GEMV1_Q8_K)
def test_gemv1_q8_exact(kernels, K):
    """The single-row int8 kernel in every ``q8_cfg`` class (K <= 1024, 2048, 4096, 8192), on both sides
    of each class edge, and the K loop beyond 8192."""
    for N in GEMV_N:
        _plain_exact("gemv", True, 1, N, K)


@pytest.mark.parametrize("K", SKINNY_K)
def test_skinny_gemm_exact(kernels, K):
    """``nsa_skinny_gemm``, MT = 1, 2, 4 on both sides of each row-group edge; K of 1 and 3 units, one
    full round of 4 x 8 units, one unit into the second round, and three rounds."""
    for rows in SKINNY_ROWS:
        for N in SKINNY_N:
            _plain_exact("skinny_gemm", False, rows, N, K)


@pytest.mark.parametrize("K", SKINNY_Q8_K)
def test_skinny_gemm_q8_exact(kernels, K):
    """``nsa_skinny_gemm_q8``, UN = 4 and 8 on both sides of their round sizes, tail columns."""
    for rows in SKINNY_Q8_ROWS:
        for N in SKINNY_Q8_N:
            _plain_exact("skinny_gemm", True, rows, N, K)


# ================================================================ 2. exact pins, prologue kernels
def _row_ln_exact(q8, N, K, emb):
    """Both patterns, with and without lb, with and without branch (the LayerNorm form), with and
    without bias, fp32 and bf16 outputs: y bit for bit, the written s bit for bit (or untouched),
    pos_inc advanced by exactly one."""
    W, scale = _weights(N, K, q8)
    b = int_bias(N).to(DEV)
    for pattern in (0, 1):
        rows_s, sign = exact_ln_rows(EMB_ROWS if emb else 1, K, pattern)
        pick = EMB_POS if emb else 0
        s = rows_s[pick:pick + 1]
        if emb:
            wte, wpe = _dev(*split_tables(rows_s, EMB_TOK))
            tok, pos = torch.tensor([EMB_TOK], device=DEV), torch.tensor([EMB_POS], device=DEV)
        else:
            res, branch = _dev(*split_res_branch(s))
        s = s.to(DEV)
        for with_lb in (True, False):
            lw, lb = exact_ln_params(K, with_lb)
            x = exact_ln_x(sign[pick:pick + 1], lw, lb).to(DEV)
            lw, lb = _dev(lw, lb)
            for i, (bias, f32) in enumerate(((None, 0), (b, 1), (b, 0), (None, 1))):
                ref = linear_ref(x, W, scale, bias)[0]
                for br in ((None,) if emb else (None, branch)):
                    tag = (q8, N, K, emb, pattern, with_lb, bias is not None, f32, br is not None)
                    g, so = _out(1, N, f32), Guarded((K,), F32)
                    if emb:
                        call_emb_ln(q8, tok, pos, wte, wpe, so.view, lw, lb, W, scale, bias, g.view, N, K, 0, f32)
                        assert int(tok) == EMB_TOK and int(pos) == EMB_POS
                    else:
                        r = res if br is not None else s
                        r0 = r.clone()
                        p = torch.tensor([41, 41], device=DEV) if (i + pattern) % 2 or N > 4096 else None
                        call_row_ln(q8, r, br, so.view, lw, lb, W, scale, bias, g.view, N, K, 0, f32, p)
                        assert p is None or p.tolist() == [42, 41], tag
                        assert torch.equal(r, r0), tag
                    _exact(g, ref, f32, tag)
                    if emb or br is not None:
                        assert so.written() and torch.equal(so.view, s.view(K)), tag
                    else:
                        assert so.untouched(), tag


@_by_kind(ROW_LN_K)
@pytest.mark.parametrize("emb", [False, True], ids=["ln", "emb-ln"])
def test_row_prologue_exact(kernels, q8, emb, K):
    """``nsa_gemv_ln`` and ``nsa_gemv_emb_ln`` (tok, pos != 0 in tables whose other rows hold other
    patterns): the vector prologue up to its limit, the scalar loop just past it, the widest row."""
    for N in ROW_LN_N:
        _row_ln_exact(q8, N, K, emb)


@KINDS
@pytest.mark.parametrize("emb", [False, True], ids=["ln", "emb-ln"])
def test_row_prologue_exact_past_the_grid_cap(kernels, q8, emb):
    """N = 4103: more column blocks than the 1024-workgroup cap, so workgroups loop and prefetch a
    second block, the last one a partial tail; pos_inc advances by exactly one."""
    for N, K in ROW_LN_WIDE[q8]:
        _row_ln_exact(q8, N, K, emb)


@KINDS
@pytest.mark.parametrize("ki", range(4))
def test_skinny_ln_exact(kernels, q8, ki):
    """``nsa_skinny_ln_gemm``: every row has its own sign pattern and the rows alternate (c, a), so a
    row normalised by the wrong wave or with another row's statistics changes integers."""
    K = SKINNY_LN_K[q8][ki]
    for N in SKINNY_LN_N[q8]:
        W, scale = _weights(N, K, q8)
        b = int_bias(N).to(DEV)
        for M in SKINNY_LN_ROWS:
            for pattern in (0, 1):
                s, sign = exact_ln_rows(M, K, pattern)
                res, branch = _dev(*split_res_branch(s))
                s = s.to(DEV)
                with_lb = bool((M + pattern) % 2)
                lw, lb = exact_ln_params(K, with_lb)
                x = exact_ln_x(sign, lw, lb).to(DEV)
                lw, lb = _dev(lw, lb)
                for bias, f32 in ((None, 0), (b, 1), (b, 0)):
                    ref = linear_ref(x, W, scale, bias)[0]
                    for br in (None, branch):
                        tag = (q8, N, K, M, pattern, with_lb, bias is not None, f32, br is not None)
                        g, so = _out(M, N, f32), Guarded((M, K), F32)
                        r = res if br is not None else s
                        r0 = r.clone()
                        call_skinny_ln(q8, r, br, so.view, lw, lb, W, scale, bias, g.view, M, N, K, 0, f32)
                        _exact(g, ref, f32, tag)
                        assert torch.equal(r, r0), tag
                        if br is not None:
                            assert so.written() and torch.equal(so.view, s), tag
                        else:
                            assert so.untouched(), tag


def _attn_identity(ns):
    """Hand-made partials through ``nsa_gemv_attn_q8`` with an int8 identity (scale 1): the float64
    combine within one bf16 rounding, and the bf16 kernel's output bit for bit."""
    sets, _ = _handmade(ns)
    n = sets.shape[0]
    K = n * D
    ws = torch.full((n, ns, 4 + D), NAN, device=DEV, dtype=F32)
    ws[..., :2], ws[..., 4:] = sets[..., :2].to(DEV), sets[..., 2:].to(DEV)
    ws0 = ws.clone()
    ys = []
    for q8 in (True, False):
        W = torch.eye(K, device=DEV, dtype=torch.int8 if q8 else BF)
        scale = torch.ones(K, device=DEV) if q8 else None
        g = _out(1, K, 0)
        call_attn(q8, ws, W, scale, None, g.view, K, K)
        torch.cuda.synchronize()
        assert g.written() and torch.equal(ws.view(torch.int32), ws0.view(torch.int32))
        ys.append(g.view)
    ref, mag = combine_ref(ws0.cpu()[..., [0, 1] + list(range(4, 4 + D))])
    _within(ys[0].cpu().view(n, D), ref, _combine_bound(ref, mag, ns), f"n_split {ns}")
    assert torch.equal(ys[0], ys[1])


def test_gemv_attn_q8_identity(kernels):
    _attn_identity(5)


@KINDS
def test_ops_launch_the_pinned_kernels(kernels, monkeypatch, q8):
    """``ops.decode_linear`` and ``ops.decode_linear_ln`` reach these kernels, in one launch each and
    without a fallback to ``linear``, and hand back the same exact integers (recorded as in
    ``test_quant_gpu.py``)."""
    from nanosandbox_amd import ops
    from test_quant_gpu import _record

    for cap, rows in (("GEMV_MAX_ROWS", 1), ("SKINNY_MAX_ROWS", 16), ("SKINNY_LN_MAX_ROWS", 8)):  # the defaults
        monkeypatch.setattr(ops.functional, cap, rows)
    calls = _record(monkeypatch)
    sfx = "_q8" if q8 else ""
    N, K = 48, 1088
    W, scale = _weights(N, K, q8)
    w = ops.QuantWeight(W, scale) if q8 else W
    b = int_bias(N).to(DEV)
    lw, lb = exact_ln_params(K, True)
    for rows, plain, fused in ((1, "nsa_gemv", "nsa_gemv_ln"), (5, "nsa_skinny_gemm", "nsa_skinny_ln_gemm")):
        x = int_x(rows, K).to(DEV)
        del calls[:]
        y = ops.decode_linear(x.view(rows, 1, K), w, b, out_f32=True)
        assert calls == [plain + sfx], calls
        assert torch.equal(y.view(rows, N), linear_ref(x, W, scale, b)[0].float())
        s, sign = exact_ln_rows(rows, K, 1)
        res, branch = _dev(*split_res_branch(s))
        xi = exact_ln_x(sign, lw, lb).to(DEV)
        for br in (branch, None):
            r = res if br is not None else s.to(DEV)
            del calls[:]
            s_new, y = ops.decode_linear_ln(r.view(rows, 1, K), None if br is None else br.view(rows, 1, K),
                                            lw.to(DEV), lb.to(DEV), w, b)
            assert calls == [fused + sfx], calls
            assert torch.equal(s_new.view(rows, K), s.to(DEV))
            assert y.dtype == BF and torch.equal(y.view(rows, N), linear_ref(xi, W, scale, b)[0].to(BF))


# ======================================================================== 3. random, per element
def _ratio(g, ref, bound, tag):
    torch.cuda.synchronize()
    assert g.written(), tag
    ratio = float(((g.view.double() - ref).abs() / bound).max())
    assert ratio <= 1.0, f"{tag}: error / bound {ratio:.4f}"
    return ratio


ACTS = ((0, 0), (0, 1), (1, 0))  # (act, out_f32)


@KINDS
def test_plain_random_per_element(kernels, q8):
    """Random operands, bias / GELU / fp32 output, per element against float64 within
    ``plain_bound``.  Worst error / bound on an MI355X: bf16 weights 0.9522 (bf16 output), 0.0021
    (fp32), 0.9346 (GELU); int8 0.9420, 0.0014, 0.9493."""
    worst = {a: 0.0 for a in ACTS}
    shapes = [("gemv", s) for s in RAND_GEMV[q8]]
    shapes += [("skinny_gemm", s) for s in (RAND_SKINNY_Q8 if q8 else RAND_SKINNY)]
    for kind, (rows, N, K) in shapes:
        x, W, scale, b = _dev(*rand_linear(rows, N, K, q8))
        for bias in (b, None):
            for act, f32 in ACTS:
                ref, mag, u = linear_ref(x, W, scale, bias, act)
                g = _out(rows, N, f32)
                call_plain(kind, q8, x, W, scale, bias, g.view, rows, N, K, act, f32)
                r = _ratio(g, ref, plain_bound(ref, mag, u, act, f32), (kind, q8, rows, N, K, act, f32))
                worst[(act, f32)] = max(worst[(act, f32)], r)
    print(f"plain linears, int8 {q8}: worst error / bound bf16 {worst[(0, 0)]:.4f}, fp32 {worst[(0, 1)]:.4f}, "
          f"GELU {worst[(1, 0)]:.4f}")


def _ln_random(q8, rows, N, K, emb, worst):
    _, W, scale, b = _dev(*rand_linear(rows, N, K, q8))
    for branch in ((False,) if emb else (False, True)):
        res, br, s, lw, lb = rand_ln(rows, K, branch)
        if emb:
            wte, wpe = rand_tables(K)
            s = (wte[EMB_TOK].float() + wpe[EMB_POS].float()).view(1, K)
            wte, wpe = _dev(wte, wpe)
            tok, pos = torch.tensor([EMB_TOK], device=DEV), torch.tensor([EMB_POS], device=DEV)
        res, br, s, lw, lb = _dev(res, br, s, lw, lb)
        for act, f32 in ACTS:
            ref, mag, u = ln_linear_ref(s, lw, lb, W, scale, b, act)
            bound, amb = ln_bound(s, lw, lb, W, scale, ref, mag, u, act, f32)
            assert float(amb.double().mean(-1).max()) < AMBIGUOUS_SHARE
            tag = (q8, rows, N, K, emb, branch, act, f32)
            g, so = _out(rows, N, f32), Guarded((rows, K), F32)
            if emb:
                call_emb_ln(q8, tok, pos, wte, wpe, so.view, lw, lb, W, scale, b, g.view, N, K, act, f32)
            elif rows == 1:
                call_row_ln(q8, res, br, so.view, lw, lb, W, scale, b, g.view, N, K, act, f32)
            else:
                call_skinny_ln(q8, res, br, so.view, lw, lb, W, scale, b, g.view, rows, N, K, act, f32)
            worst[0] = max(worst[0], _ratio(g, ref, bound, tag))
            if emb or branch:
                assert so.written() and torch.equal(so.view, s), tag  # one exact fp32 sum: bit for bit
            else:
                assert so.untouched(), tag


@KINDS
def test_ln_random_per_element(kernels, q8):
    """The prologue kernels on random rows, per element against float64 within ``ln_bound`` (the
    ambiguous elements' share included); s = res + branch and wte[tok] + wpe[pos] bit for bit.
    Worst error / bound on an MI355X: bf16 weights 0.9643, int8 0.9752."""
    worst = [0.0]
    for rows, N, K in RAND_ROW_LN:
        _ln_random(q8, rows, N, K, False, worst)
        _ln_random(q8, rows, N, K, True, worst)
    for rows, N, K in RAND_SKINNY_LN:
        _ln_random(q8, rows, N, K, False, worst)
    print(f"prologue kernels, int8 {q8}: worst error / bound {worst[0]:.4f}")


# ================================================================================== 4. refusals
def _refused(fn, *gs):
    """The call returns hipErrorInvalidValue, launches nothing and leaves every NaN buffer as it was."""
    with pytest.raises(RuntimeError, match=f"hipError {HIP_INVALID_VALUE}$"):
        fn()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in gs)


@KINDS
def test_refusals(kernels, q8):
    """Every guard of the entry points: rows 0 / 9 / 17 / 65, K off its multiple or past its limit, N
    off 16 on the bf16 skinny kernels, GELU into an fp32 output, a branch without s_out, res_out
    aliasing res.  The same arguments with the offending one put right launch."""
    N, K = 16, 64
    buf = lambda *shape, dt=BF: torch.zeros(*shape, device=DEV, dtype=dt)  # noqa: E731
    W = buf(N, 8192 + 64, dt=torch.int8 if q8 else BF)
    scale = torch.ones(N, device=DEV)
    x, res, br = buf(65, 8192 + 64), buf(17, 8192 + 64, dt=F32) + 1.0, buf(17, 8192 + 64)
    res[:, ::2] = -1.0
    lw, lb = buf(8192 + 64) + 1.0, buf(8192 + 64)
    tok, pos = torch.zeros(1, device=DEV, dtype=I64), torch.zeros(1, device=DEV, dtype=I64)
    ws = buf(1, 1, 4 + D, dt=F32)
    ws[..., 1] = 1.0                           # one live chunk: m = 0, l = 1
    kq = 16 if q8 else 8                       # the K granule of the row kernels
    ks = 64 if q8 else 32                      # and of the skinny kernels
    y, so = Guarded((65, 100), F32), Guarded((17, 8192 + 64), F32)

    def plain(kind, rows=2, n=N, k=K, act=0, f32=0):
        return lambda: call_plain(kind, q8, x, W, scale, None, y.view, rows, n, k, act, f32)

    def row_ln(k=K, act=0, f32=0, branch=None, out=so.view):
        return lambda: call_row_ln(q8, res, branch, out, lw, lb, W, scale, None, y.view, N, k, act, f32)

    def emb_ln(k=K, act=0, f32=0, out=so.view):
        return lambda: call_emb_ln(q8, tok, pos, x, x, out, lw, lb, W, scale, None, y.view, N, k, act, f32)

    def skinny_ln(rows=2, n=N, k=K, act=0, f32=0, branch=None, out=so.view):
        return lambda: call_skinny_ln(q8, res, branch, out, lw, lb, W, scale, None, y.view, rows, n, k, act, f32)

    def row_ln_n0():
        return lambda: call_row_ln(q8, res, None, so.view, lw, lb, W, scale, None, y.view, 0, K)

    def emb_ln_n0():
        return lambda: call_emb_ln(q8, tok, pos, x, x, so.view, lw, lb, W, scale, None, y.view, 0, K)

    def attn(k=K, act=0, f32=0, ns=1):
        return lambda: _call(_name("gemv_attn", q8), ws, ns, *_w(W, scale, q8), None, y.view, N, k, act, f32)

    bad = [plain("gemv", rows=0), plain("gemv", rows=9), plain("gemv", k=K + kq // 2), plain("gemv", act=1, f32=1),
           plain("skinny_gemm", rows=0), plain("skinny_gemm", rows=17 if q8 else 65),
           plain("skinny_gemm", k=K + ks // 2), plain("skinny_gemm", act=1, f32=1),
           row_ln(k=K + kq // 2), row_ln(k=8192 + kq), row_ln(act=1, f32=1), row_ln(branch=br, out=None),
           row_ln(branch=br, out=res),
           emb_ln(k=K + kq // 2), emb_ln(k=8192 + kq), emb_ln(act=1, f32=1), emb_ln(out=None),
           skinny_ln(rows=0), skinny_ln(rows=17), skinny_ln(k=K + ks // 2), skinny_ln(k=1920 + ks),
           skinny_ln(act=1, f32=1), skinny_ln(branch=br, out=None),
           attn(k=K + 32), attn(k=8192 + 64), attn(act=1, f32=1), attn(ns=0),
           plain("gemv", n=0), row_ln_n0(), emb_ln_n0()]
    if not q8:
        bad += [plain("skinny_gemm", n=N + 8), skinny_ln(n=N + 8)]
    for fn in bad:
        _refused(fn, y, so)
    good = [plain("gemv"), plain("gemv", rows=8), plain("skinny_gemm", rows=16 if q8 else 64), plain("skinny_gemm"),
            row_ln(), row_ln(k=8192), row_ln(branch=br), emb_ln(), emb_ln(k=8192), skinny_ln(), skinny_ln(rows=16),
            skinny_ln(k=1920), skinny_ln(branch=br), attn()]
    for fn in good:
        fn()
    torch.cuda.synchronize()
    assert not y.untouched()


# ============================================================= 5. the environment-only instantiations
ENV_CONFIGS = [{"NSA_GEMV_NC": "8", "NSA_GEMV1_NC": "8", "NSA_GEMV_GRID": "3"},
               {"NSA_GEMV_NC": "16", "NSA_GEMV1_NC": "4", "NSA_GEMV_GRID": "1"}]


def env_pins():
    """The exact pins the three variables reach, at a handful of shapes: the one-row ``nsa_gemv``
    (NSA_GEMV1_NC), the row kernels with their prologues (NSA_GEMV_NC, bf16 only; NSA_GEMV_GRID, both
    kinds: at N = 100 a workgroup loops over many column blocks) and the attention combine."""
    for q8 in (False, True):
        for N in (9, 100):
            for K in (16, 2064):
                _plain_exact("gemv", q8, 1, N, K)
            for K in (64, 2064):
                _row_ln_exact(q8, N, K, False)
                _row_ln_exact(q8, N, K, True)
    _attn_identity(2)
    _attn_identity(5)


def test_env_only_instantiations(kernels):
    """The column-block instantiations only NSA_GEMV_NC, NSA_GEMV1_NC and NSA_GEMV_GRID select (the
    library reads them once per process): the exact pins in two fresh child processes, one after
    the other."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    here = os.path.dirname(os.path.abspath(__file__))
    for cfg in ENV_CONFIGS:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, here]), **cfg)
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0 and "env pins ok" in p.stdout, (cfg, p.stdout[-2000:], p.stderr[-4000:])


if __name__ == "__main__":
    assert all(os.environ.get(k) for k in ENV_CONFIGS[0]), "run by test_env_only_instantiations"
    from nanosandbox_amd.ops import _lib
    _lib.lib()
    env_pins()
    torch.cuda.synchronize()
    print("env pins ok", {k: os.environ[k] for k in ENV_CONFIGS[0]})
