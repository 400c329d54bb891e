"""High-precision references for the LayerNorm kernels (``layernorm.hip``), as plain functions
that run on any device, with their own CPU checks.

``test_layernorm_gpu.py`` compares the HIP kernels with these element by element.  Every bound
is ``k * 2^-24 * scale``: ``scale`` is the sum of the absolute values of the terms that form the
value (returned by the float64 references), ``k`` the number of fp32 roundings on the longest
path to it (``ln_counts``), each rounding being at most 2^-24 relative (u).  With
``nk = ceil(C / 512)`` register groups per lane:

  k_sum  = 8 nk + 6        a row sum: 8 nk sequential adds in a lane, log2(64) butterfly steps
  k_mean = k_sum + 1       and the division by C                      scale mean|s|
  k_rstd = (k_sum + 5) / 2 + 2
           d = s - mean (1), d * d (2: the square doubles d's error, and its own rounding),
           the sum (k_sum), / C (1), + eps (1) -- halved by the power -1/2 -- and rsqrtf's
           1 ulp = 2 u                                                scale rstd
           The rounded mean also moves the variance by dm^2 (dm <= the mean's bound): a term
           q = rstd - (var + eps + dm^2)^-1/2 is added, which only matters where
           |mean| >> std (the offset rows).
  k_h    = k_mean + 4      the mean's error times rstd |w|; rstd's (k_rstd) and the roundings
           of s - mean, * rstd, * w (3) and + b (1) on the product     scale (mean|s| + |s - mean|) rstd |w| + |b|
           plus |s - mean| |w| q, and for the 16-bit store half an ulp of the output type at the
           reference: 2^(e-8) for bf16 and 2^(e-11) for fp16 where 2^e <= |ref| < 2^(e+1).  For
           fp16 that is at most 2^-11 |ref|; for bf16 it lies between 2^-9 |ref| and 2^-8 |ref|
           (2^-9 of the next power of two): a correctly rounded bf16 value misses 2^-9 |ref|.
  k_dx   = k_sum + 8       dy * w is exact (two 16-bit factors); g - m1 (1), xhat (2),
           xhat * m2 + .. (1), rstd * t + dres (1) on every term; m1 = sum / C (k_sum + 1)
           on mean|g|; m2 (k_sum + 1, and 3 for g * xhat) on |xhat| mean|g xhat|
                                                                      scale rstd (|g| + mean|g| + |xhat| mean|g xhat|) + |dres|
  k_dw   = nw + 6          per partial row: xhat (2), dy * xhat (1), nw = ceil(N / (4 nblk))
           adds in the wave's LDS slice, 3 adds over the four waves    scale sum|dy xhat|
  k_db   = nw + 3          the adds alone (dy is exact)                scale sum|dy|

The CPU test below holds an fp32 numpy emulation of the kernel's order of operations
(``ln_fp32_model``) to half of each bound, for every input pattern and width.  Worst
error / bound the kernels reached on an MI355X (``test_layernorm_gpu.py``, all cases):

  mean 0.226   rstd 0.240   h 0.9993 (the 16-bit store's half ulp, which rounding reaches)
  dx 0.126 (fp32 stream), 0.9993 (bf16 stream: the store's half ulp)
  dw_part 0.459   db_part 0.095   through autograd: dw 0.302, db 0.075
"""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_streaming_refs import F64, f32

F32 = torch.float32
BF = torch.bfloat16
FH = torch.float16
U = 2.0 ** -24

# every width the GPU file runs: the NK boundaries and remaps of NSA_NK_SWITCH, and the
# backward's limit (32 C bytes of LDS <= 160 KiB)
LN_BWD_MAX_C = 5120
WIDTHS = (8, 64, 504, 512, 520, 1032, 1280, 1544, 2056, 3080, 4104, LN_BWD_MAX_C)
PATTERNS = ("normal", "offset", "constant", "outlier", "tiny", "zero", "spread")
CONSTANTS = (2.5, -3.0, 0.75, 96.0)  # few mantissa bits: C of them sum exactly in fp32


# ------------------------------------------------------------------------------ inputs
def ln_rows(N, C, seed, stream_dtype=F32):
    """[N, C] residual-stream input, one pattern per row, cycling through the 7 patterns (coprime
    with the 4 wave slots of a block, so every pattern lands in every slot).  Returns the tensor
    (CPU, ``stream_dtype``) and the list of pattern names per row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(N, C)
    names = []
    for r in range(N):
        p = PATTERNS[r % len(PATTERNS)]
        names.append(p)
        z = torch.randn(C, generator=g)
        if p == "normal":
            x[r] = z
        elif p == "offset":  # |mean| >> std
            x[r] = 1e3 + 1e-2 * z if stream_dtype == F32 else 16 + z
        elif p == "constant":  # var = 0
            x[r] = CONSTANTS[(r // len(PATTERNS)) % len(CONSTANTS)]
        elif p == "outlier":  # one large element in the last 8 columns (the clamped vector)
            x[r] = z
            x[r, C - 8 + r % 8] = 1e4
        elif p == "tiny":  # std << sqrt(eps)
            x[r] = 1e-4 * z
        elif p == "zero":
            x[r] = 0.0
        else:  # spread over decades
            x[r] = z * torch.exp(3 * torch.randn(C, generator=g))
    return x.to(stream_dtype), names


def ln_res(names, C, seed, dtype):
    """The branch tensor of the fused add, scaled per row so that the sum keeps the row's
    pattern: zero on constant and zero rows, 1e-4 on tiny rows, with exact zeros elsewhere."""
    g = torch.Generator().manual_seed(seed)
    scale = {"constant": 0.0, "zero": 0.0, "tiny": 1e-4, "offset": 0.01 if dtype != BF else 1.0}
    res = torch.randn(len(names), C, generator=g)
    res *= torch.tensor([scale.get(p, 1.0) for p in names])[:, None]
    res[:, C // 2] = 0.0
    return res.abs().to(dtype) * torch.sign(res).to(dtype)  # no negative zeros


def ln_params(C, seed, dtype, bias=True):
    """w about 1 with negative values and exact zeros, b about 0.1 with exact zeros."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, generator=g) * 0.5 + 1
    b = torch.randn(C, generator=g) * 0.1
    w[1::5] *= -1
    w[3::11] = 0.0
    b[2::7] = 0.0
    w[C - 1], w[C - 8] = -1.25, 0.75  # the last vector is never all zero
    return w.to(dtype), (b.to(dtype) if bias else None)


def ln_dy(N, C, seed, dtype):
    """Output gradient: rows cycle through random, all positive (no cancellation in the row
    means), alternating signs, exactly zero, and random with exact zeros (5 patterns: coprime
    with the wave slots and the 7 input patterns)."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(N, C, generator=g)
    for r in range(N):
        k = r % 5
        if k == 1:
            dy[r] = dy[r].abs()
        elif k == 2:
            dy[r] = dy[r].abs() * (1 - 2 * (torch.arange(C) % 2))
        elif k == 3:
            dy[r] = 0.0
        elif k == 4:
            dy[r, ::3] = 0.0
    return dy.to(dtype)


def ln_dres(N, C, seed, dtype):
    """Gradient arriving through the residual stream: about 0.1, exact (positive) zeros."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(N, C, generator=g) * 0.1
    d[:, 1::9] = 0.0
    return d.to(dtype)


# -------------------------------------------------------------------------- references
def ln_counts(C, N=1, nblk=1):
    nk = -(-C // 512)
    k_sum = 8 * nk + 6
    nw = -(-N // (4 * nblk))
    return SimpleNamespace(nk=nk, sum=k_sum, mean=k_sum + 1, rstd=(k_sum + 5) / 2 + 2, h=k_sum + 5, dx=k_sum + 8,
                           dw=nw + 6, db=nw + 3)


def half_ulp(ref, dtype):
    """Half the spacing of ``dtype`` at |ref| (float64): the rounding of a 16-bit store.  Zero for
    fp32.  Below the smallest normal: the fp16 subnormal spacing; bf16 may be flushed to zero."""
    if dtype == F32:
        return torch.zeros_like(ref)
    bits, emin = (8, -126) if dtype == BF else (11, -14)
    _, e = torch.frexp(ref.abs())  # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, emin, e - 1).clamp(min=emin)
    hu = torch.exp2(e.to(F64) - bits)
    return hu + (2.0 ** -126 if dtype == BF else 0.0)


def ln_fwd_ref(x, res, w, b, eps, stream_dtype):
    """LayerNorm forward in float64 from the exact input bits.  The fused sum is rounded as the
    kernel rounds it (an fp32 add, then the stream dtype), and the statistics are those of the
    rounded sum.  Returns s (stream dtype), mean, var, rstd, h (float64) and the error scales
    e_mean = mean|s|, e_h = (mean|s| + |s - mean|) rstd |w| + |b|; d = s - mean, aw = |w|."""
    assert x.dtype == stream_dtype
    s = x if res is None else (x.float() + res.float()).to(stream_dtype)
    sd = s.to(F64)
    mean = sd.mean(-1)
    d = sd - mean[:, None]
    var = (d * d).mean(-1)
    epsf = f32(eps)
    rstd = (var + epsf) ** -0.5
    wd = w.to(F64)
    bd = b.to(F64) if b is not None else torch.zeros_like(wd)
    h = d * rstd[:, None] * wd + bd
    e_mean = sd.abs().mean(-1)
    e_h = (e_mean[:, None] + d.abs()) * rstd[:, None] * wd.abs() + bd.abs()
    return SimpleNamespace(s=s, mean=mean, var=var, rstd=rstd, h=h, e_mean=e_mean, e_h=e_h, d=d, aw=wd.abs(),
                           eps=epsf, C=x.shape[-1])


def ln_fwd_bounds(r, out_dtype):
    """(mean, rstd, h) bounds of a forward reference (module docstring)."""
    k = ln_counts(r.C)
    b_mean = k.mean * U * r.e_mean
    q = r.rstd - (r.var + r.eps + b_mean * b_mean) ** -0.5
    b_rstd = k.rstd * U * r.rstd + q
    b_h = k.h * U * r.e_h + r.d.abs() * r.aw * q[:, None]
    return b_mean, b_rstd, b_h + half_ulp(r.h, out_dtype)


def ln_owner(N, nblk):
    """Block that accumulates row r: waves of block b take rows 4 b + wave + 4 nblk i."""
    return (torch.arange(N) // 4) % nblk


def ln_bwd_ref(dy, x, w, mean, rstd, dres, nblk=1):
    """LayerNorm backward in float64 from the exact input bits and the fp32 statistics it is
    given (the forward's saved ones).  Returns dx, the dw / db partial row of every block (block
    b owns the rows with (r // 4) % nblk == b) and the error scales of all three."""
    N, C = x.shape
    dyd, xd, wd = dy.to(F64), x.to(F64), w.to(F64)
    r = rstd.to(F64)[:, None]
    xh = (xd - mean.to(F64)[:, None]) * r
    g = dyd * wd
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    dr = dres.to(F64) if dres is not None else torch.zeros_like(xd)
    dx = r * (g - m1 - xh * m2) + dr
    e_dx = r * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)) + dr.abs()
    own = ln_owner(N, nblk).to(x.device)
    z = lambda: torch.zeros(nblk, C, dtype=F64, device=x.device)  # noqa: E731
    dw = z().index_add_(0, own, dyd * xh)
    e_dw = z().index_add_(0, own, (dyd * xh).abs())
    db = z().index_add_(0, own, dyd)
    e_db = z().index_add_(0, own, dyd.abs())
    return SimpleNamespace(dx=dx, e_dx=e_dx, dw=dw, e_dw=e_dw, db=db, e_db=e_db, N=N, C=C, nblk=nblk)


def ln_bwd_bounds(r, stream_dtype):
    """(dx, dw_part, db_part) bounds of a backward reference (module docstring); 2^-126 for a
    flushed fp32 denormal."""
    k = ln_counts(r.C, r.N, r.nblk)
    b_dx = k.dx * U * r.e_dx + half_ulp(r.dx, stream_dtype) + 2.0 ** -126
    return b_dx, k.dw * U * r.e_dw + 2.0 ** -126, k.db * U * r.e_db


# ------------------------------------------------------- fp32 model of the kernel's order
def _lanes(a, C):
    """[N, C] fp32 -> [N, nk, 64, 8] in the kernel's layout (lane l of group k holds columns
    (64 k + l) 8 .. + 8), zero padded, and the validity mask of the padded layout."""
    nk = -(-C // 512)
    p = np.zeros((a.shape[0], nk * 512), np.float32)
    p[:, :C] = a
    valid = np.zeros(nk * 512, bool)
    valid[:C] = True
    return p.reshape(-1, nk, 64, 8), valid.reshape(nk, 64, 8)


def _lane_sum(t):
    """Per-lane sequential fp32 sum over the lane's groups and their 8 elements."""
    s = np.zeros((t.shape[0], 64), np.float32)
    for k in range(t.shape[1]):
        for j in range(8):
            s = s + t[:, k, :, j]
    return s


def _wave_sum(p):
    """common.h ``wave_sum``: xor butterfly over the 64 lanes, fp32."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ o]
    return p[:, 0]


def _fma(a, b, c):
    """fp32 fused multiply-add through float64 (the product is exact there)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ln_fp32_model(x, res, w, b, eps, stream_dtype, out_dtype, dy=None, dres=None, nblk=1):
    """numpy fp32 emulation of ``ln_fwd_kernel`` and, with ``dy``, ``ln_bwd_kernel`` in the
    kernels' order of operations: lane partial sums, the butterfly, the division by C, 1 / sqrt,
    the backward's fused multiply-adds, the waves' LDS accumulators over their rows and the sum
    over the four waves.  Not bit-exact with the GPU (rsqrtf, FMA contraction of the sums)."""
    N, C = x.shape
    one, Cf = np.float32(1), np.float32(C)
    s = x if res is None else (x.float() + res.float()).to(stream_dtype)
    v, valid = _lanes(s.float().numpy(), C)
    wl, _ = _lanes(w.float().numpy()[None], C)
    bl, _ = _lanes((b.float().numpy() if b is not None else np.zeros(C, np.float32))[None], C)
    mean = _wave_sum(_lane_sum(v)) / Cf
    d = np.where(valid, v - mean[:, None, None, None], np.float32(0))
    rstd = one / np.sqrt(_wave_sum(_lane_sum(d * d)) / Cf + np.float32(eps))
    h = (v - mean[:, None, None, None]) * rstd[:, None, None, None] * wl + bl
    unl = lambda t: torch.from_numpy(np.ascontiguousarray(t.reshape(t.shape[0], -1)[:, :C]))  # noqa: E731
    out = SimpleNamespace(s=s, mean=torch.from_numpy(mean), rstd=torch.from_numpy(rstd), h=unl(h).to(out_dtype))
    if dy is None:
        return out
    dv, _ = _lanes(dy.float().numpy(), C)
    rv, _ = _lanes(dres.float().numpy() if dres is not None else np.zeros((N, C), np.float32), C)
    xh = (v - mean[:, None, None, None]) * rstd[:, None, None, None]
    g = dv * wl
    m1 = _wave_sum(_lane_sum(np.where(valid, g, np.float32(0)))) / Cf
    m2 = _wave_sum(_lane_sum(np.where(valid, g * xh, np.float32(0)))) / Cf
    t = _fma(-xh, np.broadcast_to(m2[:, None, None, None], xh.shape), _fma(dv, np.broadcast_to(wl, dv.shape),
                                                                         np.broadcast_to(-m1[:, None, None, None], dv.shape)))
    o = _fma(np.broadcast_to(rstd[:, None, None, None], t.shape), t, rv)
    out.dx = unl(o).to(stream_dtype)
    accw = np.zeros((nblk, 4) + v.shape[1:], np.float32)
    accb = np.zeros_like(accw)
    for r in range(N):  # rows reach a wave's accumulator in increasing order
        blk, wv = (r // 4) % nblk, r % 4
        accw[blk, wv] = accw[blk, wv] + dv[r] * xh[r]
        accb[blk, wv] = accb[blk, wv] + dv[r]
    red = lambda a: unl(((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3])  # noqa: E731
    out.dw, out.db = red(accw), red(accb)
    return out


def worst(err, bound):
    """Largest err / bound over the elements (inf where a zero bound is missed)."""
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    return r.max().item() if r.numel() else 0.0


# ===================================================================== CPU checks of the above
def test_rows_cover_every_pattern_in_every_wave_slot():
    x, names = ln_rows(28, 64, seed=1)
    assert {(p, r % 4) for r, p in enumerate(names)} == {(p, s) for p in PATTERNS for s in range(4)}
    for r, p in enumerate(names):
        row = x[r].double()
        if p == "constant":
            assert row.var(unbiased=False).item() == 0.0 and row[0].item() in CONSTANTS
        elif p == "zero":
            assert not row.any()
        elif p == "offset":
            assert abs(row.mean().item()) > 1e4 * row.std().item()
        elif p == "outlier":
            assert row[-8:].max().item() == 1e4 and row[:-8].abs().max().item() < 10
        elif p == "tiny":
            assert row.std().item() < 0.1 * math.sqrt(1e-5)
    xb, _ = ln_rows(28, 64, seed=1, stream_dtype=BF)
    assert xb.dtype == BF and xb[2].float().var().item() == 0.0
    dy = ln_dy(20, 64, seed=2, dtype=BF).float()
    assert not dy[3].any() and (dy[1] >= 0).all() and (dy[2, ::2] >= 0).all() and (dy[2, 1::2] <= 0).all()
    assert {(r % 5 == 3, r % 4) for r in range(20)} >= {(True, s) for s in range(4)}
    w, b = ln_params(64, seed=3, dtype=BF)
    assert (w == 0).any() and (w < 0).any() and (b == 0).any() and w[-8:].any()
    res = ln_res(PATTERNS, 64, seed=4, dtype=BF)
    assert not res[2].any() and not res[5].any() and res[4].abs().max() < 1e-3
    assert not (res.view(torch.int16) == -32768).any()  # no -0


def test_refs_match_torch_float64_layer_norm_and_autograd():
    torch.manual_seed(5)
    for C in (8, 520, 1280):
        N = 9
        x = (torch.randn(N, C) * 2 + 0.5)
        w, b = ln_params(C, seed=6, dtype=BF)
        dy = ln_dy(N, C, seed=7, dtype=BF)
        dres = ln_dres(N, C, seed=8, dtype=F32)
        xq = x.double().requires_grad_(True)
        wq, bq = w.double().requires_grad_(True), b.double().requires_grad_(True)
        hq = torch.nn.functional.layer_norm(xq, (C,), wq, bq, f32(1e-5))
        hq.backward(dy.double())
        r = ln_fwd_ref(x, None, w, b, 1e-5, F32)
        assert torch.allclose(r.h, hq.detach(), rtol=1e-12, atol=1e-13)
        assert torch.equal(r.s, x) and (r.e_h >= r.h.abs() * (1 - 1e-12)).all()
        for nblk in (1, 2, 5):
            g = ln_bwd_ref(dy, x, w, r.mean, r.rstd, dres, nblk)
            assert torch.allclose(g.dx, xq.grad + dres.double(), rtol=1e-10, atol=1e-12)
            assert torch.allclose(g.dw.sum(0), wq.grad, rtol=1e-10, atol=1e-12)
            assert torch.allclose(g.db.sum(0), bq.grad, rtol=1e-10, atol=1e-12)
            assert (g.e_dx >= g.dx.abs() * (1 - 1e-12)).all() and (g.e_dw >= g.dw.abs()).all()
        # the fused sum: an fp32 add, then the stream's rounding; statistics of the rounded sum
        res = torch.randn(N, C).to(BF)
        rs = ln_fwd_ref(x.to(BF), res, w, b, 1e-5, BF)
        assert rs.s.dtype == BF and torch.equal(rs.s, (x.to(BF).float() + res.float()).to(BF))
        assert torch.equal(rs.mean, rs.s.double().mean(-1))
        # no bias: h of a zero-mean unit row is xhat * w
        r0 = ln_fwd_ref(x, None, w, None, 1e-5, F32)
        assert torch.allclose(r0.h, r.h - b.double(), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("N,nblk", [(1, 1), (3, 1), (5, 16), (37, 1), (37, 16), (130, 3), (37, 2), (300, 16)])
def test_block_ownership_against_the_kernel_loop(N, nblk):
    """(r // 4) % nblk against the kernel's loop: wave wv of block b starts at row 4 b + wv and
    strides by 4 nblk."""
    own = [-1] * N
    for b in range(nblk):
        for wv in range(4):
            row = b * 4 + wv
            while row < N:
                assert own[row] == -1
                own[row] = b
                row += nblk * 4
    assert own == ln_owner(N, nblk).tolist()
    nw = ln_counts(8, N, nblk).dw - 6  # rows per wave that k_dw counts
    assert max(own.count(b) for b in range(nblk)) <= 4 * nw


def test_half_ulp():
    v = torch.tensor([1.0, 1.999, 2.0, 3.0, 2.0 ** -20, 0.0], dtype=F64)
    assert torch.equal(half_ulp(v, F32), torch.zeros(6, dtype=F64))
    hb = half_ulp(v, BF) - 2.0 ** -126
    assert hb[:4].tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7] and hb[4].item() == 2.0 ** -28
    hh = half_ulp(v, FH)
    assert hh[:4].tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10] and hh[4].item() == 2.0 ** -25
    assert hh[5].item() == 2.0 ** -25
    # a correctly rounded value stays within it, and reaches more than 2^-9 |v| for bf16
    x = (torch.randn(1 << 16) * 3).double()  # fp32 values: one rounding to the 16-bit type
    for dt in (BF, FH):
        err = (x.to(dt).double() - x).abs()
        assert (err <= half_ulp(x, dt)).all()
    assert ((x.to(BF).double() - x).abs() > 2.0 ** -9 * x.abs()).any()


@pytest.mark.parametrize("stream,out", [(F32, BF), (F32, FH), (BF, BF)], ids=["x32", "x32_h", "bf16"])
@pytest.mark.parametrize("C", WIDTHS)
def test_fp32_model_within_half_of_every_bound(C, stream, out):
    """The fp32 emulation of the kernel's order of operations against the float64 references,
    every input pattern in every wave slot at every width: within half of each bound (the fp32
    part: the half ulp of a 16-bit store is the store's own and is left whole)."""
    N, nblk = 28, 2
    x, names = ln_rows(N, C, seed=C, stream_dtype=stream)
    w, b = ln_params(C, seed=C + 1, dtype=out)
    dy = ln_dy(N, C, seed=C + 2, dtype=out)
    dres = ln_dres(N, C, seed=C + 3, dtype=stream)
    for res in (None, ln_res(names, C, seed=C + 4, dtype=out)):
        m = ln_fp32_model(x, res, w, b, 1e-5, stream, out, dy, dres, nblk)
        r = ln_fwd_ref(x, res, w, b, 1e-5, stream)
        assert torch.equal(m.s.view(torch.int16 if stream == BF else torch.int32),
                           r.s.view(torch.int16 if stream == BF else torch.int32))
        b_mean, b_rstd, b_h = ln_fwd_bounds(r, out)
        hu = half_ulp(r.h, out)
        assert worst((m.mean.double() - r.mean).abs(), b_mean) <= 0.5
        assert worst((m.rstd.double() - r.rstd).abs(), b_rstd) <= 0.5
        assert worst((m.h.double() - r.h).abs(), (b_h - hu) * 0.5 + hu) <= 1.0
        g = ln_bwd_ref(dy, r.s, w, m.mean, m.rstd, dres, nblk)
        b_dx, b_dw, b_db = ln_bwd_bounds(g, stream)
        hu = half_ulp(g.dx, stream)
        assert worst((m.dx.double() - g.dx).abs(), (b_dx - hu) * 0.5 + hu) <= 1.0
        assert worst((m.dw.double() - g.dw).abs(), b_dw) <= 0.5
        assert worst((m.db.double() - g.db).abs(), b_db) <= 0.5
        # the exact cases the GPU file asserts hold in the model
        for i, p in enumerate(names):
            if p == "constant":
                assert m.mean[i].item() == x[i, 0].item() and torch.equal(m.h[i].float(), b.float())
            if i % 5 == 3:
                assert torch.equal(m.dx[i].float(), dres[i].float())
