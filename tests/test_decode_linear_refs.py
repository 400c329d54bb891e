"""Float64 references and input builders for the weight-streaming decode linears (``nsa_gemv``,
``nsa_gemv_ln``, ``nsa_gemv_emb_ln``, ``nsa_gemv_attn``, ``nsa_skinny_gemm``, ``nsa_skinny_ln_gemm``
and their ``_q8`` forms), as plain functions that run on any device, with their own CPU checks.
``test_decode_linear_gpu.py`` holds the HIP kernels to them bit for bit and per element.

Two devices leave the kernels nothing to round, so the outputs are compared bit for bit:

  integer operands   x in [-4, 4], bf16 weights in [-8, 8] or any int8 weight (+-127 forced at
             k = 0 and k = K - 1 of every row), a power-of-two scale 2^-3 .. 2^2 that differs by row
             and a bias in eighths.  sum_k |x| |W| < 2^24 on every input, so every partial sum in
             any order, on the VALU or the MFMA, is an exact fp32 integer; the scale is exact and
             the bias costs no bit.  The fp32 output is the float64 result and the bf16 output its
             one rounding.
  exact LayerNorm    the row is s = c +- a with exactly K/2 of each sign, (c, a) in {(0, 1), (3, 2)},
             placed at random and differently for every row.  The sum is exact, the mean exactly
             c, the variance exactly a^2 and rstd = rsqrt(a^2 + 1e-5) within 2^-17 of 1 / a.  With
             lw in +-{1, 2, 4} and lb in {-16, -8, 0, 8, 16} the value (s - mean) rstd lw + lb is
             within 2^-15 of the integer +-lw + lb, |lb| != |lw| keeps it from 0, and its bf16
             rounding is that integer (|x| <= 20) whatever the reduction order or the rsqrt.
             ``test_exact_ln_premise`` replays the prologue in fp32 under three summation orders
             with rstd off by +-2^-10.  For the branch form s splits into an fp32 ``res`` in
             half-integers plus a bf16 ``branch``, for the embedding form into wte[tok] + wpe[pos]:
             both sums are exact, so the written s is compared bit for bit too.

Bounds of the random-valued tests (the distributions of ``test_decode_gpu.py``):

  plain      |y - ref| <= rel |ref| + 2^-16 (|x| |W|^T scale + |b|), rel = 2^-8 for a bf16 and
             2^-20 for an fp32 output: ``test_gemm_gpu.check``'s form and figures.
  GELU       ``gelu_bounds`` of ``test_streaming_refs.py`` on the float64 pre-activation u (one
             output rounding and the erf term) plus max |gelu'| = 1.13 times the fp32 bound of u.
  LayerNorm  the reference is act(bf16(h64) W^T scale + b) with h64 the float64 LayerNorm of the fp32
             row s.  An fp32 LayerNorm may round an element to the neighbouring bf16: element k is
             ambiguous when h64[k] lies within TAU m[k] of a bf16 rounding boundary,
             m = (|s| + |mean|) rstd |lw| + |lb|, and the bound gains sum over the ambiguous k of
             |W[n, k]| ulp_bf16(h[k]) scale[n] (1.13 times that under GELU).
             TAU = 2^-18 covers four times the worst |h32 - h64| / m of the fp32 replica over the
             inputs of the GPU file and the three summation orders, 8.02e-7 = 2^-20.25 (the
             sequential sum of the widest rows; the pairwise and per-lane orders stay under
             2.4e-7).  ``test_tau_and_ambiguous_share`` asserts it and holds the ambiguous share of
             every row under 1 % of K (worst row 0.87 %); where a shape's first seed missed either
             condition its rows were drawn again (``RAND_LN_RESEED``).
``test_fp32_replica_within_bounds`` runs an fp32 replica that sums in the kernels' order (a strided
fmaf chain per lane, a butterfly over the wave, then the four waves) on the very inputs of the GPU
file; its worst error / bound: plain fp32 0.0018, bf16 0.9144 and GELU 0.9493 (the output's own
rounding, whose half-ulp is the 2^-8 |ref| term), LayerNorm 0.9527.  On an MI355X the kernels
measure: plain bf16 0.9522 / int8 0.9420, fp32 0.0021 / 0.0014, GELU 0.9346 / 0.9493, the prologue
kernels 0.9643 / 0.9752 (the docstrings of ``test_decode_linear_gpu.py``).
"""

import functools

import numpy as np
import pytest
import torch

from test_decode_attn_refs import combine_ref
from test_streaming_refs import gelu_bounds

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
EPS = 1e-5
REL_BF16 = 2.0 ** -8     # test_gemm_gpu.check: a bf16 output
REL_F32 = 2.0 ** -20     # an fp32 output
K_ABS = 2.0 ** -16       # the share of |x| |W|^T + |b|
GELU_SLOPE = 1.13        # max |gelu'|
TAU = 2.0 ** -18         # the ambiguity band of a LayerNorm output, relative to m (docstring)
AMBIGUOUS_SHARE = 0.01
PATTERNS = [(0, 1), (3, 2)]

# ---------------------------------------------------------------- the cases of the GPU file
GEMV_ROWS = [1, 2, 3, 4, 5, 6, 7, 8]
GEMV_K = {False: [8, 16, 520, 2048, 2056, 2064, 3072], True: [16, 528, 2048, 2064, 3072]}
GEMV_N = [1, 7, 9, 100]
GEMV_WIDE = (4103, 64)                                   # an odd N past 4096 columns, K = 64
GEMV1_Q8_K = [1024, 1040, 2048, 2064, 4096, 4112, 8192, 8208]   # the q8_cfg classes, their edges, the K loop
SKINNY_ROWS = [2, 15, 16, 17, 31, 32, 33, 63, 64]
SKINNY_K = [32, 96, 1024, 1056, 3072]
SKINNY_N = [16, 48, 784]
SKINNY_Q8_ROWS = [2, 3, 8, 15, 16]
SKINNY_Q8_K = [64, 448, 1024, 1088, 2048, 2112]
SKINNY_Q8_N = [16, 100, 33]
ROW_LN_K = {False: [8, 64, 768, 2048, 2056, 8192], True: [16, 64, 768, 2048, 2064, 8192]}
ROW_LN_N = [9, 100]
ROW_LN_WIDE = {False: [(4103, 64)], True: [(4103, 64), (4103, 8192)]}   # past the 1024-workgroup grid cap
SKINNY_LN_ROWS = [2, 3, 4, 5, 8, 9, 15, 16]
SKINNY_LN_K = {False: [32, 96, 1056, 1920], True: [64, 128, 1088, 1920]}
SKINNY_LN_N = {False: [16, 48], True: [16, 48, 100]}
EMB_ROWS, EMB_TOK, EMB_POS = 5, 3, 2                     # table rows, and the row each index picks
# random-valued: (rows, N, K)
RAND_GEMV = {False: [(1, 100, 2056), (3, 9, 768), (8, 100, 3072)],
             True: [(1, 100, 2064), (1, 9, 8208), (3, 9, 768), (8, 100, 3072)]}
RAND_SKINNY = [(2, 48, 1056), (17, 16, 96), (64, 784, 1024)]
RAND_SKINNY_Q8 = [(2, 33, 1088), (15, 100, 448), (16, 784, 2112)]
RAND_ROW_LN = [(1, 100, 768), (1, 9, 2064), (1, 4103, 64), (1, 100, 8192)]
RAND_SKINNY_LN = [(2, 48, 1088), (9, 16, 128), (16, 48, 576)]
# (rows, K, branch) -> seed of the random LayerNorm rows (rows = 0: the embedding tables) where seed 0
# misses test_tau_and_ambiguous_share
RAND_LN_RESEED = {(1, 64, False): 1, (1, 8192, False): 1, (1, 8192, True): 3, (2, 1088, True): 1, (9, 128, False): 2,
                  (16, 576, False): 6, (16, 576, True): 6}


def _gen(*key):
    seed = 20261
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------- the integer operands
def int_x(rows, K, seed=0):
    return torch.randint(-4, 5, (rows, K), generator=_gen(1, rows, K, seed)).to(BF)


@functools.lru_cache(maxsize=4)
def int_weight(N, K, q8):
    """-> (W, scale): bf16 integers in [-8, 8] and None, or int8 with +-127 at both ends of every
    row and the scales 2^(n % 6 - 3)."""
    g = _gen(2, N, K, q8)
    if not q8:
        return torch.randint(-8, 9, (N, K), generator=g).to(BF), None
    q = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
    q[:, 0], q[:, K - 1] = 127, -127
    return q, torch.pow(2.0, (torch.arange(N) % 6 - 3).float())


def int_bias(N):
    return (torch.randint(-16, 17, (N,), generator=_gen(3, N)).float() / 8).to(BF)


def exact_ln_rows(M, K, pattern, seed=0):
    """-> (s [M, K] fp32, sign [M, K] in +-1): row m is c +- a of PATTERNS[(pattern + m) % 2], K/2 of
    each sign in an order of its own."""
    g = _gen(4, M, K, pattern, seed)
    sign = torch.ones(M, K)
    s = torch.empty(M, K)
    for m in range(M):
        sign[m, torch.randperm(K, generator=g)[:K // 2]] = -1.0
        c, a = PATTERNS[(pattern + m) % 2]
        s[m] = c + a * sign[m]
    return s, sign


def exact_ln_params(K, with_lb):
    g = _gen(5, K)
    lw = (2.0 ** torch.randint(0, 3, (K,), generator=g)) * (2.0 * torch.randint(0, 2, (K,), generator=g) - 1)
    lb = 8.0 * torch.randint(-2, 3, (K,), generator=g)
    return lw.to(BF), (lb.to(BF) if with_lb else None)


def exact_ln_x(sign, lw, lb):
    """The integer row the prologue must hand the linear: +-lw + lb."""
    x = sign.double() * lw.double() + (lb.double() if lb is not None else 0.0)
    assert bool((x != 0).all()) and float(x.abs().max()) <= 20
    return x


def split_res_branch(s, seed=0):
    """s = res + branch exactly: branch bf16 half-integers in [-3.5, 3.5], res fp32 half-integers."""
    g = _gen(6, s.shape[0], s.shape[1], seed)
    branch = (torch.randint(-4, 4, s.shape, generator=g).float() + 0.5).to(BF)
    res = s - branch.float()
    assert torch.equal(res + branch.float(), s)
    return res, branch


def split_tables(rows_s, tok):
    """rows_s [R, K]: valid rows.  -> (wte, wpe) bf16 [R, K] with wte[tok] + wpe[p] == rows_s[p] for
    every p; the other wte rows differ from wte[tok] in every element."""
    R, K = rows_s.shape
    g = _gen(7, R, K, tok)
    base = torch.randint(-4, 4, (K,), generator=g).float() + 0.5
    step = torch.randint(1, 3, (R, K), generator=g).float() * (2.0 * torch.randint(0, 2, (R, K), generator=g) - 1)
    wte = base + step  # half-integers in [-5.5, 5.5]
    wte[tok] = base
    wpe = rows_s - wte[tok]
    assert torch.equal(wte.to(BF).float(), wte) and torch.equal(wpe.to(BF).float(), wpe)
    return wte.to(BF), wpe.to(BF)


# ---------------------------------------------------------------------------- the references
def gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / 2.0 ** 0.5))


def linear_ref(x, W, scale=None, bias=None, act=False):
    """act((x W^T) scale + b) in float64 -> (y, absab = |x| |W|^T scale + |b|, u = the pre-activation)"""
    x, W = x.to(F64), W.to(F64)
    u, mag = x @ W.t(), x.abs() @ W.abs().t()
    if scale is not None:
        u, mag = u * scale.to(F64), mag * scale.to(F64)
    if bias is not None:
        u, mag = u + bias.to(F64), mag + bias.to(F64).abs()
    return (gelu64(u) if act else u), mag, u


def ln_ref(s, lw, lb, eps=EPS):
    """Float64 LayerNorm of the rows s -> (h, m = (|s| + |mean|) rstd |lw| + |lb|)"""
    s, lw = s.to(F64), lw.to(F64)
    mean = s.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((s - mean) ** 2).mean(-1, keepdim=True) + eps)
    lbd = lb.to(F64) if lb is not None else torch.zeros_like(lw)
    return (s - mean) * rstd * lw + lbd, (s.abs() + mean.abs()) * rstd * lw.abs() + lbd.abs()


def ln_linear_ref(s, lw, lb, W, scale=None, bias=None, act=False):
    """nsa_gemv_ln / nsa_skinny_ln_gemm on the row(s) s = res + branch: x = bf16(LN(s))"""
    h, _ = ln_ref(s, lw, lb)
    return linear_ref(h.to(BF), W, scale, bias, act)


def emb_ln_linear_ref(tok, pos, wte, wpe, lw, lb, W, scale=None, bias=None, act=False):
    """nsa_gemv_emb_ln -> (s, (y, absab, u))"""
    s = (wte[tok].to(F64) + wpe[pos].to(F64)).view(1, -1)
    return s, ln_linear_ref(s, lw, lb, W, scale, bias, act)


def attn_linear_ref(parts, W, scale=None, bias=None):
    """nsa_gemv_attn on the partials [H, n_split, 66]: x = bf16(combine)"""
    x, _ = combine_ref(parts)
    return linear_ref(x.reshape(1, -1).to(BF), W, scale, bias)


def ulp_bf16(h):
    """The bf16 spacing at |h| (float64), taken on the side of the larger neighbour."""
    a = h.abs() * (1 + 2.0 ** -8) + 2.0 ** -126
    return 2.0 ** (torch.floor(torch.log2(a)) - 7)


def ambiguous(h, m, tau=TAU):
    """bool mask: h lies within tau m of a boundary between two bf16 values."""
    a = h.abs()
    lo = a.to(BF)                                            # the nearest bf16, and its two neighbours
    up = (lo.view(torch.int16) + 1).view(BF).double()
    dn = (lo.view(torch.int16) - 1).clamp(min=0).view(BF).double()
    lo = lo.double()
    d = torch.minimum(((lo + up) / 2 - a).abs(), ((lo + dn) / 2 - a).abs())
    return d <= tau * m


def plain_bound(ref, absab, u, act, f32):
    """The per-element bound of a linear's output (docstring): plain, or composed with GELU."""
    if not act:
        return (REL_F32 if f32 else REL_BF16) * ref.abs() + K_ABS * absab + 1e-30
    pre = REL_F32 * u.abs() + K_ABS * absab
    return gelu_bounds(u, torch.ones_like(u), ref, torch.zeros_like(u), BF)[0] + GELU_SLOPE * pre


def ln_bound(s, lw, lb, W, scale, ref, absab, u, act, f32):
    """plain_bound plus the ambiguous elements' share -> (bound, ambiguous mask [M, K])"""
    h, m = ln_ref(s, lw, lb)
    amb = ambiguous(h, m)
    extra = (amb.double() * ulp_bf16(h)) @ W.to(F64).abs().t()
    if scale is not None:
        extra = extra * scale.to(F64)
    return plain_bound(ref, absab, u, act, f32) + (GELU_SLOPE if act else 1.0) * extra, amb


# ------------------------------------------------------------------------ the random inputs
def rand_linear(rows, N, K, q8, bias=True):
    """x ~ N(0, 1) bf16, W ~ 0.05 N(0, 1) (bf16, or quantized per row as ops.quantize_rows_int8:
    scale = absmax / 127, q = rint(w / scale)), b ~ 0.1 N(0, 1) bf16 -> (x, W, scale, b)"""
    g = _gen(8, rows, N, K, q8)
    x = torch.randn(rows, K, generator=g).to(BF)
    w = torch.randn(N, K, generator=g) * 0.05
    b = (torch.randn(N, generator=g) * 0.1).to(BF) if bias else None
    if not q8:
        return x, w.to(BF), None, b
    scale = w.abs().amax(1) / 127.0
    return x, torch.round(w / scale[:, None]).clamp(-127, 127).to(torch.int8), scale, b


def rand_ln(rows, K, branch):
    """res ~ 3 N(0, 1) + 0.5 fp32, branch ~ N(0, 1) bf16, lw ~ 1 + 0.1 N, lb ~ 0.1 N (bf16)
    -> (res, branch or None, s = res + branch in fp32, lw, lb)"""
    g = _gen(9, rows, K, branch, RAND_LN_RESEED.get((rows, K, bool(branch)), 0))
    res = torch.randn(rows, K, generator=g) * 3 + 0.5
    br = torch.randn(rows, K, generator=g).to(BF) if branch else None
    lw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
    lb = (0.1 * torch.randn(K, generator=g)).to(BF)
    return res, br, (res + br.float() if branch else res), lw, lb


def rand_tables(K):
    g = _gen(10, K, RAND_LN_RESEED.get((0, K, False), 0))
    return (torch.randn(EMB_ROWS, K, generator=g) * 0.5).to(BF), (torch.randn(EMB_ROWS, K, generator=g) * 0.5).to(BF)


# ------------------------------------------------------------------------- the fp32 replicas
def _sum32(v, order):
    """fp32 sum of the last axis of a numpy float32 array in one of three orders."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if order == "sequential":
        return np.cumsum(v, axis=-1, dtype=np.float32)[..., -1]
    if order == "lanes":  # 8 per lane in sequence, then a tree across the lanes
        v = np.cumsum(v.reshape(*v.shape[:-1], -1, 8), axis=-1, dtype=np.float32)[..., -1]
    n = 1 << max(0, int(v.shape[-1] - 1).bit_length())
    v = np.concatenate([v, np.zeros((*v.shape[:-1], n - v.shape[-1]), np.float32)], axis=-1)
    while v.shape[-1] > 1:
        v = v[..., :v.shape[-1] // 2] + v[..., v.shape[-1] // 2:]
    return v[..., 0]


ORDERS = ["sequential", "pairwise", "lanes"]


def ln_replica32(s, lw, lb, order, rstd_factor=1.0, eps=EPS):
    """The prologues' LayerNorm in fp32, step by step -> h [M, K] float32 (before its bf16 rounding)"""
    s = s.numpy().astype(np.float32)
    K = np.float32(s.shape[-1])
    mean = (_sum32(s, order) / K)[..., None]
    d = s - mean
    var = _sum32(d * d, order) / K
    rstd = (np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32) * np.float32(rstd_factor))[..., None]
    h = d * rstd * lw.float().numpy()
    if lb is not None:
        h = h + lb.float().numpy()
    return torch.from_numpy(h.astype(np.float32))


def linear_replica32(x, W, scale, bias, act, f32):
    """The kernels' order in fp32: thread t of 256 owns the 8-wide chunks t, t + 256, ... (products
    of bf16 / int8 operands are exact in fp32, so fmaf is one rounding of the sum), a butterfly
    over each wave's 64 lanes, then the four waves; scale, bias, GELU and the output rounding."""
    xf, wf = x.float().numpy(), W.float().numpy()
    M, K = xf.shape
    nck = K // 8
    its = -(-nck // 256)
    p = np.zeros((M, wf.shape[0], its * 256 * 8), np.float32)
    p[..., :K] = xf[:, None, :] * wf[None]
    p = p.reshape(M, -1, its, 256, 8).transpose(0, 1, 3, 2, 4).reshape(M, -1, 4, 64, its * 8)
    acc = np.cumsum(p, axis=-1, dtype=np.float32)[..., -1]          # [M, N, 4, 64]
    while acc.shape[-1] > 1:
        acc = acc[..., :acc.shape[-1] // 2] + acc[..., acc.shape[-1] // 2:]
    o = ((acc[..., 0, 0] + acc[..., 1, 0]) + acc[..., 2, 0]) + acc[..., 3, 0]
    o = torch.from_numpy(o)
    if scale is not None:
        o = o * scale.float()
    if bias is not None:
        o = o + bias.float()
    if act:
        o = torch.nn.functional.gelu(o)
    return o if f32 else o.to(BF)


# ---------------------------------------------------------------------------- the CPU checks
def _exact_ks():
    ks = set(SKINNY_LN_K[False] + SKINNY_LN_K[True] + ROW_LN_K[False] + ROW_LN_K[True])
    return sorted(ks | {K for _, K in ROW_LN_WIDE[True]})


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("K", _exact_ks())
def test_exact_ln_premise(K, pattern):
    """The exact-LayerNorm rows: mean and variance exact, and the fp32 prologue gives the integer
    row under every summation order with rstd off by +-2^-10, so no kernel has a rounding to
    choose.  The split forms add up exactly."""
    M = 16 if K <= 1920 else 2
    s, sign = exact_ln_rows(M, K, pattern)
    for m in range(M):
        c, a = PATTERNS[(pattern + m) % 2]
        assert float(s[m].double().mean()) == c and float(((s[m].double() - c) ** 2).mean()) == a * a
        assert int((sign[m] < 0).sum()) == K // 2
    assert M < 2 or not torch.equal(sign[0], sign[1])
    for with_lb in (True, False):
        lw, lb = exact_ln_params(K, with_lb)
        want = exact_ln_x(sign, lw, lb)
        h64, _ = ln_ref(s, lw, lb)
        assert torch.equal(h64.to(BF).double(), want)
        for order in ORDERS:
            for f in (1.0, 1.0 + 2.0 ** -10, 1.0 - 2.0 ** -10):
                assert torch.equal(ln_replica32(s, lw, lb, order, f).to(BF).double(), want), (order, f)
    res, branch = split_res_branch(s)
    assert res.dtype == F32 and branch.dtype == BF
    wte, wpe = split_tables(s[:min(M, EMB_ROWS)], 1)
    assert torch.equal(wte[1].float()[None] + wpe.float(), s[:min(M, EMB_ROWS)])
    assert all(bool((wte[r] != wte[1]).all()) for r in range(wte.shape[0]) if r != 1)


def _sums_below_2_24(x, W):
    return float((x.double().abs() @ W.double().abs().t()).max()) < 2 ** 24


@pytest.mark.parametrize("q8", [False, True], ids=["bf16", "int8"])
def test_integer_premise(q8):
    """Integer operands: sum |x| |W| < 2^24 at the widest rows of the GPU file (every partial sum
    in any order is an exact fp32 integer) and the float64 result, scaled and biased, is itself
    an fp32 number; the same for the integer rows the exact LayerNorm hands on."""
    for rows, N, K in [(8, 100, 3072), (1, 100, 8208 if q8 else 2056), (16, 48, 2112) if q8 else (64, 48, 3072)]:
        x, (W, scale), b = int_x(rows, K), int_weight(N, K, q8), int_bias(N)
        assert _sums_below_2_24(x, W)
        ref, _, _ = linear_ref(x, W, scale, b)
        assert torch.equal(ref.float().double(), ref)
    for K in (1920, 8192):
        _, sign = exact_ln_rows(2, K, 1)
        lw, lb = exact_ln_params(K, True)
        x = exact_ln_x(sign, lw, lb)
        W, scale = int_weight(100, K, q8)
        assert _sums_below_2_24(x, W)
        ref, _, _ = linear_ref(x, W, scale, int_bias(100))
        assert torch.equal(ref.float().double(), ref)


def rand_ln_cases():
    """(rows, K, branch) of every random LayerNorm row set the GPU file runs, the embedding rows as
    rows = 0."""
    out = []
    for shapes in (RAND_ROW_LN, RAND_SKINNY_LN):
        for rows, _, K in shapes:
            for branch in (False, True):
                if (rows, K, branch) not in out:
                    out.append((rows, K, branch))
    return out + [(0, K, False) for K in sorted({K for _, _, K in RAND_ROW_LN})]


def rand_ln_rows(rows, K, branch):
    """-> (s fp32 [M, K], lw, lb) of a case of rand_ln_cases"""
    if rows:
        _, _, s, lw, lb = rand_ln(rows, K, branch)
        return s, lw, lb
    wte, wpe = rand_tables(K)
    _, _, _, lw, lb = rand_ln(1, K, False)
    return (wte[EMB_TOK].float() + wpe[EMB_POS].float()).view(1, K), lw, lb


def test_tau_and_ambiguous_share(capsys):
    """TAU is at least four times the worst distance of the fp32 replica from float64, relative to
    m, over every random LayerNorm input of the GPU file and the three orders; under it fewer than
    1 % of a row's elements are ambiguous."""
    worst, share = 0.0, 0.0
    for rows, K, branch in rand_ln_cases():
        s, lw, lb = rand_ln_rows(rows, K, branch)
        h64, m = ln_ref(s, lw, lb)
        for order in ORDERS:
            worst = max(worst, float(((ln_replica32(s, lw, lb, order).double() - h64).abs() / m).max()))
        share = max(share, float(ambiguous(h64, m).double().mean(-1).max()))
    with capsys.disabled():
        print(f"\nfp32 LayerNorm replica: worst |h32 - h64| / m {worst:.3e} = 2^{np.log2(worst):.2f}; "
              f"worst ambiguous share of a row {100 * share:.2f} %")
    assert 4 * worst <= TAU
    assert share < AMBIGUOUS_SHARE


def test_fp32_replica_within_bounds(capsys):
    """An fp32 replica in the kernels' summation order stays within the bounds of the random-valued
    GPU tests on their very inputs (the 784-column shapes on their first 64 columns)."""
    worst = {"f32": 0.0, "bf16": 0.0, "gelu": 0.0, "ln": 0.0}
    for q8 in (False, True):
        for rows, N, K in RAND_GEMV[q8] + (RAND_SKINNY_Q8 if q8 else RAND_SKINNY):
            x, W, scale, b = rand_linear(rows, N, K, q8)
            W, scale, b = W[:64], (scale[:64] if q8 else None), b[:64]
            for act, f32 in ((0, 0), (0, 1), (1, 0)):
                ref, mag, u = linear_ref(x, W, scale, b, act)
                y = linear_replica32(x, W, scale, b, act, f32)
                r = float(((y.double() - ref).abs() / plain_bound(ref, mag, u, act, f32)).max())
                key = "gelu" if act else "f32" if f32 else "bf16"
                worst[key] = max(worst[key], r)
        for rows, N, K in RAND_ROW_LN + RAND_SKINNY_LN:
            if K % (64 if rows > 1 and q8 else 16 if q8 else 8) or N > 128:
                continue
            res, br, s, lw, lb = rand_ln(rows, K, True)
            _, W, scale, b = rand_linear(rows, N, K, q8)
            for act in (0, 1):
                ref, mag, u = ln_linear_ref(s, lw, lb, W, scale, b, act)
                bound, amb = ln_bound(s, lw, lb, W, scale, ref, mag, u, act, False)
                y = linear_replica32(ln_replica32(s, lw, lb, "lanes").to(BF), W, scale, b, act, False)
                worst["ln"] = max(worst["ln"], float(((y.double() - ref).abs() / bound).max()))
    with capsys.disabled():
        print("\nfp32 replica, worst error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
