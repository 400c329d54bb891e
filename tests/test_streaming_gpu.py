"""The optimizer and streaming kernels (``optim.hip``, ``elementwise.hip``) element by element.

Every entry point is called raw through ``_lib.call`` with buffers this module owns, into
NaN-prefilled outputs, at sizes that run every loop at least twice (past the grid caps) and
leave a partial stride, a partial unrolled group and a scalar tail.  The references are the
float64 / bit-exact functions of ``test_streaming_refs.py``; each bound is stated from the
roundings that form the value, next to the worst ratio the kernel reached on an MI355X.
"""

import math
import time

import numpy as np
import pytest
import torch

from test_streaming_refs import (F64, adamw_ref, adamw_scalars, cast_specials, dropout_ref, f32, finite_patterns,
                                 gelu_bounds, gelu_ref, same_bits_or_nan)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
FH = torch.float16
F32 = torch.float32
I16 = torch.int16
I32 = torch.int32
LS_SCALE, LS_TRACKER, LS_FOUND, LS_SKIPPED, LS_STEP = range(5)


def _nan(*shape, dt=F32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dt)


def _sym(name, h):
    return name + "_h" if h else name


def _dt(h):
    return FH if h else BF


def _worst(name, err, bound):
    """Largest err / bound over the elements (inf where a zero bound is missed); printed so a
    run with ``-s`` shows how close the kernel comes to each bound."""
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    r = r.max().item() if r.numel() else 0.0
    print(f"worst ratio {name}: {r:.4f}")
    return r


def _within(name, got, ref, bound):
    err = (got.to(F64) - ref).abs()
    _worst(name, err, bound)
    assert torch.isfinite(got).all(), name
    assert (err <= bound).all(), name


def _spread(n, gen):
    """Random values with magnitudes over several decades."""
    return torch.randn(n, device=DEV, generator=gen) * torch.exp(3 * torch.randn(n, device=DEV, generator=gen))


# =============================================================================== AdamW
# two full grid strides (4096 blocks x 256 lanes x 4 elements) and a partial third
N_BIG = 2 * 4096 * 256 * 4 + 192
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.95, 1e-8, 0.1
COEF2 = f32(0.125 * 0.37)


def _adamw_inputs(n, seed):
    """fp32 p, g, m, v >= 0 spread over decades, exact zeros in each (and in all four at
    once), a random decay flag per 64-element chunk, and chunks of values whose p' is p
    itself (g = m = 0, no decay) sitting on the compute shadow's rounding edges."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    p, g, m, v = _spread(n, gen), _spread(n, gen), _spread(n, gen), _spread(n, gen).abs()
    mask = torch.randint(0, 2, (n // 64,), device=DEV, generator=gen, dtype=torch.uint8)
    for k, t in enumerate((p, g, m, v)):
        t[torch.tensor([3 + k, n // 2 + 5 + k, n - 9 - k], device=DEV) % n] = 0.0
    for t in (p, g, m, v):
        t[torch.tensor([1, n // 3, n - 2], device=DEV)] = 0.0
    s = cast_specials()
    s = s[torch.isfinite(s)].to(DEV)
    assert s.numel() <= 56
    # first stride, second stride, and the last chunk of the partial third (n = 64: the only chunk)
    edge = sorted({min(2, n // 64 - 1), (4096 * 256 * 4 + 64 * 7) // 64 % (n // 64), n // 64 - 1})
    idx = torch.cat([c * 64 + 8 + torch.arange(s.numel(), device=DEV) for c in edge])
    p[idx] = s.repeat(len(edge))
    g[idx] = 0.0
    m[idx] = 0.0
    if n > 64 or seed % 2 == 0:
        mask[torch.tensor(edge, device=DEV)] = 0
    return p, g, m, v, mask, idx


def _adamw_call(h, p, g, m, v, shadow, mask, args, coef_t, ls):
    from nanosandbox_amd.ops import _lib
    _lib.call(_sym("nsa_adamw_step", h), _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(shadow),
              _lib.ptr(mask), p.numel(), *args, _lib.ptr(coef_t), _lib.ptr(ls), _lib.stream())
    torch.cuda.synchronize()


_ADAMW_CASES = [
    (N_BIG, False, 1, 1.0, "host"), (N_BIG, True, 7, COEF2, "host"), (N_BIG, False, 1000, COEF2, "ls"),
    (N_BIG, True, 7, 1.0, "ls"), (N_BIG, True, 7, 1.0, "found"), (N_BIG, False, 7, 1.0, "null"),
] + [(64, h, t, c, "host") for h in (False, True) for t in (1, 7, 1000) for c in (1.0, COEF2)] \
  + [(64, h, 7, COEF2, mode) for h in (False, True) for mode in ("ls", "null", "found")]


@pytest.mark.parametrize("n,h,t,coef,mode", _ADAMW_CASES)
def test_adamw_step_per_element(kernels, n, h, t, coef, mode):
    """One nsa_adamw_step(_h) from an arbitrary state against float64, every element of p', m'
    and v' within 2^-20 of the magnitude of its terms, the compute shadow bit-equal to the
    rounded p'.  mode: 'host' bias corrections from the arguments; 'ls' from the loss-scale
    state's step (the arguments' are wrong on purpose); 'null' no shadow; 'found' a step the
    loss scale skips, which writes nothing."""
    dt = _dt(h)
    p0, g, m0, v0, mask, idx = _adamw_inputs(n, seed=1000 * t + (7 if h else 0) + (n == 64) + int(coef < 1))
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    shadow = None if mode == "null" else _nan(n, dt=dt)
    sc = adamw_scalars(LR, B1, B2, EPS, WD, t)
    coef_t = torch.tensor([coef], dtype=F32, device=DEV)
    args, ls = sc["args"], None
    if mode in ("ls", "found"):
        ls = torch.zeros(8, dtype=F32, device=DEV)
        ls[LS_SCALE], ls[LS_STEP], ls[LS_FOUND] = 2.0 ** 12, float(t), float(mode == "found")
        args = args[:5] + (0.5, 0.25)  # not this step's bias corrections: the kernel must take the device step
        ls0 = ls.clone()
    _adamw_call(h, p, g, m, v, shadow, mask, args, coef_t, ls)
    if ls is not None:
        assert torch.equal(ls, ls0)
    if mode == "found":
        for a, b in ((p, p0), (m, m0), (v, v0)):
            assert torch.equal(a.view(I32), b.view(I32))
        assert torch.isnan(shadow).all()
        return
    pr, mr, vr, ep, em = adamw_ref(p0, g, m0, v0, mask, coef_t.item(), sc)
    # Each value passes through fewer than 16 fp32 roundings of 2^-24 (2^-20 of the terms'
    # magnitudes); an fp32 torch evaluation of the formula reaches 7.7 * 2^-24.  Beside each
    # bound: the kernel's worst error / bound over all cases on an MI355X (times 16 for 2^-24s).
    tag = f"adamw[{n},{'f16' if h else 'bf16'},t={t},{mode}]"
    _within(f"{tag} p", p, pr, 2.0 ** -20 * ep + 2.0 ** -126)  # worst 0.302 (4.8 * 2^-24)
    _within(f"{tag} m", m, mr, 2.0 ** -20 * em)  # worst 0.161 (2.6 * 2^-24)
    _within(f"{tag} v", v, vr, 2.0 ** -20 * vr)  # worst 0.199 (3.2 * 2^-24)
    # with g = m = 0 and no decay p' is p, bit for bit: the shadow sees the ties, the fp16
    # overflows and the fp16 subnormals that were seeded (fp32 denormals may be flushed)
    if n > 64 or not mask[0].item():
        big = p0[idx].abs() >= 2.0 ** -126
        assert torch.equal(p[idx][big].view(I32), p0[idx][big].view(I32))
        r16 = p[idx].cpu().to(dt).float()
        assert (r16 != p[idx].cpu()).any()
        if h:
            assert torch.isinf(r16).any() and ((r16 != 0) & (r16.abs() < 2.0 ** -14)).any()
    if shadow is not None:
        want = p.cpu().to(dt)
        assert torch.equal(shadow.cpu().view(I16), want.view(I16))


# ============================================================== gradient norm and clip coefficient
NB = 1024  # FusedAdamW's _NORM_BLOCKS


def _norm_call(g, pre, scale, max_norm, ls=None, growth=2.0, backoff=0.5, interval=2000.0):
    from nanosandbox_amd.ops import _lib
    partial, norm, coef = _nan(2 * NB), _nan(1), _nan(1)
    _lib.call("nsa_sumsq_partial", _lib.ptr(g), g.numel(), _lib.ptr(partial), NB, pre, _lib.ptr(ls), _lib.stream())
    _lib.call("nsa_clip_coef", _lib.ptr(partial), NB, scale, max_norm, _lib.ptr(norm), _lib.ptr(coef),
              _lib.ptr(ls), growth, backoff, interval, _lib.stream())
    torch.cuda.synchronize()
    return partial, norm.item(), coef.item()


def _coef_ok(coef, scale, max_norm, norm):
    """coef = scale * min(1, max_norm / (norm + 1e-6)) from the fp32 norm the kernel reported:
    an fp32 add, divide and multiply and the fp32 1e-6, 4 * 2^-24 relative."""
    ref = scale * min(1.0, max_norm / (float(np.float32(norm)) + float(np.float32(1e-6))))
    return abs(coef - ref) <= 4 * 2.0 ** -24 * ref


def _norm_grad(n, seed):
    """Random gradient whose last 192 elements carry about half of the sum of squares."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    g = torch.randn(n, device=DEV, generator=gen)
    if n > 192:
        g[-192:] *= math.sqrt((n - 192) / 192)
        sq = g.double().pow(2)
        assert 0.4 < (sq[-192:].sum() / sq.sum()).item() < 0.6
    return g


N_NORM = 3 * 1024 * 256 * 4 + 192  # three full strides of the 1024-block grid and 48 lanes of a fourth


def test_grad_norm_and_clip_coef(kernels):
    """nsa_sumsq_partial + nsa_clip_coef without a loss scale, grad_scale 0.125: the norm of
    g * pre within 2^-16 (128 sequential fp32 additions of positive terms per lane at worst,
    halved by the square root; one lost block of 1024 would move it by 2^-11), the coefficient
    from that norm, max_norm 0 and a max_norm above the norm leaving exactly the scale."""
    pre = scale = 0.125
    for n in (N_NORM, 3 * 256 * 4, 64):
        g = _norm_grad(n, seed=n)
        ref = (g.double() * pre).norm().item()
        partial, norm, coef = _norm_call(g, pre, scale, 0.25)
        err = abs(norm - ref)
        print(f"worst ratio norm[{n}]: {err / (2.0 ** -16 * ref):.4f}")
        assert err <= 2.0 ** -16 * ref  # worst 0.0015 of the bound (1.5 * 2^-24)
        assert ref > 0.5 and _coef_ok(coef, scale, 0.25, norm) and coef < scale
        # blocks past the data hold an exact zero; without a loss scale the second half is not written
        used = min(NB, -(-n // (256 * 4)))
        assert (partial[:used] > 0).all() and torch.equal(partial[used:NB], torch.zeros(NB - used, device=DEV))
        assert torch.isnan(partial[NB:]).all()
        assert abs(partial[:NB].double().sum().sqrt().item() - ref) <= 2.0 ** -16 * ref
        for max_norm in (0.0, 1e9):
            _, norm2, coef2 = _norm_call(g, pre, scale, max_norm)
            assert norm2 == norm and coef2 == scale


@pytest.mark.parametrize("case", ["clean", "grow", "inf_last", "nan_sparse"])
def test_grad_norm_with_loss_scale(kernels, case):
    """The same two kernels with a loss-scale state of 2^12: the norm is the unscaled
    gradient's, coef = scale / 2^12 * c, and the state moves exactly as
    DynamicLossScale.update does on the host; an inf in the very last element (the partial
    fourth stride) or a NaN alone in a block whose other elements are zero is found."""
    from nanosandbox_amd.optim.loss_scale import DynamicLossScale
    pre = scale = 0.125
    S = 2.0 ** 12
    host = DynamicLossScale(init_scale=S, growth_interval=3)
    host.state[LS_TRACKER] = 2.0 if case == "grow" else 0.0
    host.state[LS_STEP], host.state[LS_SKIPPED] = 41.0, 5.0
    if case == "nan_sparse":
        n = 3 * 256 * 4 + 64
        g = _norm_grad(n, seed=5)
        g[3 * 256 * 4:] = 0.0  # block 3 holds these 64 elements only
        g[3 * 256 * 4 + 37] = float("nan")
    else:
        n = N_NORM
        g = _norm_grad(n, seed=6)
    ref = (g.double() * pre).norm().item()
    gs = g * S
    if case == "inf_last":
        gs[-1] = float("inf")
    ls = host.state.to(DEV)
    partial, norm, coef = _norm_call(gs, pre, scale, 1.0, ls, host.growth_factor, host.backoff_factor,
                                     float(host.growth_interval))
    found = case in ("inf_last", "nan_sparse")
    host.update(found)
    assert torch.equal(ls.cpu()[:5], host.state[:5]), (ls, host.state)
    assert host.scale == {"clean": S, "grow": 2 * S}.get(case, S / 2)
    bad = partial[NB:]
    if found:
        assert norm == math.inf and coef == 0.0
        assert bad.sum().item() == 1.0 and bad[0 if case == "inf_last" else 3].item() == 1.0
    else:
        print(f"worst ratio norm[ls,{case}]: {abs(norm - ref) / (2.0 ** -16 * ref):.4f}")
        assert abs(norm - ref) <= 2.0 ** -16 * ref
        assert _coef_ok(coef, scale / S, 1.0, norm)
        assert torch.equal(bad, torch.zeros(NB, device=DEV))


@pytest.mark.parametrize("with_ls", [False, True])
def test_clip_coef_strides_over_partials(kernels, with_ls):
    """nsa_clip_coef alone over 1500 partials (its 1024 lanes stride once more): the last
    partial carries half of the sum, and with a loss scale a non-finite count sits at 1400."""
    from nanosandbox_amd.ops import _lib
    nparts = 1500
    torch.manual_seed(9)
    part = _nan(2 * nparts + 8)
    part[:nparts] = torch.rand(nparts, device=DEV) + 0.5
    part[nparts - 1] = part[:nparts - 1].sum()
    ref = part[:nparts].double().sum().sqrt().item()
    scale, max_norm = 0.125, 1.0
    for bad_at in ((None, 1400) if with_ls else (None,)):
        ls = None
        if with_ls:
            part[nparts:2 * nparts] = 0.0
            if bad_at is not None:
                part[nparts + bad_at] = 2.0
            ls = torch.zeros(8, dtype=F32, device=DEV)
            ls[LS_SCALE] = 2.0 ** 12
        norm, coef = _nan(1), _nan(1)
        _lib.call("nsa_clip_coef", _lib.ptr(part), nparts, scale, max_norm, _lib.ptr(norm), _lib.ptr(coef),
                  _lib.ptr(ls), 2.0, 0.5, 2000.0, _lib.stream())
        torch.cuda.synchronize()
        if bad_at is not None:
            assert norm.item() == math.inf and coef.item() == 0.0
            assert ls[LS_FOUND].item() == 1.0 and ls[LS_SCALE].item() == 2.0 ** 11 and ls[LS_SKIPPED].item() == 1.0
            continue
        # the partials are summed in double: one rounding of the fp32 result (and the sqrt's)
        assert abs(norm.item() - ref) <= 2.0 ** -23 * ref
        assert _coef_ok(coef.item(), scale / (2.0 ** 12 if with_ls else 1.0), max_norm, norm.item())
        if with_ls:
            assert ls[LS_FOUND].item() == 0.0 and ls[LS_STEP].item() == 1.0 and ls[LS_SCALE].item() == 2.0 ** 12


# ================================================================================ GELU
def _gelu_run(h, x, dy):
    from nanosandbox_amd.ops import _lib
    n = x.numel()
    y, dx = _nan(n, dt=x.dtype), _nan(n, dt=x.dtype)
    _lib.call(_sym("nsa_gelu_fwd", h), _lib.ptr(x), _lib.ptr(y), n, _lib.stream())
    _lib.call(_sym("nsa_gelu_bwd", h), _lib.ptr(dy), _lib.ptr(x), _lib.ptr(dx), n, _lib.stream())
    torch.cuda.synchronize()
    return y, dx


def _gelu_check(tag, x, dy, y, dx, quiet=False):
    """bf16: |y - ref| <= 2^-8 |ref| + 2^-21 |x| + 2^-126 and
    |dx - dy ref'| <= 2^-8 |dy ref'| + 2^-21 |dy| (1 + |x|) + 2^-126; fp16: 2^-11 and 2^-25
    (``gelu_bounds``).  Returns the worst ratios."""
    yr, gr = gelu_ref(x)
    bf, bb = gelu_bounds(x, dy, yr, gr, x.dtype)
    ef, eb = (y.to(F64) - yr).abs(), (dx.to(F64) - dy.to(F64) * gr).abs()
    rf, rb = (ef / bf).max().item(), (eb / bb).max().item()
    if not quiet:
        print(f"worst ratio {tag} fwd: {rf:.4f}")
        print(f"worst ratio {tag} bwd: {rb:.4f}")
    assert torch.isfinite(y).all() and torch.isfinite(dx).all(), tag
    # worst error / bound on an MI355X: bf16 fwd 0.975, bwd 0.996; fp16 fwd 0.9995, bwd 0.998.  The
    # bound is one output rounding plus the erf term, and a rounding reaches half an ulp: the
    # correctly rounded float64 value itself gives 0.975 / 0.993 (bf16) and 0.9995 / 0.997 (fp16)
    assert (ef <= bf).all(), tag
    assert (eb <= bb).all(), tag
    return rf, rb


@pytest.mark.parametrize("h", [False, True])
def test_gelu_every_finite_input(kernels, h):
    """Every finite bf16 (fp16) bit pattern through nsa_gelu_fwd / bwd (_h) with dy = 1, -0.37
    and a random value, shuffled into 8 k + 5 elements so that patterns pass through the
    vector body and the scalar tail."""
    dt = _dt(h)
    gen = torch.Generator().manual_seed(12)
    pats = finite_patterns(dt)
    pats = pats[torch.randperm(pats.numel(), generator=gen)]
    k = pats.numel()
    x = torch.cat([pats, pats, pats, torch.tensor([-0.0, 0.0]).to(dt), pats[:3]])  # both zeros in the tail
    dy = torch.cat([torch.ones(k), torch.full((k,), -0.37), torch.randn(k + 5, generator=gen)]).to(dt)
    assert x.numel() % 8 == 5 and x.numel() == dy.numel()
    x, dy = x.to(DEV), dy.to(DEV)
    y, dx = _gelu_run(h, x, dy)
    _gelu_check(f"gelu[{'f16' if h else 'bf16'},all]", x, dy, y, dx)
    zero = x == 0  # gelu(+-0) = +-0, in the body and in the tail
    assert zero[-5:].sum().item() == 2 and zero.sum().item() == 8
    assert torch.equal(y.view(I16)[zero], x.view(I16)[zero])


@pytest.mark.parametrize("h", [False, True])
def test_gelu_past_the_grid_cap(kernels, h):
    """One full stride of the 2048-block grid (256 lanes x 4 vectors x 8 elements), then a
    partial unrolled group of 300 vectors (the clamped loads followed by a second
    iteration) and a 3-element tail."""
    dt = _dt(h)
    n = 2048 * 256 * 4 * 8 + 8 * 300 + 3
    gen = torch.Generator(device=DEV)
    gen.manual_seed(13)
    x = (torch.randn(n, device=DEV, generator=gen) * 3).to(dt)
    dy = torch.randn(n, device=DEV, generator=gen).to(dt)
    y, dx = _gelu_run(h, x, dy)
    _gelu_check(f"gelu[{'f16' if h else 'bf16'},{n}]", x, dy, y, dx)


def test_gelu_nontemporal_equals_plain(kernels):
    """The nontemporal instantiation (taken from NSA_NT_MIN_BYTES = 256 MiB of input upward)
    on NSA_NT_MIN_BYTES / 2 + 8 * 257 + 3 bf16 elements: bitwise equal to the plain kernel on
    the same input, and within the bounds of float64 in slices of 16 M elements."""
    from nanosandbox_amd.ops import _lib
    n = (256 << 20) // 2 + 8 * 257 + 3
    gen = torch.Generator(device=DEV)
    gen.manual_seed(14)
    x = torch.empty(n, device=DEV, dtype=BF)
    dy = torch.empty(n, device=DEV, dtype=BF)
    step = 1 << 24
    for o in range(0, n, step):
        x[o:o + step] = (torch.randn(min(step, n - o), device=DEV, generator=gen) * 3).to(BF)
        dy[o:o + step] = torch.randn(min(step, n - o), device=DEV, generator=gen).to(BF)
    t0 = time.perf_counter()
    prev = _lib.call_ret("nsa_ew_set_nt", 1)
    try:
        y1, dx1 = _gelu_run(False, x, dy)
        _lib.call_ret("nsa_ew_set_nt", 0)
        y0, dx0 = _gelu_run(False, x, dy)
    finally:
        _lib.call_ret("nsa_ew_set_nt", prev)
    assert torch.equal(y1.view(I16), y0.view(I16))
    assert torch.equal(dx1.view(I16), dx0.view(I16))
    del y0, dx0
    worst = (0.0, 0.0)
    for o in range(0, n, step):
        s = slice(o, min(n, o + step))
        r = _gelu_check(f"gelu[nt,{o}]", x[s], dy[s], y1[s], dx1[s], quiet=True)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    torch.cuda.synchronize()
    print(f"worst ratio gelu[bf16,nt] fwd: {worst[0]:.4f}")
    print(f"worst ratio gelu[bf16,nt] bwd: {worst[1]:.4f}")
    print(f"gelu nontemporal A/B and float64 comparison: {time.perf_counter() - t0:.2f} s")


# ============================================================================= dropout
@pytest.mark.parametrize("h", [False, True])
def test_dropout_equals_hash_replica(kernels, h):
    """nsa_dropout(_h) bit for bit against the host replica of common.h's hash at the flat
    element index: vector body and scalar tail, the device step counter at 0 and 3, two
    salts, p = 0 (x itself), 0.2, 0.5 and 1 (zeros)."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.ops import _lib
    dt = _dt(h)
    torch.manual_seed(15)
    try:
        for step in (0, 3):
            ops.rng_set(DEV, step)
            for n in (5, 8, 8 * 256 * 3 + 5, (1 << 20) + 3):
                x = torch.randn(n, device=DEV).to(dt)
                x[0] = x[n - 1] = -0.0  # a kept -0 stays -0, in the body and in the tail
                xc = x.cpu()
                for salt in (0x123456789ABCDEF, (1 << 62) - 0x5DEECE66D):
                    for p in (0.0, 0.2, 0.5, 1.0):
                        y = _nan(n, dt=dt)
                        _lib.call(_sym("nsa_dropout", h), _lib.ptr(x), _lib.ptr(y), n, p, salt, _lib.stream())
                        torch.cuda.synchronize()
                        ref = dropout_ref(xc, p, salt, step)
                        assert torch.equal(y.cpu().view(I16), ref.view(I16)), (step, n, hex(salt), p)
                        if p == 0.0:
                            assert torch.equal(y.view(I16), x.view(I16))
                        if p == 1.0:
                            assert not y.view(I16).any()
    finally:
        ops.rng_set(DEV, 0)
        torch.cuda.synchronize()


# ================================================================ casts and row scaling
def _cast_inputs(n, seed):
    """fp32 inputs of n elements: random values over the decades both targets round in, with
    the block of specials at the start and again across the end (so that the scalar tail
    converts some); a size below the block walks it in windows."""
    s = cast_specials().to(DEV)
    L = s.numel()
    if n < 2 * L:
        return [s[o:o + n].clone() for o in range(0, L - n + 1, n)]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    x = torch.randn(n, device=DEV, generator=gen) * torch.exp(4 * torch.randn(n, device=DEV, generator=gen))
    x[:L] = s
    x[n - L:] = s.roll(L // 2)
    return [x]


_CAST_SIZES = [3, 8, 8 * 1025 + 7, 5 * (1 << 20) + 5]


@pytest.mark.parametrize("h", [False, True])
@pytest.mark.parametrize("n", _CAST_SIZES)
def test_cast_f32_to_16_bit_exact(kernels, n, h):
    """nsa_cast_f32_bf16(_h) against torch's round-to-nearest-even conversion, bit for bit
    (any NaN for a NaN)."""
    from nanosandbox_amd.ops import _lib
    dt = _dt(h)
    for x in _cast_inputs(n, seed=16):
        y = _nan(n, dt=dt)
        _lib.call(_sym("nsa_cast_f32_bf16", h), _lib.ptr(x), _lib.ptr(y), n, _lib.stream())
        torch.cuda.synchronize()
        assert same_bits_or_nan(y.cpu(), x.cpu().to(dt))


@pytest.mark.parametrize("h", [False, True])
@pytest.mark.parametrize("n", _CAST_SIZES)
def test_scale_rows_bit_exact(kernels, n, h):
    """nsa_scale_rows_bf16(_h): y = (x.float() * s).to(dtype) with the device scalar s, one fp32
    product and one rounding, bit for bit."""
    from nanosandbox_amd.ops import _lib
    dt = _dt(h)
    s = torch.tensor([0.3337], dtype=F32, device=DEV)
    for x32 in _cast_inputs(n, seed=17):
        x = x32.to(dt)
        y = _nan(n, dt=dt)
        _lib.call(_sym("nsa_scale_rows_bf16", h), _lib.ptr(x), _lib.ptr(y), _lib.ptr(s), n, _lib.stream())
        torch.cuda.synchronize()
        want = (x.cpu().float() * s.cpu()).to(dt)
        assert same_bits_or_nan(y.cpu(), want)
        assert torch.equal(torch.isnan(y).cpu(), torch.isnan(x).cpu())


# =================================================================== split-K reduction
@pytest.mark.parametrize("splits", [1, 2, 5])
@pytest.mark.parametrize("n", [3, 4, 4 * 777 + 2, 3 * (1 << 20) + 1])
def test_splitk_reduce_fixed_order(kernels, n, splits):
    """nsa_splitk_reduce: out + (((ws0 + ws1) + ws2) + ...) in fp32, in that order, exactly."""
    from nanosandbox_amd.ops import _lib
    gen = torch.Generator(device=DEV)
    gen.manual_seed(18 + splits)
    ws = _spread(splits * n, gen).view(splits, n)
    out0 = _spread(n, gen)
    out = out0.clone()
    _lib.call("nsa_splitk_reduce", _lib.ptr(ws), _lib.ptr(out), n, splits, _lib.stream())
    torch.cuda.synchronize()
    acc = ws[0].clone()
    for s in range(1, splits):
        acc = acc + ws[s]
    assert torch.equal(out, out0 + acc)


# ========================================================================= column sums
@pytest.mark.parametrize("h", [False, True])
@pytest.mark.parametrize("T,C,ld,nblk", [(1000, 72, 72, 16), (5, 8, 8, 16), (333, 520, 1040, 7),
                                         (257, 2304, 2304 + 64, 4), (64, 520, 520, 1)])
def test_colsum_partial_and_accum_exact(kernels, T, C, ld, nblk, h):
    """nsa_colsum_bf16_partial(_h) then nsa_colsum_accum / _ordered on small integers, whose
    fp32 sums are exact in any order: every partial row and the accumulated gradient equal
    the integer sums; T not a multiple of 4 nblk, T < nblk (empty row slices write zeros),
    C below / across / above one 512-column block, a column slice (ld > C) of a wider tensor."""
    from nanosandbox_amd.ops import _lib
    dt = _dt(h)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(19)
    wide = torch.randint(-8, 9, (T, ld), device=DEV, generator=gen).to(dt)
    c0 = ld - C  # the slice's first column (a multiple of 8)
    dy = wide[:, c0:]
    part = _nan(nblk, C)
    _lib.call(_sym("nsa_colsum_bf16_partial", h), _lib.ptr(wide) + 2 * c0, ld, T, C, _lib.ptr(part), nblk,
              _lib.stream())
    torch.cuda.synchronize()
    rpb = -(-T // nblk)
    want = torch.zeros(nblk, C, device=DEV)
    for b in range(nblk):
        want[b] = dy[b * rpb:(b + 1) * rpb].float().sum(0)
    assert torch.equal(part, want)
    assert torch.equal(want.sum(0), dy.float().sum(0))
    gb0 = torch.randint(-50, 51, (C,), device=DEV, generator=gen).float()
    gb0[0] = 17.0
    for fn in ("nsa_colsum_accum", "nsa_colsum_accum_ordered"):
        gb = gb0.clone()
        _lib.call(fn, _lib.ptr(part), _lib.ptr(gb), nblk, C, _lib.stream())
        torch.cuda.synchronize()
        assert torch.equal(gb, gb0 + dy.float().sum(0)), fn


@pytest.mark.parametrize("rows", [1, 31, 33, 100, 1100])
def test_colsum_accum_rows_and_columns(kernels, rows):
    """nsa_colsum_accum / _ordered alone on integer partials: rows below and across the
    32-row split, and 1100 > 32 splits x 32; C of one lane, one block, one block and a
    lane, many blocks."""
    from nanosandbox_amd.ops import _lib
    gen = torch.Generator(device=DEV)
    gen.manual_seed(20 + rows)
    for C in (1, 64, 65, 768):
        part = torch.randint(-8, 9, (rows, C), device=DEV, generator=gen).float()
        out0 = torch.randint(-50, 51, (C + 3,), device=DEV, generator=gen).float()
        for fn in ("nsa_colsum_accum", "nsa_colsum_accum_ordered"):
            out = out0.clone()
            _lib.call(fn, _lib.ptr(part), _lib.ptr(out), rows, C, _lib.stream())
            torch.cuda.synchronize()
            assert torch.equal(out[:C], out0[:C] + part.sum(0)), (fn, C)
            assert torch.equal(out[C:], out0[C:]), (fn, C)  # nothing past column C
