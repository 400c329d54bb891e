"""High-precision references for the optimizer and streaming kernels (``optim.hip``,
``elementwise.hip``), as plain functions that run on any device, with their own CPU checks.

``test_streaming_gpu.py`` compares the HIP kernels with these element by element; the tests
below check the references themselves where no GPU is present: the float64 AdamW step
against ``torch.optim.AdamW``, the float64 GELU against ``torch.nn.functional.gelu``, the
dropout hash replica against splitmix64's published first output, the error-bound helpers
against an fp32 evaluation of the same formulas.
"""

import math

import numpy as np
import torch

F64 = torch.float64


def f32(x) -> float:
    """x rounded to fp32 (what a ``float`` kernel argument receives), as a Python float."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------- AdamW
def adamw_scalars(lr, b1, b2, eps, wd, t):
    """The scalars of one AdamW step as the kernel uses them: every argument rounded to fp32,
    ``1 - beta``, ``1 - lr * wd``, ``lr / bc1`` and ``1 / bc2_sqrt`` formed in fp32 like the entry
    point (``adamw_entry``) and the kernel do.  The bias corrections are the host's doubles
    (``FusedAdamW.step``) rounded to fp32."""
    one = np.float32(1.0)
    beta1, beta2 = float(b1), float(b2)  # the optimizer's Python floats
    lr, b1, b2, eps, wd = (np.float32(x) for x in (lr, b1, b2, eps, wd))
    bc1 = np.float32(1.0 - beta1 ** t)
    bc2_sqrt = np.float32(math.sqrt(1.0 - beta2 ** t))
    return dict(b1=float(b1), b2=float(b2), eps=float(eps), omb1=float(one - b1), omb2=float(one - b2),
                decay=float(one - lr * wd), step=float(lr / bc1), inv_bc2=float(one / bc2_sqrt),
                args=(float(lr), float(b1), float(b2), float(eps), float(wd), float(bc1), float(bc2_sqrt)))


def adamw_ref(p, g, m, v, wd_mask, coef, sc):
    """One AdamW step in float64 (the formula in the ``optim.hip`` header) from fp32 state.

    p, g, m, v: fp32 tensors; wd_mask: one uint8 per 64 elements; coef: the device scalar
    (fp32 value as a float); sc: ``adamw_scalars``.  Returns float64 (p', m', v') and the error
    scales (ep, em) that the per-element bounds multiply by 2^-20: the sums of the absolute
    values of the terms that form p' and m'."""
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    d = torch.where(wd_mask.repeat_interleave(64).bool(), sc["decay"], 1.0).to(F64)
    gj = g * coef
    m1 = sc["b1"] * m + sc["omb1"] * gj
    v1 = sc["b2"] * v + sc["omb2"] * gj * gj
    denom = v1.sqrt() * sc["inv_bc2"] + sc["eps"]
    p1 = p * d - sc["step"] * m1 / denom
    em = sc["b1"] * m.abs() + sc["omb1"] * gj.abs()
    ep = (p * d).abs() + sc["step"] * em / denom
    return p1, m1, v1, ep, em


# -------------------------------------------------------------------------------- GELU
def gelu_ref(x):
    """(x Phi(x), Phi(x) + x phi(x)) in float64; Phi through erfc, which keeps the left
    tail's relative precision."""
    x = x.to(F64)
    cdf = 0.5 * torch.special.erfc(-x * math.sqrt(0.5))
    pdf = torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))
    return x * cdf, cdf + x * pdf


def finite_patterns(dtype):
    """Every finite value of a 16-bit float type (both zeros and the subnormals included):
    65280 for bfloat16, 63488 for float16."""
    bits = torch.arange(1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(dtype)
    return x[torch.isfinite(x.float())]


def gelu_bounds(x, dy, y_ref, g_ref, dtype):
    """Per-element error bounds of the GELU forward / backward for 16-bit ``dtype``: one output
    rounding (2^-8 bf16, 2^-11 fp16) of the value, the erf approximation's absolute error
    (1.5e-7, times x for the forward and (1 + |x|) for the backward) with room for the fast
    reciprocal and exp, and the smallest normal (bf16; a GPU may flush below it) or half the
    subnormal spacing (fp16)."""
    rel, tiny = (2.0 ** -11, 2.0 ** -25) if dtype == torch.float16 else (2.0 ** -8, 2.0 ** -126)
    x, dy = x.to(F64), dy.to(F64)
    bf = rel * y_ref.abs() + 2.0 ** -21 * x.abs() + tiny
    bb = rel * (dy * g_ref).abs() + 2.0 ** -21 * dy.abs() * (1 + x.abs()) + tiny
    return bf, bb


# ----------------------------------------------------------------------------- dropout
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_MIX1 = np.uint64(0xBF58476D1CE4E5B9)
_MIX2 = np.uint64(0x94D049BB133111EB)
_STEP_MUL = np.uint64(0xD1B54A32D192ED03)


def nsa_seed(salt: int, step: int) -> np.uint64:
    """common.h ``nsa_seed``: the host salt mixed with the device step counter."""
    with np.errstate(over="ignore"):
        return np.uint64(salt) ^ (np.uint64(step) * _STEP_MUL)


def nsa_hash(seed, idx):
    """common.h ``nsa_hash`` on a uint64 index array: the top 32 bits of splitmix64's output for
    state ``seed + idx * golden``."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (idx + np.uint64(1)) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _MIX1
        z = (z ^ (z >> np.uint64(27))) * _MIX2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def nsa_drop_thresh(p) -> int:
    """common.h ``nsa_drop_thresh`` of the fp32 probability the entry point receives."""
    t = float(np.float32(p)) * 4294967296.0
    if t >= 4294967295.0:
        return 0xFFFFFFFF
    if t <= 0.0:
        return 0
    return int(t)


def nsa_keep(seed, idx, thresh: int):
    return nsa_hash(seed, idx) >= np.uint32(thresh)


def dropout_scale(p) -> np.float32:
    """``1 / (1 - p)`` in fp32 as ``nsa_dropout`` forms it (0 for p = 1)."""
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p) if p < 1 else np.float32(0.0)


def dropout_ref(x, p, salt, step):
    """Bit-exact ``nsa_dropout``: where(keep, (x.float() * scale).to(dtype), 0), ``keep`` from
    the hash at the flat element index."""
    keep = torch.from_numpy(nsa_keep(nsa_seed(salt, step), np.arange(x.numel(), dtype=np.uint64),
                                     nsa_drop_thresh(p))).to(x.device)
    y = (x.float() * float(dropout_scale(p))).to(x.dtype)
    return torch.where(keep, y, torch.zeros_like(y))


# ----------------------------------------------------------------------- cast specials
def cast_specials() -> torch.Tensor:
    """fp32 values at which a conversion to bf16 / fp16 can go wrong: signed zeros, fp32
    denormals, exact ties in both directions, the largest value that stays finite and the first
    that rounds to inf for each type, fp16 subnormal results, 2^-25 (the tie to zero), infs, NaN."""
    bits = [
        0x00000000, 0x80000000,              # +-0
        0x00000001, 0x80000001, 0x007FFFFF,  # fp32 denormals: smallest, largest
        0x00400000, 0x00018000,              # denormals that are bf16 denormals / ties
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # bf16 ties: down to even, up to even
        0x3F808001, 0x3F807FFF,              # one ulp either side of a bf16 tie
        0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000,  # fp16 ties (1 + 2^-11, 1 + 3 * 2^-11)
        0x3F801001, 0x3F800FFF,              # one ulp either side of an fp16 tie
        0x7F7F7FFF, 0x7F7F8000, 0xFF7F7FFF, 0xFF7F8000,  # bf16: last finite, first inf
        0x7F7FFFFF, 0xFF7FFFFF,              # fp32 max
        0x477FE000, 0x477FEFFF, 0x477FF000, 0xC77FEFFF, 0xC77FF000,  # fp16: 65504, < 65520, 65520
        0x47800000, 0x7E967699,              # beyond the fp16 range
        0x38800000, 0x387FC000, 0x387FE000,  # 2^-14 and just below: the fp16 normal / subnormal edge
        0x35800000, 0x33800000, 0x33C00000, 0x34200000,  # 2^-20, 2^-24, 1.5 * 2^-24 (tie), 2.5 * 2^-24 (tie)
        0x33000000, 0xB3000000, 0x33000001, 0x32FFFFFF, 0x32800000,  # 2^-25: tie to zero, either side
        0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,  # infs, NaNs
    ]
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def same_bits_or_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    """16-bit tensors equal bit for bit (the sign of zero included), NaN matching any NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    ia, ib = a.view(torch.int16), b.view(torch.int16)
    return bool(torch.equal(ia[~na], ib[~nb]))


# ===================================================================== CPU checks of the above
def test_hash_replica_is_splitmix64():
    # splitmix64's first output for state 0 is 0xE220A8397B1DCDAF
    assert int(nsa_hash(0, [0])[0]) == 0xE220A839
    assert int(nsa_hash(nsa_seed(0, 0), np.arange(3))[0]) == 0xE220A839
    # second output of the same stream (state 2 * golden): 0x6E789E6AA1B965F4
    assert int(nsa_hash(0, [1])[0]) == 0x6E789E6A
    # the step counter moves the seed, salt 0 and step 0 leave it 0
    assert int(nsa_seed(0, 0)) == 0 and int(nsa_seed(5, 0)) == 5
    assert int(nsa_seed(0, 3)) == (3 * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    assert int(nsa_seed(1 << 61, 1)) == (1 << 61) ^ 0xD1B54A32D192ED03


def test_drop_thresh_and_keep():
    assert nsa_drop_thresh(0.0) == 0
    assert nsa_drop_thresh(1.0) == 0xFFFFFFFF
    # float32(0.2) = 13421773 * 2^-26, times 2^32
    assert nsa_drop_thresh(np.float32(0.2)) == 13421773 * 64 == 858993472
    assert nsa_drop_thresh(0.5) == 1 << 31
    idx = np.arange(1 << 16, dtype=np.uint64)
    assert nsa_keep(7, idx, 0).all()
    h = nsa_hash(7, idx)
    for p in (0.2, 0.5):
        keep = nsa_keep(7, idx, nsa_drop_thresh(p))
        assert np.array_equal(keep, h.astype(np.float64) >= float(np.float32(p)) * 2.0 ** 32)
        assert abs(keep.mean() - (1 - p)) < 4 * math.sqrt(p * (1 - p) / idx.size)
    assert float(dropout_scale(0.2)) == 1.25 and float(dropout_scale(0.5)) == 2.0
    assert float(dropout_scale(0.0)) == 1.0 and float(dropout_scale(1.0)) == 0.0


def test_dropout_ref_edges():
    x = torch.randn(1000).to(torch.bfloat16)
    assert torch.equal(dropout_ref(x, 0.0, 11, 0).view(torch.int16), x.view(torch.int16))
    assert torch.equal(dropout_ref(x, 1.0, 11, 0).view(torch.int16), torch.zeros(1000, dtype=torch.int16))
    y = dropout_ref(x, 0.5, 11, 2)
    kept = y != 0
    assert torch.equal(y[kept].float(), x[kept].float() * 2)
    assert not torch.equal(y, dropout_ref(x, 0.5, 11, 3)) and not torch.equal(y, dropout_ref(x, 0.5, 12, 2))


def test_finite_patterns_count():
    assert finite_patterns(torch.bfloat16).numel() == 65280
    assert finite_patterns(torch.float16).numel() == 63488


def test_gelu_ref_matches_torch_and_bounds_hold_for_fp32_formula():
    """The float64 reference against torch's fp64 GELU and autograd; and the bounds the GPU
    test asserts hold, before the output rounding, for an fp32 evaluation of the kernel's
    Abramowitz-Stegun 7.1.26 formula over every finite bf16 and fp16 input."""
    for dtype in (torch.bfloat16, torch.float16):
        x16 = finite_patterns(dtype)
        x = x16.to(F64).requires_grad_(True)
        y = torch.nn.functional.gelu(x)
        y.sum().backward()
        yr, gr = gelu_ref(x16)
        # torch forms Phi as 0.5 (1 + erf): absolute error of one double rounding of 1 in the left tail
        xa = x.detach().abs()
        assert ((yr - y.detach()).abs() <= 1e-12 * yr.abs() + 2.0 ** -52 * xa).all()
        assert ((gr - x.grad).abs() <= 1e-12 * gr.abs() + 2.0 ** -52 * (1 + xa)).all()
        xf = x16.float()
        z = xf.abs() * 0.70710678118654752
        t = 1.0 / (1.0 + 0.3275911 * z)
        poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
        e = torch.exp(-z * z)
        erf = torch.where(xf < 0, -(1.0 - poly * e), 1.0 - poly * e)
        cdf = 0.5 * (1.0 + erf)
        dy = torch.full_like(xf, -0.37).to(dtype)
        bf, bb = gelu_bounds(x16, dy, yr, gr, dtype)
        rel = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
        # the value terms of the bounds are the output rounding's: left out here
        assert ((xf * cdf).to(F64) - yr).abs().le(bf - rel * yr.abs()).all()
        gk = dy.float() * (cdf + xf * (e * 0.39894228040143268))
        assert (gk.to(F64) - dy.to(F64) * gr).abs().le(bb - rel * (dy.to(F64) * gr).abs()).all()


def test_adamw_ref_matches_torch_adamw():
    """Three float64 reference steps from zero state equal torch.optim.AdamW in float64
    (fp32-exact hyperparameters, so the fp32-formed scalars are the doubles torch uses)."""
    torch.manual_seed(0)
    n = 256
    lr, b1, b2, eps, wd = 0.5, 0.75, 0.875, 2.0 ** -20, 0.25
    p0 = torch.randn(n)
    w = torch.nn.Parameter(p0.to(F64).clone())
    opt = torch.optim.AdamW([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.to(F64), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    mask = torch.ones(n // 64, dtype=torch.uint8)
    for t in (1, 2, 3):
        g = torch.randn(n)
        w.grad = g.to(F64)
        opt.step()
        sc = adamw_scalars(lr, b1, b2, eps, wd, t)
        p, m, v, ep, em = adamw_ref(p, g, m, v, mask, 1.0, sc)
        rt = 2.0 ** -22  # bc1 and bc2_sqrt are rounded to fp32
        assert torch.allclose(p, w.detach(), rtol=rt, atol=rt)
        assert (ep >= 0).all() and (em >= 0).all()
    # no decay where the chunk's flag is 0; coef scales the gradient
    sc = adamw_scalars(lr, b1, b2, eps, wd, 1)
    z = torch.zeros(n)
    mask[1] = 0
    p1, _, _, _, _ = adamw_ref(p0, z, z, z, mask, 1.0, sc)
    assert torch.equal(p1[64:128], p0[64:128].to(F64)) and torch.equal(p1[:64], p0[:64].to(F64) * 0.875)
    a = adamw_ref(p0, g * 0.25, z, z, mask, 1.0, sc)
    b = adamw_ref(p0, g, z, z, mask, 0.25, sc)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_adamw_bounds_hold_for_fp32_formula():
    """The per-element bounds of the GPU test (2^-20 times the terms' magnitudes) hold for a
    torch fp32 evaluation of the same step from states spread over several decades."""
    torch.manual_seed(1)
    n = 1 << 16
    spread = lambda: torch.randn(n) * torch.exp(3 * torch.randn(n))  # noqa: E731
    p, g, m, v = spread(), spread(), spread(), spread().abs()
    mask = (torch.rand(n // 64) < 0.5).to(torch.uint8)
    for t in (1, 7, 1000):
        for coef in (1.0, f32(0.125 * 0.37)):
            sc = adamw_scalars(1e-3, 0.9, 0.95, 1e-8, 0.1, t)
            pr, mr, vr, ep, em = adamw_ref(p, g, m, v, mask, coef, sc)
            F = lambda k: torch.tensor(sc[k], dtype=torch.float32)  # noqa: E731
            gj = g * torch.tensor(coef, dtype=torch.float32)
            m1 = F("b1") * m + F("omb1") * gj
            v1 = F("b2") * v + F("omb2") * gj * gj
            d = torch.where(mask.repeat_interleave(64).bool(), F("decay"), torch.tensor(1.0))
            p1 = p * d - F("step") * m1 / (v1.sqrt() * F("inv_bc2") + F("eps"))
            assert ((p1.to(F64) - pr).abs() <= 2.0 ** -20 * ep + 2.0 ** -126).all()
            assert ((m1.to(F64) - mr).abs() <= 2.0 ** -20 * em).all()
            assert ((v1.to(F64) - vr).abs() <= 2.0 ** -20 * vr).all()


def test_cast_specials_cover_the_edges():
    s = cast_specials()
    b, h = s.to(torch.bfloat16), s.to(torch.float16)
    one = s.view(torch.int32)
    at = lambda bits: int((one == (bits - (1 << 32) if bits >= 1 << 31 else bits)).nonzero()[0])  # noqa: E731
    assert b[at(0x3F808000)].item() == 1.0 and b[at(0x3F818000)].item() == 1.015625  # ties to even
    assert b[at(0x7F7F7FFF)].view(torch.int16).item() == 0x7F7F and torch.isinf(b[at(0x7F7F8000)])
    assert h[at(0x477FEFFF)].item() == 65504.0 and torch.isinf(h[at(0x477FF000)])
    assert h[at(0x3F801000)].item() == 1.0 and h[at(0x3F803000)].item() == 1 + 2.0 ** -9
    assert h[at(0x33000000)].item() == 0.0 and h[at(0x33000001)].item() == 2.0 ** -24
    assert h[at(0x33C00000)].item() == 2.0 ** -23 and h[at(0x34200000)].item() == 2.0 ** -23
    assert torch.isnan(b[at(0x7F800001)]) and torch.isnan(h[at(0x7FC00000)])
    assert same_bits_or_nan(b, b.clone()) and not same_bits_or_nan(b, -b)
    z = torch.zeros(2).to(torch.bfloat16)
    assert not same_bits_or_nan(z, -z)
