"""High-precision references for the cross-entropy kernels (``xent.hip`` and the small kernels
of ``xent_fused.hip``), as plain functions that run on any device, with their own CPU checks.

``test_xent_gpu.py`` compares the HIP kernels with these element by element.  Every fp32 term of
a bound is ``k * 2^-24 * scale`` (u = 2^-24 is the largest relative error of one fp32 rounding),
``k`` counting the roundings on the longest path to the value.

The separate pass (``nsa_xent_fwd``), x = l - M, E = exp(x), S = sum E, p = E / S:

  exp     ``__expf(x)`` is exp2(x * log2(e)): the product's rounding moves the exponent by
          |x| u and the constant's own error by as much again, v_exp_f32 is good to 1 ulp = 2 u and
          l - M rounds once more: relative (3 + 2 |x|) u, and 2^-126 absolute (flushed denormals).
  S       w_exp = sum E (3 + 2 |x|) / S for its terms, and k_sum for the adds (``xent_k_sum``):
            register kernels RB x RC   4 ceil(ld / 8 RB) adds of pair sums in a thread, the pair
                                       sum, 6 butterfly steps, RB / 64 waves:  4 nc + 6 + RB / 64
            streaming kernel           per 8-column chunk 8 adds and an online merge (exp 3,
                                       multiply, add); 6 + 3 merges over lanes and waves: 13 nc + 45
                                       (the merges' exponents add up to x: the 2 |x| u is w_exp's)
            scalar kernel              one merge per element:  5 ceil(V / 256) + 45
  loss    M and l_t are exact.  log S: S's error (k_sum + w_exp) u, ``__logf`` 4 u |log S|
          (v_log_f32 1 ulp and the multiply by ln 2); M + log S and - l_t round once each:
            u (k_sum + w_exp + 4 |log S| + |lse| + |loss|)
  grad    p = exp * (1 / S): the exp, S's error, the division and the multiply:
            p u (6 + 2 |x| + k_sum + w_exp), plus u on the target column (the rounding of p - 1,
            absolute because p_t - 1 cancels), plus half an ulp of the 16-bit type at the reference.
          Padding columns, invalid rows and their loss are exactly zero.

The fused helpers:

  tlogit  a lane's 8 ceil(C / 512) fused multiply-adds, 6 butterfly steps, + shift:
            (8 ceil(C / 512) + 7) u (sum |x W_t| + |shift|); exactly shift on an invalid row
  combine slots // 8 + slots % 8 + 3 adds of non-negative partials: k_c u S on S;
            loss u (k_c + 4 |log S| + |loss|), 1 / S relative (k_c + 1) u
  fixup   logits by C sequential fused multiply-adds: d_v = C u sum_c |x_c W_vc| each, d = max d_v
          for the maximum; E relative 2 d + (3 + 2 |x|) u plus the store's half ulp; S relative
          its terms' weighted mean of that plus (ceil(Vpad / 256) + 9) u; loss
            2 d + S's error + u (4 |log S| + |lse| + |loss|)
  prep    bit-exact: sc = fp32(g * invS), one multiply, round to nearest even
  dW fix  per row E_t (p - round16(p)) - g x: 3 roundings, then one add per row of the segment
          into the running row of gW: (n_seg + 3 + extra) u (|gW| + sum |terms|), extra = 2 for
          the atomic and sorted forms and G / 4 + 4 for the LDS form's G partial tables

The constants above cannot all be read off the code (the transcendental instructions, the
contraction of a * b + c).  ``xent_fp32_model`` and the ``*_model`` functions follow the
kernels' order of operations in fp32 (exp and log through exp2 / log2 with the rounded
constant), and the CPU tests below hold them to half of every bound at every shape the GPU file
runs; the mutation tests show that a subtly wrong kernel leaves the bounds.  Worst
error / bound the kernels reached on an MI355X (``test_xent_gpu.py``, all cases, bf16 and fp16):

  separate pass (bf16 / fp16)                 loss              grad
    plain 1024 x 7 (variant 0 small, 6)      0.766 / 0.742    0.9990 / 1.0000
    nontemporal loads + stores (3)           0.766 / 0.699    0.9987 / 1.0000
    nontemporal stores (4)                   0.766 / 0.555    0.9988 / 1.0000
    nontemporal loads (5)                    0.766 / 0.550    0.9990 / 1.0000
    the default at 256 MiB (bf16 only)       0.148            0.9989
    256 x 25 (1)                             0.752 / 0.629    0.9974 / 1.0000
    512 x 13 (2)                             0.549 / 0.736    0.9993 / 1.0000
    streaming                                0.311 / 0.310    0.9927 / 0.9999
    scalar                                   0.667 / 0.593    0.9983 / 0.9998
  tlogit crow 0.050 / 0.105    combine loss 0.390, 1 / S 0.450
  fixup E 0.9986 / 0.9979, loss 0.064 / 0.110, 1 / S 0.068 / 0.091
  dW fix gW: atomics 0.408 / 0.407, sorted 0.408 / 0.407, LDS 0.252 / 0.310

Above 0.5: the gradient and the fix-up's E sit on the half ulp of their 16-bit store, which a
rounding reaches (1.0000 is to four places: the assertion is <= 1; an fp32 p that is an exact
fp16 tie gives half an ulp plus p's own error).  The loss sits on its two final roundings,
u (|lse| + |loss|): on the rows offset by 300 one rounding of M + log S is up to u |lse|, and
the rest of the bound is small beside it.  The fix-up's bounds are loose at C = 8192, where
C u sum |x W| is about one.

On the parent of the commit that added this file the scalar kernel left the logits in columns
[V, ld) (ld = V + 3: 3e38 and 65504 found where 0 is required), and the fp16 atomic dW form
reached 62.8 at N = 1100, C = 264: the compiler had fused s * x with the fp16 rounding
(v_fma_mixlo_f16, one rounding of the exact product), which differs from the stored xs where
the fp32 product is an fp16 tie.  Both are fixed in the kernels.
"""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_layernorm_refs import BF, F32, FH, U, half_ulp, worst
from test_streaming_refs import F64

I64 = torch.int64
TINY = 2.0 ** -126
LOG2E = np.float32(1.4426950408889634)
LN2 = np.float32(0.6931471805599453)

# row patterns of the separate pass; the last five are the invalid targets
PATTERNS = ("gauss", "confident", "constant", "offset+", "offset-", "spread", "max_last", "tgt_first", "tgt_last",
            "tgt_alone", "inv-1", "inv-100", "invV", "inv_ld-1", "inv2^40")
FILLS = ("zero", "big", "nan")
# target kinds of the fused helpers: 7, coprime with the 4 wave slots of a block
TARGET_KINDS = ("random", "-1", "first", "last", "-100", "V", "2^40")

# every (variant, V, ld) the GPU file runs through nsa_xent_fwd(_h), and the branch it reaches
FWD_CASES = [
    # the default at small size: 1024 x 7 plain
    (0, 8, 8), (0, 7, 8), (0, 1, 8), (0, 8192, 8192), (0, 8191, 8192), (0, 8200, 8200), (0, 50257, 50304),
    (0, 50304, 50304), (0, 57344, 57344), (0, 57343, 57344), (0, 65, 256),
    # 256 x 25 up to 51200, 512 x 13 up to 53248; beyond them the default again
    (1, 8, 8), (1, 50257, 50304), (1, 51200, 51200), (1, 51199, 51208), (2, 65, 256), (2, 50257, 50304),
    (2, 53248, 53248), (2, 53255, 53256),
    # 1024 x 7: nontemporal loads and stores (the production instantiation), stores, loads, plain
    *[(v, V, ld) for v in (3, 4, 5, 6) for V, ld in ((7, 8), (8200, 8200), (50257, 50304), (57343, 57344))],
    # the streaming kernel (ld > 57344)
    (0, 57352, 57352), (0, 57351, 57352), (0, 57600, 57600), (0, 57599, 57600), (0, 65, 57600), (3, 65, 57600),
    # the scalar kernel (ld % 8 != 0)
    (0, 65, 65), (0, 1003, 1003), (0, 65, 68), (0, 1003, 1006), (1, 1003, 1006),
]


def xent_branch(variant, ld, nbytes=0):
    """The kernel ``xent_entry`` launches: (name, threads per row or 0)."""
    if ld % 8:
        return "scalar", 0
    if ld > 57344:
        return "stream", 0
    if 3 <= variant <= 5:
        return ("nt_ls", "nt_s", "nt_l")[variant - 3], 1024
    if variant == 1 and ld <= 51200:
        return "reg256", 256
    if variant == 2 and ld <= 53248:
        return "reg512", 512
    return ("plain", 1024) if variant == 6 or nbytes < (256 << 20) else ("nt_ls", 1024)


def xent_k_sum(variant, V, ld):
    name, rb = xent_branch(variant, ld)
    if name == "scalar":
        return 5 * -(-V // 256) + 45
    if name == "stream":
        return 13 * -(-ld // 2048) + 45
    return 4 * -(-ld // (8 * rb)) + 6 + rb // 64


# ------------------------------------------------------------------------------ inputs
def fill_value(fill, dtype):
    return {"zero": 0.0, "big": 3e38 if dtype == BF else 65504.0, "nan": float("nan")}[fill]


def xent_rows(N, V, ld, seed, dtype, fill="zero", first=0):
    """[N, ld] logits (CPU, ``dtype``), int64 targets and the pattern name of every row: row r
    has pattern (first + r) mod 15, so ``first`` in range(0, 15, N) shows every pattern to the
    one row slot of a block.  Columns [V, ld) hold the padding fill."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.full((N, ld), fill_value(fill, dtype), dtype=F64)
    tg = torch.empty(N, dtype=I64)
    names = []
    for r in range(N):
        p = PATTERNS[(first + r) % len(PATTERNS)]
        names.append(p)
        z = (2 * torch.randn(V, generator=g, dtype=F64)).to(dtype).to(F64)
        t = int(torch.randint(0, V, (1,), generator=g))
        if p == "confident" and V > 1:  # p_t = 0.999
            z[t] = -math.inf
            z[t] = torch.logsumexp(z, 0) + math.log(999.0)
        elif p == "constant":  # loss = log V
            z[:] = 1.5
        elif p in ("offset+", "offset-"):  # shift invariance
            z += 300.0 if p == "offset+" else -300.0
        elif p == "spread" and V > 1:  # 200 nats, the target at the bottom: p_t underflows to 0
            z = -200.0 * torch.randperm(V, generator=g).to(F64) / (V - 1)
            t = int(z.argmin())
        elif p == "max_last":
            z[V - 1] = z.max() + 4.0
        elif p == "tgt_first":
            t = 0
        elif p == "tgt_last":
            t = V - 1
        elif p == "tgt_alone":  # first column of the last 8-column chunk (alone in it when V % 8 == 1)
            t = 8 * ((V - 1) // 8)
        elif p.startswith("inv"):
            t = {"inv-1": -1, "inv-100": -100, "invV": V, "inv_ld-1": ld - 1, "inv2^40": 2 ** 40}[p]
        lg[r, :V] = z
        tg[r] = t
    return lg.to(dtype), tg, names


def fused_inputs(M, C, V, Vp, seed, dtype, first=0, ldx=None):
    """x [M, ldx] (columns >= C are NaN: never read), W [Vp, C] and int64 targets whose kind is
    (first + r) mod 7; ``first`` in range(7) shows every kind to every wave slot r mod 4."""
    g = torch.Generator().manual_seed(seed)
    ldx = ldx or C
    x = torch.full((M, ldx), float("nan"))
    x[:, :C] = torch.randn(M, C, generator=g)
    x[:, C // 2] = 0.0
    W = torch.randn(Vp, C, generator=g) * (2.0 / math.sqrt(C))
    tg = torch.randint(0, V, (M,), generator=g)
    kinds = [TARGET_KINDS[(first + r) % 7] for r in range(M)]
    for r, k in enumerate(kinds):
        if k != "random":
            tg[r] = {"-1": -1, "first": 0, "last": V - 1, "-100": -100, "V": V, "2^40": 2 ** 40}[k]
    return x.to(dtype), W.to(dtype), tg, kinds


# -------------------------------------------------------------------------- references
def xent_fwd_ref(logits, targets, V):
    """The separate pass in float64 from the 16-bit logits: lse, loss = lse - l_t and
    p - onehot over the columns < V; padding columns and invalid rows (t outside [0, V)) are
    zero.  Also x = l - M, p, S, M, l_t and w_exp (module docstring)."""
    N, ld = logits.shape
    l = logits[:, :V].to(F64)
    M = l.max(-1).values
    x = l - M[:, None]
    E = x.exp()
    S = E.sum(-1)
    valid = (targets >= 0) & (targets < V)
    t = torch.where(valid, targets, 0)
    lt = l.gather(1, t[:, None])[:, 0]
    lse = M + S.log()
    p = E / S[:, None]
    onehot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    grad = torch.zeros(N, ld, dtype=F64, device=logits.device)
    grad[:, :V] = (p - onehot) * valid[:, None]
    loss = torch.where(valid, lse - lt, 0.0)
    w_exp = (E * (3 + 2 * x.abs())).sum(-1) / S
    return SimpleNamespace(loss=loss, grad=grad, valid=valid, t=t, x=x, p=p, S=S, M=M, lt=lt, lse=lse, w_exp=w_exp,
                           onehot=onehot, V=V)


def xent_fwd_bounds(r, dtype, k_sum):
    """Bounds of a separate-pass reference (module docstring): the loss's, the fp32 part of the
    gradient's, the half ulp of the gradient's 16-bit store, and the part of the loss's bound that
    is the two final roundings (M + log S and - l_t: like the store's half ulp, one rounding
    reaches it)."""
    rel_s = k_sum + r.w_exp
    rnd = U * (r.lse.abs() + r.loss.abs()) * r.valid
    b_loss = U * (rel_s + 4 * r.S.log().abs()) * r.valid + rnd
    b = torch.zeros_like(r.grad)
    b[:, :r.V] = (r.p * U * (6 + 2 * r.x.abs() + rel_s[:, None]) + r.onehot * U + TINY) * r.valid[:, None]
    return b_loss, b, half_ulp(r.grad, dtype) * (r.grad != 0), rnd


def tlogit_ref(x, W, tgt, C, V, shift):
    """c_r = x_r . W[t_r] + shift (shift alone on an invalid row), its scale, and t32."""
    valid = (tgt >= 0) & (tgt < V)
    t = torch.where(valid, tgt, 0)
    prod = x[:, :C].to(F64) * W[t, :C].to(F64) * valid[:, None]
    t32 = torch.where(valid, tgt, -1).to(torch.int32)
    return SimpleNamespace(crow=prod.sum(-1) + shift, scale=prod.abs().sum(-1) + abs(shift) * valid, t32=t32,
                           k=8 * -(-C // 512) + 7)


def combine_ref(part, t32, lo, hi, shift):
    """S (float64 sum of the [slots, M] partials), log S + shift and 1 / S on the kept rows (0 on
    flagged and ignored ones), and the flag of every row: S outside [lo, hi] (NaN included), an
    ignored row only when not S <= hi."""
    slots = part.shape[0]
    S = part.to(F64).sum(0)
    ign = t32 < 0
    flag = torch.where(ign, ~(S <= hi), ~((S >= lo) & (S <= hi)))
    keep = ~flag & ~ign
    Sk = torch.where(keep, S, 1.0)
    loss = torch.where(keep, Sk.log() + shift, 0.0)
    inv = torch.where(keep, 1.0 / Sk, 0.0)
    k = slots // 8 + slots % 8 + 3
    b_loss = U * (k + 4 * Sk.log().abs() + loss.abs()) * keep
    return SimpleNamespace(S=S, flag=flag, keep=keep, loss=loss, invS=inv, b_loss=b_loss, b_inv=(k + 1) * U * inv)


def fixup_ref(x, W, t32, rows, C, V, Vpad, dtype):
    """The exact recompute of the listed rows: E [len(rows), Vpad] (zero padding; all zero on
    an ignored row), loss, 1 / S and their bounds.  The kernel leaves loss and 1 / S of an ignored
    row as nsa_xent_combine wrote them, 0; that is what stands here, with a zero bound."""
    xr = x[rows][:, :C].to(F64)
    Wd = W[:V, :C].to(F64)
    l = xr @ Wd.T
    d = (C * U * (xr.abs() @ Wd.abs().T)).max(-1).values
    m = l.max(-1).values
    z = l - m[:, None]
    ign = t32[rows] < 0
    keep = ~ign
    t = torch.where(ign, 0, t32[rows]).to(I64)
    E = torch.zeros(len(rows), Vpad, dtype=F64, device=x.device)
    E[:, :V] = z.exp() * keep[:, None]
    S = z.exp().sum(-1)
    lt = l.gather(1, t[:, None])[:, 0]
    lse = m + S.log()
    loss = torch.where(ign, 0.0, lse - lt)
    rel = 2 * d[:, None] + (3 + 2 * z.abs()) * U
    b_E = torch.zeros_like(E)
    b_E[:, :V] = (z.exp() * rel + TINY) * keep[:, None]
    rel_s = (z.exp() * rel).sum(-1) / S + (-(-Vpad // 256) + 9) * U
    b_loss = (2 * d + rel_s + U * (4 * S.log().abs() + lse.abs() + loss.abs())) * keep
    return SimpleNamespace(E=E, loss=loss, invS=keep / S, b_E=b_E, hu_E=half_ulp(E, dtype) * (E != 0), b_loss=b_loss,
                           b_inv=(rel_s + U) / S * keep, ign=ign)


def bwd_prep_ref(x, W, t32, invS, g, C):
    """coef [M, 2], wrows and xs of the backward prologue as an fp32 replica, bit for bit:
    sc = fp32(g * invS); coef = (sc, g or 0 on an ignored row); wrows = W[t] (W[0] on an ignored
    row); xs = round16(fp32(x * sc))."""
    gt = torch.tensor(g, dtype=F32, device=x.device)
    sc = gt * invS
    coef = torch.stack([sc, torch.where(t32 < 0, torch.zeros_like(sc), gt.expand_as(sc))], 1)
    wrows = W[t32.clamp(min=0).to(I64), :C]
    return coef, wrows, (x[:, :C].float() * sc[:, None]).to(x.dtype)


def dw_fix_ref(x, E, t32, invS, g, V, C, gw0, extra=2):
    """The onehot dW term added to ``gw0`` [V, C] in float64: per valid row r with target v,
    E_rt (p - round16(p)) - g x_r with s = fp32(g invS) and p = fp32(s x) formed in fp32 as the
    kernel forms them, so the rounding that is subtracted is the same one.  Returns the sum, its
    bound and the mask of the vocabulary rows that have a target."""
    gt = torch.tensor(g, dtype=F32, device=x.device)
    valid = t32 >= 0
    t = t32.clamp(min=0).to(I64)
    xf = x[:, :C].float()
    p = (gt * invS)[:, None] * xf
    et = E.to(F64).gather(1, t[:, None])
    a = et * (p.to(F64) - p.to(x.dtype).to(F64)) * valid[:, None]
    b = float(gt) * xf.to(F64) * valid[:, None]
    z = lambda: torch.zeros(V, C, dtype=F64, device=x.device)  # noqa: E731
    term = z().index_add_(0, t, a - b)
    scale = z().index_add_(0, t, a.abs() + b.abs()) + gw0.to(F64).abs()
    n_seg = torch.zeros(V, dtype=F64, device=x.device).index_add_(0, t, valid.to(F64))
    return SimpleNamespace(gw=gw0.to(F64) + term, bound=(n_seg[:, None] + 3 + extra) * U * scale + TINY, hit=n_seg > 0)


# ------------------------------------------------------- fp32 models of the kernels' order
def _np(t):
    return t.detach().cpu().float().numpy()


def _expf(x):
    """``__expf``: exp2 of the fp32 product with the rounded log2(e), denormal results flushed."""
    with np.errstate(all="ignore"):
        y = np.exp2((x.astype(np.float32) * LOG2E).astype(np.float64)).astype(np.float32)
    return np.where(np.abs(y) < TINY, np.float32(0), y)


def _logf(x):
    with np.errstate(all="ignore"):
        return np.log2(x.astype(np.float64)).astype(np.float32) * LN2


def _butterfly(v, op):
    """xor butterfly over the last axis (64 lanes)."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lane ^ o])
    return v[..., 0]


def _merge(m, s, m2, s2, guard=False):
    """``online_merge`` on arrays; ``guard``: the wave reduction's skip of an empty partner."""
    with np.errstate(all="ignore"):
        gt = m2 > m
        sn = np.where(gt, s * _expf(m - m2) + s2, s + s2 * _expf(m2 - m)).astype(np.float32)
    mn = np.where(gt, m2, m)
    if guard:
        skip = np.isneginf(m2)
        return np.where(skip, m, mn), np.where(skip, s, sn)
    return mn, sn


def _stats_reg(l, in_max, in_sum, rb):
    """(M, S) of ``xent_reg_kernel``: l and the masks of the columns that take part in the
    maximum and in the sum, [N, nc, rb, 8] (thread t holds chunks t + c rb)."""
    with np.errstate(all="ignore"):
        M = np.where(in_max, l, np.float32(-np.inf)).max((1, 2, 3))
        e = _expf(l - M[:, None, None, None])
    e = np.where(in_sum, e, np.float32(0))
    s = np.zeros((l.shape[0], rb), np.float32)
    for c in range(l.shape[1]):
        for q in range(4):
            s = s + (e[:, c, :, 2 * q] + e[:, c, :, 2 * q + 1])
    w = _butterfly(s.reshape(-1, rb // 64, 64), np.add)
    S = w[:, 0]
    for k in range(1, rb // 64):
        S = S + w[:, k]
    return M, S


def _stats_stream(l, real, scalar):
    """(M, S) of ``xent_kernel``: thread t merges its chunks (or, scalar, its elements) online,
    then the guarded butterfly of merges and the four waves in order."""
    N, nc = l.shape[:2]
    ninf = np.float32(-np.inf)
    m = np.full((N, 256), ninf)
    s = np.zeros((N, 256), np.float32)
    for c in range(nc):
        if scalar:
            ok = real[:, c, :, 0]
            m2, s2 = _merge(m, s, l[:, c, :, 0], np.float32(1))
        else:
            f = np.where(real[:, c], l[:, c], ninf)
            bm = f.max(-1)
            ok = ~np.isneginf(bm)
            with np.errstate(all="ignore"):
                e = _expf(f - bm[..., None])
            bs = np.zeros_like(bm)
            for j in range(8):
                bs = bs + e[..., j]
            m2, s2 = _merge(m, s, bm, bs)
        m, s = np.where(ok, m2, m), np.where(ok, s2, s)
    m, s = m.reshape(N, 4, 64), s.reshape(N, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        m, s = _merge(m, s, m[..., lane ^ o], s[..., lane ^ o], guard=True)
    M, S = m[:, 0, 0], s[:, 0, 0]
    for w in range(1, 4):
        M, S = _merge(M, S, m[:, w, 0], s[:, w, 0])
    return M, S


def xent_fp32_model(logits, targets, V, variant=0, write_grad=1, mut=None):
    """numpy fp32 emulation of the kernel ``xent_entry`` picks for (variant, ld): (loss fp32,
    the logits buffer afterwards).  ``mut`` names a deliberate mistake (the mutation tests)."""
    dtype = logits.dtype
    N, ld = logits.shape
    name, rb = xent_branch(variant, ld)
    per = 1 if name == "scalar" else 8
    rb = rb or 256
    nc = -(-ld // (per * rb))
    l = np.full((N, nc * rb * per), np.float32(0))
    l[:, :ld] = _np(logits)
    shape = (N, nc, rb, per)

    def cols(n):  # mask of the columns < n in the threads' layout
        m = np.zeros(nc * rb * per, bool)
        m[:n] = True
        return np.broadcast_to(m.reshape(shape[1:]), shape)

    l, real, leak = l.reshape(shape), cols(V), cols(min(V + 1, ld))  # leak: one padding column more
    if name in ("scalar", "stream"):
        M, S = _stats_stream(l, real, name == "scalar")
    else:
        M, S = _stats_reg(l, leak if mut == "pad_in_max" else real, leak if mut == "pad_in_S" else real, rb)
    tg = targets.cpu().numpy()
    valid = (tg >= 0) & (tg < V)
    t = np.where(valid, tg, 0)
    rows = np.arange(N)
    lt = _np(logits)[rows, t]
    loss = np.where(valid, (M + _logf(S)) - lt, np.float32(0)).astype(np.float32)
    if mut == "invalid_not_zeroed":
        loss = ((M + _logf(S)) - lt).astype(np.float32)
        valid = np.ones_like(valid)
    if not write_grad:
        return torch.from_numpy(loss), logits.clone()
    with np.errstate(all="ignore"):
        inv = np.float32(1) / S
        p = _expf(l - M[:, None, None, None]) * inv[:, None, None, None]
    p = np.where(real, p, np.float32(0)).reshape(N, -1)[:, :ld]
    p = np.where(valid[:, None], p, np.float32(0))
    tcol = t if mut != "onehot_off" else np.minimum(t + 1, V - 1)
    p[rows, tcol] -= valid.astype(np.float32)
    return torch.from_numpy(loss), torch.from_numpy(np.ascontiguousarray(p)).to(dtype)


def tlogit_model(x, W, tgt, C, V, shift, mut=None):
    """``xent_tlogit_kernel`` in fp32: lane l chains columns 8 l + 512 k .. + 8, then the butterfly."""
    valid = (tgt >= 0) & (tgt < V)
    t = torch.where(valid, tgt, 0)
    n = -(-C // 512) * 512
    a = np.zeros((x.shape[0], n), np.float32)
    b = np.zeros_like(a)
    a[:, :C], b[:, :C] = _np(x[:, :C]), _np(W[t, :C])
    a, b = a.reshape(-1, n // 512, 64, 8), b.reshape(-1, n // 512, 64, 8)
    s = np.zeros((x.shape[0], 64), np.float64)
    for k in range(n // 512):
        for j in range(8):
            s = (a[:, k, :, j].astype(np.float64) * b[:, k, :, j] + s).astype(np.float32).astype(np.float64)
    s = _butterfly(s.astype(np.float32), np.add) * valid.numpy()
    out = s + np.float32(shift)
    if mut == "before_shift":
        out = np.where(valid.numpy(), s, out)
    return torch.from_numpy(out.astype(np.float32))


def combine_model(part, t32, lo, hi, shift, mut=None):
    """``xent_combine_kernel`` in fp32: 8 accumulators over the slots, the tail on the first,
    a pairwise tree; (loss, invS, flags)."""
    p = _np(part)
    slots, M = p.shape
    acc = np.zeros((8, M), np.float32)
    k = 0
    with np.errstate(all="ignore"):
        while k + 8 <= slots:
            acc = acc + p[k:k + 8]
            k += 8
        for k in range(k, slots):
            acc[0] = acc[0] + p[k]
        S = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
        lo, hi = np.float32(lo), np.float32(hi)
        ign = t32.numpy() < 0
        inside = (S > lo if mut == "half_outside" else S >= lo) & (S <= hi)
        flag = np.where(ign, ~(S <= hi), ~inside)
        keep = ~flag & ~ign
        loss = np.where(keep, _logf(S) + np.float32(shift), np.float32(0))
        inv = np.where(keep, np.float32(1) / S, np.float32(0))
    return torch.from_numpy(loss.astype(np.float32)), torch.from_numpy(inv.astype(np.float32)), torch.from_numpy(flag)


def fixup_model(x, W, t32, rows, C, V, Vpad, dtype):
    """``xent_fixup_kernel`` in fp32: logits by C sequential fused multiply-adds, thread t owns
    columns t + 256 k; (E in ``dtype``, loss, invS)."""
    xr, Wn = _np(x[rows][:, :C]).astype(np.float64), _np(W[:V, :C]).astype(np.float64)
    l = np.zeros((len(rows), V))
    for c in range(C):
        l = (xr[:, c:c + 1] * Wn[None, :, c] + l).astype(np.float32).astype(np.float64)
    l = l.astype(np.float32)
    m = l.max(-1)
    n = -(-Vpad // 256) * 256
    e = np.zeros((len(rows), n), np.float32)
    e[:, :V] = _expf(l - m[:, None])
    th = e.reshape(len(rows), -1, 256)
    s = np.zeros((len(rows), 256), np.float32)
    for k in range(th.shape[1]):
        s = s + th[:, k]
    w = _butterfly(s.reshape(-1, 4, 64), np.add)
    S = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    ign = t32[rows].numpy() < 0
    t = np.where(ign, 0, t32[rows].numpy())
    loss = np.where(ign, np.float32(0), (m + _logf(S)) - l[np.arange(len(rows)), t])
    inv = np.where(ign, np.float32(0), np.float32(1) / S)
    E = torch.from_numpy(np.where(ign[:, None], np.float32(0), e[:, :Vpad])).to(dtype)
    return E, torch.from_numpy(loss.astype(np.float32)), torch.from_numpy(inv.astype(np.float32))


def dw_fix_model(x, E, t32, invS, g, V, C, gw0, mut=None):
    """The onehot dW term in fp32, rows added to gW in row order (the sorted form's order; the
    atomic forms add the same terms in another order)."""
    g32 = np.float32(g)
    xf, inv = _np(x[:, :C]), invS.numpy()
    if mut == "inv_neighbor":
        inv = np.roll(inv, 1)
    gw = gw0.numpy().copy()
    Ef = _np(E)
    for r in range(x.shape[0]):
        t = int(t32[r])
        if t < 0:
            continue
        p = (g32 * inv[r]) * xf[r]
        pr = torch.from_numpy(p).to(x.dtype).float().numpy()
        if mut == "fused_rounding":  # one rounding of the exact product (v_fma_mixlo_f16)
            exact = np.float64(g32 * inv[r]) * xf[r].astype(np.float64)
            pr = exact.astype(np.float16).astype(np.float32)  # numpy rounds float64 to half once
        d = Ef[r, t] * (p - pr) if mut != "rounding_kept" else np.float32(0)
        gw[t] = gw[t] + (d - g32 * xf[r])
    return torch.from_numpy(gw)


def dw_inputs(N, C, V, Vp, seed, dtype):
    """Inputs of the three onehot dW forms: x, E = exp(l - c_r) synthesised from the float64
    logits (c_r the target logit plus 0, 0.5 or -0.7 so that E_rt varies), invS = 1 / sum E,
    skewed int32 targets (40% on id 3: one long segment; 10% ignored; the others on even ids
    only, so odd vocabulary rows have no target), g and a non-zero fp32 gW prefill."""
    g = torch.Generator().manual_seed(seed)
    x, W, _, _ = fused_inputs(N, C, V, Vp, seed + 1, dtype)
    u = torch.rand(N, generator=g)
    t32 = (torch.randint(0, V // 2, (N,), generator=g) * 2).to(torch.int32)
    t32[u < 0.4] = 3
    t32[u > 0.9] = -1
    l = 0.5 * (x.to(F64) @ W[:V].to(F64).T)
    c = l.gather(1, t32.clamp(min=0).to(I64)[:, None]) + torch.tensor([0.0, 0.5, -0.7], dtype=F64)[torch.arange(N) % 3, None]
    E = torch.zeros(N, Vp, dtype=F64)
    E[:, :V] = (l - c).exp()
    E = E.to(dtype)
    invS = torch.where(t32 >= 0, 1.0 / E.to(F64).sum(-1), 0.0).float()
    gw0 = (torch.randn(Vp, C, generator=g) * 0.01 + 0.003).float()
    return SimpleNamespace(x=x, W=W, E=E, t32=t32, invS=invS, g=float(np.float32(1.0 / max(1, int((t32 >= 0).sum())))),
                           gw0=gw0)


def combine_inputs(slots, M, seed, first=0):
    """[slots, M] partials and t32 whose rows cycle through 11 kinds of S; the edge values sit
    in one slot, or as two exact halves in two, so that their fp32 sum is exact in any order.
    Returns (part, t32, kinds, lo, hi)."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = 0.5, float(np.float32(1e30))
    f = lambda v: float(np.float32(v))  # noqa: E731
    edge = {"half": 0.5, "below_half": f(np.nextafter(np.float32(0.5), np.float32(0))), "hi": hi,
            "above_hi": f(np.nextafter(np.float32(1e30), np.float32(np.inf))), "inf": math.inf, "nan": math.nan,
            "ign_inf": math.inf, "ign_nan": math.nan, "ign_above": 2 * hi}
    kinds = ("generic", "half", "below_half", "hi", "above_hi", "inf", "nan", "ign_finite", "ign_inf", "ign_nan",
             "ign_above")
    part = torch.zeros(slots, M)
    t32 = torch.zeros(M, dtype=torch.int32)
    names = []
    for r in range(M):
        k = kinds[(first + r) % len(kinds)]
        names.append(k)
        t32[r] = -1 if k.startswith("ign") else r % 50
        if k in ("generic", "ign_finite"):
            part[:, r] = torch.rand(slots, generator=g) * (10.0 if r % 2 else 0.3) + 0.6 / slots
        else:
            a, b = r % slots, (r + 3) % slots
            if a == b:
                part[a, r] = edge[k]
            else:
                part[a, r] = part[b, r] = edge[k] / 2
    return part, t32, names, lo, hi


# ===================================================================== CPU checks of the above
def test_patterns_cover_every_slot():
    for N in (5, 9):
        seen = set()
        for first in range(0, len(PATTERNS), N):
            seen |= set(xent_rows(N, 65, 256, 1, BF, first=first)[2])
        assert seen == set(PATTERNS)
    lg, tg, names = xent_rows(15, 65, 256, seed=2, dtype=BF, fill="nan")
    r = xent_fwd_ref(lg, tg, 65)
    row = dict(zip(names, range(15)))
    assert abs(r.p[row["confident"], tg[row["confident"]]].item() - 0.999) < 2e-3
    assert abs(r.loss[row["constant"]].item() - math.log(65)) < 1e-12
    assert r.p[row["spread"], tg[row["spread"]]].item() < 1e-80 and r.loss[row["spread"]].item() > 200
    assert r.M[row["offset+"]].item() > 295 and r.M[row["offset-"]].item() < -290
    assert lg[row["max_last"], :65].argmax().item() == 64
    assert tg[row["tgt_first"]].item() == 0 and tg[row["tgt_last"]].item() == 64 and tg[row["tgt_alone"]].item() == 64
    assert tg[10:].tolist() == [-1, -100, 65, 255, 2 ** 40] and not r.valid[10:].any() and r.valid[:10].all()
    assert torch.isnan(lg[:, 65:].float()).all() and torch.isfinite(r.grad).all() and not r.grad[:, 65:].any()
    assert xent_rows(4, 65, 256, 2, BF, fill="big")[0][0, 65].item() > 2.9e38
    assert xent_rows(4, 65, 256, 2, FH, fill="big")[0][0, 65].item() == 65504.0
    # V = ld: ld - 1 is a valid target; V = 1: loss 0, gradient 0
    assert xent_fwd_ref(*xent_rows(15, 8, 8, 3, BF)[:2], 8).valid[13]
    one = xent_fwd_ref(*xent_rows(15, 1, 8, 3, BF)[:2], 1)
    assert not one.loss.any() and not one.grad.any()
    # the fused helpers: every target kind in every wave slot, every kind of S
    seen = {(k, r % 4) for first in range(7) for r, k in enumerate(fused_inputs(8, 8, 65, 256, 1, BF, first)[3])}
    assert seen == {(k, s) for k in TARGET_KINDS for s in range(4)}
    assert len(set(combine_inputs(7, 255, 1)[2])) == 11
    assert len({combine_inputs(9, 1, 1, first)[2][0] for first in range(11)}) == 11
    d = dw_inputs(1100, 8, 65, 256, 5, BF)
    n3 = int((d.t32 == 3).sum())
    assert n3 > 64 and (d.t32 < 0).any() and not (d.t32[(d.t32 != 3) & (d.t32 >= 0)] % 2 == 1).any()
    assert d.gw0.abs().min() > 0 and torch.isfinite(d.invS).all() and (d.invS[d.t32 >= 0] > 0).all()


def test_every_branch_of_the_entry_point_is_listed():
    got = {xent_branch(v, ld)[0] for v, V, ld in FWD_CASES}
    assert got == {"plain", "reg256", "reg512", "nt_ls", "nt_s", "nt_l", "stream", "scalar"}
    # the ninth: the default at 256 MiB of logits and above is variant 3's instantiation
    assert xent_branch(0, 8192, 16384 * 8192 * 2) == xent_branch(3, 8192) and xent_branch(0, 8192)[0] == "plain"
    # the fall-throughs of variants 1 and 2, and a variant on a row it does not take
    assert xent_branch(1, 51208)[0] == "plain" and xent_branch(2, 53256)[0] == "plain"
    assert xent_branch(3, 57600)[0] == "stream" and xent_branch(1, 1006)[0] == "scalar"


def test_refs_match_torch_float64_cross_entropy_and_autograd():
    """Loss and dlogits of the separate pass, and dX / dW recomposed from the fused helpers'
    references, against F.cross_entropy(ignore_index=-1) and autograd in float64."""
    N, C, V, Vp = 23, 24, 65, 256
    for dtype in (BF, FH):
        d = dw_inputs(N, C, V, Vp, seed=11, dtype=dtype)
        tg = d.t32.to(I64)
        xq = d.x.to(F64).requires_grad_(True)
        wq = d.W[:V].to(F64).requires_grad_(True)
        lq = (xq @ wq.T)
        lq.retain_grad()
        n_valid = int((tg >= 0).sum())
        ce = torch.nn.functional.cross_entropy(lq, tg, ignore_index=-1, reduction="none")
        (ce.sum() / n_valid).backward()
        # the separate pass on these logits (unrounded: the reference takes any float type)
        r = xent_fwd_ref(lq.detach(), tg, V)
        assert torch.allclose(r.loss, ce.detach(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(r.grad / n_valid, lq.grad, rtol=1e-10, atol=1e-14)
        # the fused form with E = exp(l - c) unrounded: softmax = E / S exactly
        tl = tlogit_ref(d.x, d.W, tg, C, V, 0.25)
        assert torch.allclose(tl.crow, torch.where(tg >= 0, r.lt + 0.25, 0.25), rtol=1e-12) and torch.equal(tl.t32, d.t32)
        E = torch.zeros(N, Vp, dtype=F64)
        E[:, :V] = (lq.detach() - tl.crow[:, None]).exp()
        cb = combine_ref(E.sum(-1)[None].float(), d.t32, 0.0, 1e30, 0.25)
        assert torch.allclose(cb.loss, ce.detach(), rtol=1e-6, atol=1e-6)
        g = float(np.float32(1.0 / n_valid))
        invS = cb.invS.float()
        coef, wrows, xs = bwd_prep_ref(d.x, d.W, d.t32, invS, g, C)
        dX = coef[:, :1].to(F64) * (E[:, :V] @ d.W[:V].to(F64)) - coef[:, 1:].to(F64) * wrows.to(F64)
        assert torch.allclose(dX, xq.grad, rtol=1e-5, atol=1e-9)
        # dW = E^T xs with xs = round16(s x); the onehot term takes the rounding back out of the
        # target entries, so there the exact s x stands
        f = dw_fix_ref(d.x, E, d.t32, invS, g, V, C, torch.zeros(V, C))
        A = E[:, :V].clone()
        valid = d.t32 >= 0
        A[valid, tg[valid]] = 0
        sx = (coef[:, :1] * d.x.float()).to(F64)
        et = E.gather(1, tg.clamp(min=0)[:, None]) * valid[:, None]
        dW = A.T @ sx + torch.zeros(V, C, dtype=F64).index_add_(0, tg.clamp(min=0), et * xs.to(F64)) + f.gw
        assert torch.allclose(dW, wq.grad, rtol=1e-5, atol=1e-9)
        assert f.hit.sum() < V and not f.gw[~f.hit].any()


def _fwd_ratios(lg, tg, V, variant, dtype, write_grad=1, mut=None):
    """Worst ratios of the model against the float64 reference (the loss without its two final
    roundings, the gradient without the store's half ulp: the parts with underived constants), and
    whether the exact assertions of the GPU file hold."""
    loss, out = xent_fp32_model(lg, tg, V, variant, write_grad, mut)
    r = xent_fwd_ref(lg, tg, V)
    b_loss, b_grad, hu, rnd = xent_fwd_bounds(r, dtype, xent_k_sum(variant, V, lg.shape[1]))
    e_loss = worst(((loss.double() - r.loss).abs() - rnd).clamp(min=0), b_loss - rnd)
    e_grad = worst(((out.double() - r.grad).abs() - hu).clamp(min=0), b_grad)
    exact = (not loss[~r.valid].any() and not out[~r.valid].any() and not out[:, V:].any()
             and bool(torch.isfinite(out.float()).all()))
    return e_loss, e_grad, exact


@pytest.mark.parametrize("dtype", [BF, FH], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", range(len(FWD_CASES)))
def test_fp32_model_of_the_separate_pass_within_half_of_every_bound(case, dtype):
    """Every (variant, V, ld) of the GPU file, every pattern, the padding fill cycling with the
    case: the fp32 part of each bound holds with a factor 2 (the half ulp of the 16-bit store and the
    loss's two final roundings are left whole), and the exact assertions hold in the model."""
    variant, V, ld = FWD_CASES[case]
    for first in range(0, len(PATTERNS), 9):
        lg, tg, _ = xent_rows(9, V, ld, seed=case, dtype=dtype, fill=FILLS[case % 3], first=first)
        e_loss, e_grad, exact = _fwd_ratios(lg, tg, V, variant, dtype)
        assert e_loss <= 0.5 and e_grad <= 0.5 and exact, (e_loss, e_grad, exact)
    loss0, same = xent_fp32_model(lg, tg, V, variant, write_grad=0)
    assert torch.equal(same.view(torch.int16), lg.view(torch.int16))


@pytest.mark.parametrize("mut", ["pad_in_S", "pad_in_max", "onehot_off", "invalid_not_zeroed"])
def test_wrong_replicas_of_the_separate_pass_leave_the_bounds(mut):
    """A padding column counted in S or in the maximum (zero fill, the column after V - 1), the
    onehot one column off, an invalid row not zeroed: each leaves a bound or an exact check."""
    lg, tg, names = xent_rows(15, 65, 256, seed=4, dtype=BF, fill="zero")
    ok = _fwd_ratios(lg, tg, 65, 0, BF)
    assert ok[0] <= 0.5 and ok[1] <= 0.5 and ok[2]
    e_loss, e_grad, exact = _fwd_ratios(lg, tg, 65, 0, BF, mut=mut)
    assert e_loss > 1 or e_grad > 1 or not exact
    if mut == "pad_in_S":  # the loss sees one leaked column on every valid row, the gradient does not
        r = xent_fwd_ref(lg, tg, 65)
        loss, _ = xent_fp32_model(lg, tg, 65, 0, mut=mut)
        b_loss = xent_fwd_bounds(r, BF, xent_k_sum(0, 65, 256))[0]
        bad = ((loss.double() - r.loss).abs() > b_loss)
        assert bad[[i for i, n in enumerate(names) if n in ("gauss", "constant", "tgt_last")]].all()


def _helper_ratios(dtype, C=264, M=8, V=65, Vp=256, mut=None):
    out = {}
    for first in range(7):
        x, W, tg, _ = fused_inputs(M, C, V, Vp, seed=C + first, dtype=dtype, first=first, ldx=C + 8)
        for shift in (0.0, 3.5):
            r = tlogit_ref(x, W, tg, C, V, shift)
            got = tlogit_model(x, W, tg, C, V, shift, mut)
            out["crow"] = max(out.get("crow", 0), worst((got.double() - r.crow).abs(), r.k * U * r.scale))
    return out


@pytest.mark.parametrize("dtype", [BF, FH], ids=["bf16", "fp16"])
def test_fp32_models_of_the_fused_helpers_within_half_of_every_bound(dtype):
    for C in (8, 64, 512, 520, 768, 8192):
        for M in (1, 5, 8):
            assert _helper_ratios(dtype, C, M)["crow"] <= 0.5
    for slots in (1, 7, 8, 9, 394):
        for M in (1, 255, 257):
            for first in (range(11) if M == 1 else (0,)):
                part, t32, _, lo, hi = combine_inputs(slots, M, slots + M, first)
                r = combine_ref(part, t32, lo, hi, 0.0)
                loss, inv, flag = combine_model(part, t32, lo, hi, 0.0)
                assert torch.equal(flag, r.flag)
                assert worst((loss.double() - r.loss).abs(), r.b_loss) <= 0.5
                assert worst((inv.double() - r.invS).abs(), r.b_inv) <= 0.5
    for C, (V, Vp) in [(8, (65, 256)), (264, (1000, 1024)), (8192, (256, 256)), (264, (65, 256)), (8, (256, 256))]:
        x, W, tg, _ = fused_inputs(9, C, V, Vp, seed=C + V, dtype=dtype)
        x[1::3] = (x[1::3].float() * 20).to(dtype)  # flagged rows: logits far from the target's
        t32 = tlogit_ref(x, W, tg, C, V, 0.0).t32
        rows = torch.tensor([7, 2, 4])
        r = fixup_ref(x, W, t32, rows, C, V, Vp, dtype)
        E, loss, inv = fixup_model(x, W, t32, rows, C, V, Vp, dtype)
        assert worst(((E.double() - r.E).abs() - r.hu_E).clamp(min=0), r.b_E) <= 0.5
        assert worst((loss.double() - r.loss).abs(), r.b_loss) <= 0.5
        assert worst((inv.double() - r.invS).abs(), r.b_inv) <= 0.5
        assert not E[:, V:].any() and not E[r.ign].any()
    for N in (37, 1100):
        for C, (V, Vp) in [(8, (65, 256)), (264, (65, 256)), (8, (1000, 1024))]:
            d = dw_inputs(N, C, V, Vp, seed=N + C, dtype=dtype)
            r = dw_fix_ref(d.x, d.E, d.t32, d.invS, d.g, Vp, C, d.gw0)
            got = dw_fix_model(d.x, d.E, d.t32, d.invS, d.g, Vp, C, d.gw0)
            assert worst((got.double() - r.gw).abs(), r.bound) <= 0.5
            assert torch.equal(got[~r.hit], d.gw0[~r.hit])


def test_wrong_replicas_of_the_fused_helpers_leave_the_bounds():
    """The target logit taken before the shift, 0.5 treated as outside the keep range, invS of
    the neighbouring row, the 16-bit rounding not taken back out of the dW term, and another
    rounding than the stored one taken out (the multiply fused with the fp16 conversion)."""
    assert _helper_ratios(BF)["crow"] <= 0.5 and _helper_ratios(BF, mut="before_shift")["crow"] > 1
    part, t32, names, lo, hi = combine_inputs(9, 255, 3)
    r = combine_ref(part, t32, lo, hi, 0.0)
    assert r.keep[names.index("half")] and r.keep[names.index("hi")] and not r.flag[names.index("ign_finite")]
    out = ("below_half", "above_hi", "inf", "nan", "ign_inf", "ign_nan", "ign_above")
    assert r.flag[[names.index(k) for k in out]].all()
    assert not torch.equal(combine_model(part, t32, lo, hi, 0.0, mut="half_outside")[2], r.flag)
    for dtype in (BF, FH):
        d = dw_inputs(37, 264, 65, 256, seed=9, dtype=dtype)
        r = dw_fix_ref(d.x, d.E, d.t32, d.invS, d.g, 256, 264, d.gw0)
        for mut in ("inv_neighbor", "rounding_kept"):
            got = dw_fix_model(d.x, d.E, d.t32, d.invS, d.g, 256, 264, d.gw0, mut)
            assert worst((got.double() - r.gw).abs(), r.bound) > 1, mut
        # bit-exact prologue: the neighbour's invS changes bits of coef and xs
        a = bwd_prep_ref(d.x, d.W, d.t32, d.invS, d.g, 264)
        b = bwd_prep_ref(d.x, d.W, d.t32, d.invS.roll(1), d.g, 264)
        assert not torch.equal(a[0], b[0]) and not torch.equal(a[2].view(torch.int16), b[2].view(torch.int16))
    # the product fused with the fp16 rounding: differs from round16(fp32 product) at fp16 ties
    d = dw_inputs(1100, 264, 65, 256, seed=1100 + 264 + 65, dtype=FH)
    r = dw_fix_ref(d.x, d.E, d.t32, d.invS, d.g, 256, 264, d.gw0)
    for mut, leaves in ((None, False), ("fused_rounding", True)):
        got = dw_fix_model(d.x, d.E, d.t32, d.invS, d.g, 256, 264, d.gw0, mut)
        assert (worst((got.double() - r.gw).abs(), r.bound) > 1) == leaves, mut


def test_bwd_prep_replica_signed_zeros_and_gather():
    x, W, tg, _ = fused_inputs(8, 8, 65, 256, seed=1, dtype=BF)
    t32 = tlogit_ref(x, W, tg, 8, 65, 0.0).t32
    invS = torch.where(t32 >= 0, torch.rand(8) + 0.5, torch.zeros(8))
    for g in (0.125, -0.125):
        coef, wrows, xs = bwd_prep_ref(x, W, t32, invS, g, 8)
        ign = t32 < 0
        assert ign.any() and torch.equal(wrows[ign], W[:1].expand(int(ign.sum()), 8))
        assert not coef[ign].any() and not xs[ign].float().any()
        # x * (+-0): the sign of the zero is sign(x) * sign(g)
        assert (x[ign] == 0).any() and torch.equal(xs[ign].view(torch.int16) < 0, (x[ign].float() < 0) != (g < 0))
        assert torch.equal(coef[~ign, 1], torch.full((int((~ign).sum()),), g))
