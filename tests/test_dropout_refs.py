"""References for the dropout that lives inside the attention and embedding kernels
(``flash_attn.hip``, ``embedding.hip``), as plain functions that run on any device, with their
own CPU checks.  ``test_dropout_gpu.py`` compares the HIP kernels with these.

The masks come from the host replica of ``common.h``'s counter hash in
``test_streaming_refs.py``.  Attention draws element ``((b*H + h)*T + q)*T + k``, the embedding
element ``row*C + c``.

Three layers:

* ``attn_keep_mask`` / ``attn_dropout_ref``: the mask and causal attention with it in float64
  (O, dQ, dK, dV by autograd) with the magnitude tensors the per-element bounds multiply.
* mask recovery: inputs under which one output of a kernel is a function of the keep bit of one
  (q, k) pair (``recovery_inputs``), decoders that read the bit back (``decode_*``) and the
  driver that walks the ``ceil(T / D)`` windows (``recover_masks``).  All (b, h) get the same
  inputs; only the mask tells them apart.
* ``attn_emulate``: an fp32 evaluation with the kernels' rounding points (P, dS, O and the
  outputs rounded to the 16-bit type).  Only the CPU checks use it: the decoders must return the
  mask it was given, and its distance from the float64 reference at the GPU test's own inputs
  sets the gradient bound's constant.

Emulation against the float64 reference, max |err| / mag over O, dQ, dK, dV at the inputs of
``ATTN_CASES`` (p = 0.2, step 3, the salt the GPU test replays):

    bf16  (1, 2, 200, 64) 0.0178   (2, 3, 320, 64) 0.0126   (1, 1, 77, 32) 0.0054
          (1, 2, 192, 128) 0.0233                                  -> c = 2^-3
    fp16  (1, 2, 200, 64) 0.0026                                   -> c = 2^-6

The bf16 maxima are dQ of the first few queries (0.0233 at q = 0, D = 128): there dS cancels to
nothing in exact arithmetic (one kept key: scale * dP - delta = 0) while delta is formed from
the rounded O, whose error scales with sum |dO| |O|, not with |delta|.  Past q = 16 every ratio
is below 0.008; O, dK and dV stay below 0.0071 everywhere.  The fp16 maximum is a dV element.

``c`` is four times the maximum rounded up to a power of two (``GRAD_C``); the margin is for what
the emulation leaves out (``fast_exp2``, the lse round trip, the fp32 accumulation order).
``test_emulation_sets_the_gradient_constant`` recomputes the maxima and fails if ``GRAD_C`` is
not what they give.
"""

import math

import numpy as np
import pytest
import torch

from test_streaming_refs import F64, dropout_scale, nsa_drop_thresh, nsa_keep, nsa_seed

F32 = torch.float32
BF = torch.bfloat16
FH = torch.float16

STEP = 3  # the device counter every check here and on the GPU runs with

# (B, H, T, D) of the mask-recovery and float64 comparisons, p = 0.2
ATTN_CASES = [(1, 2, 200, 64), (2, 3, 320, 64), (1, 1, 77, 32), (1, 2, 192, 128)]
# gradient bound |err| <= c * mag + 1e-5: four times the emulation's worst ratio, rounded up to
# a power of two (module docstring)
GRAD_C = {BF: 2.0 ** -3, FH: 2.0 ** -6}


# --------------------------------------------------------------------------- attention mask
def attn_keep_bh(bh, T, p, salt, step):
    """Keep bits of the flat (b*H + h) indices ``bh``: bool [len(bh), T, T] at element id
    ``(bh*T + q)*T + k``, in uint64 like the kernels."""
    bh = np.asarray(bh, dtype=np.uint64).reshape(-1, 1, 1)
    n = np.uint64(T)
    q = np.arange(T, dtype=np.uint64).reshape(1, -1, 1)
    k = np.arange(T, dtype=np.uint64).reshape(1, 1, -1)
    ids = (bh * n + q) * n + k
    return torch.from_numpy(nsa_keep(nsa_seed(salt, step), ids, nsa_drop_thresh(p)))


def attn_keep_mask(B, H, T, p, salt, step):
    """bool [B, H, T, T]: the mask every attention kernel draws (forward and backward alike)."""
    return attn_keep_bh(np.arange(B * H), T, p, salt, step).view(B, H, T, T)


def causal(T, device=None):
    return torch.ones(T, T, dtype=torch.bool, device=device).tril()


def pack_qkv(q, k, v):
    """[B, H, T, D] x 3 -> the packed activation [B, T, 3 * H * D]."""
    B, H, T, D = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * D).contiguous()


def to_bhtd(x, H):
    """[B, T, H * D] -> [B, H, T, D]."""
    B, T, C = x.shape
    return x.view(B, T, H, C // H).transpose(1, 2)


def from_bhtd(x):
    B, H, T, D = x.shape
    return x.transpose(1, 2).reshape(B, T, H * D).contiguous()


# ----------------------------------------------------------------- float64 reference
def attn_dropout_ref(q, k, v, do, keep, p):
    """Causal attention with an explicit keep mask in float64.  q, k, v, do: [B, H, T, D];
    keep: bool [B, H, T, T].  P = softmax, Pd = P * keep * scale, O = Pd @ v with
    scale = 1 / (1 - float32(p)).  Returns O and the gradients by autograd, and the sums of the
    absolute terms behind each output element (``mag_*``): an element all of whose terms are
    dropped has magnitude 0."""
    T, D = q.shape[-2:]
    sm = 1.0 / math.sqrt(D)
    scale = float(dropout_scale(p))
    q, k, v = (x.detach().to(F64).requires_grad_(True) for x in (q, k, v))
    do = do.to(F64)
    keep = keep.to(F64)
    vis = causal(T, q.device)
    P = torch.softmax((q @ k.transpose(-1, -2) * sm).masked_fill(~vis, -math.inf), -1)
    Pd = P * keep * scale
    O = Pd @ v
    dq, dk, dv = torch.autograd.grad(O, (q, k, v), do)
    with torch.no_grad():
        dP = do @ v.transpose(-1, -2)
        delta = (do * O).sum(-1, keepdim=True)
        ds_mag = P * (keep * scale * dP.abs() + delta.abs())
        out = dict(o=O, dq=dq, dk=dk, dv=dv, mag_o=Pd @ v.abs(), mag_dv=Pd.transpose(-1, -2) @ do.abs(),
                   mag_dq=sm * (ds_mag @ k.abs()), mag_dk=sm * (ds_mag.transpose(-1, -2) @ q.abs()))
    return {n: t.detach() for n, t in out.items()}


# ------------------------------------------------------------------- fp32 emulation
def attn_emulate(q, k, v, do, keep, p, dtype):
    """The kernels' arithmetic in fp32 with their rounding points: the forward rounds the
    dropped, un-normalised P (``exp(s - max)``) and O = (Pd @ V) / l, with l summed before the
    drop; the backward recomputes P = exp(s - lse), rounds Pd and dS = P * (keep * scale * dP -
    delta), delta from the rounded O, and rounds dQ, dK, dV.  Returns y, lse, dq, dk, dv."""
    T, D = q.shape[-2:]
    sm = torch.tensor(1.0 / math.sqrt(D), dtype=F32)
    scale = torch.tensor(float(dropout_scale(p)), dtype=F32)
    r16 = lambda x: x.to(dtype).float()  # noqa: E731
    q, k, v, do = (x.float() for x in (q, k, v, do))
    vis = causal(T)
    zero = torch.zeros((), dtype=F32)
    s = (q @ k.transpose(-1, -2) * sm).masked_fill(~vis, -math.inf)
    m = s.max(-1, keepdim=True).values
    pu = torch.exp(s - m)
    l = pu.sum(-1, keepdim=True)
    y = r16((r16(torch.where(keep, pu * scale, zero)) @ v) / l)
    lse = (m + torch.log(l)).squeeze(-1)
    P = torch.exp(s - lse.unsqueeze(-1))
    Pd = r16(torch.where(keep, P * scale, zero))
    dv = r16(Pd.transpose(-1, -2) @ do)
    delta = (y * do).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    dS = r16(P * (torch.where(keep, dP * scale, zero) - delta))
    dq = r16((dS @ k) * sm)
    dk = r16((dS.transpose(-1, -2) @ q) * sm)
    return dict(y=y, lse=lse, dq=dq, dk=dk, dv=dv)


def attn_case_inputs(B, H, T, D, dtype, seed):
    """Random q, k, v, do [B, H, T, D] of the float64 comparison, values of ``dtype`` held in
    fp32 on the CPU, and the salt ``ops.attention`` draws after ``torch.manual_seed(seed)``."""
    g = torch.Generator().manual_seed(1000 + seed)
    q, k, v, do = (torch.randn(B, H, T, D, generator=g).to(dtype).float() for _ in range(4))
    return q, k, v, do, replayed_salt(seed)


def replayed_salt(seed):
    """What ``ops.functional.new_seed`` returns as the first draw after ``manual_seed(seed)``."""
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    salt = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.set_rng_state(state)
    return salt


def worst_ratio(err, mag, floor=0.0):
    """max over the elements of (err - floor) / mag; inf if an element of zero magnitude errs by
    more than ``floor``."""
    err = (err - floor).clamp_min(0.0)
    r = torch.where(mag > 0, err / mag, torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    return r.max().item()


def emulation_ratio(B, H, T, D, dtype, seed, p=0.2):
    """max |emulation - float64 reference| / mag over O, dQ, dK, dV at one case's inputs."""
    q, k, v, do, salt = attn_case_inputs(B, H, T, D, dtype, seed)
    keep = attn_keep_mask(B, H, T, p, salt, STEP)
    ref = attn_dropout_ref(q, k, v, do, keep, p)
    emu = attn_emulate(q, k, v, do, keep, p, dtype)
    return max(worst_ratio((emu[a].to(F64) - ref[b]).abs(), ref["mag_" + b])
               for a, b in (("y", "o"), ("dq", "dq"), ("dk", "dk"), ("dv", "dv")))


def pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


# ------------------------------------------------------------------- mask recovery
def recovery_inputs(kind, T, D, w, gen):
    """(q, k, v, do), each [T, D], for window ``w`` (keys or queries [wD, wD + D)).

    "p":  Q = 0, K random, V one-hot over the key window, dO one-hot over the query window.
          y[q, d] = Pd[q, wD + d] (forward mask), dV[k, d] = Pd[wD + d, k] (dK/dV kernel, P path).
    "dq": Q = 0, K one-hot over the key window, V[:, 0] = 1, dO = e_0.  Then dP = 1,
          delta = y[q, 0] and dQ[q, d] = sm * dS[q, wD + d] (dQ kernel).
    "dk": K = 0, Q one-hot over the query window, the same V and dO.
          dK[k, d] = sm * dS[wD + d, k] (dK/dV kernel, dS path).
    Every visible score is 0 in all three, so P = 1 / (q + 1)."""
    z = lambda: torch.zeros(T, D)  # noqa: E731
    r = torch.arange(w * D, min(T, (w + 1) * D))
    hot = z()
    hot[r, r - w * D] = 1.0
    e0 = z()
    e0[:, 0] = 1.0
    if kind == "p":
        return z(), torch.randn(T, D, generator=gen), hot, hot.clone()
    if kind == "dq":
        return z(), hot, e0, e0.clone()
    if kind == "dk":
        return hot, z(), e0, e0.clone()
    raise ValueError(kind)


def decode_fwd(y, w, T, D):
    """Forward mask: slab[..., q, j] = keep[q, wD + j] from y [B, H, T, D] of kind "p"."""
    n = min(T, (w + 1) * D) - w * D
    return y[..., :n] != 0


def decode_dv(dv, w, T, D):
    """dK/dV kernel, P path: slab[..., j, k] = keep[wD + j, k] from dV of kind "p"."""
    n = min(T, (w + 1) * D) - w * D
    return (dv[..., :n] != 0).transpose(-1, -2)


def decode_dq(dq, y, w, T, D, p):
    """dQ kernel, dS path: dQ[q, d] * (q + 1) / sm + y[q, 0] is scale where (q, wD + d) is kept
    and 0 where it is dropped; decided at scale / 2.  slab[..., q, j] = keep[q, wD + j]."""
    n = min(T, (w + 1) * D) - w * D
    qp1 = torch.arange(1, T + 1, device=dq.device, dtype=F32).view(T, 1)
    val = dq[..., :n].float() * qp1 * math.sqrt(D) + y[..., :1].float()
    return val > float(dropout_scale(p)) / 2


def decode_dk(dk, y, w, T, D, p):
    """dK/dV kernel, dS path: dK[k, d] * (q + 1) / sm + y[q, 0] with q = wD + d decides the same
    way.  slab[..., j, k] = keep[wD + j, k]."""
    n = min(T, (w + 1) * D) - w * D
    qp1 = torch.arange(w * D + 1, w * D + n + 1, device=dk.device, dtype=F32).view(1, n)
    y0 = y[..., w * D:w * D + n, 0].float().unsqueeze(-2)  # [B, H, 1, n]
    val = dk[..., :n].float() * qp1 * math.sqrt(D) + y0
    return (val > float(dropout_scale(p)) / 2).transpose(-1, -2)


def recover_masks(run, B, H, T, D, p, which=("fwd", "dv", "dq", "dk"), windows=None, seed=0):
    """Rebuild the keep mask from a kernel's outputs.  ``run(q, k, v, do)`` takes [T, D] inputs
    (shared by every (b, h)) and returns y, lse, dq, dk, dv as [B, H, T, D] ([B, H, T] for lse).
    Returns {name: bool [B, H, T, T]} with the non-causal part (and any window not asked for)
    False, and the ``(w, y, lse)`` of the "p" launches for the forward's value checks."""
    gen = torch.Generator().manual_seed(seed)
    masks, fwd_outs = {}, []
    vis = None
    for w in (range((T + D - 1) // D) if windows is None else windows):
        lo, hi = w * D, min(T, (w + 1) * D)
        for kind, names in (("p", ("fwd", "dv")), ("dq", ("dq",)), ("dk", ("dk",))):
            if not any(n in which for n in names):
                continue
            out = run(*recovery_inputs(kind, T, D, w, gen))
            if vis is None:
                vis = causal(T, out["y"].device)
            for n in names:
                if n not in which:
                    continue
                m = masks.setdefault(n, torch.zeros(B, H, T, T, dtype=torch.bool, device=out["y"].device))
                if n == "fwd":
                    m[..., :, lo:hi] = decode_fwd(out["y"], w, T, D)
                elif n == "dv":
                    m[..., lo:hi, :] = decode_dv(out["dv"], w, T, D)
                elif n == "dq":
                    m[..., :, lo:hi] = decode_dq(out["dq"], out["y"], w, T, D, p)
                else:
                    m[..., lo:hi, :] = decode_dk(out["dk"], out["y"], w, T, D, p)
            if kind == "p":
                fwd_outs.append((w, out["y"], out["lse"]))
    return {n: m & vis for n, m in masks.items()}, fwd_outs


def emulated_run(keep, p, dtype):
    """``run`` of ``recover_masks`` on the emulation with a given mask."""
    B, H = keep.shape[:2]

    def run(q, k, v, do):
        return attn_emulate(*(x.to(dtype).float().expand(B, H, -1, -1) for x in (q, k, v, do)), keep, p, dtype)

    return run


# ------------------------------------------------------------------------- embedding
def emb_keep_mask(B, T, C, p, salt, step):
    """bool [B, T, C]: the embedding kernels' mask, element ``row * C + c``, row = b * T + t."""
    ids = np.arange(B * T * C, dtype=np.uint64)
    return torch.from_numpy(nsa_keep(nsa_seed(salt, step), ids, nsa_drop_thresh(p))).view(B, T, C)


def emb_dropout_ref(idx, wte, wpe, dx, p, salt, step, dtype=F32):
    """x = drop(wte[idx] + wpe[t]) and its weight gradients, on the device of ``idx``.

    Forward, bit-exact: where(keep, (wte.float()[idx] + wpe.float()[:T]) * float32(scale), 0) in
    fp32 (an add followed by a multiply: nothing to contract), cast to ``dtype``.
    Backward, float64: dwte = index_add(keep * scale * dx), dwpe = the same summed over the
    batch; with them, per element, the sum of the absolute terms and the number of kept terms.
    Returns (x, dict(dwte, dwpe, abs_wte, abs_wpe, n_wte, n_wpe)); dwpe is [T, C]."""
    B, T = idx.shape
    V, C = wte.shape
    dev = idx.device
    keep = emb_keep_mask(B, T, C, p, salt, step).to(dev)
    scale = float(dropout_scale(p))
    x = (wte.float()[idx] + wpe.float()[:T]) * torch.tensor(scale, dtype=F32, device=dev)
    x = torch.where(keep, x, torch.zeros((), dtype=F32, device=dev)).to(dtype)
    if dx is None:
        return x, None
    terms = (keep.to(F64) * scale * dx.to(F64)).view(B * T, C)
    flat = idx.reshape(-1)
    add = lambda t: torch.zeros(V, C, dtype=F64, device=dev).index_add_(0, flat, t)  # noqa: E731
    cnt = keep.view(B * T, C).to(F64)
    g = dict(dwte=add(terms), abs_wte=add(terms.abs()), n_wte=add(cnt),
             dwpe=terms.view(B, T, C).sum(0), abs_wpe=terms.abs().view(B, T, C).sum(0), n_wpe=cnt.view(B, T, C).sum(0))
    return x, g


def fp32_sum_bound(n, abs_sum):
    """|fp32 sum of n fp32-rounded terms, any order, - exact| <= (n + 2) 2^-24 sum |terms|, plus
    the smallest normal where a GPU may flush."""
    return (n + 2) * 2.0 ** -24 * abs_sum + 2.0 ** -126


# ===================================================================== CPU checks of the above
EMU_CASES = [(1, 2, 200, 64, 0.2, BF), (1, 1, 77, 32, 0.5, BF), (1, 2, 192, 128, 0.1, BF), (2, 3, 96, 64, 0.2, BF),
             (1, 2, 200, 64, 0.2, FH)]


def _salt_with_dead_row(B, H, T, p):
    """The first small salt whose mask drops every visible key of some query."""
    for salt in range(256):
        if not (attn_keep_mask(B, H, T, p, salt, STEP) & causal(T)).any(-1).all():
            return salt
    raise AssertionError("no salt below 256 drops a whole row")


@pytest.mark.parametrize("B,H,T,D,p,dtype", EMU_CASES)
def test_decoders_return_the_emulations_mask(B, H, T, D, p, dtype):
    """Every decoder applied to the emulation's outputs returns exactly keep & causal, rows
    whose visible keys are all dropped included; the forward's kept values are scale / (q + 1)
    to one rounding and lse = ln(q + 1)."""
    keep = attn_keep_mask(B, H, T, p, _salt_with_dead_row(B, H, T, p), STEP)
    want = keep & causal(T)
    masks, fwd_outs = recover_masks(emulated_run(keep, p, dtype), B, H, T, D, p)
    assert sorted(masks) == ["dk", "dq", "dv", "fwd"]
    for name, m in masks.items():
        assert torch.equal(m, want), name
    rel = 2.0 ** -11 if dtype == FH else 2.0 ** -8
    pd = float(dropout_scale(p).astype(np.float32))
    pd = torch.tensor(pd).to(dtype).float().item()  # the dropped P is rounded too (exact for p = 0.2, 0.5)
    qp1 = torch.arange(1, T + 1, dtype=F32)
    for w, y, lse in fwd_outs:
        n = min(T, (w + 1) * D) - w * D
        ref = want[..., w * D:w * D + n].float() * pd / qp1.view(T, 1)
        assert ((y[..., :n] - ref).abs() <= rel * ref).all()
        assert (y[..., n:] == 0).all()
        assert ((lse - torch.log(qp1)).abs() <= 1e-5 * torch.log(qp1) + 1e-6).all()


@pytest.mark.parametrize("B,H,T,D,p,dtype", [EMU_CASES[0], EMU_CASES[1], EMU_CASES[4]])
def test_decoders_see_one_wrong_bit(B, H, T, D, p, dtype):
    """A mask wrong in one place (a kept pair dropped, a dropped pair kept) makes each decoder's
    comparison fail at that element and nowhere else."""
    keep = attn_keep_mask(B, H, T, p, _salt_with_dead_row(B, H, T, p), STEP)
    want = keep & causal(T)
    for b, h, q, k in [(B - 1, H - 1, T - 1, T - 2), (0, 0, T // 2, 3), (0, H - 1, D + 1, D + 1)]:
        wrong = keep.clone()
        wrong[b, h, q, k] = ~wrong[b, h, q, k]
        masks, _ = recover_masks(emulated_run(wrong, p, dtype), B, H, T, D, p)
        for name, m in masks.items():
            assert not torch.equal(m, want), name
            assert (m != want).nonzero().tolist() == [[b, h, q, k]], name


def test_mask_statistics_and_index_width():
    B, H, T = 2, 3, 200
    vis = causal(T)
    for p in (0.1, 0.2, 0.5):
        keep = attn_keep_mask(B, H, T, p, 99, STEP)
        assert keep.shape == (B, H, T, T) and keep.dtype == torch.bool
        n = keep.numel()
        assert abs(keep.float().mean().item() - (1 - p)) < 3 * math.sqrt(p * (1 - p) / n)
        kv = keep[:, :, vis]
        assert abs(kv.float().mean().item() - (1 - p)) < 3 * math.sqrt(p * (1 - p) / kv.numel())
        # not correlated across heads: the agreement of two heads' masks is p^2 + (1 - p)^2
        agree = (keep[0, 0] == keep[1, 2]).float().mean().item()
        e = p * p + (1 - p) * (1 - p)
        assert abs(agree - e) < 4 * math.sqrt(e * (1 - e) / (T * T))
    assert not torch.equal(attn_keep_mask(1, 1, T, 0.2, 99, STEP), attn_keep_mask(1, 1, T, 0.2, 99, STEP + 1))
    assert not torch.equal(attn_keep_mask(1, 1, T, 0.2, 99, STEP), attn_keep_mask(1, 1, T, 0.2, 98, STEP))
    assert attn_keep_mask(1, 2, T, 0.0, 99, STEP).all()
    # the flat index: row (b, h) of the [B, H] mask is bh = b * H + h
    assert torch.equal(attn_keep_mask(B, H, T, 0.2, 99, STEP)[1, 1], attn_keep_bh([4], T, 0.2, 99, STEP)[0])
    # two (b, h) that are 2^32 / T^2 apart share every id's low 32 bits; the masks differ
    T = 1024
    far = (1 << 32) // (T * T)
    a, b = attn_keep_bh([3, 3 + far], T, 0.2, 99, STEP)
    assert far == 4096 and not torch.equal(a, b)
    assert abs((a == b).float().mean().item() - 0.68) < 0.01


def test_attn_dropout_ref_without_dropout_is_sdpa():
    torch.manual_seed(0)
    B, H, T, D = 2, 2, 77, 32
    q, k, v, do = (torch.randn(B, H, T, D, dtype=F64) for _ in range(4))
    keep = attn_keep_mask(B, H, T, 0.0, 5, STEP)
    ref = attn_dropout_ref(q, k, v, do, keep, 0.0)
    qa, ka, va = (x.clone().requires_grad_(True) for x in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(qa, ka, va, is_causal=True)
    o.backward(do)
    for got, want in ((ref["o"], o.detach()), (ref["dq"], qa.grad), (ref["dk"], ka.grad), (ref["dv"], va.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)
    # the magnitudes dominate the values they scale
    for n in ("o", "dq", "dk", "dv"):
        assert (ref[n].abs() <= ref["mag_" + n] * (1 + 1e-12) + 1e-300).all(), n


def test_attn_dropout_ref_masks_and_scales():
    """With dropout: O is the masked, rescaled P times V; a query whose visible keys are all
    dropped has O = 0 and zero magnitudes; dV of a key nobody keeps is exactly 0."""
    torch.manual_seed(1)
    B, H, T, D, p = 1, 2, 40, 32, 0.5
    q, k, v, do = (torch.randn(B, H, T, D) for _ in range(4))
    keep = attn_keep_mask(B, H, T, p, 7, STEP)
    ref = attn_dropout_ref(q, k, v, do, keep, p)
    P = torch.softmax((q.double() @ k.double().transpose(-1, -2) / math.sqrt(D)).masked_fill(~causal(T), -math.inf), -1)
    assert torch.allclose(ref["o"], (P * keep * 2.0) @ v.double(), rtol=1e-12, atol=1e-13)
    want = keep & causal(T)
    dead_q = ~want.any(-1)
    dead_k = ~want.any(-2)
    assert dead_q.any() and dead_k.any()
    assert (ref["o"][dead_q] == 0).all() and (ref["mag_o"][dead_q] == 0).all()
    assert (ref["dv"][dead_k] == 0).all() and (ref["mag_dv"][dead_k] == 0).all()


def test_emulation_sets_the_gradient_constant():
    """GRAD_C is four times the emulation's worst |err| / mag at the GPU test's own inputs,
    rounded up to a power of two; and a mask from another salt is nowhere near it."""
    worst = {BF: 0.0, FH: 0.0}
    for i, (B, H, T, D) in enumerate(ATTN_CASES):
        r = emulation_ratio(B, H, T, D, BF, i)
        print(f"emulation bf16 {(B, H, T, D)}: max |err| / mag = {r:.4f}")
        worst[BF] = max(worst[BF], r)
    worst[FH] = emulation_ratio(*ATTN_CASES[0], FH, 0)
    print(f"emulation fp16 {ATTN_CASES[0]}: max |err| / mag = {worst[FH]:.4f}")
    for dt in (BF, FH):
        assert pow2_ceil(4 * worst[dt]) == GRAD_C[dt], (dt, worst[dt])
    B, H, T, D = ATTN_CASES[0]
    q, k, v, do, salt = attn_case_inputs(B, H, T, D, BF, 0)
    ref = attn_dropout_ref(q, k, v, do, attn_keep_mask(B, H, T, 0.2, salt, STEP), 0.2)
    emu = attn_emulate(q, k, v, do, attn_keep_mask(B, H, T, 0.2, salt + 1, STEP), 0.2, BF)
    for a, b in (("y", "o"), ("dq", "dq"), ("dk", "dk"), ("dv", "dv")):
        assert worst_ratio((emu[a].to(F64) - ref[b]).abs(), ref["mag_" + b], 1e-5) > 16 * GRAD_C[BF], a


def test_replayed_salt_is_new_seeds_first_draw():
    from nanosandbox_amd.ops.functional import new_seed

    state = torch.get_rng_state()
    torch.manual_seed(11)
    want = new_seed()
    torch.set_rng_state(state)
    assert replayed_salt(11) == want and replayed_salt(12) != want
    assert torch.equal(torch.get_rng_state(), state)


def test_emb_dropout_ref():
    torch.manual_seed(2)
    B, T, V, C = 3, 20, 11, 16
    idx = torch.randint(0, V, (B, T))
    idx[0, :5] = 3
    idx[idx == 7] = 6  # a row no token touches
    wte, wpe = torch.randn(V, C).to(BF), torch.randn(T + 2, C).to(BF)
    dx = torch.randn(B, T, C)
    x0, g0 = emb_dropout_ref(idx, wte, wpe, dx, 0.0, 5, STEP)
    assert torch.equal(x0, wte.float()[idx] + wpe.float()[:T])
    assert torch.equal(g0["dwpe"], dx.double().sum(0)) and (g0["n_wpe"] == B).all()
    for p in (0.2, 0.5):
        keep = emb_keep_mask(B, T, C, p, 5, STEP)
        assert abs(emb_keep_mask(8, 64, 256, p, 5, STEP).float().mean().item() - (1 - p)) < 3 * math.sqrt(
            p * (1 - p) / (8 * 64 * 256))
        x, g = emb_dropout_ref(idx, wte, wpe, dx, p, 5, STEP)
        assert torch.equal(x != 0, keep & (x0 != 0))
        assert torch.equal(x[keep], x0[keep] * float(dropout_scale(p)))
        # the float64 gradients are autograd's of the same forward
        a = wte.double().requires_grad_(True)
        b = wpe.double().requires_grad_(True)
        ((a[idx] + b[:T]) * keep * float(dropout_scale(p))).backward(dx.double())
        assert torch.allclose(g["dwte"], a.grad, rtol=1e-13, atol=1e-15)
        assert torch.allclose(g["dwpe"], b.grad[:T], rtol=1e-13, atol=1e-15)
        assert (g["dwte"][7] == 0).all() and (g["n_wte"][7] == 0).all() and (g["abs_wte"][7] == 0).all()
        assert g["n_wte"].sum().item() == keep.sum().item() == g["n_wpe"].sum().item()
        # an fp32 sum of the same terms in token order stays within the bound
        t32 = torch.where(keep, dx * torch.tensor(float(dropout_scale(p))), torch.zeros(())).view(B * T, C)
        s32 = torch.zeros(V, C)
        for r in range(B * T):
            s32[idx.view(-1)[r]] += t32[r]
        assert ((s32.double() - g["dwte"]).abs() <= fp32_sum_bound(g["n_wte"], g["abs_wte"])).all()
    bf = emb_dropout_ref(idx, wte, wpe, None, 0.2, 5, STEP, dtype=BF)[0]
    assert bf.dtype == BF and torch.equal(bf, emb_dropout_ref(idx, wte, wpe, None, 0.2, 5, STEP)[0].to(BF))
