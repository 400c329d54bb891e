"""The dropout inside the attention and embedding kernels against the hash replica.

A. Mask recovery, bit for bit: the raw flash-attention entry points are driven with an explicit
   salt and a non-zero device step, on inputs under which one output element is a function of
   one (q, k) pair's keep bit (``test_dropout_refs.recovery_inputs``).  The mask read back from
   the forward, from dV (dK/dV kernel, P path), from dQ (dQ kernel, dS path) and from dK (dK/dV
   kernel, dS path) must each equal ``attn_keep_mask & causal``; one launch at B * T * T > 2^32
   checks the width of the element id.
B. Random inputs through ``ops.attention`` against the float64 reference with the replica's mask,
   per element: |err| <= 2^-5 mag + 2^-7 |ref| + 1e-4 for y (the bound of ``test_flash_attention``)
   and |err| <= c mag + 1e-5 for dQ, dK, dV, with c from the fp32 emulation of the kernels'
   rounding points measured against the same reference at these inputs (maxima 0.0233 bf16,
   0.0026 fp16; c = 2^-3 bf16, 2^-6 fp16: ``test_dropout_refs.GRAD_C``, where a CPU check
   recomputes them).  On an MI355X the kernels' own worst (err - 1e-5) / mag was 0.0176 bf16 (dQ
   of an early query, like the emulation's) and 0.0007 fp16, y's worst err / bound 0.18.
C. Workgroup orders 1 and 2 give the bits of order 0.
D. The embedding forward with dropout, bit for bit, and its backward on the atomic, sorted and
   LDS paths within the fp32 summation bound of the float64 reference.

Each test prints the worst err / bound it met (``-s`` shows them).
"""

import contextlib
import math
import time

import pytest
import torch

from test_dropout_refs import (ATTN_CASES, BF, F32, F64, FH, GRAD_C, STEP, attn_case_inputs, attn_dropout_ref,
                               attn_keep_bh, attn_keep_mask, causal, decode_fwd, emb_dropout_ref, fp32_sum_bound,
                               from_bhtd, pack_qkv, recover_masks, recovery_inputs, to_bhtd, worst_ratio)
from test_streaming_refs import dropout_scale

pytestmark = pytest.mark.gpu

DEV = "cuda"
SALT = 0x2545F4914F6CDD1D >> 2  # any 62-bit value: the raw entry points take the salt as given


@contextlib.contextmanager
def _device_step(step=STEP):
    """The kernels' device counter at ``step`` for the block, back to 0 afterwards."""
    from nanosandbox_amd import ops

    ops.rng_set(DEV, step)
    try:
        yield
    finally:
        ops.rng_set(DEV, 0)
        torch.cuda.synchronize()


@pytest.fixture
def flash_variant(kernels):
    """ops.functional.flash_variant as a fixture: selects kernels for one test, restores after."""
    from nanosandbox_amd.ops.functional import flash_variant as fv

    stack = contextlib.ExitStack()
    with stack:
        yield lambda **kw: stack.enter_context(fv(**kw))


def _nan(*shape, dtype=F32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _sym(name, dtype):
    return name + "_h" if dtype == FH else name


def _flash_fwd(qkv, H, p, salt):
    """nsa_flash_fwd(_h) into NaN-prefilled y and lse."""
    from nanosandbox_amd.ops import _lib

    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // H
    y = _nan(B, T, C, dtype=qkv.dtype)
    lse = _nan(B, H, T)
    _lib.call(_sym("nsa_flash_fwd", qkv.dtype), _lib.ptr(qkv), _lib.ptr(y), _lib.ptr(lse), B, T, H, D,
              1.0 / math.sqrt(D), p, salt, _lib.stream())
    return y, lse


def _flash_bwd(qkv, y, dy, lse, H, p, salt):
    """nsa_flash_bwd2(_h) into a NaN-prefilled dqkv (and workspace)."""
    from nanosandbox_amd.ops import _lib

    B, T, C3 = qkv.shape
    D = C3 // 3 // H
    dqkv = _nan(B, T, C3, dtype=qkv.dtype)
    ws = _nan(2, B, H, T)
    _lib.call(_sym("nsa_flash_bwd2", qkv.dtype), _lib.ptr(qkv), _lib.ptr(y), _lib.ptr(dy), _lib.ptr(lse), _lib.ptr(ws),
              _lib.ptr(dqkv), B, T, H, D, 1.0 / math.sqrt(D), p, salt, _lib.stream())
    return dqkv


def _kernel_run(B, H, p, salt, dtype, backward=True):
    """``run`` of ``recover_masks`` on the kernels: the [T, D] inputs go to every (b, h)."""

    def run(q, k, v, do):
        T, D = q.shape
        q, k, v, do = (x.to(DEV).to(dtype).expand(B, H, T, D) for x in (q, k, v, do))
        qkv = pack_qkv(q, k, v)
        y, lse = _flash_fwd(qkv, H, p, salt)
        out = dict(y=to_bhtd(y, H).float(), lse=lse)
        assert not torch.isnan(out["y"]).any() and not torch.isnan(lse).any()
        if backward:
            g = _flash_bwd(qkv, y, from_bhtd(do), lse, H, p, salt).float()
            assert not torch.isnan(g).any()
            for i, n in enumerate(("dq", "dk", "dv")):
                out[n] = to_bhtd(g.view(B, T, 3, H * D)[:, :, i], H)
        return out

    return run


def _check_fwd_values(fwd_outs, want, T, D, p, dtype):
    """The forward's kept values are scale / (q + 1) to one output rounding, everything else 0,
    and lse = ln(q + 1): the row sum is taken before the drop."""
    rel = 2.0 ** -11 if dtype == FH else 2.0 ** -8
    scale = float(dropout_scale(p))
    qp1 = torch.arange(1, T + 1, device=DEV, dtype=F32)
    lref = torch.log(qp1)
    for w, y, lse in fwd_outs:
        n = min(T, (w + 1) * D) - w * D
        ref = want[..., w * D:w * D + n].float() * scale / qp1.view(T, 1)
        assert ((y[..., :n] - ref).abs() <= rel * ref).all(), w
        assert (y[..., n:] == 0).all(), w
        assert ((lse - lref).abs() <= 1e-5 * lref + 1e-6).all(), w


# ================================================================ A. mask recovery
@pytest.mark.parametrize("B,H,T,D,p,bwd", [(1, 2, 200, 64, 0.2, None), (2, 3, 320, 64, 0.2, "v1"),
                                            (2, 3, 320, 64, 0.2, "v2"), (1, 1, 77, 32, 0.2, None),
                                            (1, 2, 192, 128, 0.2, None), (1, 2, 96, 64, 0.5, None)])
def test_attention_masks_are_the_replicas(kernels, flash_variant, B, H, T, D, p, bwd):
    """All four decoders return ``attn_keep_mask & causal`` exactly.  T = 200 has a ragged last
    tile and runs the generic backward at D = 64; T = 320 runs the generic (v1) and the v2
    kernels over three key blocks, the last one partial."""
    if bwd:
        flash_variant(bwd=bwd)
    want = (attn_keep_mask(B, H, T, p, SALT, STEP) & causal(T)).to(DEV)
    with _device_step():
        masks, fwd_outs = recover_masks(_kernel_run(B, H, p, SALT, BF), B, H, T, D, p)
        torch.cuda.synchronize()
    _check_fwd_values(fwd_outs, want, T, D, p, BF)
    assert sorted(masks) == ["dk", "dq", "dv", "fwd"]
    for name, m in masks.items():
        bad = (m != want).nonzero()
        assert bad.numel() == 0, (name, bad.shape[0], bad[:4].tolist())


def test_attention_masks_fp16(kernels):
    """The fp16 build draws the same mask as the bf16 build: forward and dV."""
    B, H, T, D, p = 1, 2, 200, 64, 0.2
    want = (attn_keep_mask(B, H, T, p, SALT, STEP) & causal(T)).to(DEV)
    got = {}
    with _device_step():
        for dtype in (FH, BF):
            got[dtype], fwd_outs = recover_masks(_kernel_run(B, H, p, SALT, dtype), B, H, T, D, p, which=("fwd", "dv"))
            _check_fwd_values(fwd_outs, want, T, D, p, dtype)
    for n in ("fwd", "dv"):
        assert torch.equal(got[FH][n], got[BF][n]), n
        assert torch.equal(got[FH][n], want), n


def test_attention_masks_move_with_salt_and_step(kernels):
    """The recovered mask follows the salt and the device step (one window, forward)."""
    B, H, T, D, p = 1, 2, 96, 64, 0.2
    vis = causal(T).to(DEV)
    for salt, step in ((SALT, 0), (SALT, 5), (SALT + 1, 5)):
        with _device_step(step):
            masks, _ = recover_masks(_kernel_run(B, H, p, salt, BF, backward=False), B, H, T, D, p, which=("fwd",))
        assert torch.equal(masks["fwd"], attn_keep_mask(B, H, T, p, salt, step).to(DEV) & vis), (salt, step)


def test_attention_bwd_v3_is_v2_under_dropout(kernels, flash_variant):
    """With dropout the v3 selection runs the v2 dK/dV instantiation: the same bits, on random
    inputs and on the dK/dV recovery inputs of one window."""
    B, H, T, D, p = 2, 3, 320, 64, 0.2
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(B, H, T, D, generator=g).to(DEV).to(BF) for _ in range(4))
    cases = [(pack_qkv(q, k, v), from_bhtd(do))]
    q, k, v, do = (x.to(DEV).to(BF).expand(B, H, T, D) for x in recovery_inputs("dk", T, D, 2, g))
    cases.append((pack_qkv(q, k, v), from_bhtd(do)))
    with _device_step():
        for qkv, dy in cases:
            y, lse = _flash_fwd(qkv, H, p, SALT)
            grads = {}
            for ver in ("v2", "v3"):
                flash_variant(bwd=ver)
                grads[ver] = _flash_bwd(qkv, y, dy, lse, H, p, SALT)
            torch.cuda.synchronize()
            assert not torch.isnan(grads["v2"].float()).any()
            assert torch.equal(grads["v3"].view(torch.int16), grads["v2"].view(torch.int16))


def test_attention_mask_index_is_64_bit(kernels):
    """One forward launch with B * H * T * T > 2^32: (b, h) 4095 lies below the 2^32-nd element
    and 4099 above it, where an id held in 32 bits would redraw the mask of (b, h) 3."""
    B, H, T, D, p, w = 4100, 1, 1024, 32, 0.2, 29
    rows = [4095, 4099]
    want = attn_keep_bh(rows, T, p, SALT, STEP).to(DEV) & causal(T).to(DEV)
    wrapped = attn_keep_bh([4099 - 4096], T, p, SALT, STEP).to(DEV) & causal(T).to(DEV)
    _, _, v1h, _ = recovery_inputs("p", T, D, w, torch.Generator().manual_seed(0))
    qkv = torch.zeros(B, T, 3 * D, device=DEV, dtype=BF)
    qkv[rows, :, 2 * D:] = v1h.to(DEV).to(BF)
    with _device_step():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y, lse = _flash_fwd(qkv, H, p, SALT)
        torch.cuda.synchronize()
        print(f"forward at B = {B}: {time.perf_counter() - t0:.3f} s with the NaN prefill")
    assert not torch.isnan(lse).any()
    assert not torch.isnan(y[rows].float()).any() and not torch.isnan(y[::257].float()).any()
    got = decode_fwd(y[rows].float().view(2, 1, T, D), w, T, D)[:, 0]
    sl = slice(w * D, (w + 1) * D)
    assert torch.equal(got, want[:, :, sl])
    assert not torch.equal(got[1], wrapped[0, :, sl])


# ================================================= B. random inputs against float64
def _attention_against_ref(ops, B, H, T, D, dtype, seed, p=0.2):
    q, k, v, do, salt = attn_case_inputs(B, H, T, D, dtype, seed)
    torch.manual_seed(seed)
    assert ops.functional.new_seed() == salt
    qkv = pack_qkv(q, k, v).to(DEV).to(dtype).requires_grad_(True)
    with _device_step():
        torch.manual_seed(seed)
        y = ops.attention(qkv, H, p, True)
        y.backward(from_bhtd(do).to(DEV).to(dtype))
        torch.cuda.synchronize()
    keep = attn_keep_mask(B, H, T, p, salt, STEP).to(DEV)
    ref = attn_dropout_ref(*(x.to(DEV) for x in (q, k, v, do)), keep, p)
    got = dict(o=to_bhtd(y.detach(), H))
    g = qkv.grad.view(B, T, 3, H * D)
    for i, n in enumerate(("dq", "dk", "dv")):
        got[n] = to_bhtd(g[:, :, i], H)
    fails = []
    for n in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all(), n
        err = (got[n].to(F64) - ref[n]).abs()
        if n == "o":
            bound = 2.0 ** -5 * ref["mag_o"] + 2.0 ** -7 * ref["o"].abs() + 1e-4
            print(f"worst ratio {n}: {(err / bound).max().item():.4f}")
        else:
            bound = GRAD_C[dtype] * ref["mag_" + n] + 1e-5
            print(f"worst ratio {n}: {(err / bound).max().item():.4f}; worst (err - 1e-5) / mag "
                  f"{worst_ratio(err, ref['mag_' + n], 1e-5):.4f} of c = {GRAD_C[dtype]}")
        bad = (err > bound).nonzero()
        if bad.numel():
            i = tuple(bad[0].tolist())
            fails.append(f"{n}: {bad.shape[0]} elements, first (b, h, t, d) = {i}: got {got[n][i].item()}, "
                         f"ref {ref[n][i].item()}, bound {bound[i].item()}")
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("case,bwd", [(0, None), (1, "v1"), (1, "v2"), (2, None), (3, None)])
def test_attention_dropout_against_float64(kernels, flash_variant, case, bwd):
    """y and the three gradients, every element, at the four shapes of A with p = 0.2; an
    element whose terms are all dropped has magnitude 0 and must be within the absolute term."""
    from nanosandbox_amd import ops

    if bwd:
        flash_variant(bwd=bwd)
    _attention_against_ref(ops, *ATTN_CASES[case], BF, case)


def test_attention_dropout_against_float64_fp16(kernels):
    from nanosandbox_amd import ops

    _attention_against_ref(ops, *ATTN_CASES[0], FH, 0)


# ============================================================ C. workgroup orders
def _attention_bits(ops, qkv, dy, H, p):
    x = qkv.clone().requires_grad_(True)
    torch.manual_seed(9)
    y = ops.attention(x, H, p, True)
    y.backward(dy)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all() and torch.isfinite(x.grad.float()).all()
    return y.detach().view(torch.int16), x.grad.view(torch.int16)


@pytest.mark.parametrize("B,H,T", [(1, 3, 320), (2, 3, 200)])
@pytest.mark.parametrize("order", [1, 2])
def test_attention_workgroup_orders_keep_the_bits(kernels, flash_variant, order, B, H, T):
    """Grids of 9 and 12 workgroups (6 for v5), none a multiple of 8: the XCD remap takes its
    remainder branch.  Each workgroup does the same arithmetic wherever it runs, so the forward
    (v1, v5, v1 with dropout) and the v2 backward (with and without dropout) give order 0's bits."""
    from nanosandbox_amd import ops

    D = 64
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(DEV).to(BF)
    dy = torch.randn(B, T, H * D, generator=g).to(DEV).to(BF)
    runs = [("v1", 0.0), ("v5", 0.0), ("v1", 0.2)]
    with _device_step():
        for fwd, p in runs:
            flash_variant(fwd=fwd, bwd="v2", order=0)
            y0, g0 = _attention_bits(ops, qkv, dy, H, p)
            flash_variant(order=order)
            y1, g1 = _attention_bits(ops, qkv, dy, H, p)
            assert torch.equal(y1, y0), (fwd, p)
            assert torch.equal(g1, g0), (fwd, p)


def test_attention_masks_under_order_1(kernels, flash_variant):
    """Forward and dV mask recovery with the XCD-grouped order (the forward and the v2 dK/dV
    kernel both map their workgroup through it; 18 workgroups)."""
    B, H, T, D, p = 2, 3, 320, 64, 0.2
    flash_variant(bwd="v2", order=1)
    want = (attn_keep_mask(B, H, T, p, SALT, STEP) & causal(T)).to(DEV)
    with _device_step():
        masks, fwd_outs = recover_masks(_kernel_run(B, H, p, SALT, BF), B, H, T, D, p, which=("fwd", "dv"))
    _check_fwd_values(fwd_outs, want, T, D, p, BF)
    for n in ("fwd", "dv"):
        assert torch.equal(masks[n], want), n


# ============================================================ D. embedding
EMB_SHAPES = [(3, 77, 65, 384), (4, 64, 300, 256), (2, 200, 50304, 768)]


class _P(torch.nn.Parameter):
    pass


def _param(t, fused):
    p = _P(t.float().clone())
    if fused:
        p.main_grad = torch.zeros_like(p, dtype=F32)
    p.compute = p.detach().to(BF)
    return p


def _emb_inputs(B, T, V, C, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, V, (B, T), generator=g).to(DEV)
    idx[0, :5] = 3  # one row with repeated tokens
    wte = (torch.randn(V, C, generator=g) * 0.02).to(DEV)
    wpe = (torch.randn(T + 5, C, generator=g) * 0.02).to(DEV)
    dx = torch.randn(B, T, C, generator=g).to(DEV)
    return idx, wte, wpe, dx


@pytest.mark.parametrize("form", ["x32", "x32_h", "bf16"])
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("B,T,V,C", EMB_SHAPES)
def test_embedding_dropout_forward_bits(kernels, B, T, V, C, p, form):
    """nsa_embedding_fwd_x32 (bf16 and fp16 weights) and nsa_embedding_fwd (bf16 stream) into a
    NaN-prefilled output: where(keep, (wte[idx] + wpe[t]) * scale, 0), every bit."""
    from nanosandbox_amd.ops import _lib

    idx, wte, wpe, _ = _emb_inputs(B, T, V, C, 20)
    wdt = FH if form == "x32_h" else BF
    odt = BF if form == "bf16" else F32
    wte, wpe = wte.to(wdt), wpe.to(wdt)
    out = _nan(B, T, C, dtype=odt)
    name = {"x32": "nsa_embedding_fwd_x32", "x32_h": "nsa_embedding_fwd_x32_h", "bf16": "nsa_embedding_fwd"}[form]
    with _device_step():
        _lib.call(name, _lib.ptr(idx), _lib.ptr(wte), _lib.ptr(wpe), _lib.ptr(out), B * T, T, C, p, SALT, _lib.stream())
        torch.cuda.synchronize()
    ref, _ = emb_dropout_ref(idx, wte, wpe, None, p, SALT, STEP, dtype=odt)
    assert not torch.isnan(out.float()).any()
    assert torch.equal(out, ref)
    kept = (out != 0).float().mean().item()
    assert abs(kept - (1 - p)) < 0.01


@pytest.mark.parametrize("xdt", [F32, BF], ids=["dx32", "dx16"])
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("shape,path,fused", [(0, "atomic", True), (0, "sorted", True), (0, "lds", True),
                                              (1, "atomic", True), (1, "sorted", True), (2, "atomic", True),
                                              (2, "sorted", True), (0, "lds", False), (1, "atomic", False)])
def test_embedding_dropout_backward(kernels, monkeypatch, shape, path, fused, p, xdt):
    """dwte and dwpe of ``ops.embedding`` with dropout, every element within the fp32 summation
    bound (n + 2) 2^-24 sum |terms| + 2^-126 of the float64 reference, on the atomic, the sorted
    and the LDS-privatised backward (the LDS table holds V x C = 65 x 384 only), for an fp32 and
    a bf16 stream; elements with no kept term, untouched rows of wte among them, are exactly 0."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.ops import functional as Fn

    B, T, V, C = EMB_SHAPES[shape]
    monkeypatch.setattr(Fn, "_EMB_SORTED_MIN_TOKENS", 0 if path == "sorted" else 1 << 40)
    if path != "lds":
        monkeypatch.setattr(Fn, "_SEG_LDS_BYTES", 0)
    assert Fn._seg_lds_fits(V, C) == (path == "lds")
    idx, wte0, wpe0, dx = _emb_inputs(B, T, V, C, 21)
    dx = dx.to(xdt)
    wte, wpe = _param(wte0, fused), _param(wpe0, fused)
    seed = 30 + shape
    torch.manual_seed(seed)
    salt = ops.functional.new_seed()
    with _device_step():
        torch.manual_seed(seed)
        x = ops.embedding(idx, wte, wpe, p, True, dtype=xdt)
        x.backward(dx)
        torch.cuda.synchronize()
    xr, g = emb_dropout_ref(idx, wte.compute, wpe.compute, dx, p, salt, STEP, dtype=xdt)
    assert torch.equal(x.detach(), xr)
    gwte = wte.main_grad if fused else wte.grad
    gwpe = wpe.main_grad if fused else wpe.grad
    assert gwte.dtype == F32 and gwpe.dtype == F32
    assert (gwpe[T:] == 0).all()
    untouched = g["n_wte"].sum(1) == 0
    assert untouched.any() or V < B * T
    for name, got, ref, n, a in (("dwte", gwte, g["dwte"], g["n_wte"], g["abs_wte"]),
                                 ("dwpe", gwpe[:T], g["dwpe"], g["n_wpe"], g["abs_wpe"])):
        assert torch.isfinite(got).all(), name
        err = (got.to(F64) - ref).abs()
        bound = fp32_sum_bound(n, a)
        print(f"worst ratio {name}: {(err / bound).max().item():.4f}")
        bad = (err > bound).nonzero()
        assert bad.numel() == 0, (name, bad.shape[0], bad[0].tolist())
        assert (got[n == 0] == 0).all(), name
