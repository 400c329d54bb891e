"""The attention kernels without dropout (the path every GPT-2 configuration trains on) against the
float64 reference of ``test_flash_refs.py``, per element.

Every launch goes through the raw entry points (``nsa_flash_fwd(_h)``, ``nsa_flash_bwd2(_h)``) with
each tensor inside a larger flat allocation: the outputs (y, lse, dqkv, the 2 x [B, H, T]
workspace) NaN-prefilled between two canary zones of at least one row, the inputs (qkv, dy) between
zones of a large finite value (2^14), which a kernel that reads a row >= T meets unmasked.  After a
call no output element is NaN (the generic backward writes only the first half of the workspace)
and every zone is untouched.

A. Forward, random inputs: v1 and v5 at D = 64 and the register-staged v1 at D = 32 / 128, at the
   smallest T where each loop structure changes (``FWD_CASES``); y and lse per element.
B. Backward at every branch (``BWD_CASES``: the generic kernels at D = 32 / 128 and at ragged T,
   v2 and v3 at D = 64), behind the project's own forward, on four input families: random, and
   three that route a query slice or a key tile or a key row into an output column of its own, so
   that a slice or tile a kernel skips, visits twice or masks wrongly is a column off by its whole
   magnitude.  y, lse, dQ, dK, dV per element.
C. fp16 build: one case per branch of A and B.
D. Bits: two runs agree; workgroup orders 1 and 2 give order 0's bits with the default (v3)
   backward; v1 and v5 agree on lse within twice its bound; ``fwd="auto"`` is v5 from 4096
   workgroups on without dropout and v1 below that or with dropout.

The bounds and their constants come from the fp32 emulation of the kernels' rounding points
(``test_flash_refs.FLASH_C``, ``LSE_C``; CPU checks recompute them and show that eight planted
defects are rejected at every T).  Each test prints its worst err / bound (``-s`` shows them).
On an MI355X the kernels' own worst err / bound were (all 180 tests within their bounds):

    forward         bf16  v1: y 0.145 lse 0.042   v5: y 0.173 lse 0.058   D = 32 / 128: y 0.151 lse 0.050
                    fp16  v1: y 0.018 lse 0.039   v5: y 0.021 lse 0.045
    backward bf16   generic  random dq 0.052 dk 0.113 dv 0.058   qzero dq 0.279 dv 0.161
                             kzero dk 0.181 dv 0.195             krow dq 0.207 dv 0.145
                    v2 = v3  random dq 0.139 dk 0.079 dv 0.051   qzero dq 0.243 dv 0.161
                             kzero dk 0.174 dv 0.193             krow dq 0.191 dv 0.144
    backward fp16   generic  random dq 0.101 dk 0.209 dv 0.195   qzero dq 0.234 dv 0.140
                             kzero dk 0.291 dv 0.257             krow dq 0.382 dv 0.221
                    v2 = v3  random dq 0.231 dk 0.195 dv 0.194   qzero dq 0.198 dv 0.140
                             kzero dk 0.288 dv 0.220             krow dq 0.239 dv 0.216
    lse of v1 against v5: 0.029 of twice the bound

(dK of "qzero" / "krow" and dQ of "kzero" are exactly 0, as their references are.)
"""

import contextlib
import math

import pytest
import torch

from test_dropout_refs import BF, F32, FH, STEP, from_bhtd, pack_qkv, to_bhtd
from test_flash_refs import (B, BWD_CASES, BWD_CASES_FP16, FAMILIES, FWD64_T, FWD_CASES, FWD_CASES_FP16, H, bounds,
                             case_data, case_id, check_outputs, first_miss)

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 2.0 ** 14    # around the inputs: large, finite, exact in bf16 and fp16
CANARY = -1024.0     # around the outputs
SALT = 0x2545F4914F6CDD1D >> 2


@pytest.fixture
def flash_variant(kernels):
    """ops.functional.flash_variant as a fixture: selects kernels for one test, restores after."""
    from nanosandbox_amd.ops.functional import flash_variant as fv

    stack = contextlib.ExitStack()
    with stack:
        yield lambda **kw: stack.enter_context(fv(**kw))


# ------------------------------------------------------------------------------ buffers
class _Buf:
    """A tensor inside a flat allocation, a zone of at least one row (``row`` elements, rounded up
    to whole 64-element blocks so the tensor keeps its alignment) on either side."""

    def __init__(self, shape, dtype, row, zone, fill=None, data=None):
        self.n = math.prod(shape)
        self.pad = (row + 63) // 64 * 64 + 64
        self.zone = zone
        self.flat = torch.full((self.n + 2 * self.pad,), zone, device=DEV, dtype=dtype)
        self.t = self.flat[self.pad:self.pad + self.n].view(shape)
        if data is not None:
            self.t.copy_(data)
        else:
            self.t.fill_(fill)
        assert self.pad >= row and self.t.data_ptr() % 128 == 0

    def zones_intact(self):
        return bool((self.flat[:self.pad] == self.zone).all() and (self.flat[self.pad + self.n:] == self.zone).all())


def _out(shape, dtype, row):
    return _Buf(shape, dtype, row, CANARY, fill=float("nan"))


def _inp(t, row):
    return _Buf(tuple(t.shape), t.dtype, row, GUARD, data=t)


def _sym(name, dtype):
    return name + "_h" if dtype == FH else name


def _flash_fwd(qkv, Hn, p=0.0, salt=0):
    """nsa_flash_fwd(_h) on a guarded qkv into guarded, NaN-prefilled y and lse."""
    from nanosandbox_amd.ops import _lib

    Bn, T, C3 = qkv.t.shape
    C = C3 // 3
    D = C // Hn
    y = _out((Bn, T, C), qkv.t.dtype, C)
    lse = _out((Bn, Hn, T), F32, T)
    _lib.call(_sym("nsa_flash_fwd", qkv.t.dtype), _lib.ptr(qkv.t), _lib.ptr(y.t), _lib.ptr(lse.t), Bn, T, Hn, D,
              1.0 / math.sqrt(D), p, salt, _lib.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(y.t.float()).any(), "y has elements the forward did not write"
    assert not torch.isnan(lse.t).any(), "lse has elements the forward did not write"
    for name, b in (("y", y), ("lse", lse), ("qkv", qkv)):
        assert b.zones_intact(), f"the forward wrote outside {name}"
    return y, lse


def _flash_bwd(qkv, y, dy, lse, Hn, v2):
    """nsa_flash_bwd2(_h) into a guarded, NaN-prefilled dqkv and workspace.  ``v2``: the launch
    runs the v2 / v3 kernels, which write both halves of the workspace (the generic ones only
    delta, the first)."""
    from nanosandbox_amd.ops import _lib

    Bn, T, C3 = qkv.t.shape
    D = C3 // 3 // Hn
    dqkv = _out((Bn, T, C3), qkv.t.dtype, C3)
    ws = _out((2, Bn, Hn, T), F32, T)
    _lib.call(_sym("nsa_flash_bwd2", qkv.t.dtype), _lib.ptr(qkv.t), _lib.ptr(y.t), _lib.ptr(dy.t), _lib.ptr(lse.t),
              _lib.ptr(ws.t), _lib.ptr(dqkv.t), Bn, T, Hn, D, 1.0 / math.sqrt(D), 0.0, 0, _lib.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(dqkv.t.float()).any(), "dqkv has elements the backward did not write"
    assert not torch.isnan(ws.t[0] if not v2 else ws.t).any(), "the workspace has elements the backward did not write"
    for name, b in (("dqkv", dqkv), ("ws", ws), ("qkv", qkv), ("dy", dy), ("y", y), ("lse", lse)):
        assert b.zones_intact(), f"the backward wrote outside {name}"
    return dqkv, ws


def _upload(x, dtype):
    """(qkv, dy) of CPU inputs q, k, v, do [B, H, T, D], guarded, and the bits they hold."""
    q, k, v, do = x
    Hn, D = q.shape[1], q.shape[3]
    qkv = _inp(pack_qkv(q, k, v).to(dtype).to(DEV), 3 * Hn * D)
    dy = _inp(from_bhtd(do).to(dtype).to(DEV), Hn * D)
    return qkv, dy


def _unpack(y, lse, dqkv=None):
    """The kernels' outputs as CPU fp32 [B, H, T, D] ([B, H, T] for lse)."""
    Hn = lse.t.shape[1]
    got = dict(y=to_bhtd(y.t.float().cpu(), Hn), lse=lse.t.cpu())
    if dqkv is not None:
        Bn, T, C3 = dqkv.t.shape
        g = dqkv.t.float().cpu().view(Bn, T, 3, C3 // 3)
        for i, n in enumerate(("dq", "dk", "dv")):
            got[n] = to_bhtd(g[:, :, i], Hn)
    return got


def _assert_within(got, ref, dtype, family, names, tag):
    ratios = check_outputs(got, ref, dtype, family, names)
    print(f"flash-ratio {tag} {family}: " + ", ".join(f"{n} {r:.4f}" for n, r in ratios.items()))
    fails = []
    for n, r in ratios.items():
        if not r <= 1.0:
            cnt, i, g, w, b = first_miss(got, ref, dtype, family, n)
            fails.append(f"{n}: {cnt} elements, worst err / bound {r:.3f}, first (b, h, t[, d]) = {i}: got {g}, "
                         f"ref {w}, bound {b}")
    assert not fails, "; ".join(fails)


def _forward_case(flash_variant, case, dtype):
    fwd, D, T = case
    if fwd:
        flash_variant(fwd=fwd)
    x, ref = case_data("random", T, D, dtype)
    qkv, _ = _upload(x, dtype)
    before = qkv.t.clone()
    y, lse = _flash_fwd(qkv, H)
    assert torch.equal(qkv.t, before)
    _assert_within(_unpack(y, lse), ref, dtype, "random", ("y", "lse"), f"fwd {case_id(case)} {dtype}")


def _backward_case(flash_variant, case, family, dtype):
    bwd, D, T = case
    if bwd:
        flash_variant(bwd=bwd)
    x, ref = case_data(family, T, D, dtype)
    qkv, dy = _upload(x, dtype)
    y, lse = _flash_fwd(qkv, H)  # the project's own forward, as in training
    v2 = D == 64 and T % 32 == 0 and bwd != "v1"
    assert v2 == (bwd in ("v2", "v3"))  # a case without a variant is one whose shape selects the generic kernels
    dqkv, _ = _flash_bwd(qkv, y, dy, lse, H, v2)
    _assert_within(_unpack(y, lse, dqkv), ref, dtype, family, ("y", "lse", "dq", "dk", "dv"),
                   f"bwd {case_id(case)} {dtype}")


# ========================================================= A, B, C: per element against float64
@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_flash_forward_against_float64(kernels, flash_variant, case):
    _forward_case(flash_variant, case, BF)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_flash_backward_against_float64(kernels, flash_variant, case, family):
    _backward_case(flash_variant, case, family, BF)


@pytest.mark.parametrize("case", FWD_CASES_FP16, ids=case_id)
def test_flash_forward_against_float64_fp16(kernels, flash_variant, case):
    _forward_case(flash_variant, case, FH)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", BWD_CASES_FP16, ids=case_id)
def test_flash_backward_against_float64_fp16(kernels, flash_variant, case, family):
    _backward_case(flash_variant, case, family, FH)


# ================================================================== D. bits that must not move
def _random_launch(Bn, Hn, T, D, seed, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(Bn, Hn, T, D, generator=g).to(dtype).float() for _ in range(4))
    return _upload((2.0 * q, k, v, do), dtype)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("bwd,T", [(None, 200), ("v2", 160), ("v3", 160)], ids=["generic-T200", "v2-T160", "v3-T160"])
def test_flash_backward_repeats_its_bits(kernels, flash_variant, bwd, T):
    """The backward has no atomics: a second run gives the same dqkv, bit for bit (each at a shape
    whose last key block is partial)."""
    if bwd:
        flash_variant(bwd=bwd)
    qkv, dy = _random_launch(B, H, T, 64, 11)
    y, lse = _flash_fwd(qkv, H)
    v2 = bwd is not None
    first, _ = _flash_bwd(qkv, y, dy, lse, H, v2)
    second, _ = _flash_bwd(qkv, y, dy, lse, H, v2)
    assert torch.equal(_bits(first.t), _bits(second.t))


@pytest.mark.parametrize("Bn,Hn,T", [(1, 3, 288), (2, 3, 160)])
@pytest.mark.parametrize("order", [1, 2])
def test_flash_workgroup_orders_keep_the_bits_v3(kernels, flash_variant, order, Bn, Hn, T):
    """Workgroup orders 1 and 2 give order 0's bits of y, lse and dqkv with the default (v3)
    backward behind either forward; grids of 9 / 12 and 6 / 12 workgroups, none a multiple of 8."""
    qkv, dy = _random_launch(Bn, Hn, T, 64, 12)
    for fwd in ("v1", "v5"):
        runs = []
        for o in (0, order):
            flash_variant(fwd=fwd, bwd="v3", order=o)
            y, lse = _flash_fwd(qkv, Hn)
            dqkv, _ = _flash_bwd(qkv, y, dy, lse, Hn, True)
            runs.append((y, lse, dqkv))
        for a, b, n in zip(*runs, ("y", "lse", "dqkv")):
            assert torch.equal(_bits(a.t), _bits(b.t)), (fwd, n)


@pytest.mark.parametrize("T", FWD64_T)
def test_flash_v1_and_v5_agree_on_lse(kernels, flash_variant, T):
    """Both forwards write lse of the same softmax: per query they are within twice its bound."""
    x, ref = case_data("random", T, 64, BF)
    qkv, _ = _upload(x, BF)
    lse = {}
    for fwd in ("v1", "v5"):
        flash_variant(fwd=fwd)
        lse[fwd] = _flash_fwd(qkv, H)[1].t.cpu().double()
    ratio = ((lse["v1"] - lse["v5"]).abs() / (2.0 * bounds(ref, BF, "random")["lse"])).max().item()
    print(f"flash-ratio lse v1 against v5, T = {T}: {ratio:.4f}")
    assert ratio <= 1.0


def _fwd_bits(qkv, Hn, p=0.0, salt=0):
    y, lse = _flash_fwd(qkv, Hn, p, salt)
    return _bits(y.t).clone(), _bits(lse.t).clone()


def test_flash_fwd_auto_threshold(kernels, flash_variant):
    """``fwd="auto"`` (the default) at D = 64, T = 32: v5's bits at B * H = 4096 workgroups, v1's at
    4095, and v1's at 4096 with dropout (same salt and device step).  The two kernels' bits differ
    on these inputs, so each equality names the kernel that ran."""
    from nanosandbox_amd import ops

    T, D = 32, 64
    for Bn, Hn, p, want in ((1024, 4, 0.0, "v5"), (1365, 3, 0.0, "v1"), (1024, 4, 0.2, "v1")):
        g = torch.Generator().manual_seed(13)
        qkv = torch.randn(Bn, T, 3 * Hn * D, generator=g)
        qkv[..., : Hn * D] *= 2.0  # q doubled, as everywhere
        qkv = _inp(qkv.to(BF).to(DEV), 3 * Hn * D)
        got = {}
        ops.rng_set(DEV, STEP)
        try:
            for fwd in ("v1", "v5", "auto"):
                flash_variant(fwd=fwd)
                got[fwd] = _fwd_bits(qkv, Hn, p, SALT)
        finally:
            ops.rng_set(DEV, 0)
            torch.cuda.synchronize()
        same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # noqa: E731
        if p == 0.0:
            assert not torch.equal(got["v1"][0], got["v5"][0]) and not torch.equal(got["v1"][1], got["v5"][1])
        else:
            assert same(got["v5"], got["v1"])  # with dropout the v5 selection runs v1
        assert same(got["auto"], got[want]), (Bn, Hn, p)
