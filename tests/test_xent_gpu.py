"""The cross-entropy kernels (``xent.hip`` and the small kernels of ``xent_fused.hip``) element
by element.

Every entry point is called raw through ``_lib.call`` with buffers this module owns: each tensor
a kernel sees lies between sentinel guards that are compared bit for bit after every call,
outputs are NaN-prefilled (gW holds known non-zero values: the dW kernels accumulate), and every
element is compared with the float64 references of ``test_xent_refs.py`` under the bounds
derived there, whose docstring lists the worst error / bound each output reached on an MI355X.
``FWD_CASES`` there lists the (variant, V, ld) of the separate pass and ``xent_branch`` the
branch of ``xent_entry`` each reaches.
"""

import numpy as np
import pytest
import torch

from test_layernorm_gpu import DEV, HIP_INVALID_VALUE, Bufs, _bits, _call, _within
from test_xent_refs import (BF, FH, FILLS, FWD_CASES, PATTERNS, U, bwd_prep_ref, combine_inputs, combine_ref,
                            dw_fix_ref, dw_inputs, fill_value, fixup_ref, fused_inputs, tlogit_ref, xent_branch,
                            xent_fwd_bounds, xent_fwd_ref, xent_k_sum, xent_rows)

pytestmark = pytest.mark.gpu

I32 = torch.int32
DTYPES = pytest.mark.parametrize("dtype", [BF, FH], ids=["bf16", "fp16"])


def _sym(name, dtype):
    return name + ("_h" if dtype == FH else "")


def _tag(dtype):
    return "bf16" if dtype == BF else "fp16"


def _code(name, *args):
    """hipError_t of an entry point (``_call`` raises on any but 0)."""
    from nanosandbox_amd.ops import _lib
    fn = getattr(_lib.lib(), name)
    return fn(*[_lib.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _lib.stream())


# ======================================================================== the separate pass
def _run_fwd(lg, tg, V, variant, dtype, write_grad, tag):
    """One call of nsa_xent_fwd(_h) on guarded copies, every output against float64 and the
    exact assertions; returns (loss, the logits buffer afterwards)."""
    N, ld = lg.shape
    B = Bufs()
    buf, tgd, loss = B.put(lg), B.put(tg), B.nan(N)
    before = buf.clone()
    _call(_sym("nsa_xent_fwd", dtype), buf, tgd, loss, N, V, ld, write_grad | (variant << 8))
    B.check(tag)
    r = xent_fwd_ref(before, tgd, V)
    b_loss, b_grad, hu, _ = xent_fwd_bounds(r, dtype, xent_k_sum(variant, V, ld))
    _within(f"{tag} loss", loss, r.loss, b_loss)
    assert not loss[~r.valid].any(), tag  # an invalid row: loss 0.0
    if not write_grad:  # the logits stay bit for bit
        assert torch.equal(_bits(buf), _bits(before)), tag
        return loss, buf
    _within(f"{tag} grad", buf, r.grad, b_grad + hu)
    assert not buf[~r.valid].any() and not buf[:, V:].any(), tag  # invalid rows and padding columns: zero
    return loss, buf


@DTYPES
@pytest.mark.parametrize("case", range(len(FWD_CASES)), ids=[f"v{v}-V{V}-ld{ld}" for v, V, ld in FWD_CASES])
def test_separate_pass_every_branch(kernels, case, dtype):
    """Every branch of ``xent_entry`` and the geometry edges of its kernels (``FWD_CASES``): 5 or
    9 rows, every row pattern, write_grad 1 and 0, and with ld > V the three padding fills."""
    variant, V, ld = FWD_CASES[case]
    N = 9 if case % 2 else 5
    tag = f"{xent_branch(variant, ld)[0]}/{_tag(dtype)}"
    for first in range(0, len(PATTERNS), N):
        lg, tg, _ = xent_rows(N, V, ld, seed=case, dtype=dtype, first=first)
        for fill in (FILLS if V < ld else FILLS[:1]):
            lg[:, V:] = fill_value(fill, dtype)
            _run_fwd(lg, tg, V, variant, dtype, 1, tag)
            if first == 0:
                _run_fwd(lg, tg, V, variant, dtype, 0, tag)


@DTYPES
@pytest.mark.parametrize("V,ld", [(7, 8), (8200, 8200), (50257, 50304), (57343, 57344)])
def test_variants_of_1024x7_are_bitwise_equal(kernels, V, ld, dtype):
    """Variants 0 (plain at this size), 3, 4, 5 (nontemporal loads and / or stores, the packed
    conversion) and 6 on the same input: loss and gradient bit for bit, as xent.hip claims."""
    lg, tg, _ = xent_rows(9, V, ld, seed=ld, dtype=dtype, fill="nan")
    outs = [_run_fwd(lg, tg, V, v, dtype, 1, f"{xent_branch(v, ld)[0]}/{_tag(dtype)}") for v in (0, 3, 4, 5, 6)]
    for loss, grad in outs[1:]:
        assert torch.equal(_bits(loss), _bits(outs[0][0])) and torch.equal(_bits(grad), _bits(outs[0][1]))


def test_default_at_256_mib_is_the_nontemporal_kernel(kernels):
    """16384 x 8192 bf16 logits are exactly NSA_NT_MIN_BYTES: variant 0 takes the nontemporal
    instantiation there (deterministic training at GPT-2 shapes runs it); bit for bit equal to
    the plain one (variant 6), and the first rows against float64."""
    N, V, ld = 16384, 8191, 8192
    assert N * ld * 2 == 256 << 20 and xent_branch(0, ld, N * ld * 2)[0] == "nt_ls"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    B = Bufs()
    src = (torch.randn(N, ld, device=DEV, generator=gen) * 2).to(BF)
    tg = B.put(torch.randint(-1, V + 1, (N,), device=DEV, generator=gen))
    a, b, la, lb = B.put(src), B.put(src), B.nan(N), B.nan(N)
    _call("nsa_xent_fwd", a, tg, la, N, V, ld, 1)
    _call("nsa_xent_fwd", b, tg, lb, N, V, ld, 1 | (6 << 8))
    B.check("nt")
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(la), _bits(lb))
    r = xent_fwd_ref(src[:9], tg[:9], V)
    b_loss, b_grad, hu, _ = xent_fwd_bounds(r, BF, xent_k_sum(3, V, ld))
    _within("nt_ls@256MiB/bf16 loss", la[:9], r.loss, b_loss)
    _within("nt_ls@256MiB/bf16 grad", a[:9], r.grad, b_grad + hu)
    assert torch.isfinite(la).all() and torch.isfinite(a).all()


@DTYPES
def test_separate_pass_rejects_ld_below_v(kernels, dtype):
    lg, tg, _ = xent_rows(5, 8, 8, seed=1, dtype=dtype)
    B = Bufs()
    buf, tgd, loss = B.put(lg), B.put(tg), B.nan(5)
    for variant in range(7):
        assert _code(_sym("nsa_xent_fwd", dtype), buf, tgd, loss, 5, 16, 8, 1 | (variant << 8)) == HIP_INVALID_VALUE
    B.check("ld<V")
    assert torch.equal(_bits(buf.cpu()), _bits(lg)) and torch.isnan(loss).all()


# ========================================================================== target logit
@DTYPES
@pytest.mark.parametrize("M", [1, 5, 8])
@pytest.mark.parametrize("C", [8, 64, 512, 520, 768, 8192])
def test_tlogit(kernels, C, M, dtype):
    """c_r within the dot-product bound (exactly the shift on an invalid row) and t32 exactly:
    every target kind in every wave slot, C off the lane loop's 512, rows 8 columns wider than C."""
    V, Vp = 65, 256
    for first in range(7):
        x, W, tg, _ = fused_inputs(M, C, V, Vp, seed=C + M + first, dtype=dtype, first=first, ldx=C + 8)
        for shift in (0.0, 3.5):
            B = Bufs()
            xd, Wd, tgd = B.put(x), B.put(W), B.put(tg)
            crow, t32 = B.nan(M), B.put(torch.full((M,), -7, dtype=I32))
            _call(_sym("nsa_xent_tlogit", dtype), xd, C + 8, Wd, C, tgd, crow, t32, M, C, V, shift)
            B.check("tlogit")
            r = tlogit_ref(xd, Wd, tgd, C, V, shift)
            _within(f"tlogit/{_tag(dtype)} crow", crow, r.crow, r.k * U * r.scale)
            assert torch.equal(t32, r.t32)
            assert (crow[r.t32 < 0] == shift).all()


@DTYPES
def test_tlogit_rejects_c_off_8(kernels, dtype):
    x, W, tg, _ = fused_inputs(4, 16, 65, 256, seed=1, dtype=dtype)
    B = Bufs()
    xd, Wd, tgd, crow, t32 = B.put(x), B.put(W), B.put(tg), B.nan(4), B.put(torch.full((4,), -7, dtype=I32))
    assert _code(_sym("nsa_xent_tlogit", dtype), xd, 16, Wd, 16, tgd, crow, t32, 4, 12, 65, 0.0) == HIP_INVALID_VALUE
    B.check("tlogit C % 8")
    assert torch.isnan(crow).all() and (t32 == -7).all()


# ================================================================================ combine
@pytest.mark.parametrize("M", [1, 255, 257])
@pytest.mark.parametrize("slots", [1, 7, 8, 9, 394])
def test_combine(kernels, slots, M):
    """S at the edges of the keep range (0.5 and the fp32 value below it, fp32(1e30) and the
    value above it, inf, NaN; ignored rows with a finite, an inf and a NaN sum): nfix exactly,
    the fix list as a set, loss and 1 / S within the bound on kept rows and exactly 0 elsewhere."""
    for first in (range(11) if M == 1 else (0,)):
        part, t32, _, lo, hi = combine_inputs(slots, M, seed=slots + M, first=first)
        shift = 0.25 * (first % 2)
        B = Bufs()
        pd, td = B.put(part), B.put(t32)
        loss, inv = B.nan(M), B.nan(M)
        nfix, fixlist = B.put(torch.zeros(1, dtype=I32)), B.put(torch.full((M,), -1, dtype=I32))
        _call("nsa_xent_combine", pd, slots, td, loss, inv, nfix, fixlist, M, lo, hi, shift)
        B.check("combine")
        r = combine_ref(pd, td, lo, hi, shift)
        n = int(nfix.item())
        assert n == int(r.flag.sum())
        assert sorted(fixlist[:n].tolist()) == r.flag.nonzero()[:, 0].tolist() and (fixlist[n:] == -1).all()
        _within("combine loss", loss, r.loss, r.b_loss)
        _within("combine invS", inv, r.invS, r.b_inv)
        assert not loss[~r.keep].any() and not inv[~r.keep].any()


# ================================================================================= fix-up
def _fixup(dtype, M, C, V, Vp, rows, seed):
    x, W, tg, _ = fused_inputs(M, C, V, Vp, seed=seed, dtype=dtype, ldx=C + 8)
    x[1::3] = (x[1::3].float() * 20).to(dtype)  # flagged rows: logits far from the target's
    g = torch.Generator().manual_seed(seed)
    E0 = (torch.rand(M, Vp, generator=g) + 0.5).to(dtype)
    loss0, inv0 = torch.rand(M, generator=g) + 1, torch.rand(M, generator=g) + 2
    B = Bufs()
    xd, Wd, E, loss, inv = B.put(x), B.put(W), B.put(E0), B.put(loss0), B.put(inv0)
    t32 = B.put(tlogit_ref(x, W, tg, C, V, 0.0).t32)
    nfix = B.put(torch.tensor([len(rows)], dtype=I32))
    fixlist = B.put(torch.tensor(rows + [0] * (M - len(rows)), dtype=I32))
    _call(_sym("nsa_xent_fixup", dtype), xd, C + 8, Wd, C, E, Vp, t32, nfix, fixlist, loss, inv, C, V, Vp)
    tag = f"fixup/{_tag(dtype)}"
    B.check(tag)
    keep = torch.ones(M, dtype=torch.bool)
    keep[rows] = False
    for got, was in ((E, E0), (loss, loss0), (inv, inv0)):  # every unflagged row bit for bit
        assert torch.equal(_bits(got.cpu()[keep]), _bits(was[keep])), tag
    if not rows:
        return
    rd = torch.tensor(rows, device=DEV)
    r = fixup_ref(xd, Wd, t32, rd, C, V, Vp, dtype)
    assert bool(r.ign.any()) and not bool(r.ign.all())
    _within(f"{tag} E", E[rd], r.E, r.b_E + r.hu_E)
    # an ignored row: its whole Vpad row of E zero, loss and 1 / S as they were (the 0 that
    # nsa_xent_combine wrote: bound 0 there, so bit for bit the prefill)
    _within(f"{tag} loss", loss[rd], torch.where(r.ign, loss0.to(DEV)[rd].double(), r.loss), r.b_loss)
    _within(f"{tag} invS", inv[rd], torch.where(r.ign, inv0.to(DEV)[rd].double(), r.invS), r.b_inv)
    assert not E[rd][:, V:].any() and not E[rd][r.ign].any()


@DTYPES
@pytest.mark.parametrize("V,Vp", [(65, 256), (1000, 1024), (256, 256)])
@pytest.mark.parametrize("C", [8, 264, 8192])
def test_fixup(kernels, C, V, Vp, dtype):
    """An empty list writes nothing; a list of 3 rows (one ignored) per element: E, its zero
    padding, loss, 1 / S; every unflagged row of E, loss and 1 / S bit-unchanged."""
    _fixup(dtype, 9, C, V, Vp, [], seed=C + V)
    _fixup(dtype, 9, C, V, Vp, [7, 2, 4], seed=C + V)


@DTYPES
def test_fixup_more_rows_than_workgroups(kernels, dtype):
    """1100 listed rows on the grid of 1024: some workgroups take two rows."""
    rows = torch.randperm(1100, generator=torch.Generator().manual_seed(3)).tolist()
    _fixup(dtype, 1100, 8, 65, 256, rows, seed=77)


@DTYPES
def test_fixup_rejects_rows_wider_than_lds(kernels, dtype):
    z = torch.zeros(1, 8208, device=DEV, dtype=dtype)
    i = torch.zeros(4, device=DEV, dtype=I32)
    f = torch.zeros(4, device=DEV)
    assert _code(_sym("nsa_xent_fixup", dtype), z, 8208, z, 8208, z, 8, i, i, i, f, f, 8200, 1, 8) == HIP_INVALID_VALUE
    torch.cuda.synchronize()


# ====================================================================== backward prologue
@DTYPES
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("C", [8, 520, 768])
def test_bwd_prep_bit_exact(kernels, C, M, dtype):
    """coef, wrows and xs bit for bit against the fp32 replica (sc = g * invS, one multiply,
    round to nearest even), the signed zeros of ignored rows included; an ignored row gathers W[0]."""
    V, Vp = 65, 256
    for first in range(7):
        x, W, tg, _ = fused_inputs(M, C, V, Vp, seed=C + M + first, dtype=dtype, first=first, ldx=C + 8)
        t32 = tlogit_ref(x, W, tg, C, V, 0.0).t32
        inv = torch.where(t32 >= 0, torch.rand(M, generator=torch.Generator().manual_seed(first)) + 0.5, torch.zeros(M))
        for g in (float(np.float32(1.0 / 7)), -float(np.float32(3.0 / 11))):
            B = Bufs()
            xd, Wd, td, invd, gsc = B.put(x), B.put(W), B.put(t32), B.put(inv), B.put(torch.tensor([g]))
            coef, wrows, xs = B.nan(M, 2), B.nan(M, C, dt=dtype), B.nan(M, C, dt=dtype)
            _call(_sym("nsa_xent_bwd_prep", dtype), xd, C + 8, Wd, C, td, invd, gsc, coef, wrows, xs, M, C)
            B.check("bwd_prep")
            rc, rw, rx = bwd_prep_ref(xd, Wd, td, invd, g, C)
            assert torch.equal(_bits(coef), _bits(rc))
            assert torch.equal(_bits(wrows), _bits(rw)) and torch.equal(_bits(xs), _bits(rx))
            ign = td < 0
            if ign.any():
                assert torch.equal(_bits(wrows[ign]), _bits(Wd[:1, :C].expand(int(ign.sum()), C)))
                assert torch.equal(_bits(xs[ign]) < 0, (xd[ign][:, :C].float() < 0) != (g < 0))


# ======================================================================== the onehot dW term
@DTYPES
@pytest.mark.parametrize("V,Vp", [(65, 256), (1000, 1024)])
@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("N", [37, 1100])
def test_onehot_dw_three_forms(kernels, N, C, V, Vp, dtype):
    """nsa_xent_dw_fix (fp32 atomics), _sorted (keys from ops.sort_keys) and _lds on the same
    inputs: skewed targets (one long segment), ignored rows, vocabulary rows without a target.
    Per element against float64 with a bound proportional to the segment length; rows of gW
    without a target keep the prefill bit for bit.  Where the V x C table does not fit the LDS
    form's budget it returns hipErrorInvalidValue and writes nothing."""
    from nanosandbox_amd.ops import _lib
    from nanosandbox_amd.ops import functional as Fn
    d = dw_inputs(N, C, V, Vp, seed=N + C + V, dtype=dtype)
    B = Bufs()
    x, E, t32, inv, gsc = B.put(d.x), B.put(d.E), B.put(d.t32), B.put(d.invS), B.put(torch.tensor([d.g]))
    gw0 = d.gw0.to(DEV)
    G = _lib.call_ret("nsa_seg_lds_parts", N)
    for form in ("atomic", "sorted", "lds"):
        gw = B.put(d.gw0)
        tag = f"dw_{form}/{_tag(dtype)}"
        if form == "atomic":
            _call(_sym("nsa_xent_dw_fix", dtype), x, C, E, Vp, t32, inv, gsc, gw, C, N, C)
        elif form == "sorted":
            ids, order, seg = Fn.sort_keys(t32, Vp)
            part = B.nan(2 * (-(-N // 16)), C)
            _call(_sym("nsa_xent_dw_fix_sorted", dtype), x, C, E, Vp, t32, inv, gsc, ids, order, seg, part, gw, C, N,
                  C, Vp)
        else:
            part = B.nan(G, V * C)
            args = (x, C, E, Vp, t32, inv, gsc, part, gw, C, N, C, V)
            if not Fn._seg_lds_fits(V, C):
                assert _code(_sym("nsa_xent_dw_fix_lds", dtype), *args) == HIP_INVALID_VALUE
                B.check(tag)
                assert torch.equal(_bits(gw), _bits(gw0)) and torch.isnan(part).all()
                continue
            _call(_sym("nsa_xent_dw_fix_lds", dtype), *args)
        B.check(tag)
        r = dw_fix_ref(x, E, t32, inv, d.g, Vp, C, gw0, extra=G // 4 + 4 if form == "lds" else 2)
        assert 0 < int(r.hit.sum()) < V and int((t32 == 3).sum()) > (64 if N > 1000 else 8)
        _within(f"{tag} gW", gw, r.gw, r.bound)
        assert torch.equal(_bits(gw[~r.hit]), _bits(gw0[~r.hit])), tag
