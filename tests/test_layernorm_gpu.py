"""The LayerNorm kernels (``layernorm.hip``) element by element.

Every entry point (the ten forward / backward ones and the fp16 split-plane backward) is
called raw through ``_lib.call`` with buffers this module owns.  Each
tensor a kernel sees, input or output, lies inside a larger allocation with one row of sentinel
bytes before and after it (16 elements for the per-row statistics); the sentinels are compared
bit for bit after every call (the column-clamped loads and the N - 1 row clamp of the backward
must never turn into stores), outputs are NaN-prefilled, and every element is compared with
the float64 references of ``test_layernorm_refs.py`` under the bounds derived there, whose
docstring lists the worst error / bound each reached on an MI355X.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_layernorm_refs import (BF, CONSTANTS, F32, FH, LN_BWD_MAX_C, WIDTHS, ln_bwd_bounds, ln_bwd_ref, ln_dres, ln_dy,
                                 ln_fwd_bounds, ln_fwd_ref, ln_owner, ln_params, ln_res, ln_rows, worst)
from test_streaming_refs import F64, dropout_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
I16, I32 = torch.int16, torch.int32
EPS = 1e-5
HIP_INVALID_VALUE = 1
SENTINEL = 0x5A
NOPIPE = 1 << 30

# stream dtype, 16-bit dtype, forward and backward entry points
FAMS = {
    "x32": (F32, BF, "nsa_layernorm_fwd_x32", "nsa_layernorm_bwd_x32"),
    "x32_h": (F32, FH, "nsa_layernorm_fwd_x32_h", "nsa_layernorm_bwd_x32_h"),
    "bf16": (BF, BF, "nsa_layernorm_fwd", "nsa_layernorm_bwd"),
}


class Bufs:
    """Device buffers with sentinel guards around them."""

    def __init__(self):
        self.guards = []

    def _alloc(self, shape, dt):
        pad = 16 if len(shape) == 1 else 1
        big = torch.empty((shape[0] + 2 * pad, *shape[1:]), device=DEV, dtype=dt)
        big.view(torch.uint8).fill_(SENTINEL)
        self.guards.append((big[:pad], big[shape[0] + pad:]))
        return big[pad:shape[0] + pad]

    def put(self, t):
        """A copy of a (CPU or device) tensor between guards; None stays None."""
        if t is None:
            return None
        v = self._alloc(tuple(t.shape), t.dtype)
        v.copy_(t)
        return v

    def nan(self, *shape, dt=F32):
        v = self._alloc(shape, dt)
        v.fill_(float("nan"))
        return v

    def check(self, tag):
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(self.guards):
            for g in (a, b):
                assert bool((g.contiguous().view(torch.uint8) == SENTINEL).all()), f"{tag}: guard of buffer {i} written"


def _bits(t):
    return t.view(I32 if t.dtype == F32 else I16)


def _within(name, got, ref, bound):
    err = (got.to(F64) - ref).abs()
    print(f"worst ratio {name}: {worst(err, bound):.4f}")
    assert torch.isfinite(got).all(), name
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, (name, bad[:4].tolist(), err[tuple(bad[0])].item(), bound[tuple(bad[0])].item())


def _call(name, *args):
    from nanosandbox_amd.ops import _lib
    _lib.call(name, *[_lib.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _lib.stream())


def _inputs(fam, N, C, seed, res=True, bias=True, dres=True):
    """Guarded device copies of the input patterns of ``test_layernorm_refs`` for a family."""
    sdt, dt = FAMS[fam][:2]
    B = Bufs()
    x, names = ln_rows(N, C, seed, sdt)
    w, b = ln_params(C, seed + 1, dt, bias)
    i = dict(B=B, N=N, C=C, names=names, fam=fam, x=B.put(x), w=B.put(w), b=B.put(b),
             res=B.put(ln_res(names, C, seed + 4, dt)) if res else None, dy=B.put(ln_dy(N, C, seed + 2, dt)),
             dres=B.put(ln_dres(N, C, seed + 3, sdt)) if dres else None)
    return SimpleNamespace(**i)


def _fwd(i, tag, entry=None, extra=(), res=None):
    """The family's forward entry into guarded NaN outputs, every output against float64."""
    sdt, dt, fwd, _ = FAMS[i.fam]
    B, N, C = i.B, i.N, i.C
    i.s_out = B.nan(N, C, dt=sdt) if i.res is not None else None
    i.h, i.mean, i.rstd = B.nan(N, C, dt=dt), B.nan(N), B.nan(N)
    _call(entry or fwd, i.x, i.res, i.s_out, i.w, i.b, i.h, i.mean, i.rstd, N, C, EPS, *extra)
    B.check(tag)
    r = ln_fwd_ref(i.x, i.res if res is None else res, i.w, i.b, EPS, sdt)
    if i.res is not None:
        assert torch.equal(_bits(i.s_out), _bits(r.s)), tag
    b_mean, b_rstd, b_h = ln_fwd_bounds(r, dt)
    _within(f"{tag} mean", i.mean, r.mean, b_mean)
    _within(f"{tag} rstd", i.rstd, r.rstd, b_rstd)
    _within(f"{tag} h", i.h, r.h, b_h)
    # exact cases: a constant row (its branch row is zero) gives h = b, mean = the value and
    # rstd = eps^-1/2 to 2 ulp; a zero row likewise with mean 0
    rs = np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))
    bb = i.b if i.b is not None else torch.zeros(C, device=DEV, dtype=dt)
    for k, p in enumerate(i.names):
        if p in ("constant", "zero"):
            val = 0.0 if p == "zero" else CONSTANTS[(k // 7) % len(CONSTANTS)]
            assert i.mean[k].item() == val, (tag, k)
            assert abs(i.rstd[k].item() - float(rs)) <= 2 * float(np.spacing(rs)), (tag, k)
            assert torch.equal(i.h[k], bb), (tag, k)
    i.xin = i.s_out if i.res is not None else i.x
    return r


def _bwd(i, tag, nblk, branch=True, check_nopipe=False):
    """The family's backward entry from the forward's statistics: dx, its 16-bit copy, and
    every block's dw / db partial row against float64; with ``check_nopipe`` the non-pipelined
    body as well."""
    sdt, dt, _, bwd = FAMS[i.fam]
    B, N, C = i.B, i.N, i.C
    x32 = sdt == F32
    g = ln_bwd_ref(i.dy, i.xin, i.w, i.mean, i.rstd, i.dres, nblk)
    b_dx, b_dw, b_db = ln_bwd_bounds(g, sdt)
    owned = torch.zeros(nblk, dtype=torch.bool)
    owned[ln_owner(N, nblk)] = True
    out = None
    for flag in ((0, NOPIPE) if check_nopipe else (0,)):
        t = tag + (",nopipe" if flag else "")
        dx, dwp = B.nan(N, C, dt=sdt), B.nan(nblk, C)
        dxb = B.nan(N, C, dt=dt) if (branch and x32) else None
        dbp = B.nan(nblk, C) if i.b is not None else None
        args = (i.dy, i.xin, i.w, i.mean, i.rstd, i.dres, dx) + ((dxb,) if x32 else ()) + (dwp, dbp, N, C, nblk | flag)
        _call(bwd, *args)
        B.check(t)
        _within(f"{t} dx", dx, g.dx, b_dx)
        _within(f"{t} dw_part", dwp, g.dw, b_dw)
        if dbp is not None:
            _within(f"{t} db_part", dbp, g.db, b_db)
        # blocks that own no row write exact zeros (nsa_colsum_accum sums every partial row)
        for p in (dwp, dbp):
            if p is not None and not owned.all():
                assert not p[~owned.to(DEV)].any(), t
        if dxb is not None:  # the branch copy is the 16-bit cast of dx
            assert torch.equal(_bits(dxb), _bits(dx.to(dt))), t
        # a zero dy row passes the residual gradient through bit for bit
        zero = [k for k in range(N) if k % 5 == 3]
        want = i.dres if i.dres is not None else torch.zeros(N, C, device=DEV, dtype=sdt)
        assert torch.equal(_bits(dx[zero]), _bits(want[zero])), t
        if out is None:
            out = (dx, dxb, dwp, dbp)
        else:  # non-pipelined: the same dx bit for bit
            assert torch.equal(_bits(dx), _bits(out[0])), t
    return out


# ============================================================================== widths
@pytest.mark.parametrize("C", WIDTHS)
def test_every_width_class(kernels, C):
    """fp32 stream, bf16 compute, N = 37, nblk = 2 at the NK boundaries and remaps of
    NSA_NK_SWITCH (NK = 1, 2, 3, 4, 5 -> 6, 7 -> 8, 9 and 10 -> 16) and at the backward's limit;
    above C = 2048 the backward launches with more than 64 KiB of dynamic LDS."""
    i = _inputs("x32", 37, C, seed=C)
    tag = f"x32[37,{C},2]"
    _fwd(i, tag)
    _bwd(i, tag, 2)


def _raw_bwd_code(entry, C, split=None):
    """hipError_t of a backward entry point at N = 1 (buffers of the full size, should it launch)."""
    from nanosandbox_amd.ops import _lib
    x32 = entry != "nsa_layernorm_bwd"
    sdt = F32 if x32 else BF
    dt = FH if entry.endswith("_h") else BF
    z = lambda dt_: torch.zeros(1, C, device=DEV, dtype=dt_)  # noqa: E731
    st = torch.ones(1, device=DEV)
    a = [z(dt), z(sdt), z(dt), st, st, z(sdt), z(sdt)] + ([z(dt)] if x32 else []) + [z(F32), z(F32)]
    fn = getattr(_lib.lib(), entry)
    return fn(*[_lib.ptr(t) for t in a], 1, C, 1, *([split] if split is not None else []), _lib.stream())


@pytest.mark.parametrize("entry", ["nsa_layernorm_bwd", "nsa_layernorm_bwd_x32", "nsa_layernorm_bwd_x32_h",
                                   "nsa_layernorm_bwd_x32s", "nsa_layernorm_bwd_x32s_h"])
def test_backward_rejects_rows_wider_than_lds(kernels, entry):
    """32 C bytes of LDS: C = limit + 8 and C = 8192 are refused on the host
    (hipErrorInvalidValue), the limit itself and the Python constant agree with the library."""
    from nanosandbox_amd.ops.functional import LN_BWD_MAX_C as limit
    assert limit == LN_BWD_MAX_C and 32 * limit == 160 * 1024
    split = 0 if "x32s" in entry else None
    for C in (limit + 8, 8192):
        assert _raw_bwd_code(entry, C, split) == HIP_INVALID_VALUE
    assert _raw_bwd_code(entry, limit, split) == 0
    torch.cuda.synchronize()


def test_autograd_names_the_limit(kernels):
    """Above the backward's limit a forward that will be differentiated is refused at once with
    a message that names the limit; without gradients the forward takes C <= 8192."""
    from nanosandbox_amd import ops
    C = LN_BWD_MAX_C + 8
    x = torch.randn(2, C, device=DEV, requires_grad=True)
    w = torch.ones(C, device=DEV, requires_grad=True)
    with pytest.raises(AssertionError, match="LN_BWD_MAX_C"):
        ops.layer_norm(x, w, None, out_dtype=BF)
    with torch.no_grad():
        h = ops.layer_norm(x, w, None, out_dtype=BF)
    assert torch.isfinite(h).all()
    h = ops.layer_norm(x.detach(), w.detach(), None, out_dtype=BF)
    assert torch.isfinite(h).all() and h.grad_fn is None


# ================================================================== row and grid tails
@pytest.mark.parametrize("N,nblk", [(1, 1), (3, 1), (5, 16), (37, 1), (37, 16), (130, 3)])
@pytest.mark.parametrize("C", [8, 520, 1280])
def test_row_and_grid_tails(kernels, C, N, nblk):
    """Fewer rows than waves, N not a multiple of 4, blocks and waves without a row, one
    block for all rows, a grid stride that leaves a partial last round; pipelined and
    non-pipelined bodies."""
    i = _inputs("x32", N, C, seed=1000 * N + C)
    tag = f"x32[{N},{C},{nblk}]"
    _fwd(i, tag)
    _bwd(i, tag, nblk, check_nopipe=True)


# ======================================================================= other families
@pytest.mark.parametrize("fam,res,bias,branch", [
    ("bf16", True, True, True), ("bf16", False, True, True), ("bf16", False, False, True),
    ("x32_h", True, True, True), ("x32_h", False, False, False),
    ("x32", True, False, True), ("x32", True, True, False), ("x32", False, True, True)])
@pytest.mark.parametrize("C", [8, 520, 1280, 2056])
def test_other_families(kernels, C, fam, res, bias, branch):
    """The bf16-stream entries (as_stream rounding of the fused sum), the fp16 entries, and the
    optional tensors: res / dres, b / db_part and dx_branch null."""
    i = _inputs(fam, 37, C, seed=7 * C + len(fam), res=res, bias=bias, dres=res)
    tag = f"{fam}[37,{C},2,res={int(res)},b={int(bias)},br={int(branch)}]"
    _fwd(i, tag)
    _bwd(i, tag, 2, branch=branch, check_nopipe=(C == 520))


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("N,nblk", [(5, 16), (37, 2)])
@pytest.mark.parametrize("C", [8, 520, 1280, 2056])
@pytest.mark.parametrize("fam", ["x32", "x32_h"])
def test_split_planes_equal_plain(kernels, fam, C, N, nblk, split):
    """nsa_layernorm_bwd_x32s(_h) against nsa_layernorm_bwd_x32(_h) bit for bit: a split dres is
    read back exactly, a split dx decodes to the plain dx and its hi plane is the host encoding
    and the plain kernel's branch copy (bf16: away from exact ties, where split8 rounds away from
    zero).  The fp16 encoding keeps |g| < 2^-14 to 2^-39 absolute only: there the plain kernel
    gets the dres that the split reader sees, and a split dx is compared to 2^-39."""
    from nanosandbox_amd.ops import functional as Fn
    h = fam == "x32_h"
    dt = FAMS[fam][1]
    enc, dec = (Fn.split_planes_h, Fn.unsplit_planes_h) if h else (Fn.split_planes, Fn.unsplit_planes)
    i = _inputs(fam, N, C, seed=31 * C + N)
    B = i.B
    planes = enc(i.dres)
    if h:
        small = i.dres.abs() < 2.0 ** -14
        assert torch.equal(_bits(dec(planes))[~small], _bits(i.dres)[~small])
        i.dres = B.put(dec(planes))
    else:
        assert torch.equal(_bits(dec(planes)), _bits(i.dres))
    tag = f"{fam}s[{N},{C},{nblk},{split}]"
    _fwd(i, tag)
    dx0, dxb0, dwp0, dbp0 = _bwd(i, tag, nblk)
    din = B.put(planes) if split & 1 else i.dres
    dx1, dwp1, dbp1 = B.nan(N, C), B.nan(nblk, C), B.nan(nblk, C)
    _call("nsa_layernorm_bwd_x32s" + ("_h" if h else ""), i.dy, i.xin, i.w, i.mean, i.rstd, din, dx1, None, dwp1,
          dbp1, N, C, nblk, split)
    B.check(tag)
    if split & 2:
        back = dec(dx1)
        hi = dx1.contiguous().view(dt).reshape(-1)[:N * C].view(N, C)
        assert torch.equal(_bits(hi), _bits(enc(dx0).view(dt).reshape(-1)[:N * C].view(N, C)))
        if h:
            normal = dx0.abs() >= 2.0 ** -14
            assert torch.equal(_bits(back)[normal], _bits(dx0)[normal])
            assert ((back - dx0).abs()[~normal] <= 2.0 ** -39).all()
            assert torch.equal(_bits(hi), _bits(dxb0)) and torch.equal(_bits(hi), _bits(dx0.to(FH)))
        else:
            assert torch.equal(_bits(back), _bits(dx0))
            tie = (_bits(dx0) & 0xFFFF) == 0x8000
            assert torch.equal(_bits(hi)[~tie], _bits(dxb0)[~tie])
    else:
        assert torch.equal(_bits(dx1), _bits(dx0))
    assert torch.equal(_bits(dwp1), _bits(dwp0)) and torch.equal(_bits(dbp1), _bits(dbp0))


@pytest.mark.parametrize("fam", ["x32", "x32_h"])
@pytest.mark.parametrize("C", [8, 520, 1280, 2056])
def test_fused_dropout_forward(kernels, C, fam):
    """nsa_layernorm_fwd_x32d(_h) at p = 0.2: the sum is bit for bit x + nsa_dropout(res) for
    the same seed (the kernel's, and the host replica of its hash), h within the forward
    bound of that sum."""
    from nanosandbox_amd import ops
    p, seed = 0.2, 0x1234ABCD5678
    i = _inputs(fam, 37, C, seed=13 * C)
    dt = FAMS[fam][1]
    try:
        ops.rng_set(DEV, 0)
        dropped = i.B.nan(37, C, dt=dt)
        _call("nsa_dropout" + ("_h" if dt == FH else ""), i.res, dropped, 37 * C, p, seed)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dropped.cpu().reshape(-1)), _bits(dropout_ref(i.res.cpu().reshape(-1), p, seed, 0)))
        assert (dropped == 0).float().mean().item() > 0.05
        _fwd(i, f"{fam}d[37,{C}]", entry="nsa_layernorm_fwd_x32d" + ("_h" if dt == FH else ""), extra=(p, seed),
             res=dropped)
        assert torch.equal(_bits(i.s_out), _bits(i.x + dropped.float()))
    finally:
        ops.rng_set(DEV, 0)
        torch.cuda.synchronize()


# ===================================================================== nontemporal path
def test_nontemporal_equals_plain(kernels):
    """The nontemporal instantiations (taken from common.h's NSA_NT_MIN_BYTES = 256 MiB of
    stream upward, which the library reports) at exactly that size, fp32 stream: forward with
    the fused add and backward, every output bit for bit equal to the plain kernels on the same
    input; the flag is restored."""
    from nanosandbox_amd.ops import _lib
    N, C, nblk = 65536, 1024, 512
    # at the library's own threshold: were it raised, both passes would run the plain kernels
    assert N * C * 4 == _lib.call_ret("nsa_ln_nt_min_bytes") == 256 << 20
    gen = torch.Generator(device=DEV)
    gen.manual_seed(21)
    B = Bufs()
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)  # noqa: E731
    x, res, dy, dres = B.put(rnd(N, C) * 2 + 0.5), B.put(rnd(N, C).to(BF)), B.put(rnd(N, C).to(BF)), B.put(rnd(N, C) * 0.1)
    w, b = B.put((rnd(C) * 0.5 + 1).to(BF)), B.put((rnd(C) * 0.1).to(BF))
    outs = []
    prev = _lib.call_ret("nsa_ln_set_nt", 1)
    try:
        for nt in (1, 0):
            _lib.call_ret("nsa_ln_set_nt", nt)
            s, h, mean, rstd = B.nan(N, C), B.nan(N, C, dt=BF), B.nan(N), B.nan(N)
            dx, dxb, dwp, dbp = B.nan(N, C), B.nan(N, C, dt=BF), B.nan(nblk, C), B.nan(nblk, C)
            _call("nsa_layernorm_fwd_x32", x, res, s, w, b, h, mean, rstd, N, C, EPS)
            _call("nsa_layernorm_bwd_x32", dy, s, w, mean, rstd, dres, dx, dxb, dwp, dbp, N, C, nblk)
            outs.append((s, h, mean, rstd, dx, dxb, dwp, dbp))
    finally:
        _lib.call_ret("nsa_ln_set_nt", prev)
    B.check("nt")
    assert _lib.call_ret("nsa_ln_set_nt", -1) == prev
    for a, c in zip(*outs):
        assert torch.equal(_bits(a), _bits(c)) and torch.isfinite(a).all()
    assert torch.equal(_bits(outs[0][0]), _bits(x + res.float()))


# ===================================================================== through autograd
@pytest.mark.parametrize("N,C", [(5, 1280), (37, 2056)])
@pytest.mark.parametrize("fused", [False, True])
def test_through_autograd(kernels, N, C, fused):
    """ops.layer_norm / ops.add_layer_norm per element with the same bounds: LayerNormFn's
    nblk = max(1, (N + 7) // 8) grid, its partial-row buffers and nsa_colsum_accum (one more
    fp32 add per block)."""
    from nanosandbox_amd import ops
    x0, names = ln_rows(N, C, seed=N + C)
    w0, b0 = ln_params(C, seed=N + C + 1, dtype=BF)
    x = x0.to(DEV).requires_grad_(True)
    w, b = w0.float().to(DEV).requires_grad_(True), b0.float().to(DEV).requires_grad_(True)
    dy = ln_dy(N, C, seed=N + C + 2, dtype=BF).to(DEV)
    tag = f"autograd[{N},{C},{'add' if fused else 'ln'}]"
    if fused:
        y = ln_res(names, C, seed=N + C + 4, dtype=BF).to(DEV).requires_grad_(True)
        ds = ln_dres(N, C, seed=N + C + 3, dtype=F32).to(DEV)
        s, h = ops.add_layer_norm(x, y, w, b)
        loss = (h.float() * dy.float()).sum() + (s * ds).sum()
    else:
        y, ds = None, None
        h = ops.layer_norm(x, w, b, out_dtype=BF)
        loss = (h.float() * dy.float()).sum()
    r = ln_fwd_ref(x.detach(), y.detach() if fused else None, w0.to(DEV), b0.to(DEV), EPS, F32)
    b_mean, b_rstd, b_h = ln_fwd_bounds(r, BF)
    # LayerNormFn.forward's save_for_backward order: (input or fused sum, w, b or mean, mean, rstd)
    xin, _, _, mean, rstd = h.grad_fn.saved_tensors
    _within(f"{tag} mean", mean, r.mean, b_mean)
    _within(f"{tag} rstd", rstd, r.rstd, b_rstd)
    _within(f"{tag} h", h.detach(), r.h, b_h)
    if fused:
        assert torch.equal(_bits(s.detach()), _bits(r.s)) and torch.equal(_bits(xin), _bits(r.s))
    loss.backward()
    nblk = max(1, (N + 7) // 8)
    g = ln_bwd_ref(dy, xin, w0.to(DEV), mean, rstd, ds, nblk)
    b_dx, b_dw, b_db = ln_bwd_bounds(g, F32)
    _within(f"{tag} dx", x.grad, g.dx, b_dx)
    if fused:
        assert torch.equal(_bits(y.grad), _bits(x.grad.to(BF)))
    # the partial rows summed: each block's bound, and nblk more roundings of the running sum
    more = nblk * 2.0 ** -24
    _within(f"{tag} dw", w.grad, g.dw.sum(0), b_dw.sum(0) + more * g.e_dw.sum(0))
    _within(f"{tag} db", b.grad, g.db.sum(0), b_db.sum(0) + more * g.e_db.sum(0))
