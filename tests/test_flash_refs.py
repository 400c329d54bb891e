"""References for the attention kernels on the path every GPT-2 configuration trains on (p = 0:
``flash_attn.hip`` with ``DROP = false``, the v5 forward, the v3 dK/dV kernel), with their own CPU
checks.  ``test_flash_gpu.py`` compares the HIP kernels with these.

* the case lists (``FWD_CASES``, ``BWD_CASES`` and their fp16 samples): one T per loop structure of
  a kernel, always with B = 2, H = 3.
* ``flash_inputs``: four input families.  "random" (q doubled, so the softmax is not near
  uniform); "qzero": Q = 0, K one-hot by 64-key tile, dO one-hot by 32-query slice, V random, which
  routes each query slice into its own dV column and each key tile into its own dQ column; "kzero":
  K = 0, Q one-hot by 32-query slice, V and dO random, which routes each query slice into its own
  dK column (dK[k, d] = sm * sum over the queries q >= k of the slice that owns column d of
  dS[q, k]); "krow": Q = 0, K = V one-hot by key row (column t % D), dO random signs, which routes
  each key row into a dQ column.  The last one exists because of a gap the planted defects showed:
  a dQ kernel that skips the only key tile of T <= 64 passed the first three (the rows of dS sum to
  0, so one tile's column of "qzero" is 0 anyway, and the random inputs' dQ constant is 1).
* ``flash_ref``: ``attn_dropout_ref`` with an all-true mask and p = 0 (float64, proven equal to
  SDPA in ``test_dropout_refs``) plus the float64 logsumexp of the scaled scores.
* ``flash_emulate``: ``attn_emulate`` with an all-true mask and p = 0, bit for bit
  (``test_flash_emulate_is_attn_emulate``), with hooks for the planted defects below and one more
  rounding point: the v5 forward's fast tiles (``fwd_tile5``) round P = exp2(S') with no max
  subtracted (m = 0), where v1 (``fwd_tile``) rounds exp2(S' - m); ``pmax=False`` emulates that.
  Reading the p = 0 kernels (``bwd_probs``, ``dq_tile``, ``dkdv_slice``, ``dq2_tile``) showed no
  other 16-bit rounding point: P, dS, O and the three gradients, delta from the rounded O in fp32,
  and the v2 dQ kernel rounds dS only (its P never becomes an MFMA operand), like the emulation.
* ``check_outputs``: the per-element bounds, shared with the GPU test:
  y    |err| <= 2^-5 mag_o + 2^-7 |ref| + 1e-4  (the bound of ``test_flash_attention``)
  dQ, dK, dV  |err| <= c mag + 1e-5
  lse  |err| <= c_lse (1 + |ref| + max_k |s_qk|)

Constants, from the emulation against the float64 reference at every input the GPU test runs
(``test_emulation_sets_the_constants`` recomputes them): c = pow2_ceil(4 x worst), the worst being
max (|emulation - float64| - 1e-5) / mag, so that c is what the bound's proportional term has to
cover (without the 1e-5, fp16's subnormal dS at magnitudes of 1e-7 would set c = 1).  Pooled over
everything, as one constant per element type would be, the worst is 0.138 bf16 and c = 1: dQ of a
query whose softmax has one dominant key (q doubled makes such rows common, here query 2 at T = 160
and query 77 at T = 256), where dS = P (dP - delta) cancels in exact arithmetic while delta carries
the rounding of O, an error of the size of sum |dO| |O| that ``mag_dq`` does not see.  That is no
tighter than the 2^-3 of the dropout path, so the constants are kept per input family and per
kernel (dQ | dK and dV), each by the same rule over its own inputs and so never looser than the
pooled one:

            bf16  worst dQ  dK/dV    c dQ   dK/dV     fp16  worst dQ   dK/dV     c dQ    dK/dV
    random        0.1383   0.0171    2^0    2^-3            0.00350  0.00092    2^-6    2^-8
    qzero         0.0030   0.0042    2^-6   2^-5            0.00021  0.00054    2^-10   2^-8
    kzero         0 (=ref) 0.0060    -      2^-5            0        0.00039    -       2^-9
    krow          0.0050   0.0044    2^-5   2^-5            0.00016  0.00029    2^-10   2^-9

The random inputs' dQ bound is therefore weak (it still catches a read past T, a NaN, a row that
was not written); the routing families carry the structural weight, and the random dK / dV bound
is the dropout path's.  Worst lse ratio 1.3e-7 bf16, 2.2e-7 fp16 (fp32 rounding of scores of
magnitude up to 12), so c_lse = pow2_ceil(8 x worst) = 2^-19: the kernels' hardware exp2 / log2 are
not in the emulation.

``test_planted_defects_are_rejected`` applies eight defects to the emulation (a skipped query
slice, the last slice of an odd count, a skipped key tile in dQ and in the forward, the diagonal
masked, rows >= T unmasked, lse off by 1e-3, head 0's K/V everywhere) and requires the same check,
with these constants, to reject each wherever it can occur: 325 instances in bf16, 68 in fp16, the
weakest at 31 times its bound.
"""

import functools
import math

import pytest
import torch

from test_dropout_refs import (BF, F32, F64, FH, attn_dropout_ref, attn_emulate, causal, pow2_ceil, worst_ratio)

B, H = 2, 3  # different data per (b, h); grids that are no multiple of 8
FAMILIES = ("random", "qzero", "kzero", "krow")

# gradient bound |err| <= c mag + 1e-5, c per element type, input family and kernel: (dQ, dK and dV);
# None where the reference and its magnitude are identically 0 and the bound is the 1e-5 alone.
# lse bound |err| <= c_lse (1 + |ref| + max |s|).  Module docstring.
FLASH_C = {BF: {"random": (2.0 ** 0, 2.0 ** -3), "qzero": (2.0 ** -6, 2.0 ** -5), "kzero": (None, 2.0 ** -5),
                "krow": (2.0 ** -5, 2.0 ** -5)},
           FH: {"random": (2.0 ** -6, 2.0 ** -8), "qzero": (2.0 ** -10, 2.0 ** -8), "kzero": (None, 2.0 ** -9),
                "krow": (2.0 ** -10, 2.0 ** -9)}}
LSE_C = {BF: 2.0 ** -19, FH: 2.0 ** -19}

# forward: (fwd variant, D, T).  v1: 128 queries per workgroup, 32 per wave, 64-key tiles; v5: 256
# queries per workgroup, 64 per wave, two tiles per barrier, 4-slot ring
FWD64_T = (1, 31, 32, 33, 64, 65, 127, 129, 192, 255, 257, 320)
FWD_CASES = [(f, 64, T) for f in ("v1", "v5") for T in FWD64_T] + \
            [(None, D, T) for D in (32, 128) for T in (1, 33, 77, 129, 160)]
# backward: (bwd variant, D, T).  None = what the shape selects: the generic kernels
BWD_CASES = [(None, D, T) for D in (32, 128) for T in (1, 33, 129, 160)] + \
            [(None, 64, T) for T in (1, 31, 65, 200, 257)] + [("v1", 64, 288)] + \
            [(v, 64, T) for v in ("v2", "v3") for T in (32, 64, 96, 160, 256, 288)]
FWD_CASES_FP16 = [("v1", 64, 257), ("v5", 64, 257)]
BWD_CASES_FP16 = [(None, 64, 200), (None, 32, 77), (None, 128, 160), ("v2", 64, 288), ("v3", 64, 288)]


def case_id(case):
    v, D, T = case
    return f"{v or 'generic'}-D{D}-T{T}"


def distinct_shapes(cases):
    """The (T, D) of a case list, each once: the inputs do not depend on the kernel variant."""
    return sorted({(T, D) for _, D, T in cases})


# ------------------------------------------------------------------------------- inputs
def flash_inputs(family, T, D, dtype):
    """q, k, v, do [B, H, T, D]: values of ``dtype`` held in fp32 on the CPU, from a generator
    seeded by the shape."""
    g = torch.Generator().manual_seed(5000 + 1000 * FAMILIES.index(family) + 7 * T + D + (500 if dtype == FH else 0))
    rnd = lambda: torch.randn(B, H, T, D, generator=g).to(dtype).float()  # noqa: E731
    t = torch.arange(T)
    n_slices, n_tiles = (T + 31) // 32, (T + 63) // 64
    # every column holds at most one slice / one tile
    assert n_slices <= D and n_tiles <= D, (T, D)
    by_slice = torch.zeros(B, H, T, D)
    by_slice[:, :, t, (t // 32) % D] = 1.0
    by_tile = torch.zeros(B, H, T, D)
    by_tile[:, :, t, (t // 64) % D] = 1.0
    assert (by_slice.sum(-1) == 1).all() and (by_tile.sum(-1) == 1).all()
    assert len({int(c) for c in (t // 32) % D}) == n_slices and len({int(c) for c in (t // 64) % D}) == n_tiles
    if family == "random":
        q, k, v, do = rnd(), rnd(), rnd(), rnd()
        return 2.0 * q, k, v, do  # doubling is exact in bf16 and fp16
    if family == "qzero":
        return torch.zeros(B, H, T, D), by_tile, rnd(), by_slice
    if family == "kzero":
        return by_slice, torch.zeros(B, H, T, D), rnd(), rnd()
    if family == "krow":
        by_row = torch.zeros(B, H, T, D)
        by_row[:, :, t, t % D] = 1.0
        return torch.zeros(B, H, T, D), by_row, by_row.clone(), torch.sign(rnd())
    raise ValueError(family)


# ----------------------------------------------------------------------- float64 reference
def flash_ref(q, k, v, do):
    """``attn_dropout_ref`` without dropout, plus lse = logsumexp of the visible scaled scores and
    smax = their largest magnitude, per query, in float64."""
    Bq, Hq, T, D = q.shape
    ref = attn_dropout_ref(q, k, v, do, torch.ones(Bq, Hq, T, T, dtype=torch.bool), 0.0)
    s = q.to(F64) @ k.to(F64).transpose(-1, -2) / math.sqrt(D)
    vis = causal(T)
    ref["lse"] = torch.logsumexp(s.masked_fill(~vis, -math.inf), -1)
    ref["smax"] = s.abs().masked_fill(~vis, 0.0).amax(-1)
    return ref


@functools.lru_cache(maxsize=None)
def case_data(family, T, D, dtype):
    """(inputs, reference) of one shape, computed once and shared; nobody writes to them."""
    x = flash_inputs(family, T, D, dtype)
    return x, flash_ref(*x)


# --------------------------------------------------------------------------- fp32 emulation
def flash_emulate(q, k, v, do, dtype, pmax=True, defect=None):
    """``attn_emulate(q, k, v, do, all-true, 0.0, dtype)``: the kernels' arithmetic in fp32 with
    their rounding points.  ``pmax=False`` rounds P = exp(s) as v5's fast tiles do.  ``defect`` is
    a dict that plants one defect in one of the three paths (forward, dQ, dK/dV):

    path      "fwd" | "dq" | "dkdv": the path the defect is in
    vis       bool [T, T] (query, key): the pairs that path visits instead of ``causal(T)``
    kv0       every head reads head 0's K and V
    phantom   n: the dK/dV path also sums n rows past T, which the loads clamp to row T - 1
    lse_shift added to the lse the forward returns

    Returns y, lse, dq, dk, dv."""
    T, D = q.shape[-2:]
    d = defect or {}
    sm = torch.tensor(1.0 / math.sqrt(D), dtype=F32)
    r16 = lambda x: x.to(dtype).float()  # noqa: E731
    q, k, v, do = (x.float() for x in (q, k, v, do))

    def path(name):
        hit = d.get("path") == name
        vis = d["vis"] if hit and "vis" in d else causal(T)
        if hit and d.get("kv0"):
            return vis, k[:, :1].expand_as(k), v[:, :1].expand_as(v)
        return vis, k, v

    vis, kk, vv = path("fwd")
    s = (q @ kk.transpose(-1, -2) * sm).masked_fill(~vis, -math.inf)
    m = s.max(-1, keepdim=True).values if pmax else torch.zeros(())
    pu = torch.exp(s - m)
    l = pu.sum(-1, keepdim=True)
    y = r16((r16(pu) @ vv) / l)
    lse = (m + torch.log(l)).squeeze(-1)
    delta = (y * do).sum(-1, keepdim=True)

    vis, kk, vv = path("dq")
    s = (q @ kk.transpose(-1, -2) * sm).masked_fill(~vis, -math.inf)
    P = torch.exp(s - lse.unsqueeze(-1))
    dS = r16(P * (do @ vv.transpose(-1, -2) - delta))
    dq = r16((dS @ kk) * sm)

    vis, kk, vv = path("dkdv")
    qx, dox, lsex, deltax = q, do, lse, delta
    n = d.get("phantom", 0) if d.get("path") == "dkdv" else 0
    if n:
        ext = lambda x: torch.cat([x] + n * [x.narrow(2, T - 1, 1)], 2)  # noqa: E731  (rows are dim 2 of all four)
        qx, dox, lsex, deltax = ext(q), ext(do), ext(lse), ext(delta)
        vis = torch.cat([vis, torch.ones(n, T, dtype=torch.bool)], 0)
    s = (qx @ kk.transpose(-1, -2) * sm).masked_fill(~vis, -math.inf)
    P = torch.exp(s - lsex.unsqueeze(-1))
    Pd = r16(P)
    dv = r16(Pd.transpose(-1, -2) @ dox)
    dS = r16(P * (dox @ vv.transpose(-1, -2) - deltax))
    dk = r16((dS.transpose(-1, -2) @ qx) * sm)
    return dict(y=y, lse=lse + d.get("lse_shift", 0.0), dq=dq, dk=dk, dv=dv)


# ------------------------------------------------------------------------ the per-element check
def bounds(ref, dtype, family):
    """The bound of every element of y, lse, dq, dk, dv."""
    out = dict(y=2.0 ** -5 * ref["mag_o"] + 2.0 ** -7 * ref["o"].abs() + 1e-4,
               lse=LSE_C[dtype] * (1.0 + ref["lse"].abs() + ref["smax"]))
    c_dq, c_dkdv = FLASH_C[dtype][family]
    for n, c in (("dq", c_dq), ("dk", c_dkdv), ("dv", c_dkdv)):
        out[n] = (c or 0.0) * ref["mag_" + n] + 1e-5
    return out


def check_outputs(got, ref, dtype, family, names=("y", "lse", "dq", "dk", "dv")):
    """{name: worst |got - ref| / bound}; an element that is not finite counts as infinitely far.
    ``got`` holds [B, H, T, D] tensors ([B, H, T] for lse) on the reference's device."""
    bd = bounds(ref, dtype, family)
    out = {}
    for n in names:
        r = (got[n].to(F64) - ref["o" if n == "y" else n]).abs() / bd[n]
        out[n] = torch.nan_to_num(r, nan=math.inf).max().item()
    return out


def first_miss(got, ref, dtype, family, name):
    """(count, index, value, reference, bound) of the elements of ``name`` outside their bound."""
    bd = bounds(ref, dtype, family)[name]
    want = ref["o" if name == "y" else name]
    bad = (~((got[name].to(F64) - want).abs() <= bd)).nonzero()
    i = tuple(bad[0].tolist())
    return bad.shape[0], i, got[name][i].item(), want[i].item(), bd[i].item()


# ===================================================================== CPU checks of the above
def _all_bwd_shapes(dtype):
    return distinct_shapes(BWD_CASES if dtype == BF else BWD_CASES_FP16)


def _all_fwd_shapes(dtype):
    return distinct_shapes(FWD_CASES if dtype == BF else FWD_CASES_FP16)


def test_case_lists_and_inputs():
    assert len(FWD_CASES) == 34 and len(BWD_CASES) == 26
    for T, D in distinct_shapes(FWD_CASES + BWD_CASES):
        assert T <= 320
        for fam in FAMILIES:
            q, k, v, do = flash_inputs(fam, T, D, BF)
            for x in (q, k, v, do):
                assert x.shape == (B, H, T, D) and torch.equal(x.to(BF).float(), x)
    # each column of the routing inputs holds one slice (tile) and no other
    T, D = 320, 32
    q = flash_inputs("kzero", T, D, BF)[0]
    _, k, _, do = flash_inputs("qzero", T, D, BF)
    for c in range(D):
        assert set((torch.arange(T)[q[0, 0, :, c] == 1] // 32).tolist()) == ({c} if c < 10 else set())
        assert set((torch.arange(T)[do[0, 0, :, c] == 1] // 32).tolist()) == ({c} if c < 10 else set())
        assert set((torch.arange(T)[k[0, 0, :, c] == 1] // 64).tolist()) == ({c} if c < 5 else set())
    # different data per (b, h)
    v = flash_inputs("random", 33, 64, BF)[2]
    assert not torch.equal(v[0, 0], v[1, 0]) and not torch.equal(v[0, 0], v[0, 1])
    # fp16 inputs are fp16 values
    q = flash_inputs("random", 77, 32, FH)[0]
    assert torch.equal(q.to(FH).float(), q)


@pytest.mark.parametrize("T,D,dtype", [(77, 32, BF), (200, 64, BF), (160, 128, FH)])
def test_flash_emulate_is_attn_emulate(T, D, dtype):
    """Without a defect the emulation is ``attn_emulate`` with an all-true mask and p = 0, every
    bit, lse included."""
    for fam in FAMILIES:
        x = flash_inputs(fam, T, D, dtype)
        a = flash_emulate(*x, dtype)
        b = attn_emulate(*x, torch.ones(B, H, T, T, dtype=torch.bool), 0.0, dtype)
        for n in ("y", "lse", "dq", "dk", "dv"):
            assert torch.equal(a[n], b[n]), (fam, n)


def test_flash_ref_lse_and_routing():
    """lse of the reference is ln(q + 1) where the scores are 0; on the "kzero" family dK's
    column d is the sum over the slice that owns it, and the other columns are exactly 0."""
    T, D = 160, 64
    x, ref = case_data("kzero", T, D, BF)
    qp1 = torch.arange(1, T + 1, dtype=F64)
    assert torch.allclose(ref["lse"], torch.log(qp1).expand(B, H, T), rtol=1e-14, atol=1e-14)
    assert (ref["smax"] == 0).all()
    q, k, v, do = (t.to(F64) for t in x)
    P = (causal(T).to(F64) / qp1.view(T, 1))
    dS = P * (do @ v.transpose(-1, -2) - (do * ref["o"]).sum(-1, keepdim=True))
    want = torch.zeros(B, H, T, D, dtype=F64)
    for s in range(T // 32):
        want[..., s] = dS[:, :, 32 * s:32 * s + 32].sum(2) / math.sqrt(D)
    assert torch.allclose(ref["dk"], want, rtol=1e-12, atol=1e-14)
    assert (ref["dk"][..., T // 32:] == 0).all() and (ref["mag_dk"][..., T // 32:] == 0).all()
    assert (ref["dq"] == 0).all() and (ref["mag_dq"] == 0).all()


def _emulation_worst(dtype):
    """{(family, group): worst (|emulation - float64| - 1e-5) / mag} over the backward inputs of the
    GPU test, group "dq" or "dkdv", the 1e-5 being the bound's own absolute term (it covers what
    fp16's subnormal dS and outputs lose, which no multiple of mag does); and the worst lse ratio
    over every input, under both forward roundings."""
    grad, lse = {}, 0.0
    bwd = _all_bwd_shapes(dtype)
    shapes = {(fam, T, D) for T, D in bwd for fam in FAMILIES}
    shapes |= {("random", T, D) for T, D in _all_fwd_shapes(dtype)}
    for fam, T, D in sorted(shapes):
        x, ref = case_data(fam, T, D, dtype)
        for pmax in (True, False) if D == 64 else (True,):  # v5 is a D = 64 kernel
            emu = flash_emulate(*x, dtype, pmax=pmax)
            r = worst_ratio((emu["lse"].to(F64) - ref["lse"]).abs(), 1.0 + ref["lse"].abs() + ref["smax"])
            lse = max(lse, r)
            if not pmax or (T, D) not in bwd:
                continue  # the backward cases run behind the default forward (v1 at these sizes)
            for n in ("dq", "dk", "dv"):
                r = worst_ratio((emu[n].to(F64) - ref[n]).abs(), ref["mag_" + n], 1e-5)
                key = (fam, "dq" if n == "dq" else "dkdv")
                grad[key] = max(grad.get(key, 0.0), r)
    return grad, lse


@pytest.mark.parametrize("dtype", [BF, FH], ids=["bf16", "fp16"])
def test_emulation_sets_the_constants(dtype):
    """Each constant of FLASH_C is pow2_ceil(4 x the emulation's worst gradient ratio) over its
    family's inputs and its kernel's outputs, LSE_C pow2_ceil(8 x its worst lse ratio), all
    measured at the GPU test's own inputs."""
    grad, lse = _emulation_worst(dtype)
    print(f"emulation {dtype}: worst lse ratio {lse:.3e} -> c_lse = 2^{math.log2(8 * lse):.2f}")
    assert pow2_ceil(8 * lse) == LSE_C[dtype], lse
    for fam in FAMILIES:
        for g, c in zip(("dq", "dkdv"), FLASH_C[dtype][fam]):
            w = grad[(fam, g)]
            print(f"emulation {dtype} {fam} {g}: worst (|err| - 1e-5) / mag = {w:.5f}"
                  + (f" -> c = 2^{math.log2(4 * w):.2f}" if w else ""))
            if c is None:
                assert w == 0.0, (fam, g, w)
            else:
                assert pow2_ceil(4 * w) == c, (fam, g, w)
    # pooled over families and tensors, as one constant per element type would be: no tighter than
    # the 2^-3 / 2^-6 of the dropout path (the random inputs' dQ sets it)
    pooled = pow2_ceil(4 * max(grad.values()))
    assert pooled >= {BF: 2.0 ** -3, FH: 2.0 ** -6}[dtype]


@pytest.mark.parametrize("dtype", [BF, FH], ids=["bf16", "fp16"])
def test_unmutated_emulation_passes_with_room(dtype):
    """Every case, every family: the emulation is within a quarter of y's bound, an eighth of lse's,
    and needs at most a quarter of a gradient bound's proportional term (|err| <= c / 4 mag + 1e-5),
    all by construction of the constants; and v5's fast tiles stay in their range at these inputs,
    so ``pmax=False`` is what the kernel does there."""
    worst = {}
    fwd, bwd = _all_fwd_shapes(dtype), _all_bwd_shapes(dtype)
    for T, D in sorted(set(fwd) | set(bwd)):
        for fam in FAMILIES if (T, D) in bwd else ("random",):
            x, ref = case_data(fam, T, D, dtype)
            for pmax in (True, False) if D == 64 else (True,):
                emu = flash_emulate(*x, dtype, pmax=pmax)
                for n, r in check_outputs(emu, ref, dtype, fam, ("y", "lse")).items():
                    worst[n] = max(worst.get(n, 0.0), r)
                if not pmax or (T, D) not in bwd:
                    continue
                assert max(check_outputs(emu, ref, dtype, fam).values()) < 1.0
                for n, c in zip(("dq", "dk", "dv"), (FLASH_C[dtype][fam][i] for i in (0, 1, 1))):
                    r = worst_ratio((emu[n].to(F64) - ref[n]).abs(), ref["mag_" + n], 1e-5)
                    assert c is not None or r == 0.0
                    worst[n] = max(worst.get(n, 0.0), r / c if c else 0.0)
            if D == 64:
                l = torch.exp(ref["lse"])  # v5 keeps the fast tiles while the row sums stay in range
                hi, lo = (2.0 ** 15, 2.0 ** -8) if dtype == FH else (2.0 ** 64, 2.0 ** -60)
                assert (l <= hi).all() and (l >= lo).all(), (fam, T)
    print(f"unmutated emulation {dtype}: worst share of the bound "
          + ", ".join(f"{n} {r:.4f}" for n, r in worst.items()))
    for n, r in worst.items():
        assert r <= (0.125 if n == "lse" else 0.25), (n, r)


# ------------------------------------------------------------------------ planted defects
def _skip_rows(T, lo, hi):
    vis = causal(T).clone()
    vis[lo:hi] = False
    return vis


def _skip_cols(T, lo, hi):
    vis = causal(T).clone()
    vis[:, lo:hi] = False
    return vis


def planted_defects(T, forward, backward):
    """[(name, defect)]: every instance of the eight defects that can occur at length T."""
    out = []
    n_slices, n_tiles = (T + 31) // 32, (T + 63) // 64
    diag = causal(T) & ~torch.eye(T, dtype=torch.bool)
    if backward:
        for s in range(n_slices):
            out.append((f"dK/dV skips query slice {s}", dict(path="dkdv", vis=_skip_rows(T, 32 * s, 32 * s + 32))))
        # the pair loop's tail: the last slice, in the 128-key blocks that visit an odd number of slices
        odd = [kb for kb in range((T + 127) // 128) if (n_slices - 4 * kb) % 2 == 1]
        if odd:
            vis = causal(T).clone()
            for kb in odd:
                vis[32 * (n_slices - 1):, 128 * kb:128 * kb + 128] = False
            out.append(("dK/dV skips the last slice of an odd count", dict(path="dkdv", vis=vis)))
        out.append(("dkdv: diagonal masked", dict(path="dkdv", vis=diag)))
        if T > 1:
            # at T = 1 the softmax of one key has no gradient: dQ and dK are 0 and dV = dO whatever
            # K and V hold, so neither the dQ path nor a wrong K/V head has anything to get wrong
            for j in range(n_tiles):
                out.append((f"dQ skips key tile {j}", dict(path="dq", vis=_skip_cols(T, 64 * j, 64 * j + 64))))
            out.append(("dq: diagonal masked", dict(path="dq", vis=diag)))
            out.append(("dq: head 0's K/V", dict(path="dq", kv0=True)))
            out.append(("dkdv: head 0's K/V", dict(path="dkdv", kv0=True)))
        if T % 32:
            out.append(("dK/dV: rows >= T unmasked", dict(path="dkdv", phantom=32 - T % 32)))
    if forward:
        for j in range(n_tiles):
            out.append((f"forward skips key tile {j}", dict(path="fwd", vis=_skip_cols(T, 64 * j, 64 * j + 64))))
        out.append(("fwd: diagonal masked", dict(path="fwd", vis=diag)))
        out.append(("fwd: head 0's K/V", dict(path="fwd", kv0=True)))
        out.append(("lse off by 1e-3", dict(lse_shift=1e-3)))
    return out


@pytest.mark.parametrize("dtype", [BF, FH], ids=["bf16", "fp16"])
def test_planted_defects_are_rejected(dtype):
    """Each planted defect, at every T of the case lists where it can occur, is rejected by the
    per-element check with the derived constants: a forward defect on the random inputs (the only
    family the forward cases run), a backward defect on at least one of the four families.  The
    rejecting tensor must belong to the defective path, and the margin is printed."""
    fwd, bwd = _all_fwd_shapes(dtype), _all_bwd_shapes(dtype)
    owns = dict(fwd=("y", "lse"), dq=("dq",), dkdv=("dk", "dv"))
    weakest, n_defects, by_family = (math.inf, None), 0, {f: 0 for f in FAMILIES}
    for T, D in sorted(set(fwd) | set(bwd)):
        for name, defect in planted_defects(T, (T, D) in fwd, (T, D) in bwd):
            names = owns.get(defect.get("path"), ("lse",))
            fams = ("random",) if names[0] in ("y", "lse") else FAMILIES
            best = 0.0
            for fam in fams:
                x, ref = case_data(fam, T, D, dtype)
                r = max(check_outputs(flash_emulate(*x, dtype, defect=defect), ref, dtype, fam, names).values())
                if r > 1.0:
                    by_family[fam] += 1
                best = max(best, r)
            n_defects += 1
            assert best > 1.0, f"not rejected at T = {T}, D = {D}: {name} (worst err / bound {best:.3f})"
            if best < weakest[0]:
                weakest = (best, (name, T, D))
    print(f"{dtype}: {n_defects} planted defects rejected; rejections per family {by_family}; "
          f"weakest rejection {weakest[0]:.2f} x the bound: {weakest[1]}")


def test_routing_families_see_what_random_inputs_miss():
    """One skipped slice out of nine at T = 288 removes about a ninth of an early key's dK terms:
    the routing family rejects it by a whole column (far past the bound), not by a margin."""
    T, D = 288, 64
    defect = dict(path="dkdv", vis=_skip_rows(T, 256, 288))
    x, ref = case_data("kzero", T, D, BF)
    emu = flash_emulate(*x, BF, defect=defect)
    err = (emu["dk"].to(F64) - ref["dk"]).abs()
    bound = bounds(ref, BF, "kzero")["dk"]
    wrong = (err > bound)
    # the wrong elements are column 8 (slice 8) and nothing else, and nearly all of that column
    assert wrong[..., :8].sum() == 0 and wrong[..., 9:].sum() == 0
    assert wrong[..., 8].float().mean() > 0.75
    assert (err / bound)[..., 8].max() > 8.0
