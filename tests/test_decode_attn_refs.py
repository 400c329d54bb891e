"""Float64 references and input builders for the decode-side attention kernels
(``decode_attn_chunk`` and the combines of ``decode_attn.h`` / ``decode_shared.hip``,
``shared_prompt_chunk``, ``prefix_attn_kernel``, ``kv_append_kernel``), as plain functions that
run on any device, with their own CPU checks.  ``test_decode_attn_gpu.py`` holds the HIP kernels
to them per key and per element.

Three pins, each proved here for the reference alone before a kernel meets it:

  counting   q = 0, so every live score is 0, every weight 2^0 = 1 and every fp32 sum an exact
             integer.  V is one-hot in one of two layouts: column ``k % 64`` (the key's place
             inside its chunk) or column ``(k // G) % 64`` (its chunk, wave or round of G keys).
             A live chunk's partial is exactly (m, l, o) = (0, live keys, a count per column)
             and the output is count / n: one lost or doubled key changes an integer.
  selecting  key k carries K[k] = 8 s_k, s_k in {+-1}^64, and the query that must select key t
             is 8 s_t: the target scores 64 * 64 / 8 = 512 nats, any other key 8 (s_k . s_t).
             ``code_margin`` <= 51 leaves the others at least 8 * (64 - 51) = 104 nats = 150
             log2 units below, so their fp32 weights 2^-150 and less are exactly 0 and the
             output is V[t] (integers in +-[1, 127], exact in bf16) bit for bit.
  peaked     q ~ 3 N(0, 1), k, v ~ N(0, 1), all bf16: a few dozen keys carry the weight.  The
             bound on an output element is
               |y - ref64| <= 2^-8 |ref64| + 2^-12 mag + 1e-30,      mag = sum_k p_k |v_k|
             the one bf16 rounding of the output, and for the rest (fp32 accumulation over at
             most ~1k keys, fp32 exp2 on scores of this size, p entering the MFMA kernels as
             hi + lo bf16: 16 bits) 2^-12 of the absolute terms.  The constant is not tuned on
             the kernels: ``emulate_fp32`` runs the chunked algorithm (per-chunk (m, l, o), then
             the combine) in fp32 torch and ``test_fp32_emulation_a_quarter_of_the_bound``
             holds its error under 2^-14 mag on every input the GPU file runs.  Worst
             emulation error / (2^-14 mag) here: decode 0.0107, shared prompt 0.0181, prefix
             0.0220 (that is 0.003 - 0.006 of the 2^-12 term).

A partial is (m, l, o[64]) in log2 units: m = max_k s_k log2(e), l = sum_k 2^(s_k log2 e - m),
o = sum_k 2^(..) v_k; the empty partial is (-inf, 0, 0 ...).  The combine of partials s is
sum_s 2^(m_s - M) o_s / sum_s 2^(m_s - M) l_s.
"""

import math

import pytest
import torch

BF = torch.bfloat16
F64 = torch.float64
H, D = 2, 64
C = H * D
SCALE = 1.0 / math.sqrt(D)
LOG2E = 1.4426950408889634
INF = float("inf")
U16 = 2.0 ** -8     # one bf16 rounding, relative
K_MAG = 2.0 ** -12  # the peaked bound's share of mag
MARGIN = 51         # max |s_k . s_t| the selecting pin tolerates

# ---------------------------------------------------------------- the cases of the GPU file
DEC_B, DEC_T, DEC_G = 3, 600, 256        # two full 256-key chunks and one of 88
DEC_POS = [0, 1, 7, 8, 63, 64, 254, 255, 256, 257, 511, 512, 598, 599]
SH_TP, SH_R = 300, 260                   # prompt chunks of 128, 128, 44; row chunks of 256 and 4
SH_GP, SH_GR = 128, 256
SH_BS = [1, 15, 16, 17, 33]
SH_PS = [1, 31, 32, 33, 127, 128, 129, 256, 299, 300]
SH_OFFS = [0, 1, 255, 256, 259]
PF_TP = 320
PF_BS = [1, 3]
PF_PS = [1, 31, 32, 33, 127, 128, 129, 300]
PF_SS = [1, 15, 16, 17, 31, 32, 33, 65]
PF_G = 32
SEED_CODES, SEED_VALS, SEED_PEAK = 20251, 20252, 20253


def dec_row_positions(i):
    """Three unequal per-row positions for the i-th entry of DEC_POS, which sits in row i % 3."""
    n = len(DEC_POS)
    ps = [DEC_POS[i], DEC_POS[(i + 5) % n], DEC_POS[(i + 9) % n]]
    return ps[-(i % 3):] + ps[:-(i % 3)] if i % 3 else ps


def sh_configs(i, B):
    """The two launches of prompt length SH_PS[i]: (row offsets pos - P, append).  One offset: a
    shared position; B offsets: one per row."""
    n = len(SH_OFFS)
    return [([SH_OFFS[i % n]], i % 2), ([SH_OFFS[(b + i) % n] for b in range(B)], (i + 1) % 2)]


# ---------------------------------------------------------------------------- the references
def attend64(q, k, v, vis):
    """q [..., Q, D], k / v [..., N, D], vis bool [..., Q, N]: softmax attention of every query
    over the keys it sees, in float64 -> (out, mag = sum_k p_k |v_k|, p)."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    s = torch.einsum("...qd,...kd->...qk", q, k) * SCALE
    p = torch.softmax(s.masked_fill(~vis, -INF), dim=-1)
    return p @ v, p @ v.abs(), p


def decode_ref(q, kc, vc, pos):
    """q [B, H, D], caches [B, H, T, D], pos: B positions; row b over keys 0 .. pos[b] ->
    (out, mag) [B, H, D]."""
    T = kc.shape[2]
    ar = torch.arange(T, device=q.device)
    vis = ar[None, :] <= torch.as_tensor(pos, device=q.device)[:, None]    # [B, T]
    out, mag, _ = attend64(q[:, :, None], kc, vc, vis[:, None, None, :])
    return out[:, :, 0], mag[:, :, 0]


def shared_keys(pk, kc, P):
    """The virtual key list of the shared-prompt form: prompt rows 0 .. P - 1 ([H, Tp, D]), then
    the row's own slots ([B, H, R, D]) -> [B, H, P + R, D]."""
    return torch.cat([pk[None, :, :P].expand(kc.shape[0], -1, -1, -1), kc], dim=2)


def shared_ref(q, pk, pv, kc, vc, P, pos):
    """Row b over prompt keys 0 .. P - 1, then its slots 0 .. pos[b] - P -> (out, mag) [B, H, D]."""
    k, v = shared_keys(pk, kc, P), shared_keys(pv, vc, P)
    ar = torch.arange(k.shape[2], device=q.device)
    vis = ar[None, :] <= torch.as_tensor(pos, device=q.device)[:, None]
    out, mag, _ = attend64(q[:, :, None], k, v, vis[:, None, None, :])
    return out[:, :, 0], mag[:, :, 0]


def prefix_ref(q, k, v, pk, pv, P):
    """q, k, v [B, H, S, D], prefix caches [H, Tp, D]: query i of row b over prefix keys
    0 .. P - 1, then its row's keys 0 .. i -> (out, mag) [B, H, S, D]."""
    S = q.shape[2]
    kk, vv = shared_keys(pk, k, P), shared_keys(pv, v, P)
    vis = torch.arange(P + S, device=q.device)[None, :] <= P + torch.arange(S, device=q.device)[:, None]
    out, mag, _ = attend64(q, kk, vv, vis)
    return out, mag


def partial_ref(q, k, v, lo, hi):
    """One chunk's partial: q [..., D] against keys lo .. hi - 1 of k / v [..., N, D] ->
    ((m, l, o[64]) [..., 66] float64, mag [..., 64]); hi <= lo: the empty partial."""
    lead = q.shape[:-1]
    if hi <= lo:
        part = torch.zeros(*lead, 2 + D, dtype=F64, device=q.device)
        part[..., 0] = -INF
        return part, part[..., 2:].clone()
    kd, vd = k[..., lo:hi, :].to(F64), v[..., lo:hi, :].to(F64)
    s = torch.einsum("...d,...kd->...k", q.to(F64), kd) * (SCALE * LOG2E)
    m = s.amax(dim=-1, keepdim=True)
    p = torch.exp2(s - m)
    o = torch.einsum("...k,...kd->...d", p, vd)
    mag = torch.einsum("...k,...kd->...d", p, vd.abs())
    return torch.cat([m, p.sum(-1, keepdim=True), o], dim=-1), mag


def combine_ref(parts):
    """parts [..., n, 66] (m, l, o) -> (out [..., 64] float64, mag = sum_s f_s |o_s| / L)."""
    parts = parts.to(F64)
    m = parts[..., 0]
    f = torch.exp2(m - m.amax(dim=-1, keepdim=True))  # empty: 2^-inf = 0
    L = (f * parts[..., 1]).sum(-1, keepdim=True)
    o = parts[..., 2:]
    return (f[..., None] * o).sum(-2) / L, (f[..., None] * o.abs()).sum(-2) / L


def emulate_fp32(q, k, v, vis, chunks):
    """The kernels' algorithm in fp32 torch: per chunk (lo, hi) of the key list the partial
    (m, l, o) in log2 units, then the combine.  q [..., Q, D], k / v [..., N, D], vis [..., Q, N]
    -> out [..., Q, D] fp32."""
    q, k, v = q.float(), k.float(), v.float()
    s = torch.einsum("...qd,...kd->...qk", q, k) * torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    s = s.masked_fill(~vis, -INF)
    ms, ls, os_ = [], [], []
    for lo, hi in chunks:
        sc = s[..., lo:hi]
        m = sc.amax(dim=-1, keepdim=True)
        p = torch.exp2(sc - torch.where(m == -INF, torch.zeros_like(m), m))
        ms.append(m)
        ls.append(p.sum(-1, keepdim=True))
        os_.append(p @ v[..., lo:hi, :])
    m, l, o = torch.cat(ms, -1), torch.cat(ls, -1), torch.stack(os_, -2)   # [..., Q, n], [..., Q, n, D]
    f = torch.exp2(m - m.amax(dim=-1, keepdim=True))
    return (f[..., None] * o).sum(-2) / (f * l).sum(-1, keepdim=True)


def peaked_bound(ref, mag):
    return U16 * ref.abs() + K_MAG * mag + 1e-30


def chunk_ranges(n, G, base=0):
    return [(base + lo, base + min(lo + G, n)) for lo in range(0, n, G)]


# -------------------------------------------------------------------------- the counting pin
def onehot_v(idx, layout, G):
    """V rows of the keys idx (int64 tensor): one-hot at column idx % 64 (layout 0) or
    (idx // G) % 64 (layout 1) -> [len(idx), 64] bf16."""
    col = idx % D if layout == 0 else (idx // G) % D
    return torch.nn.functional.one_hot(col, D).to(BF)


def count_cols(lo, hi, layout, G):
    """Closed form: how many keys of lo .. hi - 1 are one-hot at each column -> [64] float64."""
    c = torch.zeros(D, dtype=F64)
    if hi <= lo:
        return c
    if layout == 0:
        for d in range(D):
            c[d] = (hi - d + D - 1) // D - (lo - d + D - 1) // D
    else:
        for g in range(lo // G, (hi - 1) // G + 1):
            c[g % D] += min(hi, (g + 1) * G) - max(lo, g * G)
    return c


def count_partial(lo, hi, layout, G):
    """The partial of the live keys lo .. hi - 1 under the counting pin -> [66] float64."""
    if hi <= lo:
        return torch.tensor([-INF] + [0.0] * (1 + D), dtype=F64)
    return torch.cat([torch.tensor([0.0, float(hi - lo)], dtype=F64), count_cols(lo, hi, layout, G)])


# ------------------------------------------------------------------------- the selecting pin
def sign_codes(n, seed=SEED_CODES):
    """s_k in {+-1}^64 for n keys per head -> [H, n, 64] float32."""
    g = torch.Generator().manual_seed(seed + n)
    return (torch.randint(0, 2, (H, n, D), generator=g) * 2 - 1).float()


def int_values(shape, seed=SEED_VALS):
    """Non-zero integers in +-[1, 127] (exact in bf16), shape [..., 64] -> bf16."""
    g = torch.Generator().manual_seed(seed + int(torch.tensor(shape).sum()))
    mag = torch.randint(1, 128, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(BF)


def code_margin(codes):
    """max over heads and pairs k != t of |s_k . s_t|."""
    gram = torch.einsum("hkd,htd->hkt", codes, codes).abs()
    gram -= torch.diag_embed(torch.diagonal(gram, dim1=1, dim2=2))
    return int(gram.max())


# the code pools: one per kernel family, a spare code last (a K row that is no key's)
def dec_codes():
    return sign_codes(DEC_T + 1)


def sh_codes():
    return sign_codes(SH_TP + SH_R + 1)    # prompt keys, then row slots at SH_TP + j


def pf_codes():
    return sign_codes(PF_TP + max(PF_SS) + 1)  # prefix keys, then row keys at PF_TP + j


# ------------------------------------------------------------------------------ peaked inputs
def peaked(shape_q, shape_kv, seed):
    """q ~ 3 N(0, 1) [shape_q], k, v ~ N(0, 1) [shape_kv], rounded to bf16."""
    g = torch.Generator().manual_seed(SEED_PEAK + seed)
    q = (3.0 * torch.randn(shape_q, generator=g)).to(BF)
    return q, torch.randn(shape_kv, generator=g).to(BF), torch.randn(shape_kv, generator=g).to(BF)


def dec_peaked():
    """(q [B, H, D], kn, vn: the new token's rows [B, H, D], K, V [B, H, T, D])."""
    q, K, V = peaked((DEC_B, H, D), (DEC_B, H, DEC_T, D), 1)
    _, kn, vn = peaked((1,), (DEC_B, H, D), 2)
    return q, kn, vn, K, V


def sh_peaked(B):
    """The first B rows of the 33-row inputs: (q, kn, vn [B, H, D], pk, pv [H, Tp, D], K, V [B, H, R, D])."""
    Bm = max(SH_BS)
    q, K, V = peaked((Bm, H, D), (Bm, H, SH_R, D), 3)
    _, kn, vn = peaked((1,), (Bm, H, D), 4)
    _, pk, pv = peaked((1,), (H, SH_TP, D), 5)
    return q[:B], kn[:B], vn[:B], pk, pv, K[:B], V[:B]


def pf_peaked(B, S):
    """The first B rows and S tokens of the 3-row, 65-token inputs: (q, k, v [B, H, S, D], pk, pv)."""
    Bm, Sm = max(PF_BS), max(PF_SS)
    q, k, v = peaked((Bm, H, Sm, D), (Bm, H, Sm, D), 6)
    _, pk, pv = peaked((1,), (H, PF_TP, D), 7)
    return q[:B, :, :S], k[:B, :, :S], v[:B, :, :S], pk, pv


# ==================================================================================== CPU tests
def _brute(q, ks, vs):
    """One query against an explicit list of keys, in Python floats."""
    s = [sum(float(a) * float(b) for a, b in zip(q, k)) * SCALE for k in ks]
    mx = max(s)
    w = [math.exp(x - mx) for x in s]
    tot = sum(w)
    out = [sum(wk / tot * float(v[d]) for wk, v in zip(w, vs)) for d in range(D)]
    mag = [sum(wk / tot * abs(float(v[d])) for wk, v in zip(w, vs)) for d in range(D)]
    return torch.tensor(out, dtype=F64), torch.tensor(mag, dtype=F64)


def _close(a, b):
    return bool(((a - b).abs() <= 1e-12 * (1 + b.abs())).all())


def test_references_against_brute_force():
    g = torch.Generator().manual_seed(5)
    B, T, Tp, R, S, P = 2, 9, 6, 5, 3, 4
    q = torch.randn(B, H, D, generator=g).to(BF)
    kc, vc = torch.randn(B, H, T, D, generator=g).to(BF), torch.randn(B, H, T, D, generator=g).to(BF)
    pk, pv = torch.randn(H, Tp, D, generator=g).to(BF), torch.randn(H, Tp, D, generator=g).to(BF)
    pos = [3, 8]
    out, mag = decode_ref(q, kc, vc, pos)
    sout, smag = shared_ref(q, pk, pv, kc[:, :, :R], vc[:, :, :R], P, [P + 2, P + 4])
    qs = torch.randn(B, H, S, D, generator=g).to(BF)
    pout, pmag = prefix_ref(qs, kc[:, :, :S], vc[:, :, :S], pk, pv, P)
    for b in range(B):
        for h in range(H):
            o, m = _brute(q[b, h], list(kc[b, h, :pos[b] + 1]), list(vc[b, h, :pos[b] + 1]))
            assert _close(out[b, h], o) and _close(mag[b, h], m)
            n = [3, 5][b]  # slots 0 .. pos - P
            o, m = _brute(q[b, h], list(pk[h, :P]) + list(kc[b, h, :n]), list(pv[h, :P]) + list(vc[b, h, :n]))
            assert _close(sout[b, h], o) and _close(smag[b, h], m)
            for i in range(S):
                o, m = _brute(qs[b, h, i], list(pk[h, :P]) + list(kc[b, h, :i + 1]),
                              list(pv[h, :P]) + list(vc[b, h, :i + 1]))
                assert _close(pout[b, h, i], o) and _close(pmag[b, h, i], m)
    # the partials of three chunks, combined, are the attention over all of their keys
    parts = torch.stack([partial_ref(q, kc, vc, lo, hi)[0] for lo, hi in [(0, 4), (4, 4), (4, 9)]], dim=-2)
    assert bool((parts[..., 1, 0] == -INF).all()) and not parts[..., 1, 1:].any()
    cout, _ = combine_ref(parts)
    full, _ = decode_ref(q, kc, vc, [8, 8])
    assert _close(cout, full)
    s = torch.einsum("bhd,bhkd->bhk", q.double(), kc[:, :, :4].double()) * SCALE * LOG2E
    assert _close(parts[..., 0, 0], s.amax(-1)) and _close(parts[..., 0, 1], torch.exp2(s - s.amax(-1, keepdim=True)).sum(-1))


@pytest.mark.parametrize("layout,G", [(0, 256), (1, 256), (1, 128), (1, 32)])
def test_counting_pin_closed_form(layout, G):
    """q = 0 and one-hot V: the float64 partial of any key range is (0, its length, the closed-form
    counts), the brute-force count agrees, and the attention output is count / n."""
    T = DEC_T
    v = onehot_v(torch.arange(T), layout, G)
    q = torch.zeros(D, dtype=BF)
    k = int_values((T, D))
    for lo, hi in [(0, 1), (0, 64), (0, 65), (0, 256), (256, 512), (512, 600), (256, 258), (128, 300), (288, 300),
                   (32, 63), (0, 600), (7, 7)]:
        part, _ = partial_ref(q, k, v, lo, hi)
        assert torch.equal(part, count_partial(lo, hi, layout, G)), (lo, hi)
        brute = torch.zeros(D, dtype=F64)
        for key in range(lo, hi):
            brute[key % D if layout == 0 else (key // G) % D] += 1
        assert torch.equal(count_cols(lo, hi, layout, G), brute), (lo, hi)
    for n in (1, 65, 257, 600):
        out, _, _ = attend64(q[None], k, v, (torch.arange(T) < n)[None])
        assert _close(out[0], count_cols(0, n, layout, G) / n)


def test_selecting_pin_margin_and_weight():
    """Every code pool the GPU file uses keeps max |s_k . s_t| <= 51, the value rows differ from
    key to key, and in float64 the target's weight is 1.0 and the output rounds to V[t]."""
    for codes in (dec_codes(), sh_codes(), pf_codes()):
        assert code_margin(codes) <= MARGIN, code_margin(codes)
        n = codes.shape[1]
        v = int_values((H, n, D))
        assert bool((v != 0).all()) and int(v.float().abs().max()) <= 127
        assert all(len(torch.unique(v[h].float(), dim=0)) == n for h in range(H))
        k = (8 * codes).to(BF)
        assert torch.equal(k.float(), 8 * codes)
        for t in (0, 1, n // 2, n - 2, n - 1):
            q = k[:, t]                                      # [H, D]
            out, _, p = attend64(q[:, None], k, v, torch.ones(1, n, dtype=torch.bool))
            assert bool((p[:, 0, t] == 1.0).all()) and float(p.sum() - H) == 0.0
            assert torch.equal(out[:, 0].to(BF), v[:, t])
            # in log2 units the runner-up lies at least 150 below: 2^-150 rounds to 0 in fp32
            s = torch.einsum("hd,hkd->hk", q.double(), k.double()) * SCALE * LOG2E
            s[:, t] = -INF
            assert float(512 * LOG2E - s.max()) >= 150.0


def _ratio(emu, ref, mag):
    return float(((emu.double() - ref).abs() / (2.0 ** -14 * mag + 1e-30)).max())


def test_fp32_emulation_a_quarter_of_the_bound():
    """The chunked algorithm in fp32 torch stays under 2^-14 mag on the peaked inputs of every
    case the GPU file runs: a quarter of the bound's 2^-12 mag, which is therefore not tuned on
    the kernels."""
    worst = {"decode": 0.0, "shared": 0.0, "prefix": 0.0}
    q, kn, vn, K, V = dec_peaked()
    ar = torch.arange(DEC_T)
    for i, p in enumerate(DEC_POS):
        for pos, append in [(ps, a) for ps in ([p] * DEC_B, dec_row_positions(i)) for a in (0, 1)]:
            Ke, Ve = K.clone(), V.clone()
            if append:  # the new token's rows at pos
                for b, pb in enumerate(pos):
                    Ke[b, :, pb], Ve[b, :, pb] = kn[b], vn[b]
            ref, mag = decode_ref(q, Ke, Ve, pos)
            vis = (ar[None, :] <= torch.tensor(pos)[:, None])[:, None, None, :]
            emu = emulate_fp32(q[:, :, None], Ke, Ve, vis, chunk_ranges(DEC_T, DEC_G))[:, :, 0]
            worst["decode"] = max(worst["decode"], _ratio(emu, ref, mag))
    B = max(SH_BS)
    q, kn, vn, pk, pv, K, V = sh_peaked(B)
    for i, P in enumerate(SH_PS):
        for offs, append in sh_configs(i, B):
            offs = offs * B if len(offs) == 1 else offs
            Ke, Ve = K.clone(), V.clone()
            for b, o in enumerate(offs if append else []):
                Ke[b, :, o], Ve[b, :, o] = kn[b], vn[b]
            pos = [P + o for o in offs]
            ref, mag = shared_ref(q, pk, pv, Ke, Ve, P, pos)
            kk, vv = shared_keys(pk, Ke, P), shared_keys(pv, Ve, P)
            vis = (torch.arange(P + SH_R)[None, :] <= torch.tensor(pos)[:, None])[:, None, None, :]
            chunks = chunk_ranges(P, SH_GP) + chunk_ranges(SH_R, SH_GR, base=P)
            emu = emulate_fp32(q[:, :, None], kk, vv, vis, chunks)[:, :, 0]
            worst["shared"] = max(worst["shared"], _ratio(emu, ref, mag))
    B = max(PF_BS)
    for P in PF_PS:
        for S in PF_SS:
            q, k, v, pk, pv = pf_peaked(B, S)
            ref, mag = prefix_ref(q, k, v, pk, pv, P)
            vis = torch.arange(P + S)[None, :] <= P + torch.arange(S)[:, None]
            emu = emulate_fp32(q, shared_keys(pk, k, P), shared_keys(pv, v, P), vis, chunk_ranges(P + S, PF_G))
            worst["prefix"] = max(worst["prefix"], _ratio(emu, ref, mag))
    print("worst fp32 emulation error / (2^-14 mag):", {k: round(x, 4) for k, x in worst.items()})
    assert max(worst.values()) <= 1.0, worst
