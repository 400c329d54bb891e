"""The drawn ids of the device sampler, pinned: the cases of tests/golden/sampling_draws.json
(recorded by scripts/record_sampling_golden.py, replayed by tests/test_sampling_golden_gpu.py),
the CPU generators of their logits, and the two conditions that make the pin meaningful:

* every case whose reference kept set (``ops.filter_logits``) holds more than one id shows
  more than one distinct drawn id in the fixture;
* every row of a case reaches the kernel path the case is there for.  The path is derived
  from the logits by ``kernel_path``, which follows the kernel's own integer steps: the
  order-preserving keys, the element-to-thread layout, the bisection for the candidate bound
  ``lo0`` over the 1024 per-thread maxima and the candidate count against the LDS capacity.

Each case draws 32 rows at 2 positions, with one shared position and with one position per
row, at a fixed salt and temperature."""

import functools
import json
import math
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_draws.json")
ROWS, SALT, TEMPERATURE, GEN_LD = 32, 4321, 1.0, 16
POSITIONS = (3, 7)
THREADS, MAXC, CAP = 1024, 52, 4096  # SMP_THREADS, SMP_MAXC, SMP_CAP of csrc/kernels/sample.hip
NUC_LO, NUC_HI = 832, 928            # SMP_NUC_LO, SMP_NUC_HI


def _randn(V, seed):
    return torch.randn(ROWS, V, generator=torch.Generator().manual_seed(seed)) * 2


def _zipf(s, V=50304):
    """-s ln(rank), every row in its own fixed permutation."""
    base = (-s * torch.log(torch.arange(1, V + 1, dtype=torch.float64))).float()
    return torch.stack([base[torch.randperm(V, generator=torch.Generator().manual_seed(100 + b))]
                        for b in range(ROWS)])


LOGITS = {
    "randn": lambda: _randn(50304, 11),
    "randn-b": lambda: _randn(50304, 20),  # top_k 480: 1165 .. 2782 candidates in every row
    "randn63": lambda: _randn(63, 12),
    "randn64": lambda: _randn(64, 13),
    # every logit of a row equal (rows differ): any lo0 has all 50304 keys at or above it
    "equal": lambda: (torch.arange(ROWS, dtype=torch.float32) * 0.25 - 4.0).view(ROWS, 1).repeat(1, 50304),
    "zipf1.3": lambda: _zipf(1.3),
    "zipf1.1": lambda: _zipf(1.1),
}


@functools.lru_cache(maxsize=None)
def logits_of(name):
    return LOGITS[name]()


# (name, logits, top_k, top_p, min_p, the path every row reaches); top_p / min_p None: the
# top-k sampler's own entry points, otherwise the filtered one (1.0 / 0.0: its defaults).
# top_k 1024 does not reach the block-wide select: from top_k 512 on, 2 top_k covers all 1024
# thread maxima, so the bound search stops at its first point below every maximum (about
# key(-0) on these rows), half the row is a candidate and the row goes the wide way.  The
# select over more than 1024 candidates needs top_k < 512 and is what k480 is for.
_TOPK = [
    ("k200", "randn", 200, "candidates/wave-select"),
    ("k1024", "randn", 1024, "wide/bisection"),
    ("k480", "randn-b", 480, "candidates/block-select"),
    ("k2000", "randn", 2000, "wide/bisection"),
    ("v63-k5", "randn63", 5, "candidates/wave-select"),
    ("v64-full", "randn64", 0, "wide/full"),
    ("equal-k200", "equal", 200, "wide/bisection"),
]
CASES = [(n, l, k, None, None, p) for n, l, k, p in _TOPK]
CASES += [(n + "-filtered", l, k, 1.0, 0.0, p) for n, l, k, p in _TOPK]
CASES += [
    ("zipf1.3-p", "zipf1.3", 0, 0.9, 0.0, "candidates/nucleus"),
    ("zipf1.3-kp", "zipf1.3", 200, 0.9, 0.0, "candidates/wave-select"),
    ("zipf1.1-p", "zipf1.1", 0, 0.9, 0.0, "wide/nucleus"),
    ("randn-m", "randn", 0, 1.0, 0.05, "candidates/min-p"),
    ("v64-kpm", "randn64", 50, 0.9, 0.02, "wide/bisection"),
]
CASE_IDS = [c[0] for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


# ---------------------------------------------------------------------------
# the kernel's path, from the logits
# ---------------------------------------------------------------------------

def keys_of(row):
    """fkey(): fp32 -> order-preserving uint32 keys (as int64)."""
    u = row.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 1 << 31, u ^ 0xFFFFFFFF, u | (1 << 31))


def thread_maxima(keys):
    """The largest key of each of the 1024 threads (0: a thread without an element).  Rows
    with V % 4 == 0 are loaded 16 bytes at a time: element 4 (j 1024 + t) + e belongs to
    thread t; otherwise element j 1024 + t does."""
    pad = torch.zeros(THREADS * MAXC, dtype=torch.int64)
    pad[:keys.numel()] = keys
    if keys.numel() % 4 == 0:
        return pad.view(MAXC // 4, THREADS, 4).amax(dim=(0, 2))
    return pad.view(MAXC, THREADS).amax(dim=0)


def wave_bound(v, k, kcap, lo, hi):
    """wave_bound16(): the first bisection point with k .. kcap entries of v at or above it."""
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        c = int((v >= mid).sum())
        if c >= k:
            lo = mid
            if c <= kcap:
                break
        else:
            hi = mid - 1
    return lo


def kernel_path(row, top_k, top_p, min_p):
    """(path, candidates) of one row.  The two comparisons the kernel makes in floating point
    (the min-p bound, the nucleus mass at lo0) are made in float64 here and must not be close."""
    V = row.numel()
    keys = keys_of(row)
    kmax = int(keys.max())
    scale = math.log2(math.e) / TEMPERATURE
    filtered = top_p is not None
    use_k = 0 < top_k < V
    use_p = filtered and top_p < 1.0
    thr_m = 0
    if filtered and min_p > 0.0:
        lm = float(row.max()) + math.log2(min_p) / scale
        thr_m = min(int(keys_of(torch.tensor([lm], dtype=torch.float32))[0]), kmax)
        # the bound's own rounding cannot move the row across the capacity
        assert (int((row >= lm - 1e-3).sum()) <= CAP) == (int((row >= lm + 1e-3).sum()) <= CAP)
    cand, lo0, kind = False, 1, None
    if (top_k <= THREADS) if use_k else use_p:
        tmax = thread_maxima(keys)
        cand = True
        if use_k:
            lo0 = wave_bound(tmax, top_k, 2 * top_k, 0, kmax)
        else:
            lo0 = max(wave_bound(tmax, NUC_LO, NUC_HI, 0, kmax), 1)
            kind = "nucleus"
            if thr_m >= lo0:
                lo0 = thr_m
            else:
                w = torch.exp2((row.double() - float(row.max())) * scale)
                share = float(w[keys >= lo0].sum() / w.sum())
                assert abs(share - top_p) > 1e-3, f"mass at lo0 {share} too close to top_p"
                cand = share >= top_p
    elif filtered and not use_k and thr_m > 0:
        cand, lo0, kind = True, thr_m, "min-p"
    if cand:
        n = int((keys >= lo0).sum()) + (THREADS * MAXC - V if lo0 == 0 else 0)
        if n <= CAP:
            if use_k:
                kind = "block-select" if (n + 255) // 256 * 256 > 1024 else "wave-select"
            return "candidates/" + kind, n
    return "wide/" + ("bisection" if use_k else "nucleus" if use_p else "full"), None


def kept_counts(name):
    """Ids in the reference kept set, per row."""
    from nanosandbox_amd import ops

    _, lname, k, p, mp, _ = case(name)
    z = ops.filter_logits(logits_of(lname) / TEMPERATURE, k, p, mp)
    return (z > -float("Inf")).sum(-1)


def check_case(name, ids):
    """The two conditions on one case; ids: [form][position][row]."""
    _, lname, k, p, mp, path = case(name)
    logits = logits_of(lname)
    paths = [kernel_path(logits[b], k, p, mp) for b in range(ROWS)]
    assert all(q[0] == path for q in paths), (name, path, paths)
    flat = torch.tensor(ids).view(-1)
    assert flat.numel() == 2 * len(POSITIONS) * ROWS and int(flat.min()) >= 0 and int(flat.max()) < logits.size(1)
    if int(kept_counts(name).max()) > 1:
        assert flat.unique().numel() > 1, name
    return paths


# ---------------------------------------------------------------------------
# drawing on the device (the recorder and the GPU test)
# ---------------------------------------------------------------------------

def draw(name, dev="cuda"):
    """{"ids": [form][position][row], "stats": the same shape of [kept, low bits]} (stats for
    the filtered entry only); form 0: one shared position, form 1: row b draws at P + b % 3."""
    from nanosandbox_amd import ops

    _, lname, k, p, mp, _ = case(name)
    logits = logits_of(lname).to(dev)
    out = {"ids": []}
    if p is not None:
        out["stats"] = []
    for per_row in (False, True):
        ids, sts = [], []
        for P in POSITIONS:
            pos = (torch.arange(ROWS) % 3 + P if per_row else torch.tensor([P])).to(dev)
            tok = torch.full((ROWS, 1), -1, dtype=torch.int64, device=dev)
            gen = torch.full((ROWS, GEN_LD), -1, dtype=torch.int64, device=dev)
            kw = {}
            if p is not None:
                kw = dict(top_p=p, min_p=mp, stats=torch.full((ROWS, 2), -1, dtype=torch.int32, device=dev))
            ops.sample_topk_(logits, TEMPERATURE, k, SALT, pos, tok, gen, **kw)
            got = gen.gather(1, pos.expand(ROWS).view(ROWS, 1))
            assert torch.equal(got, tok) and int((gen >= 0).sum()) == ROWS  # one id per row, where it belongs
            ids.append(tok.view(-1).tolist())
            if kw:
                sts.append(kw["stats"].tolist())
        out["ids"].append(ids)
        if p is not None:
            out["stats"].append(sts)
    return out


# ---------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_header():
    g = golden()
    assert os.path.getsize(GOLDEN) < 64 * 1024
    assert (g["rows"], g["salt"], g["temperature"], g["positions"]) == (ROWS, SALT, TEMPERATURE, list(POSITIONS))
    assert sorted(g["cases"]) == sorted(CASE_IDS)


@pytest.mark.parametrize("name", CASE_IDS)
def test_fixture_case(name):
    rec = golden()["cases"][name]
    paths = check_case(name, rec["ids"])
    print(f"{name}: {paths[0][0]}, candidates {sorted({q[1] for q in paths}, key=str)}")
    _, _, k, p, mp, _ = case(name)
    assert ("stats" in rec) == (p is not None)
    if p is not None:
        # the kept counts the device reported against the reference's (float64 against fp32
        # sums: the nucleus edge may move by a few ids)
        kept = torch.tensor(rec["stats"])[..., 0]
        want = kept_counts(name).view(1, 1, ROWS).expand_as(kept)
        assert bool(((kept - want).abs() <= 0.02 * want + 2).all()), (name, kept[0, 0].tolist(), want[0, 0].tolist())
    if name.endswith("-filtered"):  # the filtered entry at its defaults draws the top-k sampler's ids
        assert rec["ids"] == golden()["cases"][name[:-len("-filtered")]]["ids"]
