"""The device sampling kernel alone: microseconds per launch for the top-k, nucleus and
min-p settings on GPT-2's vocabulary.

Logits are ``-s ln(rank)`` in a fixed random permutation, V = 50304: s = 1.3 is peaked
like a trained model (the nucleus of top_p 0.9 is a few hundred ids), s = 0 is flat like
random-init weights (every id is in the nucleus: the kernel's wide path).  Each setting is
timed at batch 1 and 16 as a HIP graph of 100 back-to-back launches, replayed between two
hip events (>= 200 launches after warm-up); ``--repeat N`` runs the whole list N times,
interleaved, and prints the median per setting.  One JSON line per (s, batch, setting).

    python scripts/sample_bench.py [--repeat 3] [--calibrate] [--settings top_k200,top_p0.9]

``top_k200`` goes through the top-k sampler's own entry point, so it also runs against a
kernel library built from an earlier tree (``NSA_KERNEL_LIB=<path>``).
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanosandbox_amd import ops  # noqa: E402

DEV = "cuda"
V = 50304
SETTINGS = {
    "top_k200": dict(top_k=200),
    "top_p0.9": dict(top_k=0, top_p=0.9),
    "top_k200+top_p0.9": dict(top_k=200, top_p=0.9),
    "min_p0.05": dict(top_k=0, min_p=0.05),
}


def timed(fn, reps=100, replays=4):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()  # warm-up
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / (replays * reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--slopes", default="1.3,0", help="s of the logits -s ln(rank)")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--calibrate", action="store_true", help="first print the box calibration GEMM (utils/boxcal.py)")
    a = ap.parse_args()
    if a.calibrate:
        from nanosandbox_amd.utils.boxcal import calibration_gemm
        print(json.dumps({"calibration_gemm": calibration_gemm()}), flush=True)
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(1))
    rank = torch.arange(1, V + 1, dtype=torch.float64)
    cases = []
    for s in [float(x) for x in a.slopes.split(",")]:
        row = (-s * torch.log(rank))[perm].float()
        for B in [int(b) for b in a.batches.split(",")]:
            logits = row.to(DEV).expand(B, V).contiguous()
            tok = torch.zeros(B, 1, dtype=torch.int64, device=DEV)
            gen = torch.zeros(B, 8, dtype=torch.int64, device=DEV)
            pos = torch.tensor([3], dtype=torch.int64, device=DEV)
            stats = torch.zeros(B, 2, dtype=torch.int32, device=DEV)
            for name in a.settings.split(","):
                kw = dict(SETTINGS[name])
                top_k = kw.pop("top_k")
                kept = None
                if kw:  # the kept count, from a launch outside the timing (stats is NULL in the timed ones)
                    ops.sample_topk_(logits, 1.0, top_k, 1, pos, tok, gen, stats=stats, **kw)
                    kept = int(stats[0, 0])
                fn = lambda lg=logits, k=top_k, kw=kw, t=tok, g=gen: ops.sample_topk_(lg, 1.0, k, 1, pos, t, g, **kw)  # noqa: E731
                cases.append((s, B, name, kept, fn))
    times = {i: [] for i in range(len(cases))}
    for _ in range(a.repeat):
        for i, c in enumerate(cases):
            times[i].append(timed(c[4]))
    for i, (s, B, name, kept, _) in enumerate(cases):
        us = sorted(times[i])
        print(json.dumps({"op": "sample", "V": V, "s": s, "batch": B, "setting": name, "kept": kept,
                          "us": round(statistics.median(us), 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}),
              flush=True)


if __name__ == "__main__":
    main()
