"""Scoring throughput: ``GPT.score`` against ``forward_logits`` + ``F.cross_entropy``.

Random-init GPT-2 weights of the named size, bf16, --batch rows of --tokens random ids.  Both ways
give the log-probability of every given token; ``score`` feeds the lm_head GEMM's padded bf16 result
straight into the log-probability kernel, chunk by chunk, the other materialises fp32 [B, T, V]
logits and lets torch reduce them.  Prints one JSON line per (mode, repeat), interleaved: tokens/s
over the B (T - 1) scored tokens and the peak allocated bytes above what was allocated before.

    python scripts/score_bench.py [--model gpt2] [--batch 8] [--tokens 1024] [--top 0,5] [--repeat 3]
"""

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanosandbox_amd.models import GPT, GPTConfig  # noqa: E402

DIMS = {"gpt2": (12, 12, 768), "gpt2-medium": (24, 16, 1024), "gpt2-large": (36, 20, 1280), "gpt2-xl": (48, 25, 1600)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--top", default="0,5", help="alternatives per token of the score modes")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--calibrate", action="store_true", help="first print the box calibration GEMM (utils/boxcal.py)")
    a = ap.parse_args()
    if a.calibrate:
        from nanosandbox_amd.utils.boxcal import calibration_gemm
        print(json.dumps({"calibration_gemm": calibration_gemm()}), flush=True)
    L, H, C = DIMS[a.model]
    torch.manual_seed(0)
    model = GPT(GPTConfig(n_layer=L, n_head=H, n_embd=C, dropout=0.0, bias=True)).eval().cuda()
    model.set_compute_dtype(torch.bfloat16)
    idx = torch.randint(0, 50257, (a.batch, a.tokens), device="cuda")
    V = model.config.vocab_size

    def xent():
        logits = model.forward_logits(idx)[:, :-1]
        return -F.cross_entropy(logits.reshape(-1, V), idx[:, 1:].reshape(-1), reduction="none")

    modes = [("forward_logits+cross_entropy", xent)]
    modes += [(f"score_top{int(n)}", lambda n=int(n): model.score(idx, top=n).token) for n in a.top.split(",")]
    with torch.no_grad():
        for _, fn in modes:  # warm-up: tuner, allocator, weight shadows
            fn()
        for _ in range(a.repeat):
            for name, fn in modes:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                mem0 = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                n = a.batch * (a.tokens - 1)
                print(json.dumps({"model": a.model, "batch": a.batch, "tokens": a.tokens, "mode": name,
                                  "tokens_per_s": round(n / dt, 1), "ms": round(dt * 1e3, 3),
                                  "peak_mb": round((torch.cuda.max_memory_allocated() - mem0) / 2 ** 20, 1),
                                  "mean_logprob": round(float(out.float().mean()), 4)}), flush=True)


if __name__ == "__main__":
    main()
