"""Per-call times of the three prompt-side linears of an int8 decoder on the four block shapes of a model: the W8A8
path (``ops.quantize_act_rows`` + ``nsa_a8_gemm``, timed together as ``a8_linear`` and the quantizer alone as
``quantize_act_rows``), the weight-only ``ops.quant_linear`` (``nsa_quant_gemm_q8``) and the bf16 ``ops.linear`` on
the dequantized shadow (c_fc without its GELU, which the bf16 path fuses into the GEMM's epilogue).  The ops of one
shape are interleaved round by round; a line per (shape, rows, op) with the median of the rounds, each round
``--calls`` calls between two device events.

    python scripts/a8_op_bench.py --model gpt2-xl --rows 1024,8192 > profiles/a8_op_bench.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/a8_op_bench.py --rounds 1 --calls 20
      (the kernel-stats run: ``--summarize DIR/.../*_kernel_trace.csv`` then prints calls and mean microseconds per
      (kernel, grid), which tells the shapes of one kernel apart)
"""

import argparse
import csv
import json
import os
import sys
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = {"gpt2": 768, "gpt2-medium": 1024, "gpt2-large": 1280, "gpt2-xl": 1600}


def summarize(path):
    rows = defaultdict(list)
    for r in csv.DictReader(open(path)):
        grid = "x".join(r[k] for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if k in r)
        rows[(r["Kernel_Name"], grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("kernel,grid,calls,mean_us,min_us")
    for (k, g), v in sorted(rows.items()):
        print(f'"{k}",{g},{len(v)},{sum(v) / len(v):.2f},{min(v):.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-xl")
    ap.add_argument("--rows", default="1024,8192")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--summarize", default="", help="a rocprofv3 kernel-trace CSV: print per (kernel, grid) times")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    from nanosandbox_amd import ops
    C = DIMS[a.model]
    shapes = [("c_attn", 3 * C, C, False), ("attn_proj", C, C, False), ("c_fc", 4 * C, C, True),
              ("mlp_proj", C, 4 * C, False)]
    torch.manual_seed(0)
    for name, N, K, gelu in shapes:
        w = ops.quantize_rows_int8(torch.randn(N, K, device="cuda") * 0.02)
        wd = ops.dequantize(w).to(torch.bfloat16)
        b = torch.zeros(N, device="cuda", dtype=torch.bfloat16)
        for M in [int(m) for m in a.rows.split(",")]:
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            fns = {"a8_linear": lambda: ops.a8_linear(x, w, b, gelu=gelu),
                   "quantize_act_rows": lambda: ops.quantize_act_rows(x),
                   "quant_linear": lambda: ops.quant_linear(x, w, b, gelu=gelu),
                   "linear": lambda: ops.linear(x, wd, b)}  # no GELU: the bf16 decoder has it in the GEMM's epilogue
            times = defaultdict(list)
            with torch.no_grad():
                for fn in fns.values():  # warm-up: code objects, the bf16 GEMM's dispatch
                    fn()
                for _ in range(a.rounds):
                    for op, fn in fns.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.calls):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        times[op].append(e0.elapsed_time(e1) / a.calls * 1e3)
            for op, ts in times.items():
                us = sorted(ts)[len(ts) // 2]
                print(json.dumps({"model": a.model, "linear": name, "rows": M, "N": N, "K": K, "gelu": gelu, "op": op,
                                  "us_per_call": round(us, 2), "tflops": round(2 * M * N * K / us / 1e6, 1),
                                  "rounds": a.rounds, "calls": a.calls}), flush=True)


if __name__ == "__main__":
    main()
