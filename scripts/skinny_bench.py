"""Per-call time of the decode linears at GPT-2 shapes: one-row GEMV, the MFMA skinny
GEMM (2..16 rows), the wide split-K GEMM (17..64 rows), the tall all-rows GEMM (65..256 rows) and
``linear`` (+ bias, + GELU: the small-tile / NT kernels) at the same row counts.

    python scripts/skinny_bench.py [--rows 1,4,8,16,32,64,128,256] [--iters 200] [--ksplits 1,2,4]

Above 16 rows a line holds ``wide_us`` (``nsa_wide_gemm`` under its own split rule, the split in
``ksplit``), ``skinny_us`` (``nsa_skinny_gemm`` with its cap raised to 64) and ``library_us``
(``linear``).  ``*_weight_GBps`` is a call-level rate: N K 2 bytes of weights over the time of one
call in a back-to-back loop (launch gaps included), not a share of any peak.  ``--ksplits`` adds
``wide_ks<n>_us``: raw launches with that split instead of the rule's.  Above 64 rows a line holds ``tall_us``
(``nsa_tall_gemm`` under its own rule, the split in ``ksplit``) beside ``library_us``, and ``--ksplits`` adds
``tall_ks<n>_us``.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanosandbox_amd.ops import _lib, functional  # noqa: E402

SHAPES = {"gpt2": [("c_attn", 2304, 768), ("c_proj", 768, 768), ("c_fc", 3072, 768), ("mlp.c_proj", 768, 3072),
                   ("lm_head", 50304, 768)],
          "gpt2-xl": [("c_attn", 4800, 1600), ("c_proj", 1600, 1600), ("c_fc", 6400, 1600),
                      ("mlp.c_proj", 1600, 6400), ("lm_head", 50304, 1600)]}


def timed(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def with_caps(fn, iters, gemv=1, skinny=16, wide=0, tall=0):
    """Time ``fn`` under the given row caps of ``decode_linear`` (wide / tall 0: that kernel off)."""
    f = functional
    saved = f.GEMV_MAX_ROWS, f.SKINNY_MAX_ROWS, f.WIDE_MAX_ROWS, f.TALL_MAX_ROWS
    f.GEMV_MAX_ROWS, f.SKINNY_MAX_ROWS, f.WIDE_MAX_ROWS, f.TALL_MAX_ROWS = gemv, skinny, wide, tall
    try:
        return round(timed(fn, iters), 2)
    finally:
        f.GEMV_MAX_ROWS, f.SKINNY_MAX_ROWS, f.WIDE_MAX_ROWS, f.TALL_MAX_ROWS = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,4,8,16,32,64")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ksplits", default="", help="also time raw nsa_wide_gemm (17..64 rows) / nsa_tall_gemm "
                                                  "(above 64) launches with these splits of K")
    a = ap.parse_args()
    for model, shapes in SHAPES.items():
        for op, N, K in shapes:
            w = (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)
            b = None if op == "lm_head" else torch.zeros(N, device="cuda", dtype=torch.bfloat16)
            gelu = op == "c_fc"
            f32 = op == "lm_head"
            for rows in [int(r) for r in a.rows.split(",")]:
                x = torch.randn(rows, 1, K, device="cuda").to(torch.bfloat16)
                rec = {"model": model, "op": op, "N": N, "K": K, "rows": rows}
                rate = lambda us: round(N * K * 2 / us / 1e3, 1)  # noqa: E731

                def run():
                    return functional.decode_linear(x, w, b, gelu=gelu, out_f32=f32)

                if rows <= 16:
                    rec["ours_us"] = with_caps(run, a.iters)
                    rec["weight_GBps"] = rate(rec["ours_us"])
                elif rows > 64:
                    rec["ksplit"] = _lib.call_ret("nsa_tall_gemm_ksplit", rows, N, K)
                    rec["tall_us"] = with_caps(run, a.iters, wide=64, tall=256)
                    rec["tall_weight_GBps"] = rate(rec["tall_us"])
                else:
                    rec["ksplit"] = _lib.call_ret("nsa_wide_gemm_ksplit", rows, N, K)
                    rec["wide_us"] = with_caps(run, a.iters, wide=64)
                    rec["skinny_us"] = with_caps(run, a.iters, skinny=64)
                    rec["wide_weight_GBps"], rec["skinny_weight_GBps"] = rate(rec["wide_us"]), rate(rec["skinny_us"])
                rec["library_us"] = with_caps(run, a.iters, gemv=0, skinny=1)
                raw = "tall" if rows > 64 else "wide"
                for ks in [int(k) for k in a.ksplits.split(",") if k and rows > 16 and int(k) <= K // 32]:
                    need = _lib.call_ret(f"nsa_{raw}_gemm_ws_bytes", rows, N, K, ks)
                    ws = torch.zeros(max(need, 16), device="cuda", dtype=torch.uint8)
                    y = torch.empty(rows, N, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
                    args = (x.data_ptr(), w.data_ptr(), _lib.ptr(b), y.data_ptr(), rows, N, K, int(gelu), int(f32), ks,
                            ws.data_ptr(), ws.numel())
                    rec[f"{raw}_ks{ks}_us"] = round(timed(lambda: _lib.call(f"nsa_{raw}_gemm", *args, _lib.stream()),
                                                          a.iters), 2)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
