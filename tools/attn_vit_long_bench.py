#!/usr/bin/env python3
"""ViT self-attention past 288 tokens (attention_vit_long.hip behind vmc_attention_vit_fwd) against the generic tiled kernel of
attention_long.hip (vmc_attention_fwd with q = qkv, k = qkv + D, v = qkv + 2D, ld 3D, no mask), on the same packed random-normal
operands, alternating per round in one process, HIP events, medians.  H = 16, head_dim 64, F in {16, 64, 256}, N in {289, 577, 1025},
bf16 and f16.  The class-query call (NQ = 1, the last encoder block) is timed against its K / V-bytes floor.

  python tools/attn_vit_long_bench.py [--reps N] [--rounds R] [--json OUT] [--quick]

Rates: 4 N^2 64 FLOPs per (frame, head) (Q K^T and P V); share of the 2.5 PFLOP/s dense bf16 / f16 MFMA peak.  The class-query
floor: the K and V bytes of every (frame, head) (2 N 64 x 2 B) read once at the 8 TB/s HBM peak."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vimo_clip_amd import ops  # noqa: E402

PEAK, HBM = 2.5e15, 8.0e12
H = 16


def time_rounds(fns, reps, rounds):
    out = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            out[n].append(e0.elapsed_time(e1) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="F = 256, N = 577 only")
    a = ap.parse_args()
    D = H * 64
    g = torch.Generator().manual_seed(0)
    rows = []
    shapes = [(256, 577)] if a.quick else [(F, N) for N in (289, 577, 1025) for F in (16, 64, 256)]
    for dtype in (torch.bfloat16, torch.float16):
        for F, N in shapes:
            qkv = torch.randn((F * N, 3 * D), generator=g).to(dtype).cuda()
            fns = {
                "vit_long": lambda: ops.attention_vit(qkv, F, N, H),
                "generic": lambda: ops.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], None, F, H, N, N, 64),
            }
            o1, o2 = fns["vit_long"]()[0], fns["generic"]()[0]
            diff = (o1.float() - o2.float()).abs().max().item()
            torch.cuda.synchronize()
            t = time_rounds(fns, a.reps, a.rounds)
            flops = 4.0 * F * H * N * N * 64
            row = {"dtype": str(dtype).split(".")[-1], "F": F, "N": N, "H": H, "max_abs_diff": diff}
            for n, v in t.items():
                ms = statistics.median(v)
                row[n] = {"ms": ms, "min_ms": min(v), "max_ms": max(v), "tflops": flops / ms / 1e9, "peak_share": flops / ms * 1e3 / PEAK}
            row["speedup"] = row["generic"]["ms"] / row["vit_long"]["ms"]
            rows.append(row)
            print(f"{row['dtype']} F={F:4d} N={N:5d}: vit_long {row['vit_long']['ms'] * 1e3:9.1f} us {row['vit_long']['tflops']:6.1f} TF/s "
                  f"({100 * row['vit_long']['peak_share']:.1f} %)  generic {row['generic']['ms'] * 1e3:9.1f} us {row['generic']['tflops']:6.1f} TF/s "
                  f"({100 * row['generic']['peak_share']:.1f} %)  x{row['speedup']:.2f}  max|diff| {diff:.1e}", flush=True)
            del qkv
    cls_rows = []
    for dtype in (torch.bfloat16, torch.float16):
        for F in ((256,) if a.quick else (16, 64, 256)):
            N = 577
            qkv = torch.randn((F * N, 3 * D), generator=g).to(dtype).cuda()
            q_cls = qkv.view(F, N, 3 * D)[:, 0, :D].contiguous()
            kv = qkv[:, D:].contiguous()
            t = time_rounds({"cls": lambda: ops.attention_vit_cls(q_cls, kv, F, N, H)}, a.reps, a.rounds)
            ms = statistics.median(t["cls"])
            floor_ms = F * H * 2 * N * 64 * 2 / HBM * 1e3
            cls_rows.append({"dtype": str(dtype).split(".")[-1], "F": F, "N": N, "H": H, "ms": ms, "floor_ms": floor_ms,
                             "floor_share": floor_ms / ms})
            print(f"class query {cls_rows[-1]['dtype']} F={F:4d} N={N}: {ms * 1e3:8.1f} us, K/V floor {floor_ms * 1e3:7.1f} us "
                  f"({100 * floor_ms / ms:.0f} % of it)", flush=True)
            del qkv, kv
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "full": rows, "class_query": cls_rows}, f, indent=1)


if __name__ == "__main__":
    main()
