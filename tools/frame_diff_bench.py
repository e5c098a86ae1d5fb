#!/usr/bin/env python3
"""Frame-difference motion frames on the device: 256 RGB frames of 360 x 640 (the AK geometry of SURVEY.md K0), NHWC and NCHW.

  (a) torch composition: integer grey and |difference| out of plain torch ops on the device (uses nothing of libvmc's frame
      difference, so ``--legs a`` also runs on a checkout that does not have it);
  (b) vmc_frame_diff_gray_u8: microseconds and algorithmic bytes / time against the 8 TB/s HBM figure;
  (c) student export preprocessing of the motion frames (difference -> Resize(224, BICUBIC) + CenterCrop -> exact patch operands,
      ViT-B/32 geometry): through three materialised channels versus through one plane.

Timing: device events around a window of back-to-back calls sized to about 0.1 s, after a warm-up of every shape; 5 windows, the
median is reported with min and max.  Cache state: input (177 MB) plus output (59 MB) of one call fit the 256 MiB Infinity Cache,
so back-to-back calls on ONE buffer re-read part of the input on-die ("warm").  The headline numbers are "cold": the calls rotate
over three input / output sets (708 MB between two uses of a line), so every call streams from HBM as it does in an export.

python tools/frame_diff_bench.py [--legs abc] [--frames 256] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0
W_R, W_G, W_B, SHIFT = 9798, 19235, 3735, 15


def torch_frame_diff(frames, layout):
    """Leg (a): the same integers from stock torch ops."""
    r, g, b = (frames[..., c] for c in range(3)) if layout == "nhwc" else (frames[:, c] for c in range(3))
    gray = (r.int() * W_R + g.int() * W_G + b.int() * W_B + (1 << (SHIFT - 1))) >> SHIFT
    return (gray[1:] - gray[:-1]).abs().to(torch.uint8).unsqueeze(1)


def timed(fn, nsets, windows=5, target_s=0.1):
    """fn(i) runs one call on buffer set i % nsets.  Returns microseconds per call: (median, min, max) over the windows."""
    for i in range(max(3, nsets)):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(3):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    iters = max(6, int(target_s / max(e0.elapsed_time(e1) / 3e3, 1e-6)))
    iters = (iters + nsets - 1) // nsets * nsets
    us = []
    for _ in range(windows):
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {"us": statistics.median(us), "us_min": min(us), "us_max": max(us), "iters": iters, "windows": windows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_diff_bench: no GPU; nothing is measured without one")
    T, H, W = args.frames, args.height, args.width
    NSETS = 3
    gen = torch.Generator(device="cuda").manual_seed(1)
    nhwc = [torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(NSETS)]
    in_bytes, out_bytes = 3 * T * H * W, (T - 1) * H * W
    res = {"geometry": {"frames": T, "height": H, "width": W}, "input_MB": in_bytes / 1e6, "output_MB_one_channel": out_bytes / 1e6,
           "device": torch.cuda.get_device_name(0), "hbm_TBs_assumed": HBM_TBS, "legs": {}}
    lines = [f"# Frame-difference motion frames: {T} frames of {H} x {W}", "",
             f"Device: {res['device']}.  Input {in_bytes / 1e6:.0f} MB, one-channel output {out_bytes / 1e6:.0f} MB.",
             "Microseconds per call, median of 5 windows of about 0.1 s (min .. max).  cold = calls rotate over three buffer sets "
             "(every call streams from HBM); warm = back-to-back calls on one set (input + output fit the 256 MiB Infinity Cache, "
             "part of the input is re-read on-die).", ""]

    for layout in ("nhwc", "nchw"):
        sets = nhwc if layout == "nhwc" else None
        if layout == "nchw":
            sets = [t.permute(0, 3, 1, 2).contiguous() for t in nhwc]
        leg = res["legs"].setdefault(layout, {})
        if "a" in args.legs:
            leg["a_torch_cold"] = timed(lambda i: torch_frame_diff(sets[i % NSETS], layout), NSETS)
        if "b" in args.legs:
            from vimo_clip_amd import ops
            outs = [torch.empty((T - 1, 1, H, W), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
            want = torch_frame_diff(sets[0], layout)
            assert torch.equal(ops.frame_diff_gray(sets[0], layout=layout), want), "kernel and torch composition differ"
            del want
            for state, n in (("cold", NSETS), ("warm", 1)):
                r = timed(lambda i: ops.frame_diff_gray(sets[i % n], layout=layout, out=outs[i % n]), n)
                r["bytes"] = in_bytes + out_bytes
                r["TBs"] = r["bytes"] / r["us"] / 1e6
                r["share_of_hbm"] = r["TBs"] / HBM_TBS
                leg[f"b_kernel_{state}"] = r
            del outs
        if layout == "nchw":
            del sets
        torch.cuda.empty_cache()

    if "c" in args.legs:
        from vimo_clip_amd import ops
        from vimo_clip_amd.preprocess import resize_center_crop_u8
        R, P, dt16 = 224, 32, torch.bfloat16
        perm = [t.permute(0, 3, 1, 2) for t in nhwc]              # what the exporter's decoder hands over

        def route(i, ch):
            d = ops.frame_diff_gray(perm[i % NSETS], channels=ch)
            fr, wrap = resize_center_crop_u8(d, R, "torchvision", True)
            return (ops.patches_u8_exact if ch == 3 else ops.patches_gray_u8_exact)(fr, P, dt16, wrap)

        assert torch.equal(route(0, 3).view(torch.int16), route(0, 1).view(torch.int16)), "one-plane and three-plane patches differ"
        res["legs"]["c_export_preprocess"] = {"geometry": f"ViT-B/32: R {R}, patch {P}, bf16 exact patch operands, wrap quirk on",
                                              "three_planes_cold": timed(lambda i: route(i, 3), NSETS),
                                              "one_plane_cold": timed(lambda i: route(i, 1), NSETS)}

    def cell(r):
        return f"{r['us']:.1f} ({r['us_min']:.1f} .. {r['us_max']:.1f})"

    lines += ["| layout | (a) torch composition, cold | (b) kernel, cold | (b) TB/s, share of 8 TB/s | (b) kernel, warm | (a) / (b) |", "|---|---|---|---|---|---|"]
    for layout in ("nhwc", "nchw"):
        leg = res["legs"][layout]
        a, bc, bw = leg.get("a_torch_cold"), leg.get("b_kernel_cold"), leg.get("b_kernel_warm")
        lines.append(f"| {layout} | {cell(a) if a else 'not run'} | {cell(bc) if bc else 'not run'} | "
                     + (f"{bc['TBs']:.2f}, {100 * bc['share_of_hbm']:.0f} %" if bc else "not run") + f" | {cell(bw) if bw else 'not run'} | "
                     + (f"{a['us'] / bc['us']:.1f}x" if a and bc else "-") + " |")
    c = res["legs"].get("c_export_preprocess")
    if c:
        t3, t1 = c["three_planes_cold"], c["one_plane_cold"]
        lines += ["", f"(c) student export preprocessing of the motion frames ({c['geometry']}), difference + resize + crop + patch operands, cold:", "",
                  "| route | us |", "|---|---|", f"| three materialised channels | {cell(t3)} |", f"| one plane | {cell(t1)} |",
                  "", f"one plane / three planes = {t1['us'] / t3['us']:.2f}"]
    lines += ["", "Algorithmic bytes of (b): 3 B read + 1 B written per output pixel (each input frame counted once).  Kernel and torch "
              "composition were compared with torch.equal on the timed input before timing; so were the two routes of (c)."]
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "frame_diff.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out_dir, "frame_diff.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
