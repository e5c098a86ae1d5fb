#!/usr/bin/env python3
"""Bilinear resize of decoded frames on the device: 256 RGB frames of 360 x 640 -> 224 x 224 (the MammalNet student's data path),
channels-last ([T,H,W,3], what a decoder hands over, read in place) and planar ([T,3,H,W]).

  (a) torch on the device, what a user without the kernel would run: F.interpolate(frames.float() / 255, (224, 224), "bilinear") on
      device tensors -> float frames (the dataset's output), then .mul(255).byte() -> the pixels to_pil_image makes of them;
  (b) vmc_resize_bilinear_u8: f32 output and u8 output, both recipes, microseconds and algorithmic bytes / time against the
      8 TB/s HBM figure.

Algorithmic bytes of (b): the whole source once (1 B per source sample) + 4 B (f32) or 1 B (u8) per output sample.
Timing: device events around a window of back-to-back calls sized to about 0.1 s, after a warm-up of every shape; 5 windows, the
median is reported with min and max.  Calls rotate over three input / output sets so that every call streams from HBM ("cold"): one
set (177 MB in, 154 MB f32 out) would partly stay in the 256 MiB Infinity Cache.
The kernel's outputs are compared with each other (u8 == quantised f32) before timing, and the share of torch's DEVICE bytes that
differ from the kernel's is reported: torch's device kernel is not aten's CPU arithmetic, which is what the kernel reproduces.

python tools/resize_bilinear_bench.py [--legs ab] [--frames 256] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0


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


def torch_resize(frames_nchw, size, as_u8):
    y = F.interpolate(frames_nchw.float() / 255.0, size=size, mode="bilinear", align_corners=False)
    return y.mul(255).byte() if as_u8 else y


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--size", type=int, nargs=2, default=(224, 224))
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resize_bilinear_bench: no GPU; nothing is measured without one")
    T, H, W, size = args.frames, args.height, args.width, tuple(args.size)
    NSETS = 3
    gen = torch.Generator(device="cuda").manual_seed(1)
    nhwc = [torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(NSETS)]
    in_bytes, n_out = 3 * T * H * W, 3 * T * size[0] * size[1]
    res = {"geometry": {"frames": T, "height": H, "width": W, "size": list(size)}, "input_MB": in_bytes / 1e6, "output_MB_f32": 4 * n_out / 1e6,
           "output_MB_u8": n_out / 1e6, "device": torch.cuda.get_device_name(0), "hbm_TBs_assumed": HBM_TBS, "legs": {}}
    lines = [f"# Bilinear resize on the device: {T} frames of {H} x {W} -> {size[0]} x {size[1]}", "",
             f"Device: {res['device']}.  Input {in_bytes / 1e6:.0f} MB u8, output {4 * n_out / 1e6:.0f} MB as f32 or {n_out / 1e6:.0f} MB as u8.",
             "Microseconds per call, median of 5 windows of about 0.1 s (min .. max), device events around back-to-back calls that rotate "
             "over three buffer sets, so every call streams from HBM.  Algorithmic bytes: the source once + the output; TB/s and the share "
             f"of {HBM_TBS:.0f} TB/s are those bytes over the median time.", ""]

    for layout in ("nhwc", "nchw"):
        if layout == "nhwc":
            sets = [t.permute(0, 3, 1, 2) for t in nhwc]                    # the view a decoder's stack gives; nothing is copied
        else:
            sets = [t.permute(0, 3, 1, 2).contiguous() for t in nhwc]
        leg = res["legs"].setdefault(layout, {})
        if "a" in args.legs:
            leg["a_torch_f32"] = timed(lambda i: torch_resize(sets[i % NSETS], size, False), NSETS)
            leg["a_torch_u8"] = timed(lambda i: torch_resize(sets[i % NSETS], size, True), NSETS)
        if "b" in args.legs:
            from vimo_clip_amd import ops
            for recipe in ("separable", "weights4"):
                f32 = ops.resize_bilinear_u8(sets[0], size, recipe=recipe)
                u8 = ops.resize_bilinear_u8(sets[0], size, as_u8=True, recipe=recipe)
                assert torch.equal(ops.unit_f32_to_u8(f32), u8), "u8 output is not the quantised f32 output"
                if "a" in args.legs:
                    leg[f"torch_device_bytes_differing_from_{recipe}"] = float((torch_resize(sets[0], size, True) != u8).float().mean())
                del f32, u8
                for as_u8 in (False, True):
                    outs = [torch.empty((T, 3) + size, dtype=torch.uint8 if as_u8 else torch.float32, device="cuda") for _ in range(NSETS)]
                    r = timed(lambda i: ops.resize_bilinear_u8(sets[i % NSETS], size, out=outs[i % NSETS], as_u8=as_u8, recipe=recipe), NSETS)
                    r["bytes"] = in_bytes + n_out * (1 if as_u8 else 4)
                    r["TBs"] = r["bytes"] / r["us"] / 1e6
                    r["share_of_hbm"] = r["TBs"] / HBM_TBS
                    leg[f"b_{recipe}_{'u8' if as_u8 else 'f32'}"] = r
                    del outs
        del sets
        torch.cuda.empty_cache()

    def cell(r):
        return f"{r['us']:.1f} ({r['us_min']:.1f} .. {r['us_max']:.1f})" if r else "not run"

    def bw(r):
        return f"{r['TBs']:.2f}, {100 * r['share_of_hbm']:.0f} %" if r else "not run"

    lines += ["| layout | output | (a) torch on the device | (b) separable | TB/s, share | (b) weights4 | TB/s, share | (a) / (b) separable |",
              "|---|---|---|---|---|---|---|---|"]
    for layout in ("nhwc", "nchw"):
        leg = res["legs"][layout]
        for out in ("f32", "u8"):
            a, s, w = leg.get(f"a_torch_{out}"), leg.get(f"b_separable_{out}"), leg.get(f"b_weights4_{out}")
            lines.append(f"| {layout} | {out} | {cell(a)} | {cell(s)} | {bw(s)} | {cell(w)} | {bw(w)} | "
                         + (f"{a['us'] / s['us']:.1f}x" if a and s else "-") + " |")
    diffs = {f"{layout} / {k.rsplit('_', 1)[1]}": v for layout, leg in res["legs"].items() for k, v in leg.items() if k.startswith("torch_device_bytes")}
    if diffs:
        lines += ["", "Share of torch's device-side bytes (F.interpolate on the GPU, then .mul(255).byte()) that differ from the kernel's, "
                  "which reproduces aten's CPU arithmetic: " + ", ".join(f"{k}: {100 * v:.4f} %" for k, v in diffs.items()) + "."]
    lines += ["", "(a) allocates its intermediates (float frames, divided frames, resized frames) from torch's caching allocator on every "
              "call, as user code would; (b) writes into a preallocated output.  The kernel's u8 output was compared with its quantised "
              "f32 output (torch.equal) on the timed input before timing."]
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "resize_bilinear.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out_dir, "resize_bilinear.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
