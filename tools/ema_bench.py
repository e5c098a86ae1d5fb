#!/usr/bin/env python3
"""Weight average on the device (optim.FusedAdam.enable_ema): the two kernels alone, the student step with the average on and off, and
what an evaluation under ``ema_weights()`` pays for the two swaps and refreshes.

Kernel legs (``--arenas``, default the arena sizes of ViT-B/32 and ViT-L/14): vmc_ema_update against vmc_grad_accumulate mode 1 -- the
existing kernel with the same stream, two fp32 reads and one fp32 write per element, 12 B -- and vmc_ema_swap (16 B per element).  HIP
events around windows of ``--reps`` calls; the windows ALTERNATE between the kernels, and the operand sets are rotated so that more
than 1 GiB passes between two uses of a buffer (the 256 MiB Infinity Cache holds none of it).  Median, fastest and slowest window;
achieved TB/s = the bytes the operation must move over the time.

Step legs (``--legs``, default ViT-B/32 at 32 x 16 frames and ViT-L/14 at 16 x 16): the step of bench.py's student leg (forward, cosine
distillation + BCE, backward into a GradArena, fused Adam) with the average ``off`` and ``on``; both models of a leg are resident and
the timed windows alternate between them.  ``--tree PATH --modes off --tag NAME`` imports the package from another checkout and stores
its off leg beside the others as ``off@NAME``: the off path of an older commit, measured the same way.

python tools/ema_bench.py [--legs ViT-B/32:32x16,ViT-L/14:16x16] [--modes off,on] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARENAS = {"ViT-B/32": 88_600_000, "ViT-L/14": 304_000_000}


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def summary(ms):
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def kernel_legs(arenas, reps, windows):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    e0, e1 = events()
    out = {}
    for name, n in arenas.items():
        n_sets = int((1 << 30) // (8 * n)) + 2                     # more than 1 GiB of other operands between two uses of a set
        sets = [(torch.randn(n, device="cuda"), torch.randn(n, device="cuda")) for _ in range(n_sets)]
        calls = {
            "vmc_ema_update": (12, lambda a, b: check(lib.vmc_ema_update(ptr(a), ptr(b), n, 1e-4, 0, 0, None, None, stream()), "ema_update")),
            "vmc_grad_accumulate mode 1": (12, lambda a, b: check(lib.vmc_grad_accumulate(ptr(b), ptr(a), ptr(b), n, 1e-4, 1, stream()), "grad_accumulate")),
            "vmc_ema_swap": (16, lambda a, b: check(lib.vmc_ema_swap(ptr(a), ptr(b), n, stream()), "ema_swap")),
        }
        for _, call in calls.values():
            for s in sets:
                call(*s)
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        i = 0
        for _ in range(windows):
            for k, (_, call) in calls.items():                      # alternating: one window of every kernel per round
                e0.record()
                for _ in range(reps):
                    call(*sets[i % n_sets])
                    i += 1
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / reps)
        out[name] = {"elements": n, "operand_sets": n_sets}
        for k, (per, _) in calls.items():
            r = summary(ms[k])
            r.update(bytes=per * n, tbps=per * n / r["ms"] / 1e9, tbps_min=per * n / r["ms_max"] / 1e9, tbps_max=per * n / r["ms_min"] / 1e9)
            out[name][k] = r
            print(f"{name} arena ({n / 1e6:.1f} M): {k}: {r['ms'] * 1e3:.1f} us ({r['ms_min'] * 1e3:.1f} .. {r['ms_max'] * 1e3:.1f}), "
                  f"{r['bytes'] / 1e9:.2f} GB, {r['tbps']:.2f} TB/s", flush=True)
        del sets
        torch.cuda.empty_cache()
    return out


def build(name, clips, T, mode, decay, dtype):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    R, _p, _D, _L, _H, E = synth.vit_geometry(name)
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=dtype).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=False)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=1e-4)
    if mode == "on":
        opt.enable_ema(decay)
    vids = synth.randint_u8(3, "vids", (clips, T, 3, R, R)).cuda()
    teacher = synth.normal(3, "teacher", (clips, T + 1, E)).cuda()
    labels = synth.multi_hot_labels(3, "labels", clips, 140).cuda()

    def step():
        _emb, emb_d, logits = m(vids)
        loss = distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)
        loss.backward()
        opt.step()
    return dict(step=step, opt=opt, arena=arena)


def step_leg(name, clips, T, modes, decay, dtype, steps, warmup, windows):
    legs = {mode: build(name, clips, T, mode, decay, dtype) for mode in modes}
    for leg in legs.values():
        for _ in range(warmup):
            leg["step"]()
    torch.cuda.synchronize()
    e0, e1 = events()
    ms = {mode: [] for mode in modes}
    for _ in range(windows):
        for mode in modes:
            e0.record()
            for _ in range(steps):
                legs[mode]["step"]()
            e1.record()
            torch.cuda.synchronize()
            ms[mode].append(e0.elapsed_time(e1) / steps)
    out = {}
    for mode in modes:
        out[mode] = summary(ms[mode])
        out[mode].update(frames_per_s=clips * T / out[mode]["ms"] * 1e3, arena_bytes=legs[mode]["arena"].numel * 4)
    if "on" in legs:                                                 # two swaps and two refreshes of the 16-bit copies: one evaluation
        opt, swaps = legs["on"]["opt"], []
        for _ in range(windows + 1):
            e0.record()
            with opt.ema_weights():
                pass
            e1.record()
            torch.cuda.synchronize()
            swaps.append(e0.elapsed_time(e1))
        out["on"]["swap_and_refresh_per_evaluation"] = summary(swaps[1:])
    return out


def write_md(doc, path):
    lines = ["# Weight average on the device: kernels, step time, swap cost", "",
             "Written by tools/ema_bench.py on " + doc.get("device", "?") + " (one GPU, " + doc.get("dtype", "bf16") + ").  Every figure is the median "
             "over alternating windows of back-to-back calls between two HIP events after warm-up, with the fastest and slowest window: the "
             "spread is what two figures must differ by before the difference means anything.", "",
             "Kernels alone (operand sets rotated, more than 1 GiB between two uses of a buffer; bytes = what the operation must move):", "",
             "| arena | kernel | GB moved | us (min .. max) | TB/s (min .. max) |", "|---|---|---|---|---|"]
    for arena, ks in doc.get("kernels", {}).items():
        for k, r in ks.items():
            if isinstance(r, dict):
                lines.append(f"| {arena}, {ks['elements'] / 1e6:.1f} M fp32 | {k} | {r['bytes'] / 1e9:.2f} | {r['ms'] * 1e3:.1f} ({r['ms_min'] * 1e3:.1f} .. "
                             f"{r['ms_max'] * 1e3:.1f}) | {r['tbps']:.2f} ({r['tbps_min']:.2f} .. {r['tbps_max']:.2f}) |")
    lines += ["", "Student step, average off and on (`off@NAME`: the off leg of another checkout, measured by the same tool):", "",
              "| leg | mode | ms / step (min .. max) | vs off | frames / s | arena, MB |", "|---|---|---|---|---|---|"]
    for leg, modes in doc.get("steps", {}).items():
        off = modes.get("off", {}).get("ms")
        for mode, r in sorted(modes.items()):
            lines.append(f"| {leg} | {mode} | {r['ms']:.2f} ({r['ms_min']:.2f} .. {r['ms_max']:.2f}) | " + (f"{r['ms'] / off:.4f}" if off else "-")
                         + f" | {r['frames_per_s']:.0f} | {r['arena_bytes'] / 1e6:.1f} |")
    lines += ["", "One evaluation under `ema_weights()`: two vmc_ema_swap launches and two refreshes of the 16-bit copies:", "",
              "| leg | ms (min .. max) |", "|---|---|"]
    for leg, modes in doc.get("steps", {}).items():
        r = modes.get("on", {}).get("swap_and_refresh_per_evaluation")
        if r:
            lines.append(f"| {leg} | {r['ms']:.3f} ({r['ms_min']:.3f} .. {r['ms_max']:.3f}) |")
    notes = ""
    if os.path.exists(path):                          # everything from "## Notes" on is kept as it is
        with open(path) as f:
            text = f.read()
        notes = text[text.index("## Notes"):] if "## Notes" in text else ""
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n\n" + notes)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--legs", default="ViT-B/32:32x16,ViT-L/14:16x16")
    ap.add_argument("--arenas", default="ViT-B/32,ViT-L/14")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--tree", default=HERE, help="import vimo_clip_amd from this checkout")
    ap.add_argument("--tag", default=None, help="store the legs as MODE@TAG (with --tree: another commit's off leg)")
    ap.add_argument("--out-dir", default=os.path.join(HERE, "profiles"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        sys.exit("ema_bench: no GPU; nothing is measured without one")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "ema.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(device=torch.cuda.get_device_name(0), dtype=args.dtype, decay=args.decay)
    if not args.no_kernels:
        doc["kernels"] = kernel_legs({k: ARENAS[k] for k in args.arenas.split(",") if k}, args.reps, args.windows)
    for leg in [s for s in args.legs.split(",") if s]:
        name, shape = leg.rsplit(":", 1)
        clips, T = (int(v) for v in shape.split("x"))
        res = step_leg(name, clips, T, args.modes.split(","), args.decay, dtype, args.steps, args.warmup, args.windows)
        for mode, r in res.items():
            key = mode if args.tag is None else f"{mode}@{args.tag}"
            doc.setdefault("steps", {}).setdefault(f"{name} {clips}x{T}", {})[key] = r
            print(f"{name} {clips}x{T} {key}: {r['ms']:.2f} ms/step ({r['ms_min']:.2f} .. {r['ms_max']:.2f}), arena {r['arena_bytes'] / 1e6:.1f} MB"
                  + (f", swap + refresh per evaluation {r['swap_and_refresh_per_evaluation']['ms']:.3f} ms" if "swap_and_refresh_per_evaluation" in r else ""),
                  flush=True)
        from vimo_clip_amd import autograd_ops
        autograd_ops.weights.clear()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    write_md(doc, os.path.join(args.out_dir, "ema.md"))


if __name__ == "__main__":
    main()
