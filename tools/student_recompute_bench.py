#!/usr/bin/env python3
"""Student training step with and without per-block activation recomputation (VisionTransformer.recompute).

One leg = one tower and batch, the step of bench.py's student leg (forward, cosine distillation + BCE, backward into a GradArena,
fused Adam) on one GPU, in every requested mode:

  * ms per step: HIP events around windows of ``--steps`` steps after ``--warmup`` steps; ``--windows`` windows, the median is
    reported with min and max (the spread);
  * peak allocated bytes over a step above what is allocated between steps (torch.cuda.max_memory_allocated);
  * what autograd_vit.saved_activation_bytes predicts for the batch, and the largest frame count per step it predicts to fit the
    card (activations only, against the memory that is free once model, optimiser state and inputs are resident);
  * parameters after the timed steps: "block" must equal "none" bit for bit (both start from the same state and see the same data).

A checkout without the switch (the parent of the change) is measured with ``--modes none``: the constructor is then called without
the keyword.  ``--tag`` names the result inside the JSON file, which is merged, so several runs fill one table.

python tools/student_recompute_bench.py [--model ViT-B/32] [--clips 32] [--frames 16] [--modes none,block] [--tag this] [--out-dir profiles]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_leg(name, clips, T, mode, dtype, steps, warmup, windows):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    kw = {"recompute": mode} if "recompute" in inspect.signature(FlowStudentModel.__init__).parameters else {}
    if mode != "none" and not kw:
        raise SystemExit("this checkout has no recompute switch: run it with --modes none")
    R, p, D, L, H, E = synth.vit_geometry(name)
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=dtype, **kw).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=True)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=1e-3)
    vids = synth.randint_u8(3, "vids", (clips, T, 3, R, R)).cuda()
    teacher = synth.normal(3, "teacher", (clips, T + 1, E)).cuda()
    labels = synth.multi_hot_labels(3, "labels", clips, 140).cuda()

    def step():
        emb, emb_d, logits = m(vids)
        loss = distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(windows):
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    peak = torch.cuda.max_memory_allocated() - base
    free, total = torch.cuda.mem_get_info()
    res = {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "windows": windows, "steps_per_window": steps,
           "warmup_steps": warmup, "peak_step_bytes": peak, "resident_between_steps_bytes": base,
           "frames_per_s": clips * T / statistics.median(ms) * 1e3}
    params = arena.flat_param.detach().cpu().clone()
    del m, arena, opt, vids, teacher, labels
    from vimo_clip_amd import autograd_ops
    autograd_ops.weights.clear()                    # the 16-bit copies of this leg's weights would stay resident in the next leg
    torch.cuda.empty_cache()
    return res, params, total


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--modes", default="none,block")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("student_recompute_bench: no GPU; nothing is measured without one")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    frames = args.clips * args.frames
    leg = f"{args.model} {args.clips}x{args.frames} {args.dtype}"
    out = {"device": torch.cuda.get_device_name(0), "frames_per_step": frames, "modes": {}}
    params = {}
    for mode in args.modes.split(","):
        r, params[mode], total = run_leg(args.model, args.clips, args.frames, mode, dtype, args.steps, args.warmup, args.windows)
        try:
            from vimo_clip_amd.autograd_vit import saved_activation_bytes
            r["model_saved_bytes"] = saved_activation_bytes(args.model, frames, mode)
            per_frame = saved_activation_bytes(args.model, 1, mode)
            if mode == "block":                     # one recomputed block is alive on top of the streams
                from vimo_clip_amd.synth import vit_geometry
                per_frame += saved_activation_bytes(args.model, 1, "none", cls_only=False) // vit_geometry(args.model)[3]
            r["model_bytes_per_frame_with_live_block"] = per_frame
            r["predicted_max_frames_per_step"] = int((total - r["resident_between_steps_bytes"]) // per_frame)
        except ImportError:
            pass                                    # a checkout without the byte model
        out["modes"][mode] = r
        print(f"{leg} [{args.tag}] recompute={mode}: {r['ms']:.2f} ms/step ({r['ms_min']:.2f} .. {r['ms_max']:.2f}), "
              f"peak over a step {r['peak_step_bytes'] / 1e9:.3f} GB, resident {r['resident_between_steps_bytes'] / 1e9:.3f} GB", flush=True)
    if "none" in params and "block" in params:
        out["block_equals_none_bitwise"] = bool(torch.equal(params["none"], params["block"]))
        print(f"parameters after the timed steps, block == none: {out['block_equals_none_bitwise']}")
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "student_recompute.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault(leg, {})[args.tag] = out
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    lines = ["| leg | checkout | recompute | ms / step (min .. max) | frames / s | peak over a step, GB | byte model (saved), GB | "
             "predicted max frames / step | block == none |", "|---|---|---|---|---|---|---|---|---|"]
    for leg_name, tags in sorted(doc.items()):
        for tag, o in sorted(tags.items()):
            if "modes" not in o:                    # hand-kept notes
                continue
            for mode, r in o["modes"].items():
                lines.append(f"| {leg_name} | {tag} | {mode} | {r['ms']:.2f} ({r['ms_min']:.2f} .. {r['ms_max']:.2f}) | {r['frames_per_s']:.0f} | "
                             f"{r['peak_step_bytes'] / 1e9:.3f} | "
                             + (f"{r['model_saved_bytes'] / 1e9:.3f}" if "model_saved_bytes" in r else "-") + " | "
                             + (str(r["predicted_max_frames_per_step"]) if "predicted_max_frames_per_step" in r else "-") + " | "
                             + (str(o["block_equals_none_bitwise"]) if "block_equals_none_bitwise" in o else "-") + " |")
    md = os.path.join(args.out_dir, "student_recompute.md")
    notes = ""
    if os.path.exists(md):                          # everything from "## Notes" on is kept as it is
        with open(md) as f:
            text = f.read()
        notes = text[text.index("## Notes"):] if "## Notes" in text else ""
    head = ["# Student training step: per-block activation recomputation", "",
            "Written by tools/student_recompute_bench.py (one GPU; forward, cosine distillation + BCE, backward into a GradArena, fused "
            "Adam).  ms / step: median over windows of back-to-back steps between two HIP events after warm-up steps, with the "
            "fastest and slowest window.  Peak: torch.cuda.max_memory_allocated over the timed steps above what is allocated between "
            "steps.  Byte model: autograd_vit.saved_activation_bytes for the batch; the predicted frame count divides the card's memory "
            "minus what is resident between steps by the model's bytes per frame (in \"block\" mode plus one live block).", ""]
    with open(md, "w") as f:
        f.write("\n".join(head + lines) + "\n\n" + notes)


if __name__ == "__main__":
    main()
