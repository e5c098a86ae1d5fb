#!/usr/bin/env python3
"""Gradient accumulation on the gradient arena (GradArena.accumulate / vmc_grad_accumulate): what it costs and what it saves.

  kernel  One leg per arena (the student's ViT-B/32 and ViT-L/14, the TFAM block at d_model 768): the three modes of
          vmc_grad_accumulate over the whole arena and, as the yardstick, the optimiser pass over the same arena in device-state
          mode (FusedAdam.tick + step: vmc_train_tick, then vmc_adam_cast_multi and its small second launch).  The variants
          ALTERNATE inside every round; a round times `--inner` back-to-back launches of each between two HIP events after
          warm-up launches; the median over `--rounds` rounds is reported with the fastest and the slowest round.  Bytes are the
          algorithm's: 8 n (mode 0), 12 n (modes 1, 2); 28 n for Adam plus 2 B for every element that has a 16-bit compute copy.
  step    One leg per (tower, clips x frames): the training step of tools/student_recompute_bench.py (forward, cosine
          distillation + BCE, backward into the arena, fused Adam; inputs resident on the device) in every requested variant
          `micro-batches:recompute`, e.g. 1:none,4:none,1:block,4:block.  The variants alternate window by window; ms per step is
          the median over the windows; the peak is torch.cuda.max_memory_allocated over one step above what is allocated between
          steps.  The byte model (autograd_vit.saved_activation_bytes) is printed beside it.

Results are merged into <out-dir>/grad_accum.json under --tag; <out-dir>/grad_accum.md is rewritten from the JSON, and everything
from "## Notes" on is kept as it is.

python tools/grad_accum_bench.py kernel [--arenas ViT-B/32,ViT-L/14,TFAM-768] [--inner 20] [--rounds 7]
python tools/grad_accum_bench.py step --model ViT-L/14 --clips 16 --frames 16 --variants 1:none,4:none,1:block,4:block
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


# ---- kernel -------------------------------------------------------------------------------------------------------------------------
def _student_arena(name):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    R, p, D, L, H, E = synth.vit_geometry(name)
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=torch.bfloat16).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=True)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=1e-4).enable_device_state()
    vids = synth.randint_u8(3, "vids", (1, 2, 3, R, R)).cuda()
    teacher = synth.normal(3, "teacher", (1, 3, E)).cuda()
    labels = synth.multi_hot_labels(3, "labels", 1, 140).cuda()

    def one_step():                                  # the 16-bit compute copies exist after it: the optimiser takes its fused pass
        opt.tick()
        emb, emb_d, logits = m(vids)
        (distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)).backward()
        opt.step()
    return m, arena, opt, one_step


def _tfam_arena(d_model):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad
    from vimo_clip_amd.optim import FusedAdam, GradArena
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    dev = torch.device("cuda", 0)
    m = AMO_CLIP(d_model=d_model, nhead=8, num_layers=4, dim_feedforward=2048, num_classes=140, dropout=0.1, mlp_dropout=0.1, device=dev).to(dev).train()
    m.load_state_dict(synth.tfam_state_dict(d_model, 8, 4, 2048, 140, 4), strict=True)
    arena = GradArena(m.used_parameters())
    opt = FusedAdam(arena, lr=1e-4, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=0)
    m.use_device_seeds(opt)
    B = 8
    rgb, mot = synth.normal(30, "rgb", (B, 16, d_model)).to(dev), synth.normal(30, "mot", (B, 16, d_model)).to(dev)
    mk = torch.ones(B, 16, dtype=torch.bool, device=dev)
    y = synth.multi_hot_labels(30, "lab", B, 140).to(dev)

    def one_step():
        opt.tick()
        out = m(rgb, mot, mask_rgb=mk, mask_flow=mk)
        _, dl = loss_and_grad(bce_with_logits_loss, out, y)
        out.backward(dl)
        opt.step()
    return m, arena, opt, one_step


def kernel_leg(name, inner, rounds):
    from vimo_clip_amd import autograd_ops
    from vimo_clip_amd._lib import check, lib, ptr, stream
    m, arena, opt, one_step = _tfam_arena(int(name.split("-")[1])) if name.startswith("TFAM-") else _student_arena(name)
    for _ in range(2):
        one_step()
    torch.cuda.synchronize()
    fused = getattr(opt, "_fused_plan", None) is not None
    n = arena.numel
    copies = sum(p.numel() for p in arena.params if p.dim() >= 2) if fused else 0
    arena.flat_grad.normal_(generator=torch.Generator(device="cuda").manual_seed(1))
    arena.flat_grad.mul_(1e-3)
    arena.flat_acc = torch.zeros_like(arena.flat_grad)
    g, acc = arena.flat_grad, arena.flat_acc

    def accum(mode):
        return lambda: check(lib.vmc_grad_accumulate(ptr(g), ptr(acc), ptr(g), n, 0.25, mode, stream()), "grad_accumulate")

    def adam():
        opt.tick()
        opt.step()
    variants = {"mode0": (accum(0), 8 * n), "mode1": (accum(1), 12 * n), "mode2": (accum(2), 12 * n), "adam_pass": (adam, 28 * n + 2 * copies)}
    for fn, _ in variants.values():                  # warm every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, _) in variants.items():
            ms[k].append(_events_ms(fn, inner))
    res = {"elements": n, "bytes_per_buffer": 4 * n, "adam_pass_is_adam_cast_multi": fused, "elements_with_16bit_copy": copies,
           "inner": inner, "variants": {}}
    for k, (fn, nbytes) in variants.items():
        s = _summary(ms[k])
        res["variants"][k] = {"us": s["median"] * 1e3, "us_min": s["min"] * 1e3, "us_max": s["max"] * 1e3, "rounds": s["n"], "bytes": nbytes,
                              "TB_per_s": nbytes / (s["median"] * 1e-3) / 1e12}
    a = res["variants"]["adam_pass"]["TB_per_s"]
    for k in ("mode0", "mode1", "mode2"):
        res["variants"][k]["rate_vs_adam_pass"] = res["variants"][k]["TB_per_s"] / a
        print(f"{name} ({n / 1e6:.1f} M elements) {k}: {res['variants'][k]['us']:.1f} us ({res['variants'][k]['us_min']:.1f} .. "
              f"{res['variants'][k]['us_max']:.1f}), {res['variants'][k]['TB_per_s']:.2f} TB/s = {res['variants'][k]['rate_vs_adam_pass']:.2f} x the Adam pass",
              flush=True)
    print(f"{name} adam_pass (fused cast: {fused}): {res['variants']['adam_pass']['us']:.1f} us, {a:.2f} TB/s", flush=True)
    del m, arena, opt, g, acc, variants
    autograd_ops.weights.clear()
    torch.cuda.empty_cache()
    return res


# ---- step ---------------------------------------------------------------------------------------------------------------------------
def _make_variant(name, clips, T, k, mode, dtype):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    from vimo_clip_amd.train import split_micro_batches
    R, p, D, L, H, E = synth.vit_geometry(name)
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=dtype, recompute=mode).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=True)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=1e-3)
    batch = {"flow_frames": synth.randint_u8(3, "vids", (clips, T, 3, R, R)).cuda(), "rgb_emb": synth.normal(3, "teacher", (clips, T + 1, E)).cuda(),
             "labels": synth.multi_hot_labels(3, "labels", clips, 140).cuda()}
    micro = split_micro_batches(batch, k)

    def step():
        for j, (sub, w) in enumerate(micro):
            emb, emb_d, logits = m(sub["flow_frames"])
            loss = distillation_loss(emb_d, sub["rgb_emb"][:, :-1, :], mode="cosine") + classification_loss(logits, sub["labels"], positive_weight=9)
            loss.backward()
            arena.accumulate(w, final=j == len(micro) - 1)      # one micro-batch: launches nothing
        opt.step()
    return {"step": step, "keep": (m, arena, opt, batch), "micro": len(micro)}


def step_leg(args):
    from vimo_clip_amd import synth
    from vimo_clip_amd.autograd_vit import saved_activation_bytes
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    frames = args.clips * args.frames
    layers = synth.vit_geometry(args.model)[3]
    specs = [(int(v.split(":")[0]), v.split(":")[1]) for v in args.variants.split(",")]
    variants = {}
    for k, mode in specs:
        tag = f"{k}:{mode}"
        v = variants[tag] = _make_variant(args.model, args.clips, args.frames, k, mode, dtype)
        for _ in range(args.warmup):
            v["step"]()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        v["step"]()
        torch.cuda.synchronize()
        v["peak"] = torch.cuda.max_memory_allocated() - base
        v["ms"] = []
        print(f"{args.model} {args.clips}x{args.frames} {tag}: warmed, peak over a step {v['peak'] / 1e9:.3f} GB", flush=True)
    for _ in range(args.windows):
        for tag, v in variants.items():
            v["ms"].append(_events_ms(v["step"], args.steps))
    out = {"frames_per_step": frames, "steps_per_window": args.steps, "warmup_steps": args.warmup, "variants": {}}
    arena_bytes = 4 * next(iter(variants.values()))["keep"][1].numel
    for (k, mode), (tag, v) in zip(specs, variants.items()):
        s = _summary(v["ms"])
        micro_frames = -(-args.clips // k) * args.frames
        live_block = saved_activation_bytes(args.model, micro_frames, "none", cls_only=False) // layers
        out["variants"][tag] = {"ms": s["median"], "ms_min": s["min"], "ms_max": s["max"], "windows": s["n"], "micro_batches": v["micro"],
                                "peak_step_bytes": v["peak"], "frames_per_s": frames / s["median"] * 1e3,
                                "model_saved_bytes": saved_activation_bytes(args.model, micro_frames, mode) + (live_block if mode == "block" else 0)
                                + (arena_bytes if v["micro"] > 1 else 0)}
        print(f"{args.model} {args.clips}x{args.frames} {tag}: {s['median']:.2f} ms/step ({s['min']:.2f} .. {s['max']:.2f}), peak {v['peak'] / 1e9:.3f} GB, "
              f"byte model {out['variants'][tag]['model_saved_bytes'] / 1e9:.3f} GB", flush=True)
    return out


# ---- output -------------------------------------------------------------------------------------------------------------------------
def render(doc):
    lines = ["# Gradient accumulation on the gradient arena", "",
             "Written by tools/grad_accum_bench.py on one GPU.  Kernel legs: the variants alternate inside every round, a round times "
             "back-to-back launches of one variant between two HIP events after warm-up launches; median over the rounds with the "
             "fastest and the slowest round.  Bytes are the algorithm's (8 n, 12 n, 12 n; the Adam pass 28 n plus 2 B per element "
             "with a 16-bit copy).  adam pass = FusedAdam.tick + step in device-state mode on the same arena: vmc_train_tick (one "
             "workgroup), vmc_adam_cast_multi and its small second launch.  Step legs: forward, cosine distillation + BCE, backward "
             "into the arena, fused Adam, inputs resident; `k:mode` = micro-batches : recompute; the variants alternate window by "
             "window; peak = torch.cuda.max_memory_allocated over one step above what is allocated between steps; byte model = "
             "saved_activation_bytes of one micro-batch (+ one live block with recomputation, + the 4 B / parameter accumulator).", ""]
    for tag, runs in sorted(doc.items()):
        if "kernel" in runs:
            lines += [f"## Kernel ({tag}, {runs.get('device', '?')})", "",
                      "| arena | elements | variant | us (min .. max) | bytes | TB/s | rate / optimiser pass (tick + step: three launches) |", "|---|---|---|---|---|---|---|"]
            for arena, r in runs["kernel"].items():
                for k, v in r["variants"].items():
                    lines.append(f"| {arena} | {r['elements']} | {k} | {v['us']:.1f} ({v['us_min']:.1f} .. {v['us_max']:.1f}) | {v['bytes']} | "
                                 f"{v['TB_per_s']:.2f} | " + (f"{v['rate_vs_adam_pass']:.2f}" if "rate_vs_adam_pass" in v else "1") + " |")
            lines.append("")
        if "step" in runs:
            lines += [f"## Step ({tag}, {runs.get('device', '?')})", "",
                      "| leg | variant | micro-batches | ms / step (min .. max) | frames / s | vs first variant | peak over a step, GB | byte model, GB |",
                      "|---|---|---|---|---|---|---|---|"]
            for leg, r in runs["step"].items():
                first = next(iter(r["variants"].values()))["ms"]
                for k, v in r["variants"].items():
                    lines.append(f"| {leg} | {k} | {v['micro_batches']} | {v['ms']:.2f} ({v['ms_min']:.2f} .. {v['ms_max']:.2f}) | {v['frames_per_s']:.0f} | "
                                 f"{v['ms'] / first:.3f} | {v['peak_step_bytes'] / 1e9:.3f} | {v['model_saved_bytes'] / 1e9:.3f} |")
            lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--arenas", default="ViT-B/32,ViT-L/14,TFAM-768")
    k.add_argument("--inner", type=int, default=20)
    k.add_argument("--rounds", type=int, default=7)
    s = sub.add_parser("step")
    s.add_argument("--model", default="ViT-B/32")
    s.add_argument("--clips", type=int, default=32)
    s.add_argument("--frames", type=int, default=16)
    s.add_argument("--variants", default="1:none,4:none")
    s.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    s.add_argument("--steps", type=int, default=3)
    s.add_argument("--warmup", type=int, default=2)
    s.add_argument("--windows", type=int, default=5)
    for p in (k, s):
        p.add_argument("--tag", default="this")
        p.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grad_accum_bench: no GPU; nothing is measured without one")
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "grad_accum.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    run = doc.setdefault(args.tag, {})
    run["device"] = torch.cuda.get_device_name(0)
    if args.cmd == "kernel":
        for name in args.arenas.split(","):
            run.setdefault("kernel", {})[name] = kernel_leg(name, args.inner, args.rounds)
    else:
        run.setdefault("step", {})[f"{args.model} {args.clips}x{args.frames} {args.dtype}"] = step_leg(args)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=False)
    md = os.path.join(args.out_dir, "grad_accum.md")
    notes = ""
    if os.path.exists(md):
        with open(md) as f:
            text = f.read()
        notes = text[text.index("## Notes"):] if "## Notes" in text else ""
    with open(md, "w") as f:
        f.write(render(doc) + "\n" + notes)


if __name__ == "__main__":
    main()
