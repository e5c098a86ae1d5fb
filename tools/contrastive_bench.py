#!/usr/bin/env python3
"""Contrastive distillation mode (losses.distillation_loss(mode="contrastive")): the loss chain launch by launch, the student step with
``cosine`` against ``contrastive``, and the gradient error of the 16-bit chain against the unrounded float64 model.

Chain legs (``--chains``, MxE): every entry point of the chain -- vmc_contrastive_prep, the logits GEMM, vmc_contrastive_softmax, the
gradient GEMM, vmc_contrastive_norm_bwd -- in windows of ``--reps`` back-to-back calls between two HIP events, the windows alternating
between the entry points, and the whole ``distillation_loss`` forward (gradient included) the same way.  The operands of these shapes
are a few MB and stay in the caches between calls: the GB/s figures are the bytes an entry point must move (inputs once, outputs once)
over its time, not HBM traffic.

Step legs (``--legs``): the step of bench.py's student leg (forward, distillation + BCE, backward into a GradArena, fused Adam) per
distillation mode; the models of a leg are resident and the timed windows alternate between them.  ``--tree PATH --modes cosine --tag
NAME`` imports the package from another checkout and stores its leg as ``cosine@NAME``: an older commit measured the same way.

Accuracy (``--accuracy BxTxE``): max |ds - ds64| / max |ds64| of the bf16 and f16 chains against tests/contrastive_refs.loss_exact
without any rounding, beside the same figure of the float64 model with both roundings (what the definition itself costs).

python tools/contrastive_bench.py [--chains 480x512,928x512,480x768,4096x512] [--legs ViT-B/32:32x16] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.07


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def summary(ms):
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def chain_leg(M, E, dtype, reps, windows):
    from vimo_clip_amd import ops
    from vimo_clip_amd._lib import check, dt, lib, ptr, stream
    from vimo_clip_amd.losses import distillation_loss
    T = 29 if M % 29 == 0 else (15 if M % 15 == 0 else 16)
    Mp = (M + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(M + E)
    t = torch.randn(M, E, device="cuda", generator=g)
    s = 0.5 * t + torch.randn(M, E, device="cuda", generator=g)
    u16, v16 = torch.empty(Mp, E, dtype=dtype, device="cuda"), torch.empty(Mp, E, dtype=dtype, device="cuda")
    vt16, dz16 = torch.empty(E, Mp, dtype=dtype, device="cuda"), torch.empty(M, Mp, dtype=dtype, device="cuda")
    z, du, ds = torch.empty(M, Mp, device="cuda"), torch.empty(M, E, device="cuda"), torch.empty(M, E, device="cuda")
    inv, lr, lc = (torch.empty(M, device="cuda") for _ in range(3))
    loss, top1 = torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    nb = lib.vmc_contrastive_partials_bytes(M)
    part = torch.empty(nb, dtype=torch.uint8, device="cuda")
    d16 = dt(dtype)
    sg = s.clone().requires_grad_(True)
    calls = {
        "vmc_contrastive_prep": (8 * M * E + 6 * Mp * E + 4 * M, 2,
                                 lambda: check(lib.vmc_contrastive_prep(ptr(s), ptr(t), ptr(u16), ptr(v16), ptr(vt16), ptr(inv), M, E, M, M * E, d16, stream()), "prep")),
        "logits GEMM (vmc_linear)": (2 * M * E + 2 * Mp * E + 4 * M * Mp, 1, lambda: ops.linear(u16[:M], v16, alpha=1.0 / TAU, out=z)),
        "vmc_contrastive_softmax": (4 * M * M + 2 * M * Mp + 8 * M, 4,
                                    lambda: check(lib.vmc_contrastive_softmax(ptr(z), M, Mp, T, ptr(lr), ptr(lc), ptr(loss), ptr(top1), ptr(dz16), d16,
                                                                              ptr(part), nb, stream()), "softmax")),
        "gradient GEMM (vmc_linear)": (2 * M * Mp + 2 * E * Mp + 4 * M * E, 1, lambda: ops.linear(dz16, vt16, alpha=0.5 / (M * TAU), out=du)),
        "vmc_contrastive_norm_bwd": (12 * M * E + 4 * M, 1, lambda: check(lib.vmc_contrastive_norm_bwd(ptr(du), ptr(s), ptr(inv), ptr(ds), M, E, stream()), "norm_bwd")),
        "distillation_loss, forward with gradient": (0, 9, lambda: distillation_loss(sg.view(M // T, T, E), t.view(M // T, T, E), mode="contrastive",
                                                                                     temperature=TAU, compute_dtype=dtype)),
    }
    for _, _, call in calls.values():                              # in chain order: every later call has real inputs
        call()
    torch.cuda.synchronize()
    e0, e1 = events()
    ms = {k: [] for k in calls}
    for _ in range(windows):
        for k, (_, _, call) in calls.items():
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    out = {"M": M, "E": E, "rows_per_clip": T, "workspace_bytes": lib.vmc_contrastive_workspace_bytes(M, E)}
    for k, (nbytes, launches, _) in calls.items():
        r = summary(ms[k])
        r.update(launches=launches, bytes=nbytes)
        if nbytes:
            r.update(gbps=nbytes / r["ms"] / 1e6)
        out[k] = r
        print(f"M {M} E {E}: {k}: {r['ms'] * 1e3:.1f} us ({r['ms_min'] * 1e3:.1f} .. {r['ms_max'] * 1e3:.1f}), {launches} launch(es)"
              + (f", {nbytes / 1e6:.2f} MB, {r['gbps']:.0f} GB/s" if nbytes else ""), flush=True)
    out["sum of the five entry points"] = {"ms": sum(out[k]["ms"] for k in list(calls)[:5])}
    return out


def build(name, clips, T, mode, dtype):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    R, _p, _D, _L, _H, E = synth.vit_geometry(name)
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=dtype).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=False)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=1e-4)
    vids = synth.randint_u8(3, "vids", (clips, T, 3, R, R)).cuda()
    teacher = synth.normal(3, "teacher", (clips, T + 1, E)).cuda()
    labels = synth.multi_hot_labels(3, "labels", clips, 140).cuda()
    kw = {"temperature": TAU, "compute_dtype": dtype} if mode == "contrastive" else {}

    def step():
        _emb, emb_d, logits = m(vids)
        loss = distillation_loss(emb_d, teacher[:, :-1, :], mode=mode, **kw) + classification_loss(logits, labels, positive_weight=9)
        loss.backward()
        opt.step()
    return step


def step_leg(name, clips, T, modes, dtype, steps, warmup, windows):
    legs = {mode: build(name, clips, T, mode, dtype) for mode in modes}
    for step in legs.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    e0, e1 = events()
    ms = {mode: [] for mode in modes}
    for _ in range(windows):
        for mode in modes:
            e0.record()
            for _ in range(steps):
                legs[mode]()
            e1.record()
            torch.cuda.synchronize()
            ms[mode].append(e0.elapsed_time(e1) / steps)
    return {mode: dict(summary(ms[mode]), frames_per_s=clips * T / statistics.median(ms[mode]) * 1e3) for mode in modes}


def accuracy(B, T, E):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import contrastive_refs as R
    from vimo_clip_amd.losses import distillation_loss
    t = R.randn((B * T, E), 9100)
    s = (0.5 * t + R.randn((B * T, E), 9200)).to(torch.float32)
    exact = R.loss_exact(s, t, T)
    top = exact["ds"].abs().max().item()
    out = {"shape": [B, T, E], "loss64": float(exact["loss"])}
    for name, d in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        sd = s.view(B, T, E).cuda().requires_grad_(True)
        loss = distillation_loss(sd, t.view(B, T, E).cuda(), mode="contrastive", temperature=R.TAU, compute_dtype=d)
        loss.backward()
        model = R.loss_exact(s, t, T, dtype16=d)
        out[name] = {"gpu": (sd.grad.cpu().view(B * T, E).double() - exact["ds"]).abs().max().item() / top,
                     "float64 model with both roundings": (model["ds"] - exact["ds"]).abs().max().item() / top,
                     "loss_gpu": float(loss), "loss_model": float(model["loss"])}
        print(f"accuracy {B}x{T}x{E} {name}: gpu {out[name]['gpu']:.2e}, float64 model with both roundings "
              f"{out[name]['float64 model with both roundings']:.2e} of max|ds64|", flush=True)
    return out


def write_md(doc, path):
    lines = ["# Contrastive distillation mode: the loss chain, the student step, the gradient error", "",
             "Written by tools/contrastive_bench.py on " + doc.get("device", "?") + " (one GPU, " + doc.get("dtype", "bf16") + ").  Every time is the "
             "median over alternating windows of back-to-back calls between two HIP events after warm-up, with the fastest and slowest window.", "",
             "The chain, entry point by entry point (operands stay in the caches between calls; MB = what the entry point must move, inputs "
             "and outputs once; GB/s = MB over the time):", "",
             "| M x E | entry point | launches | MB | us (min .. max) | GB/s |", "|---|---|---|---|---|---|"]
    for leg, ks in doc.get("chains", {}).items():
        for k, r in ks.items():
            if isinstance(r, dict) and "launches" in r:
                lines.append(f"| {leg} | {k} | {r['launches']} | " + (f"{r['bytes'] / 1e6:.2f}" if r["bytes"] else "-")
                             + f" | {r['ms'] * 1e3:.1f} ({r['ms_min'] * 1e3:.1f} .. {r['ms_max'] * 1e3:.1f}) | " + (f"{r['gbps']:.0f}" if "gbps" in r else "-") + " |")
        lines.append(f"| {leg} | sum of the five entry points | 9 | - | {ks['sum of the five entry points']['ms'] * 1e3:.1f} | - |")
    lines += ["", "Student step per distillation mode (`MODE@NAME`: the leg of another checkout, measured by the same tool):", "",
              "| leg | mode | ms / step (min .. max) | vs cosine | frames / s |", "|---|---|---|---|---|"]
    for leg, modes in doc.get("steps", {}).items():
        base = modes.get("cosine", {}).get("ms")
        for mode, r in sorted(modes.items()):
            lines.append(f"| {leg} | {mode} | {r['ms']:.2f} ({r['ms_min']:.2f} .. {r['ms_max']:.2f}) | " + (f"{r['ms'] / base:.4f}" if base else "-")
                         + f" | {r['frames_per_s']:.0f} |")
    acc = doc.get("accuracy")
    if acc:
        lines += ["", f"Gradient error against the unrounded float64 model at {acc['shape']}, max |ds - ds64| / max |ds64|:", "",
                  "| compute dtype | GPU chain | float64 model with both roundings |", "|---|---|---|"]
        lines += [f"| {d} | {acc[d]['gpu']:.2e} | {acc[d]['float64 model with both roundings']:.2e} |" for d in ("bf16", "f16") if d in acc]
    notes = ""
    if os.path.exists(path):                          # everything from "## Notes" on is kept as it is
        with open(path) as f:
            text = f.read()
        notes = text[text.index("## Notes"):] if "## Notes" in text else ""
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n\n" + notes)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--chains", default="480x512,928x512,480x768,4096x512")
    ap.add_argument("--legs", default="ViT-B/32:32x16")
    ap.add_argument("--modes", default="cosine,contrastive")
    ap.add_argument("--accuracy", default="32x29x512")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tree", default=HERE, help="import vimo_clip_amd from this checkout")
    ap.add_argument("--tag", default=None, help="store the step legs as MODE@TAG (with --tree: another commit's leg)")
    ap.add_argument("--out-dir", default=os.path.join(HERE, "profiles"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        sys.exit("contrastive_bench: no GPU; nothing is measured without one")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "contrastive.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(device=torch.cuda.get_device_name(0), dtype=args.dtype, temperature=TAU)
    for chain in [c for c in args.chains.split(",") if c]:
        M, E = (int(v) for v in chain.split("x"))
        doc.setdefault("chains", {})[f"{M} x {E}"] = chain_leg(M, E, dtype, args.reps, args.windows)
    for leg in [s for s in args.legs.split(",") if s]:
        name, shape = leg.rsplit(":", 1)
        clips, T = (int(v) for v in shape.split("x"))
        for mode, r in step_leg(name, clips, T, args.modes.split(","), dtype, args.steps, args.warmup, args.windows).items():
            key = mode if args.tag is None else f"{mode}@{args.tag}"
            doc.setdefault("steps", {}).setdefault(f"{name} {clips}x{T}", {})[key] = r
            print(f"{name} {clips}x{T} {key}: {r['ms']:.2f} ms/step ({r['ms_min']:.2f} .. {r['ms_max']:.2f})", flush=True)
        from vimo_clip_amd import autograd_ops
        autograd_ops.weights.clear()
        torch.cuda.empty_cache()
    if args.accuracy:
        doc["accuracy"] = accuracy(*(int(v) for v in args.accuracy.split("x")))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    write_md(doc, os.path.join(args.out_dir, "contrastive.md"))


if __name__ == "__main__":
    main()
