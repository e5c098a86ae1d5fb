#!/usr/bin/env python3
"""Dynamic loss scaling on the device (FusedAdam.enable_loss_scaling / vmc_loss_scale_check): what it costs and what it buys.

  step    The student's ViT-B/32 step (8 clips x 16 frames, device-state mode, eager: tick + forward + cosine distillation + BCE +
          backward + fused Adam) and the TFAM step at d_model 768, B = 8, 16 tokens (one captured graph, GraphedTrainStep), in the
          variants off / on / off+clip / on+clip (clip: max_grad_norm 1.0).  The variants ALTERNATE window by window; a window times
          `--steps` steps between two HIP events; the median over `--windows` windows is reported with the fastest and the slowest.
          `--root DIR` imports the package of another checkout (one that has no loss scaling runs the off variants only): run this
          tree and the parent alternately in ONE session and compare the off variants -- their spread between invocations of the
          same tree is the yardstick for "equal".
  kernel  vmc_loss_scale_check and vmc_grad_clip_dev over flat gradients of the two arenas' sizes (88.5 M and 31.9 M elements): the
          check's own time, its rate over the 4 B / element it reads and the fraction of `--hbm-tbs` (default 8.0 TB/s, the MI355X
          HBM3E peak) that is.  Same alternation.
  grads   The set-up of tests/test_gpu_loss_scale.py item 4 (ViT-tiny/32, 4 clips x 5 frames, loss x 2^-12, every gradient against
          torch autograd through the fp32 CPU oracle): per transformer block (and for the stem and the heads) the worst max-error /
          max-reference over the group's parameters and its relative L2 error, for f16 unscaled, f16 with dynamic scaling, bf16.

Results are merged into <out-dir>/loss_scale.json under --tag; <out-dir>/loss_scale.md is rewritten from the JSON, and everything from
"## Notes" on is kept as it is.

python tools/loss_scale_bench.py step [--root DIR] --tag this_1
python tools/loss_scale_bench.py kernel
python tools/loss_scale_bench.py grads
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---- step ---------------------------------------------------------------------------------------------------------------------------
def _student_variant(scaling, clip):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    name, clips, T = "ViT-B/32", 8, 16
    R, p, D, L, H, E = synth.vit_geometry(name)
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=torch.bfloat16).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=True)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=1e-4).enable_device_state()
    if scaling:
        opt.enable_loss_scaling()
    vids, teacher = synth.randint_u8(3, "vids", (clips, T, 3, R, R)).cuda(), synth.normal(3, "teacher", (clips, T + 1, E)).cuda()
    labels = synth.multi_hot_labels(3, "labels", clips, 140).cuda()

    def step():
        opt.tick()
        emb, emb_d, logits = m(vids)
        loss = distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)
        (opt.scale_loss(loss) if scaling else loss).backward()
        opt.step(max_grad_norm=clip)
    return step, (m, arena, opt), arena.numel


def _tfam_variant(scaling, clip):
    from vimo_clip_amd import synth
    from vimo_clip_amd.graphs import GraphedTrainStep
    from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad
    from vimo_clip_amd.optim import FusedAdam, GradArena
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    D, B, T = 768, 8, 16
    m = AMO_CLIP(d_model=D, nhead=8, num_layers=4, dim_feedforward=2048, num_classes=140, dropout=0.1, mlp_dropout=0.1, device="cuda").cuda().train()
    m.load_state_dict(synth.tfam_state_dict(D, 8, 4, 2048, 140, 4), strict=True)
    arena = GradArena(m.used_parameters())
    opt = FusedAdam(arena, lr=1e-4, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=0)
    if scaling:
        opt.enable_loss_scaling()
    m.use_device_seeds(opt)
    rgb, mot = synth.normal(30, "rgb", (B, T, D)).cuda(), synth.normal(30, "mot", (B, T, D)).cuda()
    mk = torch.ones(B, T, dtype=torch.bool, device="cuda")
    y = synth.multi_hot_labels(30, "lab", B, 140).cuda()

    def step(a, b, c, d, yy):
        opt.tick()
        out = m(a, b, mask_rgb=c, mask_flow=d)
        loss, dl = loss_and_grad(bce_with_logits_loss, out, yy)
        out.backward(opt.scale_grad(dl) if scaling else dl)
        opt.step(max_grad_norm=clip)
        return loss
    graphed = GraphedTrainStep(step, opt)
    return (lambda: graphed(rgb, mot, mk, mk, y)), (m, arena, opt, graphed), arena.numel


def step_legs(args):
    from vimo_clip_amd.optim import FusedAdam
    has = hasattr(FusedAdam, "enable_loss_scaling")
    specs = [("off", False, None), ("off+clip", False, 1.0)] + ([("on", True, None), ("on+clip", True, 1.0)] if has else [])
    out = {}
    for leg, make, steps in (("student ViT-B/32 8x16 bf16 (eager, device state)", _student_variant, args.steps),
                             ("TFAM d768 B8 T16 bf16 (captured)", _tfam_variant, args.steps * 20)):
        variants = {}
        for tag, scaling, clip in specs:
            fn, keep, n = make(scaling, clip)
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            variants[tag] = {"fn": fn, "keep": keep, "ms": []}
        for _ in range(args.windows):
            for v in variants.values():
                v["ms"].append(_events_ms(v["fn"], steps))
        out[leg] = {"elements": n, "steps_per_window": steps, "variants": {}}
        for tag, v in variants.items():
            s = _summary(v["ms"])
            opt = v["keep"][2]
            rec = {"ms": s["median"], "ms_min": s["min"], "ms_max": s["max"], "windows": s["n"]}
            if getattr(opt, "dev_ls", None) is not None:
                rec["loss_scale"], rec["skipped"] = float(opt.loss_scale.item()), int(opt.skipped_steps.item())
            out[leg]["variants"][tag] = rec
            print(f"{leg} {tag}: {s['median']:.4f} ms/step ({s['min']:.4f} .. {s['max']:.4f})", flush=True)
        del variants
        torch.cuda.empty_cache()
    return out


# ---- kernel -------------------------------------------------------------------------------------------------------------------------
def kernel_legs(args):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    from vimo_clip_amd.optim import LossScaleStruct
    out = {}
    for name, n in (("ViT-B/32 arena", 88541888), ("TFAM-768 arena", 31862336)):
        g = torch.empty(n, device="cuda").normal_(generator=torch.Generator(device="cuda").manual_seed(1)).mul_(1e-3)
        rec = torch.frombuffer(bytearray(bytes(LossScaleStruct(65536.0, 2.0, 0.5, 1.0, 2000, 0, 0, 0))), dtype=torch.int32).clone().cuda()
        hyper, clip = torch.zeros(4, device="cuda"), torch.tensor([1.0, 1.0, 0.0, 0.0], device="cuda")
        state = torch.zeros(4, dtype=torch.int64, device="cuda")
        ws = torch.empty(int(lib.vmc_loss_scale_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        ws2 = torch.empty(int(lib.vmc_grad_clip_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        variants = {
            "loss_scale_check": lambda: check(lib.vmc_loss_scale_check(ptr(g), n, ptr(rec), ptr(hyper), None, ptr(state), ptr(ws), ws.numel(), stream()), "check"),
            "loss_scale_check+clip": lambda: check(lib.vmc_loss_scale_check(ptr(g), n, ptr(rec), ptr(hyper), ptr(clip), ptr(state), ptr(ws), ws.numel(), stream()), "check"),
            "grad_clip_dev": lambda: check(lib.vmc_grad_clip_dev(ptr(g), n, ptr(hyper), ptr(clip), ptr(ws2), ws2.numel(), stream()), "clip"),
        }
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(_events_ms(fn, args.inner))
        out[name] = {"elements": n, "bytes": 4 * n, "inner": args.inner, "variants": {}}
        for k in variants:
            s = _summary(ms[k])
            tbs = 4 * n / (s["median"] * 1e-3) / 1e12
            out[name]["variants"][k] = {"us": s["median"] * 1e3, "us_min": s["min"] * 1e3, "us_max": s["max"] * 1e3, "TB_per_s": tbs,
                                        "fraction_of_hbm_peak": tbs / args.hbm_tbs}
            print(f"{name} {k}: {s['median'] * 1e3:.1f} us ({s['min'] * 1e3:.1f} .. {s['max'] * 1e3:.1f}), {tbs:.2f} TB/s", flush=True)
        assert int(rec[7]) == 0 and int(rec[6]) == 0
    return out


# ---- gradient accuracy --------------------------------------------------------------------------------------------------------------
def grad_legs(args):
    from oracle import student as ostudent
    from vimo_clip_amd import autograd_ops, synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    name, B, T, weight = "ViT-tiny/32", 4, 5, 2.0 ** -12
    R, p, D, L, H, E = synth.vit_geometry(name)
    sd = synth.student_state_dict(name, 71)
    vids, teacher = synth.randint_u8(71, "vids", (B, T, 3, R, R)), synth.normal(71, "teacher", (B, T + 1, E))
    labels = synth.multi_hot_labels(71, "labels", B, 140)
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    _, oe_d, ol = ostudent.student_forward(sdo, vids, H, alpha=0.1, wrap_quirk=True)
    ((ostudent.distillation_loss(oe_d, teacher[:, :-1, :], "cosine") + ostudent.classification_loss(ol, labels, 9)) * weight).backward()

    def group(k):
        if ".resblocks." in k:
            return "block " + k.split(".resblocks.")[1].split(".")[0]
        return "stem" if k.startswith("visual_encoder.") and ".ln_post" not in k and not k.endswith(".proj") else "heads"
    out = {}
    for tag, dtype, scaling in (("f16 unscaled", torch.float16, False), ("f16 scaled", torch.float16, True), ("bf16 unscaled", torch.bfloat16, False)):
        autograd_ops.weights.clear()
        m = FlowStudentModel(name, device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype).train()
        m.load_state_dict(sd, strict=True)
        arena = GradArena(m.parameters())
        opt = FusedAdam(arena, lr=0.0).enable_device_state()
        if scaling:
            opt.enable_loss_scaling()
        for attempt in range(8):
            S = float(opt.loss_scale.item()) if scaling else 1.0
            opt.tick()
            _, emb_d, logits = m(vids.cuda())
            loss = (distillation_loss(emb_d, teacher.cuda()[:, :-1, :], mode="cosine") + classification_loss(logits, labels.cuda(), positive_weight=9)) * weight
            opt.scale_loss(loss).backward()
            opt.step()
            if not scaling or opt.last_found_inf.item() == 0:
                break
        groups = {}
        for k, p_ in m.named_parameters():
            got, ref = p_.grad.cpu().double() / S, sdo[k].grad.double()
            r = groups.setdefault(group(k), {"max_rel": 0.0, "num": 0.0, "den": 0.0, "zeros": 0, "n": 0})
            r["max_rel"] = max(r["max_rel"], ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item())
            r["num"] += float((got - ref).pow(2).sum())
            r["den"] += float(ref.pow(2).sum())
            r["zeros"] += int(((got == 0) & (ref != 0)).sum())
            r["n"] += ref.numel()
        out[tag] = {"scale": S, "skipped": attempt if scaling else 0,
                    "groups": {g: {"max_rel": r["max_rel"], "rel_l2": (r["num"] / max(r["den"], 1e-300)) ** 0.5, "exact_zero_fraction": r["zeros"] / r["n"]}
                               for g, r in sorted(groups.items())}}
        for g, r in out[tag]["groups"].items():
            print(f"{tag} {g}: max-rel {r['max_rel']:.3e} rel-L2 {r['rel_l2']:.3e} zeros {r['exact_zero_fraction']:.3f}", flush=True)
    return out


# ---- output -------------------------------------------------------------------------------------------------------------------------
def render(doc):
    lines = ["# Dynamic loss scaling on the device", "", "Written by tools/loss_scale_bench.py on one GPU (see its docstring for the legs and how they are timed).", ""]
    steps = {tag: r["step"] for tag, r in sorted(doc.items()) if "step" in r}
    if steps:
        legs = sorted({leg for r in steps.values() for leg in r})
        lines += ["## Step", "", "| leg | run | variant | ms / step (min .. max) |", "|---|---|---|---|"]
        for leg in legs:
            for tag, r in steps.items():
                for k, v in r.get(leg, {}).get("variants", {}).items():
                    lines.append(f"| {leg} | {tag} | {k} | {v['ms']:.4f} ({v['ms_min']:.4f} .. {v['ms_max']:.4f}) |")
        lines.append("")
    for tag, r in sorted(doc.items()):
        if "kernel" in r:
            lines += [f"## Kernel ({tag}, {r.get('device', '?')})", "", "| gradient | elements | launch | us (min .. max) | TB/s over 4 B / element | of the HBM peak |",
                      "|---|---|---|---|---|---|"]
            for name, leg in r["kernel"].items():
                for k, v in leg["variants"].items():
                    lines.append(f"| {name} | {leg['elements']} | {k} | {v['us']:.1f} ({v['us_min']:.1f} .. {v['us_max']:.1f}) | {v['TB_per_s']:.2f} | "
                                 f"{v['fraction_of_hbm_peak']:.2f} |")
            lines.append("")
        if "grads" in r:
            tags = list(r["grads"])
            groups = list(next(iter(r["grads"].values()))["groups"])
            lines += [f"## Gradient error against the fp32 oracle, loss x 2^-12 ({tag})", "",
                      "max error / max reference over the group's parameters (relative L2 of the group; fraction of elements that are "
                      "exactly 0 where the reference is not)", "",
                      "| group | " + " | ".join(f"{t} (S = {r['grads'][t]['scale']:g})" for t in tags) + " |", "|---|" + "---|" * len(tags)]
            for g in groups:
                cells = [r["grads"][t]["groups"][g] for t in tags]
                lines.append(f"| {g} | " + " | ".join(f"{c['max_rel']:.2e} ({c['rel_l2']:.2e}; {c['exact_zero_fraction']:.3f})" for c in cells) + " |")
            lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("step")
    s.add_argument("--root", default=ROOT, help="checkout whose package is imported (default: this one)")
    s.add_argument("--steps", type=int, default=5)
    s.add_argument("--warmup", type=int, default=3)
    s.add_argument("--windows", type=int, default=7)
    k = sub.add_parser("kernel")
    k.add_argument("--inner", type=int, default=20)
    k.add_argument("--rounds", type=int, default=7)
    k.add_argument("--hbm-tbs", type=float, default=8.0)
    g = sub.add_parser("grads")
    for p in (s, k, g):
        p.add_argument("--tag", default="this")
        p.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(getattr(args, "root", ROOT)))
    if not torch.cuda.is_available():
        sys.exit("loss_scale_bench: no GPU; nothing is measured without one")
    import vimo_clip_amd
    print("package:", os.path.dirname(os.path.abspath(vimo_clip_amd.__file__)), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "loss_scale.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    run = doc.setdefault(args.tag, {})
    run["device"] = torch.cuda.get_device_name(0)
    run[args.cmd] = {"step": step_legs, "kernel": kernel_legs, "grads": grad_legs}[args.cmd](args)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=False)
    md = os.path.join(args.out_dir, "loss_scale.md")
    notes = ""
    if os.path.exists(md):
        with open(md) as f:
            text = f.read()
        notes = text[text.index("## Notes"):] if "## Notes" in text else ""
    with open(md, "w") as f:
        f.write(render(doc) + "\n" + notes)


if __name__ == "__main__":
    main()
