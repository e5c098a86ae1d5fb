#!/usr/bin/env python3
"""TFAM training step with token tensors that REQUIRE GRAD (an adapter in front of TFAM, learned tokens, saliency): the fused chains
returning d rgb / d motion (``on``: AMO_CLIP.fused_input_grads = True) against the per-op path such a step has always taken (``off``),
and the unchanged step with detached tokens (``detached``: the chains, switch on), which must not pay for the new code.

Workload: 8 heads, 4 layers, ff 2048, 140 classes, B = 8 clips, T = 16 / 15, dropout 0.1 / 0.1, bf16, d_model 512 and 768; the modes
cross attention, token concatenation (concat 1) and feature concatenation (concat -1, with fused_feature_training).  The step is
tick + forward + BCE + backward + AdamW on device-resident step state; the token leaves are made inside the step, and their gradients
land in ``.grad`` as an adapter's backward would read them.  Measured two ways:
  captured   one GraphedTrainStep graph, device events around ``--steps`` back-to-back replays
  eager      the same step without a graph (max_graphs = 0), host clock around a device synchronise
Every configuration runs ``--repeats`` times, alternating, each run with a fresh model; the figure of a run is the median over
``--chunks`` chunks of ``--steps / --chunks`` steps.  ``--root DIR`` imports the package from another checkout (the parent commit,
built): there the attribute does nothing and ``on`` is the per-op path, which is how the parent's figures are taken in the same GPU
call.

    python tools/tfam_input_grad_bench.py [--dmodels 512,768] [--modes cross,concat1,concat-1] [--configs off,on,detached]
                                        [--steps 200] [--repeats 2] [--out r.json]
    rocprofv3 --kernel-trace --stats -- python tools/tfam_input_grad_bench.py --kernel-only [--modes cross] [--dmodels 512]
        # the launch census of the fused step (switch on, grad-requiring tokens, eager)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--dmodels", default="512,768")
ap.add_argument("--modes", default="cross,concat1,concat-1")
ap.add_argument("--configs", default="off,on,detached")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--chunks", type=int, default=5)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="eager fused steps only (switch on), for rocprofv3 --kernel-trace --stats")
ARGS = ap.parse_args()

sys.path.insert(0, os.path.abspath(ARGS.root))
from vimo_clip_amd import autograd_ops as ag  # noqa: E402
from vimo_clip_amd import synth  # noqa: E402
from vimo_clip_amd.graphs import GraphedTrainStep  # noqa: E402
from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad  # noqa: E402
from vimo_clip_amd.optim import FusedAdam, GradArena  # noqa: E402
from vimo_clip_amd.TFAM.models import AMO_CLIP  # noqa: E402

H, L, FF, C, B, TR, TF = 8, 4, 2048, 140, 8, 16, 15
DEV = "cuda"
MODE_KW = {"cross": dict(use_cross_attention=True), "concat1": dict(use_cross_attention=False, concat_dim=1),
           "concat-1": dict(use_cross_attention=False, concat_dim=-1)}
CONFIGS = tuple(ARGS.configs.split(","))


def batch(D):
    lens = synth.randint(401, "inputs/lens", (B,), 5, TR + 1)
    lens[0] = TR
    mr = (torch.arange(TR).unsqueeze(0) < lens.unsqueeze(1)).to(DEV)
    mf = (torch.arange(TF).unsqueeze(0) < torch.clamp(lens - 1, min=1).unsqueeze(1)).to(DEV)
    rgb = synth.normal(402, "inputs/rgb", (B, TR, D)).to(DEV) * mr.unsqueeze(-1)
    mot = synth.normal(403, "inputs/motion", (B, TF, D)).to(DEV) * mf.unsqueeze(-1)
    y = synth.multi_hot_labels(404, "inputs/labels", B, C).to(DEV)
    return rgb.contiguous(), mot.contiguous(), mr, mf, y


def new_step(D, mode, config, seen):
    ag.weights.clear()
    torch.cuda.empty_cache()
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, dropout=0.1, mlp_dropout=0.1, device=DEV,
                 **MODE_KW[mode]).to(DEV)
    m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 4), strict=True)
    m.train()
    m.fused_feature_training = True
    m.fused_input_grads = config != "off"
    opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-4, weight_decay=0.1, decoupled=True)
    opt.enable_device_state(base_seed=0)
    m.use_device_seeds(opt)
    grads = config != "detached"

    def dev_step(rgb, mot, mr, mf, y):
        opt.tick()
        if grads:
            rgb, mot = rgb.detach().requires_grad_(), mot.detach().requires_grad_()
        out = m(rgb, mot, mask_rgb=mr, mask_flow=mf)
        seen["node"] = type(out.grad_fn).__name__
        loss, dl = loss_and_grad(bce_with_logits_loss, out, y)
        out.backward(dl)
        seen["input_grads"] = grads and rgb.grad is not None and mot.grad is not None
        opt.step()
        return loss, out.detach()
    return opt, dev_step


def bench(D, mode, config, steps, chunks, captured):
    seen = {}
    opt, dev_step = new_step(D, mode, config, seen)
    g = GraphedTrainStep(dev_step, opt, bucket=1, pooled=None, max_graphs=16 if captured else 0)
    b = batch(D)
    for _ in range(20):
        loss = g(*b)[0]
    torch.cuda.synchronize()
    per = max(1, steps // chunks)
    ms = []
    for _ in range(chunks):
        if captured:                                       # a replay is device work only: events around back-to-back replays
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                loss = g(*b)[0]
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / per)
        else:
            t0 = time.perf_counter()
            for _ in range(per):
                loss = g(*b)[0]
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / per)
    return {"ms_per_step": statistics.median(ms), "chunks_ms": ms, "fused": seen.get("node") == "TfamTrainFnBackward",
            "input_grads": bool(seen.get("input_grads")), "final_loss": float(loss)}


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("tfam_input_grad_bench: needs the GPU (there is no CPU timing)")
    dmodels = [int(x) for x in a.dmodels.split(",")]
    modes = a.modes.split(",")
    if a.kernel_only:
        for mode in modes:
            for D in dmodels:
                print(json.dumps({"mode": mode, "d_model": D, **bench(D, mode, "on", 50, 1, False)}))
        return
    result = {"label": a.label, "workload": dict(nhead=H, layers=L, ff=FF, classes=C, batch=B, dropout=0.1, T_rgb=TR, T_motion=TF,
                                                 steps=a.steps, chunks=a.chunks, repeats=a.repeats), "runs": {}}
    for mode in modes:
        for D in dmodels:
            runs = {k: {c: [] for c in CONFIGS} for k in ("captured", "eager")}
            for rep in range(a.repeats):
                for config in CONFIGS:                     # alternating, in one process
                    for kind in ("captured", "eager"):
                        r = bench(D, mode, config, a.steps, a.chunks, kind == "captured")
                        runs[kind][config].append(r)
                        print(f"{a.label} {mode} d{D} run {rep} {config:8s} {kind:8s} {r['ms_per_step']:.4f} ms/step  fused {r['fused']}  "
                              f"input grads {r['input_grads']}", flush=True)
            result["runs"][f"{mode}/d{D}"] = runs
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
