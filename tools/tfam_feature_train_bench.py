#!/usr/bin/env python3
"""TFAM feature-concatenation mode (``use_cross_attention = False``, ``concat_dim = -1``): the training step on the per-op path
(``off``: AMO_CLIP.fused_feature_training = False, what the mode has always run) against the fused chains with projection_layer
inside them (``on``).

Workload: 8 heads, 4 layers, ff 2048, 140 classes, B = 8 clips, dropout 0.1 / 0.1, d_model 512 and 768.  The step is
tick + forward + BCE + backward + AdamW on device-resident step state (what a captured step needs), measured three ways:
  fixed/captured   T_rgb = 16, T_motion = 15 (the reference batch): one GraphedTrainStep graph, device events around ``--steps``
                   back-to-back replays
  fixed/eager      the same step without a graph (max_graphs = 0): launch-bound host time is part of it; host clock around a
                   device synchronise
  bucketed         ``--batches`` ragged batches, T_rgb ~ U{9..32}, through GraphedTrainStep(bucket=32, concat="feature"): two passes,
                   the second (every graph captured) timed per batch on the host clock around a device synchronise
Both configurations run in ONE process, alternating (off, on, off, on, ...), ``--repeats`` times each with a fresh model.  The
run-to-run spread of ``off`` is the yardstick: ``on`` wins when its slowest run beats the fastest ``off`` run by more than that.

    python tools/tfam_feature_train_bench.py [--dmodels 512,768] [--steps 300] [--batches 60] [--repeats 3] [--out result.json]
    rocprofv3 --kernel-trace --stats -- python tools/tfam_feature_train_bench.py --kernel-only [--dmodels 512]
        # per-kernel times of the chain's launches (F0 is the tf_gemm_kernel with template arguments 16, 0, 2, 1024 / 1536;
        # the grouped weight gradient is tr_wgrad_group_kernel), switch on only, eager steps
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vimo_clip_amd import autograd_ops as ag  # noqa: E402
from vimo_clip_amd import synth  # noqa: E402
from vimo_clip_amd.graphs import GraphedTrainStep, pad_concat_to_bucket  # noqa: E402
from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad  # noqa: E402
from vimo_clip_amd.optim import FusedAdam, GradArena  # noqa: E402
from vimo_clip_amd.TFAM.models import AMO_CLIP  # noqa: E402

H, L, FF, C, B, BUCKET = 8, 4, 2048, 140, 8, 32
TMIN, TMAX = 9, 32
DEV = "cuda"


def fixed_batch(D):
    Tr, Tf = 16, 15
    lens = synth.randint(301, "feature/fixed/lens", (B,), 5, Tr + 1)
    lens[0] = Tr
    mr = (torch.arange(Tr).unsqueeze(0) < lens.unsqueeze(1)).to(DEV)
    mf = (torch.arange(Tf).unsqueeze(0) < torch.clamp(lens - 1, min=1).unsqueeze(1)).to(DEV)
    rgb = synth.normal(302, "feature/fixed/rgb", (B, Tr, D)).to(DEV) * mr.unsqueeze(-1)
    mot = synth.normal(303, "feature/fixed/motion", (B, Tf, D)).to(DEV) * mf.unsqueeze(-1)
    y = synth.multi_hot_labels(304, "feature/fixed/labels", B, C).to(DEV)
    return rgb.contiguous(), mot.contiguous(), mr, mf, y


def ragged_batches(D, n):
    lens = synth.randint(311, "feature/ragged/lens", (n, B), TMIN, TMAX + 1)
    pool_r = synth.normal(312, "feature/ragged/rgb", (B, TMAX + n, D)).to(DEV)
    pool_m = synth.normal(313, "feature/ragged/motion", (B, TMAX + n, D)).to(DEV)
    labels = synth.multi_hot_labels(314, "feature/ragged/labels", n * B, C).view(n, B, C).to(DEV)
    out = []
    for i in range(n):
        lr = lens[i]
        Tr, Tf = int(lr.max()), int(lr.max()) - 1
        mr = (torch.arange(Tr).unsqueeze(0) < lr.unsqueeze(1)).to(DEV)
        mf = (torch.arange(Tf).unsqueeze(0) < (lr - 1).unsqueeze(1)).to(DEV)
        out.append(((pool_r[:, i:i + Tr] * mr.unsqueeze(-1)).contiguous(), (pool_m[:, i:i + Tf] * mf.unsqueeze(-1)).contiguous(), mr, mf,
                    labels[i].contiguous()))
    return out


def new_step(D, switch):
    ag.weights.clear()
    torch.cuda.empty_cache()
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, use_cross_attention=False, concat_dim=-1, dropout=0.1,
                 mlp_dropout=0.1, device=DEV).to(DEV)
    m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 4), strict=True)
    m.train()
    m.fused_feature_training = switch
    opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-4, weight_decay=0.1, decoupled=True)
    opt.enable_device_state(base_seed=0)
    m.use_device_seeds(opt)

    def dev_step(rgb, mot, mr, mf, y, n_rgb=None, n_mot=None, T_out=None):
        opt.tick()
        kw = {} if n_rgb is None else {"token_lens": (n_rgb, n_mot), "concat_len": T_out}
        out = m(rgb, mot, mask_rgb=mr, mask_flow=mf, **kw)
        loss, dl = loss_and_grad(bce_with_logits_loss, out, y)
        out.backward(dl)
        opt.step()
        return loss, out.detach()
    return m, opt, dev_step


def bench_fixed(D, switch, steps, captured):
    _, opt, dev_step = new_step(D, switch)
    g = GraphedTrainStep(dev_step, opt, bucket=1, pooled=None, max_graphs=16 if captured else 0)
    batch = fixed_batch(D)
    for _ in range(20):
        loss = g(*batch)[0]
    torch.cuda.synchronize()
    if captured:                                       # a replay is device work only: events around back-to-back replays
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            loss = g(*batch)[0]
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
    else:
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = g(*batch)[0]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
    return {"ms_per_step": ms, "graphs": g.n_graphs, "final_loss": float(loss)}


def bench_bucketed(D, switch, batches):
    _, opt, dev_step = new_step(D, switch)
    g = GraphedTrainStep(dev_step, opt, bucket=BUCKET, pooled=None, concat="feature")
    passes = []
    for _ in range(2):
        ts = []
        for b in batches:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g(*b)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        passes.append(ts)
    return {"first_pass_mean_ms": sum(passes[0]) / len(passes[0]), "steady_median_ms": statistics.median(passes[1]),
            "steady_mean_ms": sum(passes[1]) / len(passes[1]), "graphs": g.n_graphs}


def verdict(entry, key):
    off, on = ([r[key] for r in entry[k]] for k in ("off", "on"))
    spread = max(off) - min(off)
    margin = min(off) - max(on)
    return {"off_ms": off, "on_ms": on, "off_spread_ms": spread, "margin_ms": margin, "on_beats_off_by_more_than_off_spread": margin > spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dmodels", default="512,768")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="eager fused steps only (switch on), for rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tfam_feature_train_bench: needs the GPU (there is no CPU timing)")
    dmodels = [int(x) for x in a.dmodels.split(",")]
    if a.kernel_only:
        for D in dmodels:
            print(json.dumps({"d_model": D, **bench_fixed(D, True, 50, False)}))
        return
    result = {"workload": dict(nhead=H, layers=L, ff=FF, classes=C, batch=B, dropout=0.1, concat_dim=-1, fixed=dict(T_rgb=16, T_motion=15),
                               bucketed=dict(T_rgb_range=(TMIN, TMAX), graph_bucket=BUCKET, batches=a.batches), steps=a.steps, repeats=a.repeats),
              "d_model": {}}
    for D in dmodels:
        batches = ragged_batches(D, a.batches)
        shapes = sorted({(o[0].shape[1], o[1].shape[1]) for o in (pad_concat_to_bucket(*b[:4], BUCKET, "feature") for b in batches)})
        runs = {k: {"off": [], "on": []} for k in ("captured", "eager", "bucketed")}
        for rep in range(a.repeats):
            for config in ("off", "on"):                   # alternating, in one process
                sw = config == "on"
                cap = bench_fixed(D, sw, a.steps, True)
                eag = bench_fixed(D, sw, a.steps, False)
                buc = bench_bucketed(D, sw, batches)
                runs["captured"][config].append(cap)
                runs["eager"][config].append(eag)
                runs["bucketed"][config].append(buc)
                print(f"d{D} run {rep} {config:3s}: captured {cap['ms_per_step']:.4f} ms/step  eager {eag['ms_per_step']:.4f} ms/step  "
                      f"bucketed steady median {buc['steady_median_ms']:.4f} ms (first pass mean {buc['first_pass_mean_ms']:.3f}, "
                      f"{buc['graphs']} graphs)", flush=True)
        entry = {"padded_shapes": shapes, "runs": runs,
                 "captured": verdict(runs["captured"], "ms_per_step"), "eager": verdict(runs["eager"], "ms_per_step"),
                 "bucketed": verdict(runs["bucketed"], "steady_median_ms")}
        for k in ("captured", "eager", "bucketed"):
            v = entry[k]
            print(f"d{D} {k:9s} off {min(v['off_ms']):.4f}..{max(v['off_ms']):.4f} ms  on {min(v['on_ms']):.4f}..{max(v['on_ms']):.4f} ms  "
                  f"margin {v['margin_ms']:.4f} ms (off spread {v['off_spread_ms']:.4f})  wins {v['on_beats_off_by_more_than_off_spread']}", flush=True)
        result["d_model"][str(D)] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
