#!/usr/bin/env python3
"""TFAM token-concatenation mode on ragged clip batches: captured training steps at exact shapes (``off``: what
``use_graphs`` + ``graph_bucket = 32`` does for a concatenation model without ``graph_bucket_concat`` -- the bucket is ignored, 16 exact
shapes are captured and the rest of the list runs eagerly) against length-bucketed replay (``on``: graphs.pad_concat_to_bucket +
AMO_CLIP.forward(token_lens=), one graph per padded shape).

Workload: d_model 512, 8 heads, 4 layers, ff 2048, 140 classes, ``use_cross_attention = False``, ``concat_dim = 1``, B = 8 clips per
batch, dropout 0.1 / 0.1, N ragged batches from the counter-based generator (as tools/tfam_ragged_bench.py: every clip draws
T_rgb ~ U{tmin..tmax}, T_motion = T_rgb - 1, the batch zero-padded to its own maxima).  Lists: ``short`` U{9..32} (at most 62
concatenated tokens: T_out 32 or 64, within the fused chains' 64 tokens), ``long`` U{33..64} (64..126 concatenated tokens: the
per-op path) and, not in the default set, ``whole`` U{17..300} (whole videos: more exact shapes than the manager captures).

The step is tick + forward + BCE + backward + AdamW.  Both configurations run in ONE process, alternating (off, on, off, on, ...),
``--repeats`` times each with a fresh model; a run is two passes over the list, every batch timed on the host clock around a device
synchronise:
  first_pass_mean_ms   captures included (what a first epoch pays)
  steady_median_ms     second pass: every graph that will exist has been captured
The run-to-run spread of ``off`` (max - min of its steady medians) is the yardstick: ``on`` wins when its slowest run beats the
fastest ``off`` run by more than that spread.  The concatenation kernel alone (vmc_concat_tokens_len at B = 8, T_out = 64) is timed
with device events around back-to-back launches.

    python tools/tfam_concat_ragged_bench.py [--lists short,long] [--batches 100] [--repeats 3] [--out result.json]
    rocprofv3 --kernel-trace --stats -- python tools/tfam_concat_ragged_bench.py --kernel-only      # the kernel's own time
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
from vimo_clip_amd import ops, synth  # noqa: E402
from vimo_clip_amd.graphs import GraphedTrainStep, pad_concat_to_bucket  # noqa: E402
from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad  # noqa: E402
from vimo_clip_amd.optim import FusedAdam, GradArena  # noqa: E402
from vimo_clip_amd.TFAM.models import AMO_CLIP  # noqa: E402

D, H, L, FF, C, B, BUCKET = 512, 8, 4, 2048, 140, 8, 32
LISTS = {"short": (9, 32), "long": (33, 64), "whole": (17, 300)}
DEV = "cuda"


def make_batches(name, n):
    tmin, tmax = LISTS[name]
    lens = synth.randint(201, f"concat/{name}/lens", (n, B), tmin, tmax + 1)
    pool_r = synth.normal(202, f"concat/{name}/rgb", (B, tmax + n, D)).to(DEV)
    pool_m = synth.normal(203, f"concat/{name}/motion", (B, tmax + n, D)).to(DEV)
    labels = synth.multi_hot_labels(204, f"concat/{name}/labels", n * B, C).view(n, B, C).to(DEV)
    out = []
    for i in range(n):
        lr = lens[i]
        Tr, Tf = int(lr.max()), int(lr.max()) - 1
        mr = (torch.arange(Tr).unsqueeze(0) < lr.unsqueeze(1)).to(DEV)
        mf = (torch.arange(Tf).unsqueeze(0) < (lr - 1).unsqueeze(1)).to(DEV)
        out.append({"embeddings": (pool_r[:, i:i + Tr] * mr.unsqueeze(-1)).contiguous(),
                    "flow_embeddings": (pool_m[:, i:i + Tf] * mf.unsqueeze(-1)).contiguous(),
                    "mask_rgb": mr, "mask_flow": mf, "labels": labels[i].contiguous()})
    return out


def padded_shapes(batches):
    return {(o[0].shape[1], o[1].shape[1], o[6]) for o in
            (pad_concat_to_bucket(b["embeddings"], b["flow_embeddings"], b["mask_rgb"], b["mask_flow"], BUCKET, "time") for b in batches)}


def new_model():
    ag.weights.clear()
    torch.cuda.empty_cache()
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, use_cross_attention=False, concat_dim=1, dropout=0.1,
                 mlp_dropout=0.1, device=DEV).to(DEV)
    m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 4), strict=True)
    return m.train()


def timed_passes(fn, batches):
    passes = []
    for _ in range(2):
        ts = []
        for b in batches:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(b)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        passes.append(ts)
    return {"first_pass_mean_ms": sum(passes[0]) / len(passes[0]), "steady_median_ms": statistics.median(passes[1]),
            "steady_mean_ms": sum(passes[1]) / len(passes[1]), "steady_p90_ms": sorted(passes[1])[int(0.9 * len(passes[1]))]}


def bench_train(config, batches):
    m = new_model()
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
    # off: the trainer's arguments for a concatenation model without the switch (pooled_stream(model) is None: exact shapes)
    g = GraphedTrainStep(dev_step, opt, bucket=BUCKET, pooled=None, concat="time" if config == "on" else None)
    res = timed_passes(lambda b: g(b["embeddings"], b["flow_embeddings"], b["mask_rgb"], b["mask_flow"], b["labels"]), batches)
    res["graphs"] = g.n_graphs
    return res


def bench_kernel(launches=500):
    """vmc_concat_tokens_len alone at B = 8, 32 + 32 -> 64 rows of D floats: device events around back-to-back launches."""
    rgb, mot = synth.normal(7, "k_rgb", (B, 32, D)).to(DEV), synth.normal(7, "k_mot", (B, 32, D)).to(DEV)
    mr, mf = torch.ones(B, 32, dtype=torch.bool, device=DEV), torch.ones(B, 32, dtype=torch.bool, device=DEV)
    lens = [torch.tensor([v], dtype=torch.int32, device=DEV) for v in (27, 26)]
    out = ops.concat_tokens(rgb, mot, mr, mf, 64, *lens)
    for _ in range(20):
        ops.concat_tokens(rgb, mot, mr, mf, 64, *lens, out=out)
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            ops.concat_tokens(rgb, mot, mr, mf, 64, *lens, out=out)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / launches)
    return {"shape": dict(B=B, T_rgb=32, T_motion=32, T_out=64, D=D), "bytes_moved": 2 * B * 64 * D * 4, "launches_per_run": launches,
            "us_per_launch_back_to_back": runs, "us_per_launch_median": statistics.median(runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", default="short,long")
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="only the concatenation kernel's launches, for rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tfam_concat_ragged_bench: needs the GPU (there is no CPU timing)")
    if a.kernel_only:
        print(json.dumps(bench_kernel()))
        return
    result = {"workload": dict(d_model=D, nhead=H, layers=L, ff=FF, classes=C, batch=B, dropout=0.1, concat_dim=1, graph_bucket=BUCKET,
                               batches=a.batches, repeats=a.repeats), "lists": {}}
    for name in a.lists.split(","):
        batches = make_batches(name, a.batches)
        entry = {"T_rgb_range": LISTS[name], "distinct_exact_shapes": len({b["embeddings"].shape[1] for b in batches}),
                 "padded_shapes": sorted(padded_shapes(batches)), "off": [], "on": []}
        for rep in range(a.repeats):
            for config in ("off", "on"):                   # alternating, in one process
                r = bench_train(config, batches)
                entry[config].append(r)
                print(f"{name:5s} run {rep} {config:3s} steady median {r['steady_median_ms']:7.3f} ms  mean {r['steady_mean_ms']:7.3f}  "
                      f"p90 {r['steady_p90_ms']:7.3f}  first pass mean {r['first_pass_mean_ms']:7.3f} ms  graphs {r['graphs']:3d}", flush=True)
        off, on = ([r["steady_median_ms"] for r in entry[k]] for k in ("off", "on"))
        entry["off_spread_ms"] = max(off) - min(off)
        entry["margin_ms"] = min(off) - max(on)            # the fastest parent run against the slowest bucketed run
        entry["on_beats_off_by_more_than_off_spread"] = entry["margin_ms"] > entry["off_spread_ms"]
        print(f"{name:5s} off {min(off):.3f}..{max(off):.3f} ms (spread {entry['off_spread_ms']:.3f})  on {min(on):.3f}..{max(on):.3f} ms  "
              f"margin {entry['margin_ms']:.3f} ms  wins {entry['on_beats_off_by_more_than_off_spread']}", flush=True)
        result["lists"][name] = entry
    result["concat_kernel"] = bench_kernel()
    print(f"concat kernel: {result['concat_kernel']['us_per_launch_median']:.2f} us per launch (back to back, device events)", flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
