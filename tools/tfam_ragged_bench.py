#!/usr/bin/env python3
"""TFAM on ragged clip batches: eager vs hipGraph replay at exact shapes vs length-bucketed replay (graphs.pad_to_bucket).

Workload (SURVEY §8d cfg 5): d_model 768, 8 heads, 4 layers, ff 2048, 140 classes, cross-attention mode, B = 8 clips per batch,
dropout 0.1 / 0.1, N ragged batches from the counter-based generator (synth.py): every clip draws T_rgb ~ U{tmin..tmax},
T_motion = T_rgb - 1, and the batch is zero-padded to its own maxima as collate_fn_pad does.  Two lists: ``short`` U{17..64}
and ``long`` U{17..300} (whole videos: per-op path, tiled attention).

For the training step (tick + forward + BCE + backward + AdamW) and for the eval forward, per configuration -- ``eager``,
``graphs`` (use_graphs at exact shapes; the training manager goes eager after 16 shapes) and ``bucket8/16/32`` -- two passes
over the list, every batch timed on the host clock around a device synchronise:
  first_pass_mean_ms   captures included (what a first epoch pays)
  steady_median_ms     second pass: every graph that will exist has been captured
plus the graphs captured, the share of token rows that are bucket padding and the device memory the configuration left held / reserved.

    python tools/tfam_ragged_bench.py [--lists short,long] [--batches 200] [--out result.json] [--configs eager,graphs,bucket16]
    python tools/tfam_ragged_bench.py --trace-one train|eval      # one T = 16 step / forward x 20, for rocprofv3 --kernel-trace

Runs unchanged on a tree without ``bucket`` support (only ``eager`` and ``graphs`` are measured there).
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vimo_clip_amd import autograd_ops as ag  # noqa: E402
from vimo_clip_amd import synth  # noqa: E402
from vimo_clip_amd.graphs import GraphedTrainStep  # noqa: E402
from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad  # noqa: E402
from vimo_clip_amd.optim import FusedAdam, GradArena  # noqa: E402
from vimo_clip_amd.TFAM.models import AMO_CLIP  # noqa: E402
from vimo_clip_amd.TFAM.train_and_eval import Config, GraphedEvalForward  # noqa: E402

D, H, L, FF, C, B = 768, 8, 4, 2048, 140, 8
LISTS = {"short": (17, 64), "long": (17, 300)}
HAS_BUCKET = "bucket" in inspect.signature(GraphedTrainStep.__init__).parameters
DEV = "cuda"


def make_batches(name, n):
    """n collated batches, device resident.  Tokens: rows of one generated pool per stream (a clip is a window into it, shifted per
    batch), zeroed past the clip's length; lengths and labels from the counter-based generator."""
    tmin, tmax = LISTS[name]
    lens = synth.randint(101, f"ragged/{name}/lens", (n, B), tmin, tmax + 1)
    pool_r = synth.normal(102, f"ragged/{name}/rgb", (B, tmax + n, D)).to(DEV)
    pool_m = synth.normal(103, f"ragged/{name}/motion", (B, tmax + n, D)).to(DEV)
    labels = synth.multi_hot_labels(104, f"ragged/{name}/labels", n * B, C).view(n, B, C).to(DEV)
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


def padding_share(batches, bucket):
    rows = pad = 0
    for b in batches:
        for t in (b["embeddings"].shape[1], b["flow_embeddings"].shape[1]):
            tp = -(-t // bucket) * bucket
            rows, pad = rows + tp, pad + tp - t
    return pad / rows


def new_model(train):
    ag.weights.clear()
    torch.cuda.empty_cache()
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, dropout=0.1, mlp_dropout=0.1, device=DEV).to(DEV)
    m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 4), strict=True)
    return m.train() if train else m.eval()


def _mem():
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated(), torch.cuda.memory_reserved()


def _held(mem0):
    """Device memory a configuration left behind: live tensors (static graph inputs / outputs, scratch) and what the allocator
    reserved on top (the private pools of captured graphs stay reserved for them)."""
    a, r = _mem()
    return {"device_mib_held": (a - mem0[0]) / 2 ** 20, "device_mib_reserved": (r - mem0[1]) / 2 ** 20}


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
    m = new_model(True)
    opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-4, weight_decay=0.1, decoupled=True)
    mem0 = _mem()
    if config == "eager":            # the trainer's plain step (host scalars)
        def fn(b):
            out = m(b["embeddings"], b["flow_embeddings"], mask_rgb=b["mask_rgb"], mask_flow=b["mask_flow"])
            loss = bce_with_logits_loss(out, b["labels"])
            loss.backward()
            opt.step()
        res, graphs = timed_passes(fn, batches), 0
    else:
        opt.enable_device_state(base_seed=0)
        m.use_device_seeds(opt)

        def dev_step(rgb, mot, mr, mf, y, pool_len=None):
            opt.tick()
            kw = {} if pool_len is None else {"pool_len": pool_len}
            out = m(rgb, mot, mask_rgb=mr, mask_flow=mf, **kw)
            loss, dl = loss_and_grad(bce_with_logits_loss, out, y)
            out.backward(dl)
            opt.step()
            return loss, out.detach()
        g = GraphedTrainStep(dev_step, opt) if config == "graphs" else GraphedTrainStep(dev_step, opt, bucket=int(config[6:]))
        res = timed_passes(lambda b: g(b["embeddings"], b["flow_embeddings"], b["mask_rgb"], b["mask_flow"], b["labels"]), batches)
        graphs = len(g._graphs)
    res.update(graphs=graphs, **_held(mem0))
    return res


def bench_eval(config, batches):
    m = new_model(False)
    cfg = Config(device=DEV, batch_size=B, d_model=D)
    mem0 = _mem()
    with torch.no_grad():
        if config == "eager":
            res = timed_passes(lambda b: m(b["embeddings"], b["flow_embeddings"], mask_rgb=b["mask_rgb"], mask_flow=b["mask_flow"]), batches)
            graphs = 0
        else:
            gf = GraphedEvalForward(m, cfg, streams=1) if config == "graphs" else GraphedEvalForward(m, cfg, bucket=int(config[6:]), streams=1)
            res = timed_passes(gf, batches)
            graphs = len(gf._graphs)
    res.update(graphs=graphs, **_held(mem0))
    return res


def trace_one(what):
    """20 eager steps / forwards at the headline shape (B = 8, T = 16 / 15) for a kernel trace: the fused chains' launch counts."""
    rgb, mot = synth.normal(10, "rgb", (B, 16, D)).to(DEV), synth.normal(10, "mot", (B, 15, D)).to(DEV)
    mr, mf = torch.ones(B, 16, dtype=torch.bool, device=DEV), torch.ones(B, 15, dtype=torch.bool, device=DEV)
    y = synth.multi_hot_labels(10, "lab", B, C).to(DEV)
    m = new_model(what == "train")
    if what == "train":
        opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-4, weight_decay=0.1, decoupled=True)
        for _ in range(20):
            bce_with_logits_loss(m(rgb, mot, mask_rgb=mr, mask_flow=mf), y).backward()
            opt.step()
    else:
        with torch.no_grad():
            for _ in range(20):
                m(rgb, mot, mask_rgb=mr, mask_flow=mf)
    torch.cuda.synchronize()
    print("trace-one", what, "done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", default="short,long")
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--configs", default="eager,graphs,bucket8,bucket16,bucket32")
    ap.add_argument("--legs", default="train,eval")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-one", default=None, choices=["train", "eval"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tfam_ragged_bench: needs the GPU (there is no CPU timing)")
    if a.trace_one:
        return trace_one(a.trace_one)
    configs = [c for c in a.configs.split(",") if HAS_BUCKET or not c.startswith("bucket")]
    result = {"workload": dict(d_model=D, nhead=H, layers=L, ff=FF, classes=C, batch=B, dropout=0.1, batches=a.batches),
              "bucket_support": HAS_BUCKET, "lists": {}}
    for name in a.lists.split(","):
        batches = make_batches(name, a.batches)
        shapes = {(b["embeddings"].shape[1], b["flow_embeddings"].shape[1]) for b in batches}
        entry = {"T_rgb_range": LISTS[name], "distinct_exact_shapes": len(shapes),
                 "bucket_padding_share": {str(k): padding_share(batches, k) for k in (8, 16, 32)}}
        for leg in a.legs.split(","):
            entry[leg] = {}
            for config in configs:
                r = (bench_train if leg == "train" else bench_eval)(config, batches)
                entry[leg][config] = r
                print(f"{name:5s} {leg:5s} {config:9s} steady median {r['steady_median_ms']:7.3f} ms  mean {r['steady_mean_ms']:7.3f}  "
                      f"first pass mean {r['first_pass_mean_ms']:7.3f} ms  graphs {r['graphs']:3d}  held {r['device_mib_held']:8.1f} MiB  "
                      f"reserved {r['device_mib_reserved']:8.1f} MiB", flush=True)
        result["lists"][name] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
