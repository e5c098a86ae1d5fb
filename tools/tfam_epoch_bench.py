#!/usr/bin/env python3
"""A TFAM training epoch fed by the host loader vs fed from the device-resident store (TFAM/data/device_store.py).

Writes a synthetic HDF5 pair with h5lite in the reference's layout (one group per video, ``embeddings`` gzip-compressed with
chunks (1, E), ``labels``; the motion file keyed by ``key.split(".")[0]``): 2 048 videos of 17..64 rows, E = 512, 140 classes.
Then, in one run on one tree:
  (a) loader_only_ms_per_batch   ``batches(HDF5VideoDataset, 8)`` alone: item reads + collate_fn_pad, no device work
  (b) loader_step_ms             per-step time of ``ModelTrainer.train_epoch`` through the loader, use_graphs, graph_bucket = 32
  (c) store_step_ms              the same epoch with ``device_store=True``
  (d) store_build_s / store_nbytes  DeviceClipStore.from_hdf5 of the training file pair
  (e) gather_kernel_us           mean duration of gather_clips_kernel from a separate ``rocprofv3 --kernel-trace --stats`` run of a
                                 short (c) (a fresh child process; skipped with --no-trace or when rocprofv3 is missing)
(b) and (c) time the SECOND epoch: every graph that will exist was captured in the first.  The condition the store is held to is
    store_step_ms <= loader_step_ms - 0.5 * loader_only_ms_per_batch

    python tools/tfam_epoch_bench.py [--videos 2048] [--dir DIR] [--out profiles/tfam_device_store.json] [--md profiles/tfam_device_store.md]
    python tools/tfam_epoch_bench.py --dir DIR --store-steps 64        # the child of (e): 64 captured store steps, nothing else
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vimo_clip_amd import autograd_ops as ag  # noqa: E402
from vimo_clip_amd import h5lite as h5  # noqa: E402
from vimo_clip_amd import synth  # noqa: E402
from vimo_clip_amd.TFAM.data.dataset import HDF5VideoDataset  # noqa: E402
from vimo_clip_amd.TFAM.data.device_store import DeviceClipStore  # noqa: E402
from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer, batches, build_model  # noqa: E402

E, C, B, TMIN, TMAX = 512, 140, 8, 17, 64


def write_pair(d, n, tag):
    """rgb_<tag>.h5 / flow_<tag>.h5 under d (kept when they exist with the right number of videos)."""
    rgb, flow = os.path.join(d, f"rgb_{tag}.h5"), os.path.join(d, f"flow_{tag}.h5")
    if os.path.exists(rgb) and os.path.exists(flow):
        with h5.File(rgb, "r") as f:
            if len(f.keys()) == n:
                return rgb, flow
    rng = np.random.default_rng(17 + n)
    lens = rng.integers(TMIN, TMAX + 1, n)
    labels = synth.multi_hot_labels(1, f"epoch/{tag}", n, C).numpy().astype(np.float32)
    with h5.File(rgb, "w") as f, h5.File(flow, "w") as g:
        for i, T in enumerate(lens):
            vid = f"video_{i:05d}.mp4"
            grp = f.create_group(vid)
            grp.create_dataset("embeddings", data=rng.standard_normal((T, E)).astype(np.float32), compression="gzip", chunks=(1, E))
            grp.create_dataset("labels", data=labels[i])
            g.create_group(vid.split(".")[0]).create_dataset("embeddings", data=rng.standard_normal((T - 1, E)).astype(np.float32),
                                                             compression="gzip", chunks=(1, E))
    return rgb, flow


def trainer(train, val, device_store):
    ag.weights.clear()
    torch.cuda.empty_cache()
    cfg = Config(epochs=2, batch_size=B, d_model=E, num_classes=C, device="cuda", checkpoint_dir=None, use_graphs=True, graph_bucket=32,
                 device_store=device_store)
    model = build_model(cfg)
    model.load_state_dict(synth.tfam_state_dict(cfg.d_model, cfg.nhead, cfg.num_layers, cfg.dim_feedforward, C, 4), strict=True)
    model.set_dropout_seed(cfg.seed * 1000)
    return ModelTrainer(model, train, val, cfg)


def timed_epoch(t, epoch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = t.train_epoch(epoch)              # ends with float(...) of device scalars: synchronised
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps, stats


def store_steps(a):
    """The child of (e): a short run of captured steps fed from the store, for a kernel trace."""
    train = HDF5VideoDataset(*write_pair(a.dir, a.store_steps * B, "trace"))
    t = trainer(train, train, True)
    t.train_epoch(0)
    t.train_epoch(1)
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    for _ in range(32):                      # plain launches as well, at the largest shape: a trace may not list graph nodes
        t._train_store.gather(idx, TMAX, TMAX)
    torch.cuda.synchronize()
    print("store-steps done", t._graphed_train.n_graphs, "graphs")


def gather_kernel_us(a):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    out = os.path.join(a.dir, "trace")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--dir", a.dir, "--store-steps", "64"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    except subprocess.TimeoutExpired:
        return None, "rocprofv3 run did not finish in 420 s"
    if r.returncode != 0:
        return None, f"rocprofv3 run failed ({r.returncode}): {r.stderr[-400:]}"
    files = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return None, "no kernel_stats.csv"
    rows = list(csv.DictReader(open(files[-1])))
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    for x in rows:
        if "gather_clips_kernel" in x["Name"]:
            return {"calls": int(x["Calls"]), "mean_us": float(x["AverageNs"]) / 1e3, "min_us": float(x["MinNs"]) / 1e3,
                    "max_us": float(x["MaxNs"]) / 1e3, "share_of_kernel_time": float(x["TotalDurationNs"]) / total}, None
    return None, "gather_clips_kernel not in the trace"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2048)
    ap.add_argument("--dir", default=None, help="where the HDF5 pair is written (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--store-steps", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tfam_epoch_bench: needs the GPU (there is no CPU timing)")
    tmp = None
    if a.dir is None:
        tmp = tempfile.TemporaryDirectory()
        a.dir = tmp.name
    os.makedirs(a.dir, exist_ok=True)
    if a.store_steps:
        return store_steps(a)
    t0 = time.perf_counter()
    rgb, flow = write_pair(a.dir, a.videos, "train")
    vrgb, vflow = write_pair(a.dir, 4 * B, "val")
    write_s = time.perf_counter() - t0
    train, val = HDF5VideoDataset(rgb, flow), HDF5VideoDataset(vrgb, vflow)
    steps = len(train) // B
    res = {"workload": dict(videos=a.videos, rows=[TMIN, TMAX], E=E, classes=C, batch=B, steps_per_epoch=steps, layout="gzip, chunks (1, E)",
                            trainer="use_graphs=True, graph_bucket=32, cross attention, 4 layers, dropout 0.1"),
           "hdf5_write_s": write_s}
    # (a) the host loader alone
    n_loader = min(steps, 64)
    order = torch.randperm(len(train), generator=torch.Generator().manual_seed(0)).tolist()
    t0 = time.perf_counter()
    for i, _ in enumerate(batches(train, B, order=order)):
        if i + 1 == n_loader:
            break
    res["loader_only_ms_per_batch"] = (time.perf_counter() - t0) * 1e3 / n_loader
    print(f"(a) loader alone: {res['loader_only_ms_per_batch']:.2f} ms per batch of {B} ({n_loader} batches)", flush=True)
    # (b) the epoch through the loader
    t = trainer(train, val, False)
    first, _ = timed_epoch(t, 0, steps)
    res["loader_step_ms"], stats_b = timed_epoch(t, 1, steps)
    res["loader_first_epoch_step_ms"], res["loader_graphs"] = first, t._graphed_train.n_graphs
    print(f"(b) loader epoch: {res['loader_step_ms']:.3f} ms per step (first epoch, captures included: {first:.3f}); "
          f"{res['loader_graphs']} graphs", flush=True)
    del t
    # (d) the store alone, then (c) the epoch from the store
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = DeviceClipStore.from_hdf5(rgb, flow, device="cuda")
    torch.cuda.synchronize()
    res["store_build_s"], res["store_nbytes"] = time.perf_counter() - t0, s.nbytes
    print(f"(d) store: built in {res['store_build_s']:.2f} s, {s.nbytes / 2 ** 20:.1f} MiB", flush=True)
    del s
    t = trainer(train, val, True)
    first, _ = timed_epoch(t, 0, steps)
    res["store_step_ms"], stats_c = timed_epoch(t, 1, steps)
    res["store_first_epoch_step_ms"], res["store_graphs"] = first, t._graphed_train.n_graphs
    res["store_status"] = t._train_store.read_status()
    res["second_epoch_stats_equal"] = stats_b == stats_c
    print(f"(c) store epoch:  {res['store_step_ms']:.3f} ms per step (first epoch, captures included: {first:.3f}); "
          f"{res['store_graphs']} graphs; status {res['store_status']}; epoch statistics equal to (b): {stats_b == stats_c}", flush=True)
    del t
    res["bound_ms"] = res["loader_step_ms"] - 0.5 * res["loader_only_ms_per_batch"]
    res["condition_met"] = res["store_step_ms"] <= res["bound_ms"]
    print(f"condition: (c) {res['store_step_ms']:.3f} <= (b) - (a) / 2 = {res['bound_ms']:.3f}: {res['condition_met']}", flush=True)
    # (e) the gather kernel, from a trace of its own
    if not a.no_trace:
        res["gather_kernel"], why = gather_kernel_us(a)
        if why:
            res["gather_kernel_note"] = why
        print(f"(e) gather kernel: {res['gather_kernel'] or why}", flush=True)
    line = json.dumps(res)
    print(line)
    for path, text in ((a.out, line + "\n"), (a.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    if tmp is not None:
        tmp.cleanup()


def markdown(r):
    w, g = r["workload"], r.get("gather_kernel")
    rows = [("(a) host loader alone, per batch", f"{r['loader_only_ms_per_batch']:.2f} ms"),
            ("(b) epoch through the loader, per step", f"{r['loader_step_ms']:.3f} ms"),
            ("(c) epoch from the device store, per step", f"{r['store_step_ms']:.3f} ms"),
            ("(d) store build (from_hdf5), size", f"{r['store_build_s']:.2f} s, {r['store_nbytes'] / 2 ** 20:.1f} MiB"),
            ("(e) gather kernel, mean (min .. max)", f"{g['mean_us']:.1f} us ({g['min_us']:.1f} .. {g['max_us']:.1f}), {g['calls']} calls, "
             f"{100 * g['share_of_kernel_time']:.1f} % of kernel time" if g else r.get("gather_kernel_note", "not traced"))]
    out = ["# TFAM epoch: host loader vs device-resident store", "",
           f"`tools/tfam_epoch_bench.py`: {w['videos']} videos of {w['rows'][0]}..{w['rows'][1]} rows, E = {w['E']}, {w['classes']} classes, "
           f"HDF5 written by h5lite ({w['layout']}); batch {w['batch']}, {w['steps_per_epoch']} steps per epoch; {w['trainer']}.",
           "Second epoch timed (graphs captured in the first); one run, one tree, MI355X.", "",
           "| figure | value |", "|---|---|"] + [f"| {a} | {b} |" for a, b in rows]
    out += ["", f"Condition `(c) <= (b) - (a) / 2`: {r['store_step_ms']:.3f} <= {r['bound_ms']:.3f} ms: "
            f"**{'met' if r['condition_met'] else 'NOT met'}**.",
            f"First epoch, captures included: loader {r['loader_first_epoch_step_ms']:.3f} ms per step ({r['loader_graphs']} graphs), "
            f"store {r['store_first_epoch_step_ms']:.3f} ms per step ({r['store_graphs']} graphs).  Store status word after the run: "
            f"{r['store_status']}.  Second-epoch loss / metric equal in (b) and (c): {r['second_epoch_stats_equal']}.", ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
