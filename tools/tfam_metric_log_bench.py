#!/usr/bin/env python3
"""A TFAM epoch with the loss / metric bookkeeping on the host (per step: two clones, ``total +=``, ``mAP_metric.update`` with its
device-to-host synchronisation) vs in the device-resident epoch log (``Config.device_metrics``, metrics.DeviceMetricLog).

The data of tools/tfam_epoch_bench.py: 2 048 videos of 17..64 rows, E = 512, 140 classes, B = 8, use_graphs, graph_bucket = 32,
device_store.  Two trainers on the same weights, one with device_metrics off and one with it on, in one run on one tree; the first
epoch captures the graphs, later epochs are timed with a host clock around work that ends in a synchronise:
  (a) off_step_ms        per-step time of ``train_epoch`` with device_metrics off, two epochs; |difference| = the noise figure
  (b) on_step_ms         the same with device_metrics on, alternated with (a)
  (c) replay_floor_ms    the same number of bare replays of the captured step graphs, nothing between them, one synchronise at the end
  (d) val_*_ms           ``validate()`` per batch, off and on, alternated, two repeats each
  (e) append_kernel      mean duration of metric_append_kernel and its share of kernel time from a separate
                         ``rocprofv3 --kernel-trace --stats`` run of a short logging trainer (a fresh child process; skipped with
                         --no-trace or when rocprofv3 is missing)
The condition the log is held to: (b) <= (a) + noise of (a), and the same for (d).

    python tools/tfam_metric_log_bench.py [--videos 2048] [--val-videos 512] [--dir DIR] [--out profiles/tfam_metric_log.json] [--md profiles/tfam_metric_log.md]
    python tools/tfam_metric_log_bench.py --dir DIR --trace-steps 64       # the child of (e)
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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tfam_epoch_bench import B, C, E, write_pair  # noqa: E402
from vimo_clip_amd import autograd_ops as ag  # noqa: E402
from vimo_clip_amd import synth  # noqa: E402
from vimo_clip_amd.TFAM.data.dataset import HDF5VideoDataset  # noqa: E402
from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer, build_model, index_batches  # noqa: E402


def trainer(train, val, device_metrics):
    """As tools/tfam_epoch_bench.trainer(device_store=True), without dropping the other trainer's 16-bit weight copies."""
    cfg = Config(epochs=4, batch_size=B, d_model=E, num_classes=C, device="cuda", checkpoint_dir=None, use_graphs=True, graph_bucket=32,
                 device_store=True, device_metrics=device_metrics)
    model = build_model(cfg)
    model.load_state_dict(synth.tfam_state_dict(cfg.d_model, cfg.nhead, cfg.num_layers, cfg.dim_feedforward, C, 4), strict=True)
    model.set_dropout_seed(cfg.seed * 1000)
    return ModelTrainer(model, train, val, cfg)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()                                # ends with float(...) of device scalars: synchronised
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, out


def replay_floor(t, epoch, steps):
    """The epoch's step graphs replayed back to back: no index slice, no Python between two launches but the loop itself."""
    order = torch.randperm(len(t.train_set), generator=torch.Generator().manual_seed(t.config.seed + epoch)).tolist()
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")          # the key takes its shape and dtype only
    graphs = [t._graphed_train.captured(idx[:len(ids)], *t._store_lengths(t._train_store, ids))
              for _, ids in index_batches(len(t._train_store), B, order=order)]
    assert len(graphs) == steps and None not in graphs, "an epoch that has run leaves every step shape captured"
    if t._train_log is not None:
        t._train_log.reset()
    ms, _ = timed(lambda: [g.replay() for g in graphs] and None, steps)
    ag.weights.epoch += 1                     # the replays trained: captured evaluation forwards are stale
    return ms


def trace_steps(a):
    """The child of (e): a short logging trainer (captured steps, validation) and plain appends, for a kernel trace."""
    train = HDF5VideoDataset(*write_pair(a.dir, a.trace_steps * B, "trace"))
    ag.weights.clear()
    t = trainer(train, train, True)
    t.train_epoch(0)
    t.train_epoch(1)
    t.validate(1)
    x, y = torch.randn(B, C, device="cuda"), torch.zeros(B, C, device="cuda")
    t._train_log.reset()
    for _ in range(32):                       # plain launches as well: a trace may not list graph nodes
        t._train_log.append(x, y)
    torch.cuda.synchronize()
    print("trace-steps done", t._graphed_train.n_graphs, "graphs", t._train_log.read())


def append_kernel_us(a):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    out = os.path.join(a.dir, "trace")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--dir", a.dir,
           "--trace-steps", "64"]
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
        if "metric_append_kernel" in x["Name"]:
            return {"calls": int(x["Calls"]), "mean_us": float(x["AverageNs"]) / 1e3, "min_us": float(x["MinNs"]) / 1e3,
                    "max_us": float(x["MaxNs"]) / 1e3, "share_of_kernel_time": float(x["TotalDurationNs"]) / total}, None
    return None, "metric_append_kernel not in the trace"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2048)
    ap.add_argument("--val-videos", type=int, default=512)
    ap.add_argument("--dir", default=None, help="where the HDF5 pairs are written (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tfam_metric_log_bench: needs the GPU (there is no CPU timing)")
    tmp = None
    if a.dir is None:
        tmp = tempfile.TemporaryDirectory()
        a.dir = tmp.name
    os.makedirs(a.dir, exist_ok=True)
    if a.trace_steps:
        return trace_steps(a)
    train = HDF5VideoDataset(*write_pair(a.dir, a.videos, "train"))
    val = HDF5VideoDataset(*write_pair(a.dir, a.val_videos, "val"))
    steps, vsteps = len(train) // B, len(val) // B
    res = {"workload": dict(videos=a.videos, val_videos=a.val_videos, rows=[17, 64], E=E, classes=C, batch=B, steps_per_epoch=steps,
                            val_batches=vsteps,
                            trainer="use_graphs=True, graph_bucket=32, device_store=True, cross attention, 4 layers, dropout 0.1")}
    ag.weights.clear()
    t = {False: trainer(train, val, False), True: trainer(train, val, True)}
    first = {on: timed(lambda: t[on].train_epoch(0), steps)[0] for on in (False, True)}       # captures
    ms, stats = {False: [], True: []}, {False: [], True: []}
    for epoch in (1, 2):
        for on in (False, True):
            m, s = timed(lambda: t[on].train_epoch(epoch), steps)
            ms[on].append(m)
            stats[on].append(s)
    res["first_epoch_step_ms"] = {"off": first[False], "on": first[True]}
    res["off_step_ms_repeats"], res["on_step_ms_repeats"] = ms[False], ms[True]
    res["off_step_ms"], res["on_step_ms"] = sum(ms[False]) / len(ms[False]), sum(ms[True]) / len(ms[True])
    res["off_noise_ms"] = abs(ms[False][0] - ms[False][1])
    res["epoch_stats_off"], res["epoch_stats_on"] = stats[False], stats[True]
    res["second_epoch_stats_equal"], res["all_timed_stats_equal"] = stats[False][0] == stats[True][0], stats[False] == stats[True]
    res["params_equal"] = bool(torch.equal(t[False].arena.flat_param, t[True].arena.flat_param))
    res["graphs"] = {"off": t[False]._graphed_train.n_graphs, "on": t[True]._graphed_train.n_graphs}
    res["train_log"] = dict(zip(("rows", "steps", "status", "loss_sum"), t[True]._train_log.read()))
    print(f"(a) off: {ms[False]} ms per step, noise {res['off_noise_ms']:.4f}\n(b) on:  {ms[True]} ms per step; second-epoch loss / metric "
          f"equal: {res['second_epoch_stats_equal']}, parameters equal: {res['params_equal']}", flush=True)
    # (d) validation
    vms, vstats = {False: [], True: []}, {False: [], True: []}
    for rep in range(3):                      # the first round captures the evaluation graphs
        for on in (False, True):
            m, s = timed(lambda: t[on].validate(2), vsteps)
            if rep:
                vms[on].append(m)
                vstats[on].append(s)
    res["val_off_ms_repeats"], res["val_on_ms_repeats"] = vms[False], vms[True]
    res["val_off_ms"], res["val_on_ms"] = sum(vms[False]) / len(vms[False]), sum(vms[True]) / len(vms[True])
    res["val_off_noise_ms"] = abs(vms[False][0] - vms[False][1])
    res["val_stats_equal"] = vstats[False] == vstats[True]
    print(f"(d) validate per batch: off {vms[False]} on {vms[True]} ms; loss / metric equal: {res['val_stats_equal']}", flush=True)
    # (c) the floor, last: bare replays train without the host mirrors
    res["replay_floor_ms"] = {"off": replay_floor(t[False], 2, steps), "on": replay_floor(t[True], 2, steps)}
    print(f"(c) bare replays: {res['replay_floor_ms']} ms per step", flush=True)
    res["condition_train"] = res["on_step_ms"] <= res["off_step_ms"] + res["off_noise_ms"]
    res["condition_val"] = res["val_on_ms"] <= res["val_off_ms"] + res["val_off_noise_ms"]
    del t
    if not a.no_trace:
        res["append_kernel"], why = append_kernel_us(a)
        if why:
            res["append_kernel_note"] = why
        print(f"(e) append kernel: {res['append_kernel'] or why}", flush=True)
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
    w, k = r["workload"], r.get("append_kernel")
    pair = lambda v: f"{v[0]:.3f} / {v[1]:.3f}"          # noqa: E731
    rows = [("(a) `train_epoch` per step, device_metrics off (two epochs)", f"{pair(r['off_step_ms_repeats'])} ms, mean {r['off_step_ms']:.3f}, noise {r['off_noise_ms']:.3f}"),
            ("(b) `train_epoch` per step, device_metrics on (alternated)", f"{pair(r['on_step_ms_repeats'])} ms, mean {r['on_step_ms']:.3f}"),
            ("(c) bare replays of the step graphs, per step (off / on graphs)", f"{r['replay_floor_ms']['off']:.3f} / {r['replay_floor_ms']['on']:.3f} ms"),
            ("(d) `validate` per batch, off (two repeats)", f"{pair(r['val_off_ms_repeats'])} ms, mean {r['val_off_ms']:.3f}, noise {r['val_off_noise_ms']:.3f}"),
            ("(d) `validate` per batch, on (alternated)", f"{pair(r['val_on_ms_repeats'])} ms, mean {r['val_on_ms']:.3f}"),
            ("(e) append kernel, mean (min .. max)", f"{k['mean_us']:.1f} us ({k['min_us']:.1f} .. {k['max_us']:.1f}), {k['calls']} calls, "
             f"{100 * k['share_of_kernel_time']:.2f} % of kernel time" if k else r.get("append_kernel_note", "not traced"))]
    verdict = lambda ok: "**met**" if ok else "**NOT met**"          # noqa: E731
    out = ["# TFAM epoch: loss and metric bookkeeping on the host vs in the device-resident epoch log", "",
           f"`tools/tfam_metric_log_bench.py`: {w['videos']} training / {w['val_videos']} validation videos of {w['rows'][0]}..{w['rows'][1]} rows, "
           f"E = {w['E']}, {w['classes']} classes; batch {w['batch']}, {w['steps_per_epoch']} steps per epoch, {w['val_batches']} validation "
           f"batches; {w['trainer']}.", "Graphs captured in the first epoch, later epochs timed; one run, one tree, MI355X; host clock "
           "around work that ends in a synchronise.", "", "| figure | value |", "|---|---|"] + [f"| {a} | {b} |" for a, b in rows]
    out += ["", f"Condition `(b) <= (a) + noise`, training: {r['on_step_ms']:.3f} <= {r['off_step_ms']:.3f} + {r['off_noise_ms']:.3f} ms: "
            f"{verdict(r['condition_train'])}; validation: {r['val_on_ms']:.3f} <= {r['val_off_ms']:.3f} + {r['val_off_noise_ms']:.3f} ms: "
            f"{verdict(r['condition_val'])}.",
            f"Second-epoch loss / metric equal off vs on: {r['second_epoch_stats_equal']} (every timed epoch: {r['all_timed_stats_equal']}); "
            f"parameters after the run equal: {r['params_equal']}; validation loss / metric equal: {r['val_stats_equal']}.  "
            f"Training log after the last epoch: {r['train_log']}.  First epoch, captures included: off "
            f"{r['first_epoch_step_ms']['off']:.3f}, on {r['first_epoch_step_ms']['on']:.3f} ms per step "
            f"({r['graphs']['off']} / {r['graphs']['on']} graphs).", ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
