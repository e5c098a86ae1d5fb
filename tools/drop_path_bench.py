#!/usr/bin/env python3
"""Student training step under drop path (FlowStudentModel(drop_path=p)), the default path against another checkout, and the five
drop-path launches alone.

Step legs (``--legs``, default ViT-B/32 at 32 x 16 frames and ViT-L/14 at 16 x 16): the step of bench.py's student leg (forward, cosine
distillation + BCE, backward into a GradArena, fused Adam) on one GPU at every rate of ``--rates`` (0 = the default path: none of the
drop-path launches).  All models of a leg are resident together and the timed windows ALTERNATE between the rates, so that a drift of
the machine hits all of them alike.

  * ms per step: HIP events around windows of ``--steps`` steps after ``--warmup`` steps; median over ``--windows`` windows, min, max;
  * the work model sum_l K_l / (L F), the share of (block, frame) pairs that still run, beside the measured time ratio;
  * peak allocated bytes over one step above what is allocated between steps.

``--parent-dir DIR`` (a built checkout of the parent commit): the default path of this checkout against the same step there and
against a SECOND process of the parent, whose ratio to the first is the parent's own run-to-run spread.  One worker process per
leg, all resident, windows alternating between the processes.

Kernel legs: the five launches at the shapes a dropping block of those steps issues (rate 0.2 at the last block), each timed alone
with HIP events over operand sets that are rotated so that more than 1 GiB passes between two uses of a buffer; GB/s = the bytes the
operation must move (include/vmc.h) over the time, and its share of 8 TB/s.  vmc_drop_path_sample moves next to nothing: its time alone.

``--run-kernels``: no timing, just the five launches, to be traced by ``rocprofv3 --kernel-trace --stats`` in a run of its own.
``--run-only``: steps of the first leg at the first rate, for the same purpose.

python tools/drop_path_bench.py [--legs ViT-B/32:32x16,ViT-L/14:16x16] [--rates 0,0.1,0.2,0.4] [--parent-dir DIR] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_GBPS = 8000.0


def build(name, clips, T, rate, dtype):
    import torch  # noqa: F401

    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    R, _p, _D, _L, _H, E = synth.vit_geometry(name)
    kw = {"drop_path": rate, "drop_path_seed": 3} if rate else {}       # 0: the constructor call of a checkout without the flag
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=dtype, **kw).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=True)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=1e-4)
    vids = synth.randint_u8(3, "vids", (clips, T, 3, R, R)).cuda()
    teacher = synth.normal(3, "teacher", (clips, T + 1, E)).cuda()
    labels = synth.multi_hot_labels(3, "labels", clips, 140).cuda()

    def step():
        _emb, emb_d, logits = m(vids)
        loss = distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)
        loss.backward()
        opt.step()
    return step


def window(step, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def kept_counts(name, frames, rate):
    from vimo_clip_amd import ops, synth
    L = synth.vit_geometry(name)[3]
    return [ops.drop_path_keep_count(frames, ops.drop_path_rate(rate, l, L)) for l in range(L)]


def step_leg(name, clips, T, rates, dtype, steps, warmup, windows):
    import torch

    from vimo_clip_amd.autograd_vit import saved_activation_bytes
    legs = {r: build(name, clips, T, r, dtype) for r in rates}
    for step in legs.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r in rates}
    for _ in range(windows):
        for r in rates:                                      # alternating: one window of every rate per round
            ms[r].append(window(legs[r], steps))
    out = {}
    for r in rates:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        legs[r]()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        K = kept_counts(name, clips * T, r)
        med = statistics.median(ms[r])
        out[str(r)] = {"ms": med, "ms_min": min(ms[r]), "ms_max": max(ms[r]), "frames_per_s": clips * T / med * 1e3, "peak_step_bytes": peak,
                       "kept_last_block": K[-1], "dropping_blocks": sum(k != clips * T for k in K), "work_model": sum(K) / (len(K) * clips * T),
                       "saved_activation_bytes": saved_activation_bytes(name, clips * T, drop_path=r)}
    return out


# ---- the default path against another checkout: one worker process per leg, windows alternating between the processes -----------
def worker(tree, name, clips, T, dtype_name, steps, warmup):
    sys.path.insert(0, tree)
    import torch
    step = build(name, clips, T, 0.0, torch.bfloat16 if dtype_name == "bf16" else torch.float16)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "run":
            break
        print(f"{window(step, steps):.6f}", flush=True)


def parent_ab(parent_dir, name, clips, T, dtype_name, steps, warmup, windows):
    parent = os.path.abspath(parent_dir)
    trees = {"this": HERE, "parent": parent, "parent_again": parent}
    procs = {}
    for key, tree in trees.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--legs", f"{name}:{clips}x{T}", "--dtype", dtype_name, "--steps",
               str(steps), "--warmup", str(warmup)]
        procs[key] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
    ms = {k: [] for k in trees}
    try:
        for key, p in procs.items():
            if p.stdout.readline().strip() != "ready":
                raise RuntimeError(f"drop_path_bench: the worker of the {key} leg did not start")
        for _ in range(windows):
            for key, p in procs.items():
                p.stdin.write("run\n")
                p.stdin.flush()
                ms[key].append(float(p.stdout.readline()))
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
            except OSError:
                pass
            p.wait(timeout=120)
    out = {k: {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}
    out["this_over_parent"] = out["this"]["ms"] / out["parent"]["ms"]
    out["parent_again_over_parent"] = out["parent_again"]["ms"] / out["parent"]["ms"]
    return out


# ---- the five launches alone ---------------------------------------------------------------------------------------------------------
KERNEL_SHAPES = (("ViT-B/32 512 frames", 512, 50, 768), ("ViT-L/14 256 frames", 256, 257, 1024))


def _kernel_calls(F, N, D):
    """The launches a dropping block at rate 0.2 issues on the fp32 stream: [(entry, make operands, call, bytes it must move)]."""
    import torch

    from vimo_clip_amd import ops
    K = ops.drop_path_keep_count(F, 0.2)
    row, s = N * D, F / K
    keep, slot = ops.drop_path_sample(11, 1, F, K, "cuda")
    rn = lambda rows: torch.randn(rows, row, device="cuda")
    return K, [
        ("vmc_frame_gather", lambda: (rn(F),), lambda x: ops.frame_gather(x, keep), 2 * K * row * 4),
        ("vmc_drop_path_merge", lambda: (rn(F), rn(K)), lambda x, y: ops.drop_path_merge(x, y, slot, s), (2 * F + K) * row * 4),
        ("vmc_drop_path_merge_bwd", lambda: (rn(F),), lambda d: ops.drop_path_merge_bwd(d, keep, slot, s), 2 * (F + K) * row * 4),
        ("vmc_frame_scatter_add", lambda: (rn(F), rn(K)), lambda a, b: ops.frame_scatter_add(a, b, slot), (2 * F + K) * row * 4),
    ]


def kernel_legs(reps=20):
    import torch

    from vimo_clip_amd import ops
    out = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for tower, F, N, D in KERNEL_SHAPES:
        K, calls = _kernel_calls(F, N, D)
        e0.record()
        for i in range(reps):
            ops.drop_path_sample(11 + i, 1, F, K, "cuda")
        e1.record()
        torch.cuda.synchronize()
        out.append(dict(kernel="vmc_drop_path_sample", tower=tower, F=F, K=K, us=e0.elapsed_time(e1) / reps * 1e3))
        for entry, make, call, nbytes in calls:
            one = make()
            sets = [one] + [make() for _ in range(int((1 << 30) // max(1, sum(t.numel() * t.element_size() for t in one))) + 1)]
            for s in sets[:2]:
                call(*s)
            torch.cuda.synchronize()
            e0.record()
            for i in range(reps):
                call(*sets[i % len(sets)])
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            out.append(dict(kernel=entry, tower=tower, F=F, K=K, row=N * D, us=us, bytes=nbytes, gbps=nbytes / us / 1e3,
                            share_of_8TBps=nbytes / us / 1e3 / HBM_GBPS, operand_sets=len(sets)))
            del sets, one
            torch.cuda.empty_cache()
        for k in out[-5:]:
            print(f"{k['kernel']} {tower}: {k['us']:.1f} us" + (f", {k['gbps']:.0f} GB/s ({100 * k['share_of_8TBps']:.0f} % of 8 TB/s)" if "gbps" in k
                                                                  else ""), flush=True)
    return out


def run_kernels(reps=10):
    """The five launches, `reps` times each at both shapes, nothing else: the program to trace."""
    import torch

    from vimo_clip_amd import ops
    for _tower, F, N, D in KERNEL_SHAPES:
        K, calls = _kernel_calls(F, N, D)
        for i in range(reps):
            ops.drop_path_sample(11 + i, 1, F, K, "cuda")
        for _entry, make, call, _nbytes in calls:
            args = make()
            for _ in range(reps):
                call(*args)
            del args
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def write_md(doc, path):
    lines = ["# Drop path on the student: step time, memory, the five launches", "",
             "Written by tools/drop_path_bench.py on " + doc.get("device", "?") + " (one GPU, " + doc.get("dtype", "bf16") + ").  ms / step: "
             "median over alternating windows of back-to-back steps between two HIP events after warm-up, with the fastest and slowest "
             "window.  Rate 0 is the default path (none of the drop-path launches).  Work model: sum_l K_l / (L F), the share of (block, "
             "frame) pairs that still run.  Peak: torch.cuda.max_memory_allocated over one step above what is allocated between steps.  "
             "Saved activations: autograd_vit.saved_activation_bytes(drop_path=).", "",
             "| leg | rate | blocks that drop | K of the last block | work model | ms / step (min .. max) | vs rate 0 | frames / s | "
             "peak over a step, GB | vs rate 0 | saved activations, GB |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for leg, rates in doc.get("steps", {}).items():
        zero = rates.get("0.0") or rates.get("0")
        for d, r in rates.items():
            lines.append(f"| {leg} | {d} | {r['dropping_blocks']} | {r['kept_last_block']} | {r['work_model']:.3f} | {r['ms']:.2f} ({r['ms_min']:.2f} .. "
                         f"{r['ms_max']:.2f}) | " + (f"{r['ms'] / zero['ms']:.3f}" if zero else "-") + f" | {r['frames_per_s']:.0f} | "
                         f"{r['peak_step_bytes'] / 1e9:.3f} | " + (f"{r['peak_step_bytes'] / zero['peak_step_bytes']:.3f}" if zero else "-")
                         + f" | {r['saved_activation_bytes'] / 1e9:.3f} |")
    if doc.get("parent"):
        lines += ["", "The default path against the parent commit, and the parent against itself (one process per leg, all resident, windows "
                  "alternating between them):", "",
                  "| leg | this checkout, ms / step (min .. max) | parent, ms / step (min .. max) | parent again, ms / step (min .. max) | "
                  "this / parent | parent again / parent |", "|---|---|---|---|---|---|"]
        for leg, r in doc["parent"].items():
            cell = lambda a: f"{a['ms']:.2f} ({a['ms_min']:.2f} .. {a['ms_max']:.2f})"
            lines.append(f"| {leg} | {cell(r['this'])} | {cell(r['parent'])} | {cell(r['parent_again'])} | {r['this_over_parent']:.4f} | "
                         f"{r['parent_again_over_parent']:.4f} |")
    lines += ["", "The five launches alone at the shapes of a block that keeps int(0.8 F) frames, fp32 stream (HIP events over rotated operand "
              "sets, more than 1 GiB between two uses of a buffer; bytes = what the operation must move, include/vmc.h):", "",
              "| kernel | shape | us | GB/s | of 8 TB/s |", "|---|---|---|---|---|"]
    for k in doc.get("kernels", []):
        shape = f"{k['tower']}: K {k['K']}" + (f", row {k['row']}" if "row" in k else "")
        lines.append(f"| {k['kernel']} | {shape} | {k['us']:.1f} | " + (f"{k['gbps']:.0f} | {100 * k['share_of_8TBps']:.0f} % |" if "gbps" in k else "- | - |"))
    notes = ""
    if os.path.exists(path):                          # everything from "## Notes" on is kept as it is
        with open(path) as f:
            text = f.read()
        notes = text[text.index("## Notes"):] if "## Notes" in text else ""
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n\n" + notes)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--legs", default="ViT-B/32:32x16,ViT-L/14:16x16")
    ap.add_argument("--rates", default="0,0.1,0.2,0.4")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent-dir", default=None, help="a built checkout of the parent commit: time the default path against it")
    ap.add_argument("--run-only", action="store_true",
                    help="run warmup + steps steps of the first leg at the first rate and write nothing: a program to put behind "
                         "`rocprofv3 --kernel-trace --stats --`")
    ap.add_argument("--run-kernels", action="store_true", help="run the five launches alone and write nothing: the same, for the launches")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--worker", default=None, metavar="TREE", help=argparse.SUPPRESS)
    ap.add_argument("--out-dir", default=os.path.join(HERE, "profiles"))
    args = ap.parse_args()
    legs = []
    for leg in [s for s in args.legs.split(",") if s]:
        name, shape = leg.rsplit(":", 1)
        legs.append((name,) + tuple(int(v) for v in shape.split("x")))
    if args.worker:
        return worker(args.worker, *legs[0], args.dtype, args.steps, args.warmup)
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit("drop_path_bench: no GPU; nothing is measured without one")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    if args.run_kernels:
        return run_kernels()
    if args.run_only:
        step = build(*legs[0], float(args.rates.split(",")[0]), dtype)
        for _ in range(args.warmup + args.steps):
            step()
        torch.cuda.synchronize()
        return
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "drop_path.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(device=torch.cuda.get_device_name(0), dtype=args.dtype)
    rates = [float(d) for d in args.rates.split(",")]

    def save():
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
        write_md(doc, os.path.join(args.out_dir, "drop_path.md"))

    if args.parent_dir:                               # first: nothing of this process is resident on the GPU yet
        for name, clips, T in legs:
            r = parent_ab(args.parent_dir, name, clips, T, args.dtype, args.steps, args.warmup, args.windows)
            doc.setdefault("parent", {})[f"{name} {clips}x{T}"] = r
            print(f"{name} {clips}x{T} default path: this {r['this']['ms']:.2f} ms ({r['this']['ms_min']:.2f} .. {r['this']['ms_max']:.2f}), parent "
                  f"{r['parent']['ms']:.2f} ms ({r['parent']['ms_min']:.2f} .. {r['parent']['ms_max']:.2f}), parent again "
                  f"{r['parent_again']['ms']:.2f} ms, this / parent {r['this_over_parent']:.4f}, parent again / parent "
                  f"{r['parent_again_over_parent']:.4f}", flush=True)
            save()
    for name, clips, T in ([] if args.no_steps else legs):
        res = step_leg(name, clips, T, rates, dtype, args.steps, args.warmup, args.windows)
        doc.setdefault("steps", {})[f"{name} {clips}x{T}"] = res
        for d, r in res.items():
            print(f"{name} {clips}x{T} rate {d}: work model {r['work_model']:.3f}, {r['ms']:.2f} ms/step ({r['ms_min']:.2f} .. "
                  f"{r['ms_max']:.2f}), peak {r['peak_step_bytes'] / 1e9:.3f} GB", flush=True)
        from vimo_clip_amd import autograd_ops
        autograd_ops.weights.clear()
        torch.cuda.empty_cache()
        save()
    if not args.no_kernels:
        doc["kernels"] = kernel_legs()
    save()


if __name__ == "__main__":
    main()
