#!/usr/bin/env python3
"""Student training step under patch dropout (FlowStudentModel(patch_dropout=p)), the default path against another checkout, and the
stem kernels alone.

Step legs (``--legs``, default ViT-B/32 at 32 x 16 frames and ViT-L/14 at 16 x 16): the step of bench.py's student leg (forward, cosine
distillation + BCE, backward into a GradArena, fused Adam) on one GPU at every drop fraction of ``--drops`` (0 = the default path: none
of the patch-dropout launches).  All models of a leg are resident together and the timed windows ALTERNATE between the fractions, so
that a drift of the machine hits all of them alike.

  * ms per step: HIP events around windows of ``--steps`` steps after ``--warmup`` steps; median over ``--windows`` windows, min, max;
  * the row ratio (Kp + 1) / N, which is what every per-row cost scales with, beside the measured time ratio;
  * peak allocated bytes over one step above what is allocated between steps.

``--parent-dir DIR`` (a built checkout of the parent commit): the default path of this checkout against the same step there.  One
worker process per checkout, both resident, windows alternating between the two processes; the ratio of the medians is reported beside
each side's own window spread.

Kernel legs: vmc_gather_rows16, vmc_assemble_tokens_keep and vmc_assemble_tokens_keep_bwd at the shapes those steps issue (drop
fraction 0.5), each timed alone with HIP events over operand sets that are rotated so that more than 1 GiB passes between two uses of
a buffer; GB/s = the bytes the operation must move (include/vmc.h) over the time, and its share of 8 TB/s.  vmc_patch_keep_sample moves
next to nothing: its time alone.

``--run-only``: no timing, just steps of one leg at one fraction, to be traced by rocprofv3 in a run of its own.

python tools/patch_dropout_bench.py [--legs ViT-B/32:32x16,ViT-L/14:16x16] [--drops 0,0.5,0.75] [--parent-dir DIR] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_GBPS = 8000.0


def build(name, clips, T, drop, dtype):
    import torch  # noqa: F401

    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    R, _p, _D, _L, _H, E = synth.vit_geometry(name)
    kw = {"patch_dropout": drop, "patch_dropout_seed": 3} if drop else {}       # 0: the constructor call of a checkout without the flag
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


def tokens(name, drop):
    from vimo_clip_amd import ops, synth
    R, p = synth.vit_geometry(name)[:2]
    G = (R // p) ** 2
    return (ops.patch_keep_count(G, drop) if drop else G) + 1, G + 1


def step_leg(name, clips, T, drops, dtype, steps, warmup, windows):
    import torch

    from vimo_clip_amd.autograd_vit import saved_activation_bytes
    legs = {d: build(name, clips, T, d, dtype) for d in drops}
    for step in legs.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    ms = {d: [] for d in drops}
    for _ in range(windows):
        for d in drops:                                      # alternating: one window of every fraction per round
            ms[d].append(window(legs[d], steps))
    out = {}
    for d in drops:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        legs[d]()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        n_kept, n_all = tokens(name, d)
        med = statistics.median(ms[d])
        out[str(d)] = {"ms": med, "ms_min": min(ms[d]), "ms_max": max(ms[d]), "frames_per_s": clips * T / med * 1e3, "peak_step_bytes": peak,
                       "tokens": n_kept, "row_ratio": n_kept / n_all,
                       "saved_activation_bytes": saved_activation_bytes(name, clips * T, tokens=n_kept)}
    return out


# ---- the default path against another checkout: one worker process per tree, windows alternating between the processes ----------
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
    trees = {"this": HERE, "parent": os.path.abspath(parent_dir)}
    procs = {}
    for key, tree in trees.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--legs", f"{name}:{clips}x{T}", "--dtype", dtype_name, "--steps",
               str(steps), "--warmup", str(warmup)]
        procs[key] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
    ms = {k: [] for k in trees}
    try:
        for key, p in procs.items():
            if p.stdout.readline().strip() != "ready":
                raise RuntimeError(f"patch_dropout_bench: the worker of the {key} checkout did not start")
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
    return out


# ---- the stem kernels alone ----------------------------------------------------------------------------------------------------------
def kernel_legs(dtype, reps=20):
    import torch

    from vimo_clip_amd import ops
    out = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(make, call, nbytes):
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
        return {"us": us, "bytes": nbytes, "gbps": nbytes / us / 1e3, "share_of_8TBps": nbytes / us / 1e3 / HBM_GBPS, "operand_sets": len(sets)}

    rn = lambda *s: torch.randn(*s, device="cuda").to(dtype)
    for tower, F, G, cols, D in (("ViT-B/32 512 frames", 512, 49, 3072, 768), ("ViT-L/14 256 frames", 256, 256, 640, 1024)):
        Kp = ops.patch_keep_count(G, 0.5)
        N = Kp + 1
        keep = ops.patch_keep_sample(11, F, G, Kp, "cuda")
        e0.record()
        for i in range(reps):
            ops.patch_keep_sample(11 + i, F, G, Kp, "cuda")
        e1.record()
        torch.cuda.synchronize()
        out.append(dict(kernel="vmc_patch_keep_sample", tower=tower, F=F, G=G, Kp=Kp, us=e0.elapsed_time(e1) / reps * 1e3))
        res = timed(lambda: (rn(F * G, cols),), lambda src: ops.gather_rows16(src, keep, G), 2 * F * Kp * cols * 2)
        out.append(dict(kernel="vmc_gather_rows16", tower=tower, F=F, G=G, Kp=Kp, cols=cols, **res))
        cls, pos = torch.randn(D, device="cuda"), torch.randn(G + 1, D, device="cuda")
        res = timed(lambda: (rn(F * Kp, D),), lambda xp: ops.assemble_tokens_keep(xp, cls, pos, keep, torch.float32),
                    F * Kp * D * 2 + F * N * D * 4 + (G + 1) * D * 4)          # the positional table comes through the caches: counted once
        out.append(dict(kernel="vmc_assemble_tokens_keep", tower=tower, F=F, G=G, Kp=Kp, D=D, **res))
        res = timed(lambda: (torch.randn(F * N, D, device="cuda"),), lambda dx: ops.assemble_tokens_keep_bwd(dx, keep, G, dtype),
                    2 * F * N * D * 4 + F * Kp * D * 2 + (G + 1) * D * 4)
        out.append(dict(kernel="vmc_assemble_tokens_keep_bwd", tower=tower, F=F, G=G, Kp=Kp, D=D, **res))
        for k in out[-4:]:
            print(f"{k['kernel']} {tower}: {k['us']:.1f} us" + (f", {k['gbps']:.0f} GB/s ({100 * k['share_of_8TBps']:.0f} % of 8 TB/s)" if "gbps" in k
                                                                  else ""), flush=True)
    return out


def write_md(doc, path):
    lines = ["# Patch dropout on the student: step time, memory, stem kernels", "",
             "Written by tools/patch_dropout_bench.py on " + doc.get("device", "?") + " (one GPU, " + doc.get("dtype", "bf16") + ").  ms / step: "
             "median over alternating windows of back-to-back steps between two HIP events after warm-up, with the fastest and slowest "
             "window.  Drop fraction 0 is the default path (none of the patch-dropout launches).  Row ratio: (Kp + 1) / N, what every "
             "per-row cost scales with.  Peak: torch.cuda.max_memory_allocated over one step above what is allocated between steps.  "
             "Saved activations: autograd_vit.saved_activation_bytes at the kept token count.", "",
             "| leg | drop | tokens | row ratio | ms / step (min .. max) | vs drop 0 | frames / s | peak over a step, GB | vs drop 0 | saved activations, GB |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for leg, drops in doc.get("steps", {}).items():
        zero = drops.get("0.0") or drops.get("0")
        for d, r in drops.items():
            lines.append(f"| {leg} | {d} | {r['tokens']} | {r['row_ratio']:.3f} | {r['ms']:.2f} ({r['ms_min']:.2f} .. {r['ms_max']:.2f}) | "
                         + (f"{r['ms'] / zero['ms']:.3f}" if zero else "-") + f" | {r['frames_per_s']:.0f} | {r['peak_step_bytes'] / 1e9:.3f} | "
                         + (f"{r['peak_step_bytes'] / zero['peak_step_bytes']:.3f}" if zero else "-") + f" | {r['saved_activation_bytes'] / 1e9:.3f} |")
    if doc.get("parent"):
        lines += ["", "The default path against the parent commit (one process per checkout, both resident, windows alternating between them):", "",
                  "| leg | this checkout, ms / step (min .. max) | parent, ms / step (min .. max) | this / parent |", "|---|---|---|---|"]
        for leg, r in doc["parent"].items():
            a, b = r["this"], r["parent"]
            lines.append(f"| {leg} | {a['ms']:.2f} ({a['ms_min']:.2f} .. {a['ms_max']:.2f}) | {b['ms']:.2f} ({b['ms_min']:.2f} .. {b['ms_max']:.2f}) | "
                         f"{r['this_over_parent']:.4f} |")
    lines += ["", "Stem kernels alone at drop fraction 0.5 (HIP events over rotated operand sets, more than 1 GiB between two uses of a buffer; "
              "bytes = what the operation must move, include/vmc.h):", "", "| kernel | shape | us | GB/s | of 8 TB/s |", "|---|---|---|---|---|"]
    for k in doc.get("kernels", []):
        shape = f"{k['tower']}: G {k['G']}, Kp {k['Kp']}" + (f", cols {k['cols']}" if "cols" in k else "") + (f", D {k['D']}" if "D" in k else "")
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
    ap.add_argument("--drops", default="0,0.5,0.75")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent-dir", default=None, help="a built checkout of the parent commit: time the default path against it")
    ap.add_argument("--run-only", action="store_true",
                    help="run warmup + steps steps of the first leg at the first drop fraction and write nothing: the program to put behind "
                         "`rocprofv3 --kernel-trace --stats --` when the question is which launches scale with the rows")
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
        sys.exit("patch_dropout_bench: no GPU; nothing is measured without one")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    if args.run_only:
        step = build(*legs[0], float(args.drops.split(",")[0]), dtype)
        for _ in range(args.warmup + args.steps):
            step()
        torch.cuda.synchronize()
        return
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "patch_dropout.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(device=torch.cuda.get_device_name(0), dtype=args.dtype)
    drops = [float(d) for d in args.drops.split(",")]

    def save():
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
        write_md(doc, os.path.join(args.out_dir, "patch_dropout.md"))

    if args.parent_dir:                               # first: nothing of this process is resident on the GPU yet
        for name, clips, T in legs:
            r = parent_ab(args.parent_dir, name, clips, T, args.dtype, args.steps, args.warmup, args.windows)
            doc.setdefault("parent", {})[f"{name} {clips}x{T}"] = r
            print(f"{name} {clips}x{T} default path: this {r['this']['ms']:.2f} ms ({r['this']['ms_min']:.2f} .. {r['this']['ms_max']:.2f}), parent "
                  f"{r['parent']['ms']:.2f} ms ({r['parent']['ms_min']:.2f} .. {r['parent']['ms_max']:.2f}), ratio {r['this_over_parent']:.4f}", flush=True)
            save()
    for name, clips, T in ([] if args.no_steps else legs):
        res = step_leg(name, clips, T, drops, dtype, args.steps, args.warmup, args.windows)
        doc.setdefault("steps", {})[f"{name} {clips}x{T}"] = res
        for d, r in res.items():
            print(f"{name} {clips}x{T} drop {d}: {r['tokens']} tokens (row ratio {r['row_ratio']:.3f}), {r['ms']:.2f} ms/step ({r['ms_min']:.2f} .. "
                  f"{r['ms_max']:.2f}), peak {r['peak_step_bytes'] / 1e9:.3f} GB", flush=True)
        from vimo_clip_amd import autograd_ops
        autograd_ops.weights.clear()
        torch.cuda.empty_cache()
        save()
    if not args.no_kernels:
        doc["kernels"] = kernel_legs(dtype)
    save()


if __name__ == "__main__":
    main()
