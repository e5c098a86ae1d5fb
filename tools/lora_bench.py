#!/usr/bin/env python3
"""Student training step: full fine-tuning against LoRA adapters (vimo_clip_amd/lora.py), and the two adapter kernels alone.

Step legs (``--legs``, default ViT-B/32 at 32 x 16 frames and ViT-L/14 at 16 x 16): the step of bench.py's student leg (forward, cosine
distillation + BCE, backward into a GradArena, fused Adam) on one GPU in every mode of ``--modes``: ``full`` (lora_rank = 0: the calls
of a checkout without adapters), ``attn`` and ``attn+mlp`` (rank ``--rank`` adapters on a frozen tower).  All models of a leg are
resident together and the timed windows ALTERNATE between the modes, so that a drift of the machine hits all of them alike.

  * ms per step: HIP events around windows of ``--steps`` steps after ``--warmup`` steps; median over ``--windows`` windows, min, max;
  * peak allocated bytes over one step above what is allocated between steps;
  * arena bytes (4 B per trained parameter, slot padding included = the bytes a data-parallel step all-reduces), optimiser ms
    (events around ``opt.step()`` alone) and libvmc calls per step (C-ABI entries that enqueue work; one call is one to three launches).

Kernel legs: vmc_lora_down_concat and vmc_lora_wgrad_tn at the shapes those steps issue, each timed alone with HIP events over
operand sets that are rotated so that more than 1 GiB passes between two uses of a buffer (the 256 MiB Infinity Cache holds none of
it); achieved GB/s = the bytes the operation must move (include/vmc.h) over the time, and its share of 8 TB/s.

python tools/lora_bench.py [--legs ViT-B/32:32x16,ViT-L/14:16x16] [--modes full,attn,attn+mlp] [--rank 16] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_GBPS = 8000.0


class CallCounter:
    """Counts calls of the libvmc entries that enqueue work (everything but the *_bytes / *_supported / *_offset(s) / version queries)."""

    def __init__(self):
        from vimo_clip_amd import _lib
        self.n = 0
        self.lib = _lib.lib
        self.saved = {}
        for name in _lib.SIGNATURES:
            if name.endswith(("_bytes", "_supported", "_offset", "_offsets", "_version", "_string")):
                continue
            fn = getattr(self.lib, name)
            self.saved[name] = fn
            setattr(self.lib, name, self._wrap(fn))

    def _wrap(self, fn):
        def call(*a):
            self.n += 1
            return fn(*a)
        return call

    def close(self):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def build(name, clips, T, mode, rank, dtype):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.models import FlowStudentModel
    from vimo_clip_amd.optim import FusedAdam, GradArena
    R, _p, _D, _L, _H, E = synth.vit_geometry(name)
    kw = {} if mode == "full" else {"lora_rank": rank, "lora_targets": tuple(mode.split("+"))}
    m = FlowStudentModel(name, device="cuda", num_classes=140, compute_dtype=dtype, **kw).train()
    m.load_state_dict(synth.student_state_dict(name, 3, zero_fc2=True), strict=False)
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
    return dict(step=step, opt=opt, arena=arena, model=m, trained=sum(p.numel() for p in arena.params))


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def step_leg(name, clips, T, modes, rank, dtype, steps, warmup, windows):
    legs = {mode: build(name, clips, T, mode, rank, dtype) for mode in modes}
    for leg in legs.values():
        for _ in range(warmup):
            leg["step"]()
    torch.cuda.synchronize()
    e0, e1 = events()
    ms = {mode: [] for mode in modes}
    for _ in range(windows):
        for mode in modes:                                   # alternating: one window of every mode per round
            e0.record()
            for _ in range(steps):
                legs[mode]["step"]()
            e1.record()
            torch.cuda.synchronize()
            ms[mode].append(e0.elapsed_time(e1) / steps)
    out = {}
    for mode in modes:
        leg = legs[mode]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        counter = CallCounter()
        leg["step"]()
        torch.cuda.synchronize()
        counter.close()
        peak = torch.cuda.max_memory_allocated() - base
        e0.record()
        for _ in range(20):
            leg["opt"].step()                                # on the gradient the last backward left: the arithmetic costs the same
        e1.record()
        torch.cuda.synchronize()
        med = statistics.median(ms[mode])
        out[mode] = {"ms": med, "ms_min": min(ms[mode]), "ms_max": max(ms[mode]), "frames_per_s": clips * T / med * 1e3,
                     "peak_step_bytes": peak, "arena_bytes": leg["arena"].numel * 4, "trained_parameters": leg["trained"],
                     "optimizer_ms": e0.elapsed_time(e1) / 20, "libvmc_calls_per_step": counter.n}
    return out


def kernel_legs(dtype, reps=20):
    from vimo_clip_amd import ops
    out = []
    e0, e1 = events()

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
    for tower, M, widths in (("ViT-B/32 512 frames", 25600, (768, 3072)), ("ViT-L/14 256 frames", 65792, (1024, 4096))):
        for K in widths:
            r = 16
            res = timed(lambda: (rn(M, K), rn(r, K), torch.empty((M, K + 64), dtype=dtype, device="cuda")),
                        lambda x, a, o: ops.lora_down_concat(x, a, r, 2.0, out=o), M * K * 2 + M * (K + 64) * 2)
            out.append(dict(kernel="vmc_lora_down_concat", tower=tower, M=M, K=K, r=r, **res))
            print(f"down_concat {tower} K={K}: {res['us']:.1f} us, {res['gbps']:.0f} GB/s ({100 * res['share_of_8TBps']:.0f} % of 8 TB/s)", flush=True)
        for C in widths:
            r = 16
            res = timed(lambda: (rn(M, 64), rn(M, C + 64), torch.empty((r, C), dtype=torch.float32, device="cuda")),
                        lambda t, x, o: ops.lora_wgrad_tn(t[:, :r], x[:, :C], o), M * (C + r) * 2)
            out.append(dict(kernel="vmc_lora_wgrad_tn", tower=tower, M=M, C=C, r=r, **res))
            print(f"wgrad_tn {tower} C={C}: {res['us']:.1f} us, {res['gbps']:.0f} GB/s ({100 * res['share_of_8TBps']:.0f} % of 8 TB/s)", flush=True)
    return out


def write_md(doc, path):
    lines = ["# LoRA adapters on the student: step time, memory, arena, kernels", "",
             "Written by tools/lora_bench.py on " + doc.get("device", "?") + " (one GPU, " + doc.get("dtype", "bf16") + ").  ms / step: median over "
             "alternating windows of back-to-back steps between two HIP events after warm-up, with the fastest and slowest window.  "
             "`full` is rank 0 in this checkout: the calls of a checkout without adapters.  Peak: torch.cuda.max_memory_allocated over one "
             "step above what is allocated between steps.  Arena bytes are what a data-parallel step all-reduces.", "",
             "| leg | mode | ms / step (min .. max) | vs full | frames / s | peak over a step, GB | trained parameters | arena, MB | optimiser, ms | libvmc calls / step |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for leg, modes in doc.get("steps", {}).items():
        full = modes.get("full", {}).get("ms")
        for mode, r in modes.items():
            lines.append(f"| {leg} | {mode} | {r['ms']:.2f} ({r['ms_min']:.2f} .. {r['ms_max']:.2f}) | " + (f"{r['ms'] / full:.3f}" if full else "-")
                         + f" | {r['frames_per_s']:.0f} | {r['peak_step_bytes'] / 1e9:.3f} | {r['trained_parameters']} | {r['arena_bytes'] / 1e6:.1f} | "
                         f"{r['optimizer_ms']:.3f} | {r['libvmc_calls_per_step']} |")
    lines += ["", "Kernels alone (HIP events over rotated operand sets, more than 1 GiB between two uses of a buffer; bytes = what the operation "
              "must move, include/vmc.h):", "", "| kernel | shape | us | GB/s | of 8 TB/s |", "|---|---|---|---|---|"]
    for k in doc.get("kernels", []):
        shape = f"{k['tower']}: M {k['M']}, " + (f"K {k['K']}" if "K" in k else f"C {k['C']}") + f", r {k['r']}"
        lines.append(f"| {k['kernel']} | {shape} | {k['us']:.1f} | {k['gbps']:.0f} | {100 * k['share_of_8TBps']:.0f} % |")
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
    ap.add_argument("--modes", default="full,attn,attn+mlp")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lora_bench: no GPU; nothing is measured without one")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "lora.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(device=torch.cuda.get_device_name(0), dtype=args.dtype, rank=args.rank)
    for leg in [s for s in args.legs.split(",") if s]:
        name, shape = leg.rsplit(":", 1)
        clips, T = (int(v) for v in shape.split("x"))
        res = step_leg(name, clips, T, args.modes.split(","), args.rank, dtype, args.steps, args.warmup, args.windows)
        doc.setdefault("steps", {})[f"{name} {clips}x{T}"] = res
        for mode, r in res.items():
            print(f"{name} {clips}x{T} {mode}: {r['ms']:.2f} ms/step ({r['ms_min']:.2f} .. {r['ms_max']:.2f}), peak {r['peak_step_bytes'] / 1e9:.3f} GB, "
                  f"arena {r['arena_bytes'] / 1e6:.1f} MB, optimiser {r['optimizer_ms']:.3f} ms, {r['libvmc_calls_per_step']} libvmc calls", flush=True)
        from vimo_clip_amd import autograd_ops
        autograd_ops.weights.clear()
        torch.cuda.empty_cache()
    if not args.no_kernels:
        doc["kernels"] = kernel_legs(dtype)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    write_md(doc, os.path.join(args.out_dir, "lora.md"))


if __name__ == "__main__":
    main()
