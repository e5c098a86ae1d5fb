#!/usr/bin/env python3
"""Masked attention at long sequence lengths (vmc_attention_fwd / vmc_attention_bwd beyond the short-sequence kernels): forward
and forward + backward, timed with HIP events, B = 8, H = 8, head_dim 64 / 96, T = 128 .. 4096, full / ragged / concat masks.

  python tools/attn_long_bench.py [--old PATH/libvmc.so] [--reps N] [--json OUT] [--quick] [--no-step]

--old loads a second libvmc.so (e.g. built from an earlier commit) and times it alternately with the package's own library, in
the same process, on the same inputs (the old library's generic attention stops at T = 2048: larger T are skipped for it).  Its
outputs are compared against the new ones as well.  Unless --no-step, it also times the per-op TFAM train step (AMO_CLIP,
cross-attention mode, D 768, B 8, ragged) at T = 256 and 1024 with the attention entries taken from either library.

Rates: FLOPs on the LIVE keys only (a masked key costs no work in an ideal kernel): forward 4 Tq Tk_live dh per (b, h),
forward + backward 14 Tq Tk_live dh (4 + the backward's five products 10); the share of peak is against the 2.5 PFLOP/s dense
bf16 / f16 MFMA peak."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vimo_clip_amd import _lib  # noqa: E402
from vimo_clip_amd import autograd_ops as ag  # noqa: E402
from vimo_clip_amd import ops  # noqa: E402

PEAK = 2.5e15
ENTRIES = ("vmc_attention_fwd", "vmc_attention_bwd", "vmc_attention_bwd_workspace_bytes")


class Libs:
    """Swaps the attention entries of the package's ctypes library between the new (own) and an old libvmc.so."""

    def __init__(self, old_path):
        self.new = {n: getattr(_lib.lib, n) for n in ENTRIES}
        self.old = None
        if old_path:
            old = ctypes.CDLL(old_path)
            self.old = {}
            for n in ENTRIES:
                f = getattr(old, n)
                f.restype, f.argtypes = _lib.SIGNATURES[n]
                self.old[n] = f

    def use(self, which):
        for n, f in (self.new if which == "new" else self.old).items():
            setattr(_lib.lib, n, f)


def masks(kind, B, T, g):
    ar = torch.arange(T)[None, :]
    if kind == "full":
        return None, B * T
    if kind == "ragged":                               # lengths uniform in [T/2, T]
        lens = torch.randint(T // 2, T + 1, (B,), generator=g)
        m = ar < lens[:, None]
    else:                                              # concat_dim=1: (Tr - 1) RGB then Tf flow tokens, padding in between
        tr = T // 2
        lens = torch.randint(tr // 2, tr + 1, (B,), generator=g)
        m = torch.cat([ar[:, :tr] < lens[:, None], ar[:, :T - tr] < lens[:, None]], dim=1)
    return m.to(torch.uint8).cuda(), int(m.sum())


def time_rounds(fns, reps, rounds):
    """fns: name -> callable (warmed up by the caller).  Per round reps calls between two events.  -> name -> [ms per call]."""
    out = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            out[n].append(e0.elapsed_time(e1) / reps)
    return out


def attn_points(libs, Ts, dhs, kinds, reps, rounds):
    B, H = 8, 8
    rows = []
    for dh in dhs:
        D = H * dh
        for T in Ts:
            g = torch.Generator().manual_seed(T + dh)
            q = torch.randn(B * T, D, generator=g).to(torch.bfloat16).cuda()
            kv = torch.randn(B * T, 2 * D, generator=g).to(torch.bfloat16).cuda()
            do = torch.randn(B * T, D, generator=g).to(torch.bfloat16).cuda()
            dq, dkv = torch.empty_like(q), torch.empty_like(kv)
            for kind in kinds:
                m, live = masks(kind, B, T, g)

                def fwd():
                    return ops.attention(q, kv[:, :D], kv[:, D:], m, B, H, T, T, dh, want_lse=True)

                def fwdbwd():
                    o, lse = fwd()
                    ag._attn_bwd(q, kv[:, :D], kv[:, D:], m, o, do, lse, dq, dkv[:, :D], dkv[:, D:], B, H, T, T, dh)

                sides = ["new"] + (["old"] if libs.old is not None and T <= 2048 else [])
                res = {}
                outs = {}
                for which in sides:
                    libs.use(which)
                    o, _ = fwd()
                    fwdbwd()
                    torch.cuda.synchronize()
                    outs[which] = (o.float(), dq.float().clone(), dkv.float().clone())
                r = max(1, rounds if T <= 1024 or libs.old is None else max(2, rounds // 2))
                for name, fn in (("fwd", fwd), ("fwdbwd", fwdbwd)):
                    per = {}
                    for which in sides:       # alternate by swapping the entries inside each round
                        per[which] = []
                    for _ in range(r):
                        for which in sides:
                            libs.use(which)
                            n = reps if which == "new" or T <= 512 else max(1, reps // 4)
                            per[which] += time_rounds({which: fn}, n, 1)[which]
                    for which in sides:
                        res[f"{name}_{which}_ms"] = statistics.median(per[which])
                        res[f"{name}_{which}_ms_min"] = min(per[which])
                libs.use("new")
                flop_f = 4.0 * T * live * H * dh             # sum over b of Tq * Tk_live, times H, dh
                flop_fb = 14.0 * T * live * H * dh
                row = dict(dh=dh, T=T, mask=kind, live_keys=live, **res)
                row["fwd_tflops"] = flop_f / (res["fwd_new_ms"] * 1e-3) / 1e12
                row["fwdbwd_tflops"] = flop_fb / (res["fwdbwd_new_ms"] * 1e-3) / 1e12
                row["fwd_peak_share"] = row["fwd_tflops"] * 1e12 / PEAK
                row["fwdbwd_peak_share"] = row["fwdbwd_tflops"] * 1e12 / PEAK
                if "old" in outs:
                    row["fwd_speedup"] = res["fwd_old_ms"] / res["fwd_new_ms"]
                    row["fwdbwd_speedup"] = res["fwdbwd_old_ms"] / res["fwdbwd_new_ms"]
                    for i, nm in enumerate(("out", "dq", "dkv")):
                        a, b = outs["new"][i], outs["old"][i]
                        row[f"maxdiff_{nm}"] = (a - b).abs().max().item()
                print(json.dumps(row), flush=True)
                rows.append(row)
            del q, kv, do, dq, dkv
            torch.cuda.empty_cache()
    return rows


def tfam_step(libs, Ts, reps, rounds):
    from vimo_clip_amd import synth
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    B, D = 8, 768
    rows = []
    for T in Ts:
        m = AMO_CLIP(d_model=D, nhead=8, num_layers=4, dim_feedforward=2048, num_classes=140, dropout=0.1, mlp_dropout=0.1,
                     device="cuda").cuda().train()
        m.load_state_dict(synth.tfam_state_dict(D, 8, 4, 2048, 140, 4), strict=True)
        lens = synth.randint(5, "lens", (B,), T // 2, T + 1)
        lens[0] = T
        mr = (torch.arange(T)[None, :] < lens[:, None]).cuda()
        mf = (torch.arange(T - 1)[None, :] < (lens - 1)[:, None]).cuda()
        rgb = (synth.normal(5, "rgb", (B, T, D)).cuda() * mr[..., None])
        mot = (synth.normal(5, "mot", (B, T - 1, D)).cuda() * mf[..., None])
        y = synth.multi_hot_labels(5, "lab", B, 140).cuda()

        def step():
            m.zero_grad(set_to_none=True)
            loss = bce_with_logits_loss(m(rgb, mot, mask_rgb=mr, mask_flow=mf), y)
            loss.backward()

        sides = ["new"] + (["old"] if libs.old is not None and T <= 2048 else [])
        for s in sides:                                # warm-up
            libs.use(s)
            step()
        torch.cuda.synchronize()
        per = {s: [] for s in sides}
        for _ in range(rounds):
            for s in sides:
                libs.use(s)
                per[s] += time_rounds({s: step}, reps, 1)[s]
        libs.use("new")
        row = dict(tfam_train_step=True, B=B, D=D, T=T, Tk_cross=T - 1, layers=4)
        for s in sides:
            row[f"step_{s}_ms"] = statistics.median(per[s])
            row[f"step_{s}_ms_min"] = min(per[s])
        if "old" in per:
            row["step_speedup"] = row["step_old_ms"] / row["step_new_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del m
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="path of an older libvmc.so timed alternately with the current one")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="T 512 / 4096, ragged mask only, no step (a profiler pass)")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    libs = Libs(a.old)
    if a.quick:
        rows = attn_points(libs, [512, 4096], [64, 96], ["ragged"], a.reps, 1)
    else:
        rows = attn_points(libs, [128, 256, 512, 1024, 2048, 4096], [64, 96], ["full", "ragged", "concat"], a.reps, a.rounds)
        if not a.no_step:
            rows += tfam_step(libs, [256, 1024], 2, 3)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
