#!/usr/bin/env python3
"""Drives the fused TFAM chains over a fixed list of small cases (for rocprofv3 --kernel-trace and for before / after comparisons):

    python3 tools/tfam_chain_run.py [--dump DIR]            every case: one eval forward and one training step, bf16 and f16
    python3 tools/tfam_chain_run.py B [ITERS] [f16]         the eval forward of the reference geometry ITERS times at batch B

Seeds are fixed; the training steps run with dropout 0.1.  With --dump every case writes its logits and every gradient to
DIR/<case>_<dtype>.npz, so two builds can be compared byte for byte.  A case whose shapes the chain declines is reported as such
(the per-op path then computes it), never skipped silently.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vimo_clip_amd import synth, tfam_fused, tfam_train  # noqa: E402
from vimo_clip_amd.losses import bce_with_logits_loss  # noqa: E402
from vimo_clip_amd.TFAM.models import AMO_CLIP  # noqa: E402

CASES = [
    dict(name="ref_b8_t16", D=768, H=8, ff=2048, L=4, C=140, B=8, T=16, Tk=16, cross=True, ragged=False, seed=10),
    dict(name="d512_t40_k39", D=512, H=8, ff=1024, L=2, C=140, B=3, T=40, Tk=39, cross=True, ragged=True, seed=11),
    dict(name="d768h12_t64_k20", D=768, H=12, ff=512, L=1, C=140, B=2, T=64, Tk=20, cross=True, ragged=False, seed=12),
    dict(name="d768_t17_nocross", D=768, H=8, ff=2048, L=2, C=140, B=5, T=17, Tk=17, cross=False, ragged=False, seed=13),
    dict(name="d512_l5_t16", D=512, H=8, ff=1024, L=5, C=140, B=2, T=16, Tk=16, cross=True, ragged=False, seed=14),
    dict(name="abi_b40_t16", D=768, H=8, ff=2048, L=4, C=140, B=40, T=16, Tk=16, cross=True, ragged=True, seed=15, abi_eval_only=True),
]


def build_model(c, cdt, dropout=0.0):
    m = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=c["C"], dropout=dropout,
                 mlp_dropout=dropout, use_cross_attention=c["cross"], use_only_rgb=not c["cross"], device="cuda", compute_dtype=cdt).cuda()
    m.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]), strict=True)
    return m


def inputs(c):
    B, T, Tk, D = c["B"], c["T"], c["Tk"], c["D"]
    rgb = synth.normal(c["seed"], "rgb", (B, T, D))
    mot = synth.normal(c["seed"], "mot", (B, Tk, D))
    lens = synth.randint(c["seed"], "lens", (B,), 5, T + 1) if c["ragged"] else torch.full((B,), T, dtype=torch.int64)
    lens[0] = T
    mr = torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)
    mf = torch.arange(Tk).unsqueeze(0) < torch.clamp(lens - (T - Tk), min=1).unsqueeze(1)
    return (rgb * mr.unsqueeze(-1)).cuda(), (mot * mf.unsqueeze(-1)).cuda(), mr.cuda(), mf.cuda()


def run_case(c, cdt, dump=None):
    """One eval forward and (unless the case is eval only) one training step; returns {name: array} of what they computed."""
    rgb, mot, mr, mf = inputs(c)
    out = {}
    m = build_model(c, cdt).eval()
    with torch.no_grad():
        if c.get("abi_eval_only"):       # above tfam_fused.MAX_ROWS AMO_CLIP.forward takes the per-op path: straight through the C ABI
            pack = tfam_fused.get_pack(m, cdt).refresh()
            logits = pack.forward(rgb.contiguous(), mot.contiguous(), mr.to(torch.uint8).contiguous(), mf.to(torch.uint8).contiguous(), True)
            fused_eval = True
        else:
            fused_eval = tfam_fused.supported(m, c["B"], c["T"], c["Tk"] if c["cross"] else 0, c["cross"])
            logits = m(rgb, mot, mask_rgb=mr, mask_flow=mf)
    out["eval/logits"] = logits.float().cpu().numpy()
    fused_train = None
    if not c.get("abi_eval_only"):
        m = build_model(c, cdt, dropout=0.1).train()
        m.set_dropout_seed(11)
        fused_train = tfam_train.supported(m, c["B"], c["T"], c["Tk"] if c["cross"] else 0, c["cross"])
        y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).cuda()
        logits = m(rgb, mot, mask_rgb=mr, mask_flow=mf)
        loss = bce_with_logits_loss(logits, y)
        loss.backward()
        out["train/logits"] = logits.detach().float().cpu().numpy()
        out["train/loss"] = loss.detach().float().cpu().numpy()
        for n, p in m.named_parameters():
            if p.grad is not None:
                out["grad/" + n] = p.grad.detach().float().cpu().numpy()
    torch.cuda.synchronize()
    tag = f"{c['name']}_{'f16' if cdt == torch.float16 else 'bf16'}"
    print(f"{tag}: fused eval {fused_eval}, fused train {fused_train}, {len(out)} arrays, |eval logits| max {np.abs(out['eval/logits']).max():.4f}")
    if dump:
        np.savez(os.path.join(dump, tag + ".npz"), **out)
    return out


def loop(B, iters, cdt):
    c = dict(CASES[0], B=B)
    m = build_model(c, cdt).eval()
    rgb, mot, mr, mf = inputs(c)
    with torch.no_grad():
        for _ in range(iters):
            y = m(rgb, mot, mask_rgb=mr, mask_flow=mf)
    torch.cuda.synchronize()
    print("ok", float(y.abs().max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="DIR", help="write every case's logits and gradients to DIR/<case>_<dtype>.npz")
    ap.add_argument("loop", nargs="*", metavar="B [ITERS] [f16]", help="the reference geometry's eval forward in a loop instead")
    a = ap.parse_args()
    if a.loop:
        loop(int(a.loop[0]), int(a.loop[1]) if len(a.loop) > 1 else 50, torch.float16 if a.loop[2:] == ["f16"] else torch.bfloat16)
        return
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    for c in CASES:
        for cdt in (torch.bfloat16, torch.float16):
            run_case(c, cdt, a.dump)
    print("ok")


if __name__ == "__main__":
    main()
