#!/usr/bin/env python3
"""Where the student's upstream gradients sit in the float16 range (DESIGN.md "Dynamic loss scaling"): CPU only, fp32 oracle.

oracle.student.student_forward on ViT-B/32 with synth.student_state_dict("ViT-B/32", 7), 2 clips x 4 random u8 frames, cosine
distillation + BCE with pw 9.  Tensor hooks record the gradient of the residual stream wherever it enters a LayerNorm (the dY of the
preceding out_proj / c_proj) and of the c_fc pre-activation (the dY of c_fc); for both, as they are (8 frames) and times 1/64 (what the
mean-reduced losses give at 512 frames): the median magnitude, the share below 2^-14 (float16 subnormal) and below 2^-25 (rounds to 0).

python tools/loss_scale_census.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from oracle import student as ostudent
    from oracle import vit as ovit
    from vimo_clip_amd import synth
    name, B, T = "ViT-B/32", 2, 4
    R, H, E = synth.VIT_GEOMETRY[name][0], synth.VIT_GEOMETRY[name][4], synth.VIT_GEOMETRY[name][5]
    sd = {k: v.clone().requires_grad_(True) for k, v in synth.student_state_dict(name, 7).items()}
    grads = {"residual dY": [], "c_fc dY": []}
    ln, gelu = ovit.layer_norm, ovit.quick_gelu

    def spy(fn, key):
        def wrapped(x, *a, **k):
            if x.requires_grad:
                x.register_hook(lambda g: grads[key].append(g.detach().abs().reshape(-1)))
            return fn(x, *a, **k)
        return wrapped
    ovit.layer_norm, ovit.quick_gelu = spy(ln, "residual dY"), spy(gelu, "c_fc dY")
    try:
        vids = synth.randint_u8(7, "vids", (B, T, 3, R, R))
        teacher, labels = synth.normal(7, "teacher", (B, T + 1, E)), synth.multi_hot_labels(7, "labels", B, 140)
        _, emb_d, logits = ostudent.student_forward(sd, vids, H, alpha=0.1, wrap_quirk=True)
        (ostudent.distillation_loss(emb_d, teacher[:, :-1, :], "cosine") + ostudent.classification_loss(logits, labels, 9)).backward()
    finally:
        ovit.layer_norm, ovit.quick_gelu = ln, gelu
    print("| tensor | batch | median \\|g\\| | below 2^-14 | below 2^-25 |\n|---|---|---|---|---|")
    for key, parts in grads.items():
        g = torch.cat(parts).double()
        for tag, f in (("8 frames", 1.0), ("x 1/64", 1.0 / 64)):
            x = g * f
            print(f"| {key} | {tag} | {x.median().item():.1e} | {100 * (x < 2.0 ** -14).double().mean().item():.2f} % | "
                  f"{100 * (x < 2.0 ** -25).double().mean().item():.2f} % |")


if __name__ == "__main__":
    main()
