"""MammalNet student training — the reference's train_frame_diff_mn.py on the MI355X engine: train.train with the MammalNet
dataset (dataset_frame_diff_mn.py: ``trimmed_videos/<id>`` HDF5 layout, bilinear-resized frame-difference frames in [0,1]) and the
single-label loss (CrossEntropy on ``labels.argmax(1)``, no gradient clipping; :82,102,108).  Same argument names as the reference
(its spelling with hyphens is accepted too).  ``--device_resize`` keeps the decoded frames u8, uploads 1 B per source sample and
resizes + quantises them on the GPU (bit-exact with the host path, DESIGN.md "Bilinear resize").
"""
from __future__ import annotations

import argparse
import functools
import os

from .dataset_frame_diff_mn import HDF5VideoDataset, collate_fn, collate_fn_device


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train diff_frame-only student model, MammalNet variant (MI355X engine)")

    def arg(name, **kw):
        p.add_argument("--" + name, "--" + name.replace("_", "-"), dest=name, **kw)

    arg("epochs", type=int, default=10)
    arg("batch_size", type=int, default=32)
    arg("num_workers", type=int, default=4, help="accepted for the reference's command lines; batches are assembled in-process")
    arg("learning_rate", type=float, default=1e-3)
    arg("distillation_loss_mode", default="cosine", choices=["cosine", "mse", "contrastive"],
        help="contrastive: symmetric InfoNCE over all frames of the batch (train.distill_kwargs)")
    arg("distill_temperature", type=float, default=0.07, metavar="T", help="temperature of the contrastive mode's logits")
    arg("num_classes", type=int, default=12)
    arg("sequence_length", type=int, default=30)
    arg("residual_alpha", type=float, default=0.1)
    arg("train_hdf5_path", required=True, help="HDF5 file of teacher embeddings, training split (trimmed_videos/<id>/embeddings, labels)")
    arg("val_hdf5_path", required=True)
    arg("frame_diff_videos_dir", required=True)
    arg("spatial_size", type=int, nargs=2, default=(224, 224), metavar=("H", "W"))
    arg("clip_model_name", default="ViT-B/32")
    arg("checkpoint_dir", default=None)
    arg("recompute", default="none", choices=["none", "block"],
        help="block: keep one residual stream per transformer block and recompute the block in the backward pass")
    arg("accum_steps", type=int, default=1,
        help="gradient accumulation: split every batch along its clips into at most N micro-batches (train.split_micro_batches)")
    arg("compute_dtype", default="bf16", choices=["bf16", "f16"], help="16-bit type of the GEMM and attention operands")
    arg("loss_scale", default="off", metavar="{off,dynamic,<number>}",
        help="loss scaling for float16 gradients, on the device (train.parse_loss_scale): dynamic, or a number for a static scale")
    arg("lora_rank", type=int, default=0, help="train rank-r LoRA adapters and the heads on a frozen tower (train.lora_kwargs); 0 = off")
    arg("lora_alpha", type=float, default=None, help="adapter scale numerator (s = alpha / rank); default 2 rank")
    arg("lora_targets", default="attn", help="attn, mlp or attn+mlp")
    arg("patch_dropout", type=float, default=0.0, metavar="P",
        help="training only: keep the class token and max(1, int(g^2 (1 - P))) random patch tokens per frame (train.patch_dropout_kwargs); "
             "0 = off")
    arg("ema_decay", type=float, default=None, metavar="D",
        help="evaluate and write the best checkpoint with an exponential moving average of the weights (train.ema_kwargs); default off")
    arg("ema_no_warmup", action="store_true", help="with --ema_decay: the constant decay from the first step on")
    arg("drop_path", type=float, default=0.0, metavar="P",
        help="training only: stochastic depth per frame, block l of L runs on max(1, int(F (1 - P l / (L - 1)))) random frames "
             "(train.drop_path_kwargs); 0 = off")
    arg("device_resize", action="store_true", help="upload decoded u8 frames and resize them on the GPU (collate_fn_device)")
    return p


def train(args):
    from . import train as student_train
    student_train.parse_loss_scale(args.loss_scale)         # a malformed value fails before any file is opened
    if not 0.0 <= args.patch_dropout < 1.0:
        raise ValueError(f"--patch_dropout must satisfy 0 <= p < 1, got {args.patch_dropout}")
    if not 0.0 <= args.drop_path < 1.0:
        raise ValueError(f"--drop_path must satisfy 0 <= p < 1, got {args.drop_path}")
    student_train.ema_kwargs(args)                           # --ema_decay outside (0, 1) fails here too
    student_train.distill_kwargs(args)                       # and so does a temperature that is not positive
    size = tuple(args.spatial_size)
    sets = tuple(HDF5VideoDataset(path, args.frame_diff_videos_dir, sequence_length=args.sequence_length, spatial_size=size,
                                  raw_u8=args.device_resize) for path in (args.train_hdf5_path, args.val_hdf5_path))
    args.single_label, args.class_positive_weight, args.grad_clip_norm = True, 1, None
    if not args.device_resize:
        return student_train.train(args, datasets=sets, collate=collate_fn)
    device = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"          # the device train.train gives this rank
    collate = functools.partial(collate_fn_device, spatial_size=size, device=device)
    return student_train.train(args, datasets=sets, collate=collate, forward_kwargs={"unit_u8": True})


if __name__ == "__main__":
    train(build_parser().parse_args())
