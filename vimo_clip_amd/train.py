"""MoCLIP student training loop on the MI355X engine — the hot loop of the reference's train.py (train :52-175,
evaluate :14-49) with the same argument names, one process per GPU under torchrun instead of nn.DataParallel (:64).
``--clip_embeddings_dir`` / ``--flow_videos_dir`` read the reference's HDF5 + video layout (HDF5 natively through
h5lite; decoded ``.npy`` frame stacks when no video decoder is installed); ``--synthetic N`` trains on N synthetic
segments.  ``--single_label`` is the MammalNet variant (train_frame_diff_mn.py:82,102: CrossEntropy on
``labels.argmax(dim=1)``, no gradient clipping); ``--motion_key frame_diff`` the frame-difference twin
(train_frame_diff.py: batch key ``frame_diff`` instead of ``flow_frames``).  ``--accum_steps N`` (not in the reference) runs every
batch as up to N micro-batches whose gradients are summed in the arena (optim.GradArena.accumulate); 1 is the loop as it was.
``--compute_dtype f16`` trains in float16 and ``--loss_scale dynamic|<number>`` (neither in the reference) keeps its gradients in
range: the optimiser moves to device-state mode and scales, checks and skips on the device (optim.FusedAdam.enable_loss_scaling).
``--ema_decay D`` (not in the reference) keeps an exponential moving average of the trained weights on the device
(optim.FusedAdam.enable_ema): validation and ``student_best.pth`` use the average, the per-epoch files the live weights.
``--distillation_loss_mode contrastive`` (not in the reference) replaces the frame-by-frame distillation loss by the symmetric InfoNCE
loss over all frames of the batch (losses.distillation_loss) at ``--distill_temperature``; the epoch line gains
``val_top1``.  Its negatives are the other clips of whatever one call sees: a micro-batch under ``--accum_steps``, a rank's shard
under torchrun.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import time
import warnings

import torch

from . import parallel
from .dataset import SyntheticSegmentDataset, collate_fn
from .losses import classification_loss, cross_entropy_loss, distillation_loss
from .models.student_model import FlowStudentModel
from .optim import FusedAdam, GradArena
from .synth import vit_geometry


def embed_dim(clip_model_name: str) -> int:
    """Width of the teacher / student embeddings: the tower's output_dim (KeyError for an unknown name)."""
    return vit_geometry(clip_model_name)[5]


def _batches(ds, batch_size, rank, world, collate=collate_fn):
    lo, hi = parallel.shard_range(len(ds), rank, world)
    for s in range(lo, hi - batch_size + 1, batch_size):
        yield collate([ds[i] for i in range(s, s + batch_size)])


def _frames(batch):
    return batch["flow_frames"] if "flow_frames" in batch else batch["frame_diff"]


def split_micro_batches(batch, n):
    """Split a collated batch along its clips into at most ``n`` micro-batches for gradient accumulation: [(sub_batch, weight)].
    Chunk sizes are ``torch.chunk``'s (ceil(B / n) clips each, the last one smaller, fewer than n chunks when B does not stretch);
    tensors are split as views, per-clip lists (``video_id``) are sliced alike, anything else is passed to every chunk.  weight =
    chunk clips / batch clips: the student's losses are means over rows and, the contrastive distillation mode apart, no operator
    couples the clips of a batch, so the weighted sum of the micro-batch gradients is the batch's gradient.  (In the contrastive mode
    every micro-batch draws its negatives from its own clips: the sum is a gradient, but not the batch's; `train` warns.)  n = 1
    returns the batch itself with weight 1."""
    n = int(n)
    if n < 1:
        raise ValueError(f"split_micro_batches: n must be at least 1, got {n}")
    if n == 1:
        return [(batch, 1.0)]
    B = int(batch["labels"].shape[0])
    per = -(-B // n)
    bounds = [(s, min(B, s + per)) for s in range(0, B, per)]
    out = []
    for lo, hi in bounds:
        sub = {}
        for k, v in batch.items():
            if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B:
                sub[k] = v[lo:hi]
            elif isinstance(v, (list, tuple)) and len(v) == B:
                sub[k] = v[lo:hi]
            else:
                sub[k] = v
        out.append((sub, (hi - lo) / B))
    return out


COMPUTE_DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def parse_loss_scale(text):
    """``--loss_scale`` -> None ("off"), or the keyword arguments of ``FusedAdam.enable_loss_scaling``: "dynamic" = GradScaler's
    defaults (2^16, x2 after 2000 clean steps, x0.5 after an overflow); a number = that scale, static (growth = backoff = 1; an
    overflowing step is still skipped).  Anything else raises ValueError."""
    text = str(text).strip().lower()
    if text == "off":
        return None
    if text == "dynamic":
        return {}
    try:
        scale = float(text)
    except ValueError:
        raise ValueError(f"--loss_scale must be off, dynamic or a positive number, got {text!r}") from None
    if not (scale > 0.0 and scale < float("inf")):
        raise ValueError(f"--loss_scale must be off, dynamic or a positive number, got {text!r}")
    return {"init_scale": scale, "growth_factor": 1.0, "backoff_factor": 1.0}


def _loss_scale_arg(text):
    try:
        parse_loss_scale(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return str(text).strip().lower()


def lora_kwargs(args) -> dict:
    """``--lora_rank / --lora_alpha / --lora_targets`` -> FlowStudentModel's keyword arguments; rank 0 (the default): none at all,
    the model is built exactly as before."""
    rank = int(getattr(args, "lora_rank", 0) or 0)
    if rank == 0:
        return {}
    targets = getattr(args, "lora_targets", "attn")
    targets = tuple(t for t in targets.replace("+", ",").split(",") if t) if isinstance(targets, str) else tuple(targets)
    return {"lora_rank": rank, "lora_alpha": getattr(args, "lora_alpha", None), "lora_targets": targets}


def _patch_dropout_arg(text):
    """``--patch_dropout`` values: a drop fraction 0 <= p < 1."""
    try:
        p = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--patch_dropout needs a number, got {text!r}") from None
    if not 0.0 <= p < 1.0:
        raise argparse.ArgumentTypeError(f"--patch_dropout must satisfy 0 <= p < 1, got {text!r}")
    return p


PATCH_DROPOUT_SEED = 0x5EED0D07      # base of the keep-set streams of a training run; rank r draws from base + r


def patch_dropout_kwargs(args, rank: int = 0) -> dict:
    """``--patch_dropout P`` -> FlowStudentModel's keyword arguments; 0 (the default): none at all, the model is built exactly as before.
    Every data-parallel rank draws from a stream of its own (the seed base is offset by the rank): ranks see different frames."""
    p = float(getattr(args, "patch_dropout", 0.0) or 0.0)
    if p == 0.0:
        return {}
    return {"patch_dropout": p, "patch_dropout_seed": PATCH_DROPOUT_SEED + int(rank)}


def _ema_decay_arg(text):
    """``--ema_decay`` values: a decay 0 < D < 1."""
    try:
        d = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--ema_decay needs a number, got {text!r}") from None
    if not 0.0 < d < 1.0:
        raise argparse.ArgumentTypeError(f"--ema_decay must satisfy 0 < D < 1, got {text!r}")
    return d


def ema_kwargs(args):
    """``--ema_decay D [--ema_no_warmup]`` -> the keyword arguments of ``FusedAdam.enable_ema``; None (the default): the average is
    off and the loop is the one it was."""
    decay = getattr(args, "ema_decay", None)
    if decay is None:
        return None
    if not 0.0 < float(decay) < 1.0:
        raise ValueError(f"--ema_decay must satisfy 0 < D < 1, got {decay}")
    return {"decay": float(decay), "warmup": not getattr(args, "ema_no_warmup", False)}


def _drop_path_arg(text):
    """``--drop_path`` values: a drop rate 0 <= p < 1."""
    try:
        p = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--drop_path needs a number, got {text!r}") from None
    if not 0.0 <= p < 1.0:
        raise argparse.ArgumentTypeError(f"--drop_path must satisfy 0 <= p < 1, got {text!r}")
    return p


DROP_PATH_SEED = 0x5EED0D9A      # base of the frame-draw streams of a training run; rank r draws from base + r


def drop_path_kwargs(args, rank: int = 0) -> dict:
    """``--drop_path P`` -> FlowStudentModel's keyword arguments; 0 (the default): none at all, the model is built exactly as before.
    Every data-parallel rank draws from a stream of its own (the seed base is offset by the rank): ranks see different frames."""
    p = float(getattr(args, "drop_path", 0.0) or 0.0)
    if p == 0.0:
        return {}
    return {"drop_path": p, "drop_path_seed": DROP_PATH_SEED + int(rank)}


def distill_kwargs(args) -> dict:
    """``--distillation_loss_mode contrastive [--distill_temperature T]`` -> the keyword arguments of ``distillation_loss`` beside the
    mode: the temperature, and ``--compute_dtype`` for the logits' operands.  Any other mode: none at all, the call is the one it was."""
    if getattr(args, "distillation_loss_mode", "cosine") != "contrastive":
        return {}
    tau = float(getattr(args, "distill_temperature", 0.07))
    if not tau > 0.0:
        raise ValueError(f"--distill_temperature must be positive, got {tau}")
    return {"temperature": tau, "compute_dtype": COMPUTE_DTYPES[getattr(args, "compute_dtype", "bf16")]}


def save_best(model, path: str) -> None:
    """The best-so-far checkpoint.  With live adapters it is written MERGED (lora.merged_state_dict: W + s B A, the reference's keys),
    so that it loads into the reference and runs the inference path; the per-epoch files keep the adapters as they are.  With
    ``--ema_decay`` the trainer calls it inside ``FusedAdam.ema_weights()``: the file then holds the averaged weights that were just
    evaluated (merged from the averaged adapters)."""
    from .checkpoint import add_prefix, save_state_dict
    if getattr(model.visual_encoder, "lora", None) is None:
        return save_state_dict(model, path)
    import os

    from .lora import merged_state_dict
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save(add_prefix({k: v.to("cpu") for k, v in merged_state_dict(model).items()}), path)


def _class_loss(logits, labels, class_positive_weight, single_label):
    if single_label:                                   # train_frame_diff_mn.py:102
        return cross_entropy_loss(logits, labels.argmax(dim=1))
    return classification_loss(logits, labels, positive_weight=class_positive_weight)


def evaluate(model, val_set, device, distillation_loss_mode, class_positive_weight, batch_size, rank=0, world=1, single_label=False,
             collate=collate_fn, forward_kwargs=None, distill_kwargs=None, metrics=None):
    """(distillation, classification, total) validation loss, means over the batches.  distill_kwargs: `distill_kwargs(args)`;
    metrics: a dict that receives ``val_top1`` -- the mean over the batches of the share of frames whose own teacher frame has the
    largest logit in the batch -- in the contrastive mode, and nothing in any other."""
    model.eval()
    contrastive = distillation_loss_mode == "contrastive"
    tot = torch.zeros(4, device=device)
    top1 = torch.zeros(1, device=device)
    with torch.no_grad():
        for batch in _batches(val_set, batch_size, rank, world, collate):
            _, emb_d, logits = model(_frames(batch).to(device), **(forward_kwargs or {}))
            dl = distillation_loss(emb_d, batch["rgb_emb"].to(device)[:, :-1, :], mode=distillation_loss_mode, **(distill_kwargs or {}),
                                   **({"return_top1": True} if contrastive else {}))
            if contrastive:
                dl, frac = dl
                top1 += frac
            cl = _class_loss(logits, batch["labels"].to(device), class_positive_weight, single_label)
            tot += torch.stack([dl, cl, dl + cl, torch.ones((), device=device)])
    tot = parallel.all_reduce_scalars(tot)
    n = max(1.0, float(tot[3]))
    if contrastive and metrics is not None:
        metrics["val_top1"] = float(parallel.all_reduce_scalars(top1)[0]) / n
    return float(tot[0]) / n, float(tot[1]) / n, float(tot[2]) / n


def train(args, datasets=None, collate=collate_fn, forward_kwargs=None):
    """datasets: a (train_set, val_set) pair built by the caller instead of the ones the arguments name; collate: its collate function,
    called with the list of samples (a device-side one is bound to its device by the caller); forward_kwargs: keyword arguments of
    every model call (train_frame_diff_mn.py passes ``unit_u8=True`` with its device-side collate)."""
    accum = int(getattr(args, "accum_steps", 1))
    if accum < 1:                                           # before anything touches the device
        raise ValueError(f"--accum_steps must be at least 1, got {accum}")
    ema = ema_kwargs(args)
    dkw = distill_kwargs(args)                               # a temperature that is not positive fails here
    rank, world, local = parallel.init_from_env()
    if dkw and (accum > 1 or world > 1):
        warnings.warn("contrastive distillation draws its negatives from the clips of one call: with --accum_steps > 1 or more than one "
                      "rank they come from the micro-batch or the rank's shard alone, and the summed gradient is not the gradient of "
                      "the whole batch's contrastive loss", stacklevel=2)
    device = f"cuda:{local}"
    E = embed_dim(args.clip_model_name)
    single = bool(getattr(args, "single_label", False))
    forward_kwargs = forward_kwargs or {}
    if datasets is not None:
        train_set, val_set = datasets
    elif getattr(args, "clip_embeddings_dir", None):
        from .dataset import HDF5VideoDataset
        train_set = HDF5VideoDataset(args.clip_embeddings_dir, args.flow_videos_dir, sequence_length=args.sequence_length)
        val_set = HDF5VideoDataset(args.val_clip_embeddings_dir or args.clip_embeddings_dir, args.val_flow_videos_dir or args.flow_videos_dir,
                                   sequence_length=args.sequence_length)
    else:
        train_set = SyntheticSegmentDataset(args.synthetic, args.sequence_length, E, args.num_classes, seed=3)
        val_set = SyntheticSegmentDataset(max(args.batch_size * world, args.synthetic // 8), args.sequence_length, E, args.num_classes, seed=4)
    dtype_name = getattr(args, "compute_dtype", "bf16")
    model = FlowStudentModel(clip_model_name=args.clip_model_name, device=device, num_classes=args.num_classes, alpha=args.residual_alpha,
                             recompute=getattr(args, "recompute", "none"),
                             **({} if dtype_name == "bf16" else {"compute_dtype": COMPUTE_DTYPES[dtype_name]}), **lora_kwargs(args),
                             **patch_dropout_kwargs(args, rank), **drop_path_kwargs(args, rank))
    arena = GradArena(model.parameters())
    parallel.broadcast_parameters(arena.flat_param)
    if world > 1:                                          # a frozen tower (LoRA) is outside the arena: it starts from rank 0's too
        for p in model.parameters():
            if not p.requires_grad:
                parallel.broadcast_parameters(p.data)
    optimizer = FusedAdam(arena, lr=args.learning_rate)
    reducer = parallel.GradientAllReducer(arena.flat_grad).attach(arena)     # buckets go out during the backward
    clip_norm = None if single else args.grad_clip_norm
    scaling = parse_loss_scale(getattr(args, "loss_scale", "off"))
    if scaling is not None:                                # the scaler lives in device memory: device-state mode, tick() per step
        optimizer.enable_device_state().enable_loss_scaling(**scaling)
    if ema is not None:                                    # an fp32 average of the arena, updated behind every step on the device
        optimizer.enable_ema(**ema)
    averaged = optimizer.ema_weights if ema is not None else contextlib.nullcontext      # what is evaluated and written as the best

    def micro_loss(batch):
        emb, emb_d, logits = model(_frames(batch).to(device), **forward_kwargs)
        dl = distillation_loss(emb_d, batch["rgb_emb"].to(device)[:, :-1, :], mode=args.distillation_loss_mode, **dkw)
        return dl + _class_loss(logits, batch["labels"].to(device), args.class_positive_weight, single)
    best = float("inf")
    ckpt_dir = getattr(args, "checkpoint_dir", None)       # reference: checkpoints/<run timestamp> (train.py:69-74)
    for epoch in range(args.epochs):
        model.train()
        t0, nframes = time.time(), 0
        loss_sum, nsteps = (torch.zeros((), device=device) if accum > 1 else None), 0
        for batch in _batches(train_set, args.batch_size, rank, world, collate):
            frames = _frames(batch)
            if scaling is not None:
                optimizer.tick()
            if accum > 1:
                # every chunk is uploaded, run and back-propagated on its own; only the last one exchanges and steps.  The exchange
                # is not overlapped with the last backward (it needs the finalised sum): one exchange per optimiser step
                micro = split_micro_batches(batch, accum)
                step_loss = torch.zeros((), device=device)
                for j, (sub, w) in enumerate(micro):
                    with reducer.no_sync():
                        loss = micro_loss(sub)                  # the unscaled loss: what is logged
                        optimizer.scale_loss(loss).backward()   # scaling off: loss itself
                    arena.accumulate(w, final=j == len(micro) - 1)
                    step_loss += w * loss.detach()
                optimizer.step(grad_scale=reducer.all_reduce(), max_grad_norm=clip_norm)
                loss_sum += step_loss
                nsteps += 1
                nframes += frames.shape[0] * frames.shape[1]
                continue
            emb, emb_d, logits = model(frames.to(device), **forward_kwargs)
            dl = distillation_loss(emb_d, batch["rgb_emb"].to(device)[:, :-1, :], mode=args.distillation_loss_mode, **dkw)
            cl = _class_loss(logits, batch["labels"].to(device), args.class_positive_weight, single)
            optimizer.scale_loss(dl + cl).backward()
            optimizer.step(grad_scale=reducer.all_reduce(), max_grad_norm=None if single else args.grad_clip_norm)
            nframes += frames.shape[0] * frames.shape[1]
        torch.cuda.synchronize()
        if rank == 0 and ckpt_dir:                          # train.py:164-172: every epoch (the live weights) + the best-so-far copy
            from .checkpoint import save_state_dict
            save_state_dict(model, f"{ckpt_dir}/student_epoch_{epoch + 1}.pth")
        extra = {}
        with averaged():
            vd, vc, vt = evaluate(model, val_set, device, args.distillation_loss_mode, args.class_positive_weight, args.batch_size, rank, world,
                                  single, collate, forward_kwargs, **({"distill_kwargs": dkw, "metrics": extra} if dkw else {}))
            if rank == 0 and ckpt_dir and vt < best:
                save_best(model, f"{ckpt_dir} - best/student_best.pth")
        best = min(best, vt)
        if rank == 0:
            line = {"epoch": epoch + 1, "val_distill": vd, "val_class": vc, "val_total": vt,
                    "train_frames_per_s_all_gpus": round(nframes * world / (time.time() - t0), 1)}
            if accum > 1:                                   # mean over the epoch's steps of the weighted sum of the micro-batch losses
                line["train_total"] = float(loss_sum) / max(1, nsteps)
            if scaling is not None:                         # one small read where the loop has already synchronised
                rec = optimizer.dev_ls.cpu()
                line["loss_scale"], line["skipped_steps"] = float(rec.view(torch.float32)[0]), int(rec[7])
            if ema is not None:                             # the validation figures are those of the averaged weights
                line["ema"] = True
            line.update(extra)                              # val_top1, in the contrastive mode only
            print(json.dumps(line), flush=True)
    return best


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train flow-only student model (MI355X engine)")
    p.add_argument("--synthetic", type=int, default=256)
    p.add_argument("--clip_model_name", default="ViT-B/32")
    p.add_argument("--num_classes", type=int, default=140)
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--sequence_length", type=int, default=17)
    p.add_argument("--epochs", type=int, default=1)
    p.add_argument("--learning_rate", type=float, default=1e-3)
    p.add_argument("--distillation_loss_mode", default="cosine", help="cosine or mse as in the reference; contrastive: symmetric InfoNCE over "
                   "all frames of the batch, the other frames of a frame's own clip masked out as negatives")
    # absent unless given (distill_kwargs reads it with its default), like the other options the reference does not have
    p.add_argument("--distill_temperature", type=float, default=argparse.SUPPRESS, metavar="T",
                   help="temperature of the contrastive mode's logits cos(student_i, teacher_j) / T; default 0.07")
    p.add_argument("--class_positive_weight", type=int, default=9)
    p.add_argument("--residual_alpha", type=float, default=0.1)
    p.add_argument("--grad_clip_norm", type=float, default=None)
    p.add_argument("--checkpoint_dir", default=None, help="write student_epoch_N.pth here and student_best.pth into '<dir> - best' "
                                                           "(the reference uses checkpoints/<timestamp>); omitted = no files")
    p.add_argument("--recompute", default="none", choices=["none", "block"],
                   help="block: keep one residual stream per transformer block and recompute the block in the backward pass")
    p.add_argument("--accum_steps", type=int, default=1,
                   help="gradient accumulation: split every batch along its clips into at most N micro-batches that are run and "
                        "back-propagated one after the other; one gradient exchange and one optimiser step per batch")
    p.add_argument("--compute_dtype", default="bf16", choices=list(COMPUTE_DTYPES), help="16-bit type of the GEMM and attention operands")
    p.add_argument("--loss_scale", default="off", type=_loss_scale_arg, metavar="{off,dynamic,<number>}",
                   help="loss scaling for float16 gradients, on the device: dynamic = GradScaler's defaults; a number = a static "
                        "scale; an overflowing step is skipped either way")
    # absent unless given (lora_kwargs reads them with defaults): the namespace of a run without adapters is the one it always was
    p.add_argument("--lora_rank", type=int, default=argparse.SUPPRESS,
                   help="parameter-efficient fine-tuning: freeze the tower and train rank-r adapters (a multiple of 8, at most 64) plus "
                        "the two heads; default 0 = full fine-tuning, the loop as it was")
    p.add_argument("--lora_alpha", type=float, default=argparse.SUPPRESS, help="adapter scale numerator (s = alpha / rank); default 2 rank")
    p.add_argument("--lora_targets", default=argparse.SUPPRESS, help="attn (default), mlp or attn+mlp: which linears of every block carry adapters")
    p.add_argument("--patch_dropout", type=_patch_dropout_arg, default=argparse.SUPPRESS, metavar="P",
                   help="training only: every frame keeps its class token and max(1, int(g^2 (1 - P))) randomly drawn patch tokens, the "
                        "tower runs on those rows; evaluation sees every token; default 0 = nothing is dropped")
    p.add_argument("--ema_decay", type=_ema_decay_arg, default=argparse.SUPPRESS, metavar="D",
                   help="keep an exponential moving average of the trained weights on the device (decay D, e.g. 0.9999); validation runs "
                        "on it and student_best.pth holds it; the per-epoch files keep the live weights; default off")
    p.add_argument("--ema_no_warmup", action="store_true", default=argparse.SUPPRESS,
                   help="with --ema_decay: the constant decay from the first step on, instead of min(D, (1 + t) / (10 + t))")
    p.add_argument("--drop_path", type=_drop_path_arg, default=argparse.SUPPRESS, metavar="P",
                   help="training only: stochastic depth per frame; residual block l of L runs on max(1, int(F (1 - P l / (L - 1)))) randomly "
                        "drawn frames of a forward and the others skip it; evaluation runs every block on every frame; default 0 = off")
    p.add_argument("--single_label", action="store_true", help="MammalNet variant: CrossEntropy on labels.argmax(1)")
    p.add_argument("--clip_embeddings_dir", default=None, help="HDF5 file of teacher embeddings (reference layout)")
    p.add_argument("--flow_videos_dir", default=None)
    p.add_argument("--val_clip_embeddings_dir", default=None)
    p.add_argument("--val_flow_videos_dir", default=None)
    return p


if __name__ == "__main__":
    train(build_parser().parse_args())
