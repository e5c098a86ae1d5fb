"""Student losses on libvmc kernels — same names, arguments and error behaviour as the reference's
losses.py (distillation_loss :5-44, classification_loss :47-67, reconstruction_loss :70-81).

Each loss is ONE fused forward pass that also produces the gradient (K10); the autograd backward only
scales that gradient by the incoming scalar.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import autograd_ops as ag
from . import ops
from ._lib import check, dt, lib, ptr, stream


class _DistillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, cosine):
        if student.shape != teacher.shape:
            raise RuntimeError(f"distillation_loss: shape mismatch {tuple(student.shape)} vs {tuple(teacher.shape)}")
        E = student.shape[-1]
        rows = student.numel() // E
        s = student.contiguous().float()
        # teacher may be the strided slice rgb_emb[:, :-1] of train.py:98: rows_per_clip rows out of a longer clip
        if teacher.dtype == torch.float32 and teacher.dim() == 3 and teacher.stride(-1) == 1 and teacher.stride(1) == E:
            t = teacher                                 # strided view read in place: strides of the tensor the kernel gets
            rows_per_clip, clip_stride = t.shape[1], t.stride(0)
        else:                                           # other dtypes (f16 / f64 stores): a dense fp32 copy, dense strides
            t = teacher.contiguous().float()
            rows_per_clip, clip_stride = rows, rows * E
        loss = torch.empty((), dtype=torch.float32, device=s.device)
        ds = torch.empty_like(s) if student.requires_grad else None
        nbytes = lib.vmc_loss_workspace_bytes(rows)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=s.device)
        check(lib.vmc_distill_loss(ptr(s), ptr(t), ptr(loss), ptr(ds), rows, E, rows_per_clip, clip_stride, int(cosine),
                                   ptr(ws), nbytes, stream()), "distill_loss")
        ctx.save_for_backward(ds)
        ctx.shape = student.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (ds,) = ctx.saved_tensors
        return ag.scale_by_device_scalar(ds, g).view(ctx.shape), None, None


CONTRASTIVE_MAX_ROWS = 16384


def _contrastive_check(student, teacher, temperature, compute_dtype):
    """The argument errors of the contrastive mode, before anything is launched; returns (rows, E)."""
    if not float(temperature) > 0.0:                        # nan fails too
        raise ValueError(f"distillation_loss: temperature must be positive, got {temperature}")
    if compute_dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"distillation_loss: compute_dtype must be torch.bfloat16 or torch.float16, got {compute_dtype}")
    if student.shape != teacher.shape:
        raise RuntimeError(f"distillation_loss: shape mismatch {tuple(student.shape)} vs {tuple(teacher.shape)}")
    if student.dim() not in (2, 3):
        raise ValueError(f"distillation_loss: contrastive mode expects [B, T, E] or [M, E], got {tuple(student.shape)}")
    E = student.shape[-1]
    rows = student.numel() // E if E else 0
    if E < 64 or E % 64 != 0:
        raise ValueError(f"distillation_loss: contrastive mode needs an embedding width that is a multiple of 64, got {E}")
    if not 1 <= rows <= CONTRASTIVE_MAX_ROWS:
        raise ValueError(f"distillation_loss: contrastive mode takes 1 to {CONTRASTIVE_MAX_ROWS} rows (frames) per call, got {rows}")
    return rows, E


class _ContrastiveFn(torch.autograd.Function):
    """Symmetric InfoNCE over the in-batch similarity matrix: prep, the logits GEMM, the masked softmax pass and --
    only when the student needs a gradient -- the gradient GEMM and the backward of the normalisation, all on the caller's stream
    with shape constants for arguments."""

    @staticmethod
    def forward(ctx, student, teacher, temperature, compute_dtype, mask_same_clip, need_grad):
        M, E = _contrastive_check(student, teacher, temperature, compute_dtype)
        clip_rows = student.shape[1] if student.dim() == 3 else 1
        s = student.contiguous().float()
        if teacher.dtype == torch.float32 and teacher.dim() == 3 and teacher.stride(-1) == 1 and teacher.stride(1) == E:
            t = teacher                                     # the strided rgb_emb[:, :-1] view, read in place
            rows_per_clip, clip_stride = t.shape[1], t.stride(0)
        else:
            t = teacher.contiguous().float()
            rows_per_clip, clip_stride = M, M * E
        dev, d16, st = s.device, dt(compute_dtype), stream()
        Mp = (M + 63) // 64 * 64
        off = (ctypes.c_size_t * 9)()
        check(lib.vmc_contrastive_workspace_layout(M, E, ctypes.addressof(off)), "contrastive_workspace_layout")
        ws = torch.empty(off[8], dtype=torch.uint8, device=dev)

        def part(i, dtype, *shape):
            return ws[off[i]:off[i + 1]].view(dtype)[:math.prod(shape)].view(*shape)
        u16, v16, vt16 = part(0, compute_dtype, Mp, E), part(1, compute_dtype, Mp, E), part(2, compute_dtype, E, Mp)
        z, dz16 = part(3, torch.float32, M, Mp), part(4, compute_dtype, M, Mp)
        lse_row, lse_col = part(5, torch.float32, M), part(6, torch.float32, M)
        partials = ws[off[7]:off[8]]
        inv_s = torch.empty(M, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        top1 = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.vmc_contrastive_prep(ptr(s), ptr(t), ptr(u16), ptr(v16), ptr(vt16), ptr(inv_s), M, E, rows_per_clip, clip_stride, d16, st),
              "contrastive_prep")
        ops.linear(u16[:M], v16, alpha=1.0 / temperature, out=z)                     # z = u16 v16^T / tau, K = E, N = Mp
        check(lib.vmc_contrastive_softmax(ptr(z), M, Mp, clip_rows if mask_same_clip else 0, ptr(lse_row), ptr(lse_col), ptr(loss),
                                          ptr(top1), ptr(dz16) if need_grad else None, d16, ptr(partials), partials.numel(), st),
              "contrastive_softmax")
        ds = None
        if need_grad:
            ds = torch.empty_like(s)
            ops.linear(dz16, vt16, alpha=1.0 / (2.0 * M * temperature), out=ds.view(M, E))      # du = dz16 v16 / (2 M tau), K = Mp
            check(lib.vmc_contrastive_norm_bwd(ptr(ds), ptr(s), ptr(inv_s), ptr(ds), M, E, st), "contrastive_norm_bwd")      # in place
        ctx.save_for_backward(ds)
        ctx.shape = student.shape
        ctx.mark_non_differentiable(top1)
        return loss, top1

    @staticmethod
    def backward(ctx, g, _g_top1):
        (ds,) = ctx.saved_tensors
        return ag.scale_by_device_scalar(ds, g).view(ctx.shape), None, None, None, None, None


def distillation_loss(student_embeddings, teacher_embeddings, mode="mse", *, temperature=0.07, compute_dtype=torch.bfloat16,
                      mask_same_clip=True, return_top1=False):
    """losses.py:5-44.  mode 'mse' or 'cosine' (safe cosine with eps clamps) as in the reference; anything else but 'contrastive'
    raises ValueError.

    mode 'contrastive' (not in the reference) is the symmetric InfoNCE loss over the similarity matrix of all frames of the batch,
    logits = cos(student_i, teacher_j) / temperature on operands rounded to ``compute_dtype``, with the other frames of a frame's own
    clip masked out as negatives (``mask_same_clip``; a 2-D input makes every row its own clip).  ``return_top1=True`` returns
    ``(loss, top1_fraction)``, the share of frames whose own teacher frame has the largest logit, a one-element device tensor.  The
    keywords are accepted and ignored by the other two modes."""
    if mode == "contrastive":
        _contrastive_check(student_embeddings, teacher_embeddings, temperature, compute_dtype)
        need_grad = torch.is_grad_enabled() and student_embeddings.requires_grad      # evaluation: the gradient half is not launched
        loss, top1 = _ContrastiveFn.apply(student_embeddings, teacher_embeddings, float(temperature), compute_dtype, bool(mask_same_clip),
                                          need_grad)
        if return_top1:
            return loss, top1.to(torch.float32) / float(student_embeddings.numel() // student_embeddings.shape[-1])
        return loss
    if mode not in ("mse", "cosine"):
        raise ValueError(f"Unsupported mode '{mode}'. Choose 'mse' or 'cosine'.")
    return _DistillFn.apply(student_embeddings, teacher_embeddings, mode == "cosine")


class _BceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, pw):
        x = logits.contiguous().float()
        y = targets.contiguous().float()
        if x.shape != y.shape:
            raise ValueError(f"Target size ({tuple(y.shape)}) must be the same as input size ({tuple(x.shape)})")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if logits.requires_grad else None
        ws = torch.empty(64, dtype=torch.float32, device=x.device)
        check(lib.vmc_bce_loss(ptr(x), ptr(y), ptr(loss), ptr(dx), x.numel(), float(pw), ptr(ws), 256, stream()), "bce_loss")
        ctx.save_for_backward(dx)
        ctx.shape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return ag.scale_by_device_scalar(dx, g).view(ctx.shape), None, None


def classification_loss(predictions, targets, positive_weight=None):
    """losses.py:47-67: BCE-with-logits, per-element pos_weight = positive_weight * targets + 1 (so the
    effective positive weight is positive_weight + 1), mean over all elements."""
    return _BceFn.apply(predictions, targets, -1.0 if positive_weight is None else float(positive_weight))


def bce_with_logits_loss(predictions, targets):
    """nn.BCEWithLogitsLoss() as used by TFAM/train_and_eval.py:58."""
    return _BceFn.apply(predictions, targets, -1.0)


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        x = logits.contiguous().float()
        if x.dim() != 2:
            raise ValueError(f"cross_entropy_loss expects [rows, classes] logits, got {tuple(x.shape)}")
        rows, C = x.shape
        if target.is_floating_point():
            if target.shape != x.shape:
                raise ValueError(f"probability targets must have the logits' shape {tuple(x.shape)}, got {tuple(target.shape)}")
            tidx, tprob = None, target.contiguous().float()
        else:
            if target.shape != (rows,):
                raise ValueError(f"index targets must have shape ({rows},), got {tuple(target.shape)}")
            tidx, tprob = target.contiguous().to(torch.int64), None
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if logits.requires_grad else None
        ws = torch.empty(rows, dtype=torch.float32, device=x.device)
        check(lib.vmc_cross_entropy_loss(ptr(x), ptr(tidx), ptr(tprob), ptr(loss), ptr(dx), rows, C, ptr(ws), rows * 4, stream()),
              "cross_entropy_loss")
        ctx.save_for_backward(dx)
        ctx.shape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return ag.scale_by_device_scalar(dx, g).view(ctx.shape), None


def cross_entropy_loss(predictions, targets):
    """nn.CrossEntropyLoss() (mean) as used by the MammalNet variants: class-index targets
    (train_frame_diff_mn.py:102 ``labels.argmax(dim=1)``) or float probability rows
    (TFAM/train_and_eval_frame_diff_MN.py:83 passes the one-hot ``labels`` directly)."""
    return _CrossEntropyFn.apply(predictions, targets)


def reconstruction_loss(reconstruction, input):  # noqa: A002  (reference signature)
    """losses.py:70-81."""
    raise NotImplementedError


def loss_and_grad(criterion, logits, targets):
    """(loss, d loss / d logits) of a mean-reduced criterion of this module WITHOUT autograd nodes: the loss kernels produce the
    gradient in the same launch, and ``logits.backward(dlogits)`` is what ``loss.backward()`` computes (implicit upstream gradient 1)
    minus two launches (autograd's ones fill, the scaling by it) -- the training loops of TFAM/train_and_eval.py:81-83 spelled for a
    launch-bound step.  criterion: bce_with_logits_loss or cross_entropy_loss."""
    x = logits.detach().contiguous().float()
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    if criterion is bce_with_logits_loss:
        y = targets.contiguous().float()
        if x.shape != y.shape:
            raise ValueError(f"Target size ({tuple(y.shape)}) must be the same as input size ({tuple(x.shape)})")
        ws = torch.empty(64, dtype=torch.float32, device=x.device)
        check(lib.vmc_bce_loss(ptr(x), ptr(y), ptr(loss), ptr(dx), x.numel(), -1.0, ptr(ws), 256, stream()), "bce_loss")
    elif criterion is cross_entropy_loss:
        rows, C = x.shape
        tidx, tprob = (None, targets.contiguous().float()) if targets.is_floating_point() else (targets.contiguous().to(torch.int64), None)
        ws = torch.empty(rows, dtype=torch.float32, device=x.device)
        check(lib.vmc_cross_entropy_loss(ptr(x), ptr(tidx), ptr(tprob), ptr(loss), ptr(dx), rows, C, ptr(ws), rows * 4, stream()),
              "cross_entropy_loss")
    else:
        raise ValueError("loss_and_grad: criterion must be bce_with_logits_loss or cross_entropy_loss")
    return loss, dx.view(logits.shape)
