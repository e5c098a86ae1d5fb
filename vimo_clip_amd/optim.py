"""Flat parameter/gradient arena, fused Adam/AdamW (K15) and the reference's LR schedule.

``GradArena`` lays the parameters that receive gradients out in ONE flat fp32 buffer (plus a flat
gradient buffer, Adam m and v): every ``p.data`` / ``p.grad`` becomes a 64-element-aligned view, the
backward kernels write gradients in place (autograd_ops._grad_out), the optimiser is one vmc_adam_step
launch over the whole arena (28 B/parameter of HBM traffic), and data-parallel training all-reduces the
flat gradient buffer in large buckets (parallel.py).  Every backward OVERWRITES its gradient slots;
``GradArena.accumulate`` is the opt-in way to sum the gradients of several micro-batches (vmc_grad_accumulate,
DESIGN.md "Gradient accumulation"); ``FusedAdam.enable_ema`` the opt-in way to keep an exponential moving average of the masters beside
them (vmc_ema_update behind every step, ``ema_weights()`` to compute with it).  Mirrors ``torch.optim.Adam(lr)`` (train.py:66) and
``torch.optim.AdamW(lr=1e-4, weight_decay=0.1)`` + ``CosineAnnealingLR(T_max=epochs, eta_min=1e-6)``
(TFAM/train_and_eval.py:53-56) in arithmetic.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os

import torch

from ._lib import check, lib, ptr, stream

_ALIGN = 64


class GradArena:
    def __init__(self, params):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("GradArena: no trainable parameters")
        dev = params[0].device
        self.params = params
        self.offsets = []
        off = 0
        for p in params:
            self.offsets.append(off)
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = off
        self.flat_param = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=dev)
        for p, o in zip(params, self.offsets):
            n = p.numel()
            self.flat_param[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat_param[o:o + n].view(p.shape)
            g = self.flat_grad[o:o + n].view(p.shape)
            p.grad = g
            p._vmc_grad = g
        self.flat_acc = None                       # fp32 accumulator of accumulate(), allocated on first use
        self._pending = 0
        self._overlap_owner = None                 # the FusedAdam with enable_backward_overlap on, which excludes accumulate()

    def zero_grad(self):
        """Zero the gradient buffer and DROP a pending accumulation (``pending`` becomes 0; the micro-steps folded so far are
        forgotten).  Not needed between steps: every used gradient is overwritten, not added to, by its backward kernel, which is
        also why two backward passes in a row leave the second gradient alone -- summing them takes ``accumulate``."""
        self.flat_grad.zero_()
        self._pending = 0

    # ---- gradient accumulation over micro-batches ---------------------------------------------------------------------------
    @property
    def pending(self) -> int:
        """Number of micro-steps folded into the accumulator and not yet finalised."""
        return self._pending

    def _launch_accumulate(self, mode: int, weight: float):
        check(lib.vmc_grad_accumulate(ptr(self.flat_grad), ptr(self.flat_acc), ptr(self.flat_grad), self.numel, float(weight), mode,
                                      stream()), "grad_accumulate")

    def accumulate(self, weight: float = 1.0, final: bool = False):
        """Fold the gradient the last backward wrote into a weighted sum over micro-batches (one streaming launch over the arena).

        Call it after every micro-batch's backward with that micro-batch's weight (rows of the micro-batch / rows of the batch, for
        losses that are means over rows) and ``final=True`` on the last one: the first call writes ``flat_acc = w * flat_grad``
        (no zeroing needed), later ones ``flat_acc += w * flat_grad``, the final one ``flat_grad = flat_acc + w * flat_grad`` IN
        PLACE, so the optimiser, gradient clipping, ``grad_norm`` and the data-parallel reducer read ``flat_grad`` as they always do.
        ``final=True`` with nothing pending and weight 1 launches nothing (a loop with one micro-batch is the plain, un-accumulated path).
        ``flat_acc`` costs 4 B per parameter from the first non-final call on.  The pending count lives on the host: the call raises
        while the current stream is being captured, and it excludes ``FusedAdam.enable_backward_overlap``, which consumes a
        backward's own gradients."""
        from . import autograd_ops
        if self.flat_grad.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradArena.accumulate keeps its pending count on the host: it cannot run inside a graph capture")
        weight = float(weight)
        if final and not self._pending and weight == 1.0:
            return
        if self._overlap_owner is not None:
            raise RuntimeError("GradArena.accumulate cannot be combined with FusedAdam.enable_backward_overlap: the overlapped "
                               "optimiser updates parameters from each backward's own gradients (disable_backward_overlap() first)")
        autograd_ops.wgrad_queue.flush()
        if self.flat_acc is None:
            self.flat_acc = torch.empty_like(self.flat_grad)
        if final:
            if self._pending:
                self._launch_accumulate(2, weight)
            else:                                  # one weighted micro-step on its own: flat_grad = weight * flat_grad (rare; a copy back)
                self._launch_accumulate(0, weight)
                self.flat_grad.copy_(self.flat_acc)
            self._pending = 0
            return
        self._launch_accumulate(1 if self._pending else 0, weight)
        self._pending += 1

    def grad_norm(self) -> torch.Tensor:
        from . import autograd_ops
        autograd_ops.wgrad_queue.flush()
        out = torch.zeros(1, dtype=torch.float32, device=self.flat_grad.device)
        check(lib.vmc_sumsq(ptr(self.flat_grad), self.numel, ptr(out), stream()), "sumsq")
        return out.sqrt()

    def buckets(self, bucket_bytes: int = 48 << 20):
        """Contiguous views of the flat gradient buffer of at most ``bucket_bytes`` each (all-reduce units)."""
        n = max(_ALIGN, bucket_bytes // 4 // _ALIGN * _ALIGN)
        return [self.flat_grad[s:min(self.numel, s + n)] for s in range(0, self.numel, n)]


def clipped_grad_scale(sum_grad_norm: float, grad_scale: float, max_grad_norm: float) -> float:
    """Scale to apply to the (rank-summed) arena gradient so that it equals ``clip_grad_norm_`` applied to the AVERAGED
    gradient (train.py:105-106 runs on one process; under data parallelism the arena holds the SUM until ``grad_scale`` =
    1/world is applied inside the Adam kernel): norm of the average = ||sum|| * grad_scale, torch's coefficient
    min(1, max_norm / (norm + 1e-6)), final factor = grad_scale * coefficient."""
    total = sum_grad_norm * abs(grad_scale)
    return grad_scale * min(1.0, max_grad_norm / (total + 1e-6))


class LossScaleStruct(ctypes.Structure):
    """ctypes mirror of ``vmc_loss_scale_state`` (include/vmc.h): same fields in the same order, 32 bytes."""
    _fields_ = [("scale", ctypes.c_float), ("growth_factor", ctypes.c_float), ("backoff_factor", ctypes.c_float),
                ("base_scale", ctypes.c_float), ("growth_interval", ctypes.c_int), ("growth_tracker", ctypes.c_int),
                ("found_inf", ctypes.c_int), ("skipped", ctypes.c_int)]


class _ScaleLossFn(torch.autograd.Function):
    """loss * S with S read from device memory by the kernel, forward and backward (vmc_scale_by_device_scalar): nothing of S is a
    host scalar, so the node is safe under capture and S may change between replays."""

    @staticmethod
    def forward(ctx, loss, scale):
        from . import autograd_ops
        ctx.scale = scale
        return autograd_ops.scale_by_device_scalar(loss.contiguous().float(), scale)

    @staticmethod
    def backward(ctx, g):
        from . import autograd_ops
        return autograd_ops.scale_by_device_scalar(g.contiguous().float(), ctx.scale), None


class FusedAdam:
    """Adam / AdamW over a GradArena: one kernel launch per step."""

    def __init__(self, arena: GradArena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        self.arena = arena
        self.lr, self.betas, self.eps, self.weight_decay, self.decoupled = lr, betas, eps, weight_decay, decoupled
        self.m = torch.zeros_like(arena.flat_param)
        self.v = torch.zeros_like(arena.flat_param)
        self.step_count = 0
        self.param_groups = [{"lr": lr}]          # what LR schedulers / loggers poke at
        self.ema = None                            # fp32 average of flat_param (enable_ema); None = off: nothing allocated or launched

    def zero_grad(self, set_to_none: bool = False):
        """Does nothing, for loops that call it every step: each backward overwrites its arena slots, so there is nothing to clear
        (and nothing is ever summed: gradients of several backward passes are combined with ``GradArena.accumulate``).  A pending
        accumulation is left alone, so calling this before every micro-step is harmless; ``GradArena.zero_grad`` drops it."""

    # ---- device-resident step state: what a hipGraph-captured training step needs ----------------------------
    N_SEEDS = 256                                  # dropout call sites per step a model may draw

    def enable_device_state(self, base_seed: int = 0x5EED):
        """Move the step count / bias corrections / learning rate / dropout seeds into device memory (vmc_train_tick,
        vmc_adam_step_dev): ``tick()`` + ``step()`` then enqueue only launches whose arguments never change, so a captured
        step replays correctly.  ``sync_hyper()`` must be called (outside a capture) whenever lr or grad_scale change.
        ``step(max_grad_norm=x)`` clips on the device (vmc_grad_clip_dev, ``_set_clip``)."""
        dev = self.arena.flat_param.device
        self.dev_state = torch.zeros(2 + self.N_SEEDS, dtype=torch.int64, device=dev)
        self.dev_state[0] = self.step_count
        self.dev_state[1] = int(base_seed) & 0x7FFFFFFFFFFFFFFF
        self.dev_hyper = torch.zeros(4, dtype=torch.float32, device=dev)
        self.dev_clip = self._clip_ws = self._clip_max = None
        self.dev_ls = self._ls_ws = self._ls_f32 = None
        self._hyper_host = None
        self.sync_hyper()
        return self

    def sync_hyper(self, grad_scale: float = 1.0):
        """lr and grad_scale (1, or 1 / world over a rank-summed arena) -> device memory, only when one of them changed.  While
        clipping is on, hyper[3] belongs to vmc_grad_clip_dev: grad_scale goes to dev_clip[0] (base_scale) beside the threshold.
        While loss scaling is on, hyper[3] belongs to vmc_loss_scale_check: grad_scale goes to the scaler record's base_scale (and,
        with clipping, to dev_clip[0] as well)."""
        want = (float(self.param_groups[0]["lr"]), float(grad_scale), self._clip_max, self.dev_ls is not None)
        if self._hyper_host != want:
            self.dev_hyper[0] = want[0]
            if self.dev_ls is not None:
                self._ls_f32[3] = want[1]
            if self._clip_max is not None:
                self.dev_clip[0] = want[1]
                self.dev_clip[1] = want[2]
            elif self.dev_ls is None:
                self.dev_hyper[3] = want[1]
            self._hyper_host = want

    def _set_clip(self, max_grad_norm):
        """Device-state mode: turn clipping on (first use allocates ``dev_clip`` = {base_scale, max_norm, norm, coef} and the
        reduction workspace), change the threshold, or turn it off (the host owns hyper[3] again).  All of these write device
        memory from the host, which a capture would not record: inside one they raise, as a changed ``_fused_plan`` does."""
        want = None if max_grad_norm is None else float(max_grad_norm)
        if want == self._clip_max:
            return
        if self.dev_hyper.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("max_grad_norm changed while a graph is being captured: run one eager step with it first")
        if want is not None and self.dev_clip is None:
            dev, n = self.arena.flat_param.device, self.arena.numel
            self.dev_clip = torch.zeros(4, dtype=torch.float32, device=dev)
            self._clip_ws = torch.empty(int(lib.vmc_grad_clip_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        grad_scale = self._hyper_host[1] if self._hyper_host is not None else 1.0
        self._clip_max, self._hyper_host = want, None
        self.sync_hyper(grad_scale)

    @property
    def last_grad_norm(self):
        """One-element device view: the norm of the (averaged) gradient the last clipped step saw.  No synchronisation."""
        return self._clip_view(2)

    @property
    def last_clip_coef(self):
        """One-element device view: the last clipped step's coefficient min(1, max_norm / (norm + 1e-6))."""
        return self._clip_view(3)

    def _clip_view(self, i):
        if getattr(self, "dev_clip", None) is None:
            raise RuntimeError("no device-side clipping yet: enable_device_state() and step(max_grad_norm=...) come first")
        return self.dev_clip[i:i + 1]

    # ---- dynamic loss scaling on the device (float16 training; DESIGN.md "Dynamic loss scaling") ---------------------------
    def enable_loss_scaling(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                            growth_interval: int = 2000):
        """torch.amp.GradScaler, on the device.  ``scale_loss(loss).backward()`` (or ``out.backward(scale_grad(dlogits))``) produces
        gradients multiplied by S; ``step()`` then runs vmc_loss_scale_check where it runs vmc_grad_clip_dev otherwise -- per-element
        inf / NaN test, the unscaled norm for ``max_grad_norm``, hyper[3] = grad_scale / S * coefficient, the scale update of
        ``torch._amp_update_scale_`` -- and the Adam entries behind the skip flag: after an overflow parameters, moments and 16-bit
        copies keep their bytes, S is multiplied by ``backoff_factor`` and the device step count is taken back, so the next ``tick()``
        recomputes the same bias corrections and dropout seeds.  Nothing is read back: captured and no-sync steps keep their shape.
        ``growth_factor = backoff_factor = 1`` is a static scale (an overflowing step is still skipped).
        Needs ``enable_device_state()``; excludes ``enable_backward_overlap`` (parameters updated before the gradient is complete
        cannot be skipped).  The host's ``step_count`` counts ATTEMPTS from here on; the true count is ``dev_state[0]`` (which
        ``state_dict()`` reads).  Writes device memory from the host: raises inside a capture."""
        if getattr(self, "dev_state", None) is None:
            raise RuntimeError("enable_loss_scaling needs enable_device_state() first: the scaler lives in device memory")
        if getattr(self, "_ov", None) is not None:
            raise RuntimeError("enable_loss_scaling cannot be combined with enable_backward_overlap: an overlapped step updates "
                               "parameters before the gradient is complete, so it cannot be skipped")
        if not (init_scale > 0.0 and math.isfinite(init_scale)) or growth_factor < 1.0 or not 0.0 < backoff_factor <= 1.0 or growth_interval < 1:
            raise ValueError("enable_loss_scaling: init_scale > 0, growth_factor >= 1, 0 < backoff_factor <= 1, growth_interval >= 1")
        dev = self.dev_hyper.device
        if self.dev_hyper.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("enable_loss_scaling while a graph is being captured: enable it before the first captured step")
        grad_scale = self._hyper_host[1] if self._hyper_host is not None else 1.0
        rec = LossScaleStruct(float(init_scale), float(growth_factor), float(backoff_factor), float(grad_scale), int(growth_interval), 0, 0, 0)
        self.dev_ls = torch.frombuffer(bytearray(bytes(rec)), dtype=torch.int32).clone().to(dev)
        self._ls_f32 = self.dev_ls.view(torch.float32)
        if dev.type == "cuda":
            self._ls_ws = torch.empty(int(lib.vmc_loss_scale_workspace_bytes(self.arena.numel)), dtype=torch.uint8, device=dev)
        self._hyper_host = None
        self.sync_hyper(grad_scale)
        return self

    def disable_loss_scaling(self):
        """The host owns hyper[3] again (as ``_set_clip(None)``); gradients must be unscaled from the next backward on."""
        if getattr(self, "dev_ls", None) is None:
            return
        if self.dev_hyper.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("disable_loss_scaling while a graph is being captured")
        grad_scale = self._hyper_host[1] if self._hyper_host is not None else 1.0
        self.dev_ls = self._ls_ws = self._ls_f32 = None
        self._hyper_host = None
        self.sync_hyper(grad_scale)

    @property
    def loss_scaling(self) -> bool:
        return getattr(self, "dev_ls", None) is not None

    def _ls_need(self):
        if not self.loss_scaling:
            raise RuntimeError("loss scaling is off: enable_device_state() and enable_loss_scaling() come first")

    @property
    def loss_scale(self):
        """One-element device view (fp32): the scale S the NEXT backward will use.  No synchronisation."""
        self._ls_need()
        return self._ls_f32[0:1]

    @property
    def last_found_inf(self):
        """One-element device view (int32): 1 if the last ``step()`` found inf / NaN and was skipped."""
        self._ls_need()
        return self.dev_ls[6:7]

    @property
    def skipped_steps(self):
        """One-element device view (int32): steps skipped since ``enable_loss_scaling`` (or the loaded checkpoint)."""
        self._ls_need()
        return self.dev_ls[7:8]

    def scale_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """``loss * S`` through an autograd node whose backward multiplies by S read from device memory at run time; ``loss`` itself
        stays the unscaled value for logging.  With scaling off: ``loss`` unchanged."""
        if not self.loss_scaling:
            return loss
        return _ScaleLossFn.apply(loss, self._ls_f32[0:1])

    def scale_grad(self, dlogits: torch.Tensor) -> torch.Tensor:
        """``dlogits * S`` for the ``loss_and_grad`` / ``output.backward(dlogits)`` pattern (one launch, S read on the device)."""
        if not self.loss_scaling:
            return dlogits
        from . import autograd_ops
        return autograd_ops.scale_by_device_scalar(dlogits.contiguous().float(), self._ls_f32[0:1]).view(dlogits.shape)

    def _skip_ptr(self):
        """Address of the scaler record's found_inf word: the skip flag of the Adam entries (None = no flag)."""
        return None if getattr(self, "dev_ls", None) is None else self.dev_ls.data_ptr() + 24

    def tick(self):
        """Start of a step in device-state mode: t += 1, bias corrections and this step's dropout seeds (one launch)."""
        check(lib.vmc_train_tick(ptr(self.dev_state), ptr(self.dev_hyper), float(self.betas[0]), float(self.betas[1]), self.N_SEEDS,
                                 stream()), "train_tick")
        self.step_count += 1

    def seed_address(self, i: int) -> int:
        """Seed argument (pointer form, include/vmc.h) of dropout call site i of the current step."""
        if not 0 <= i < self.N_SEEDS:
            raise IndexError("more dropout call sites per step than FusedAdam.N_SEEDS")
        return (1 << 63) | (self.dev_state.data_ptr() + 8 * (2 + i))

    # ---- exponential moving average of the weights -------------------------------------------------------------
    def enable_ema(self, decay: float = 0.9999, warmup: bool = True):
        """Keep ``self.ema``, an fp32 average of ``arena.flat_param`` (a copy of it at this moment): every ``step()`` then enqueues
        one more streaming launch behind the update, ``ema = lerp(ema, p, w)`` over the whole arena (vmc_ema_update, 12 B per
        parameter), with w = 1 - decay rounded once from float64, or with ``warmup`` max(1 - decay, 9 / (10 + t)) -- the usual
        decay_t = min(decay, (1 + t) / (10 + t)).  t is ``step_count`` in host-state mode; in device-state mode the kernel reads the
        step count and the loss scale's skip flag from device memory, so a captured step replays with the right weight and a skipped
        step leaves the average's bytes (and, the tick having been taken back, its warm-up count) alone.  Nothing is exchanged under
        data parallelism: the average is a function of parameters that are the same on every rank.  Allocates: raises inside a capture."""
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError(f"enable_ema: decay must lie strictly between 0 and 1, got {decay}")
        p = self.arena.flat_param
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("enable_ema while a graph is being captured: enable it before the first captured step")
        self._ema_w = ctypes.c_float(1.0 - decay).value      # the one rounding of 1 - decay, from float64
        self._ema_warmup = bool(warmup)
        self._ema_active = False
        self.ema = p.detach().clone()
        return self

    def disable_ema(self):
        if self.ema is not None and self._ema_active:
            raise RuntimeError("disable_ema inside ema_weights(): the average holds the live weights, leave the context first")
        self.ema = None

    def _ema_update(self):
        a, state = self.arena, getattr(self, "dev_state", None)
        check(lib.vmc_ema_update(ptr(self.ema), ptr(a.flat_param), a.numel, self._ema_w, int(self._ema_warmup),
                                 0 if state is not None else self.step_count, ptr(state), None if state is None else self._skip_ptr(),
                                 stream()), "ema_update")

    def _ema_swap(self):
        a = self.arena
        check(lib.vmc_ema_swap(ptr(a.flat_param), ptr(self.ema), a.numel, stream()), "ema_swap")
        invalidate_weight_copies(self)                 # the 16-bit copies follow the masters; a new weight epoch for every inference cache

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model computes with the AVERAGED weights: ``flat_param`` and ``ema`` trade places bit for bit
        (vmc_ema_swap: no third arena-sized buffer), the 16-bit compute copies are refreshed and the weight epoch moves; the same
        again on exit, after which the live weights are back as they were.  For evaluation and export only: ``step()`` raises
        inside it.  Raises when the average is off, inside a capture, when nested, while a gradient accumulation is pending and
        while an overlapped step is open."""
        if self.ema is None:
            raise RuntimeError("ema_weights: the average is off, enable_ema() comes first")
        if self.ema.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ema_weights while a graph is being captured: a capture must not freeze the averaged weights in")
        if self._ema_active:
            raise RuntimeError("ema_weights does not nest")
        if self.arena.pending:
            raise RuntimeError(f"ema_weights with {self.arena.pending} micro-step(s) of a gradient accumulation pending: finish the step first")
        if getattr(self, "_step_open", False):
            raise RuntimeError("ema_weights while an overlapped optimiser step is open: call step() first")
        self._ema_swap()
        self._ema_active = True
        try:
            yield self
        finally:
            self._ema_swap()
            self._ema_active = False

    def ema_state_dict(self, model):
        """``model.state_dict()`` with the averaged values (the reference's keys), cloned to the CPU; taken under the swap."""
        with self.ema_weights():
            return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    # ---- optimiser step overlapped with the backward ----------------------------------------------------------------------
    def enable_backward_overlap(self, groups):
        """groups: lists of parameters, each a contiguous run of the arena, whose gradients become final TOGETHER during the
        backward (a TFAM layer; the classifier head).  ``group_ready(i)`` -- called by the backward the moment group i's
        gradients have been enqueued (tfam_train.TfamTrainFn.backward) -- then enqueues that range's AdamW update and the refresh
        of its 16-bit compute copies on a side stream, beside the rest of the backward: the update is HBM-bound (28 B per
        parameter), the backward of the layers below is a chain of latency-bound launches that read none of the updated
        buffers.  ``step()`` afterwards updates whatever is left and joins the side stream.  Same arithmetic, element for
        element, as one whole-arena step.  Only for a single process without gradient clipping (both need the complete
        gradient first); ``step(grad_scale != 1)`` / ``max_grad_norm`` after a group was already updated raise.  Excludes
        ``GradArena.accumulate`` for the same reason: a group would be updated from one micro-batch's gradient."""
        a = self.arena
        if getattr(self, "dev_ls", None) is not None:
            raise RuntimeError("enable_backward_overlap cannot be combined with loss scaling: an overlapped step updates parameters "
                               "before the gradient is complete, so it cannot be skipped (disable_loss_scaling() first)")
        if a.pending:
            raise RuntimeError("enable_backward_overlap with a pending gradient accumulation: call arena.accumulate(final=True) and "
                               "step() (or arena.zero_grad()) first")
        index = {id(p): i for i, p in enumerate(a.params)}
        ranges = []
        for g in groups:
            idx = sorted(index[id(p)] for p in g if id(p) in index)
            if not idx:
                continue
            if idx != list(range(idx[0], idx[-1] + 1)):
                raise ValueError("enable_backward_overlap: a group must be a contiguous run of the arena's parameters")
            lo = a.offsets[idx[0]]
            hi = a.offsets[idx[-1] + 1] if idx[-1] + 1 < len(a.params) else a.numel
            ranges.append((lo, hi, frozenset(id(a.params[i]) for i in idx)))
        covered = sorted((lo, hi) for lo, hi, _ in ranges)
        rest, pos = [], 0
        for lo, hi in covered:
            if lo < pos:
                raise ValueError("enable_backward_overlap: groups overlap")
            if lo > pos:
                rest.append((pos, lo))
            pos = hi
        if pos < a.numel:
            rest.append((pos, a.numel))
        rest_ids = frozenset(id(p) for p in a.params) - frozenset().union(*[r[2] for r in ranges]) if ranges else frozenset(id(p) for p in a.params)
        self._ov = {"ranges": ranges, "rest": rest, "rest_ids": rest_ids, "done": [False] * len(ranges),
                    "stream": torch.cuda.Stream(device=a.flat_param.device, priority=int(os.environ.get("VMC_ADAM_SIDE_PRIO", "0"))),
                    "used": False}
        a._overlap_owner = self
        return self

    def disable_backward_overlap(self):
        self._ov = None
        if self.arena._overlap_owner is self:
            self.arena._overlap_owner = None

    def _open_step(self):
        if not getattr(self, "_step_open", False):
            if getattr(self, "dev_state", None) is None:
                self.step_count += 1                   # device-state mode: tick() already advanced t
            self._step_open = True

    BG_WORKGROUPS = int(os.environ.get("VMC_ADAM_BG_WGS", "512"))      # side-stream update: 2 workgroups of 256 threads per CU

    def _update_range(self, lo, hi, grad_scale=1.0, background=False):
        a, n = self.arena, hi - lo
        if n <= 0:
            return
        p, g, m, v = a.flat_param[lo:hi], a.flat_grad[lo:hi], self.m[lo:hi], self.v[lo:hi]
        if getattr(self, "dev_state", None) is not None:
            check(lib.vmc_adam_step_dev_skip(ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(self.dev_hyper), float(self.betas[0]), float(self.betas[1]),
                                             float(self.eps), float(self.weight_decay), int(self.decoupled),
                                             self.BG_WORKGROUPS if background else 2048, self._skip_ptr(), stream()), "adam_step_dev")
        else:
            check(lib.vmc_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, float(self.param_groups[0]["lr"]), float(self.betas[0]),
                                    float(self.betas[1]), float(self.eps), float(self.weight_decay), int(self.decoupled), self.step_count,
                                    float(grad_scale), stream()), "adam_step")

    def group_ready(self, i: int):
        """The gradients of overlap group i are complete (enqueued on the current stream): update it now, beside the backward."""
        ov = getattr(self, "_ov", None)
        if ov is None or i >= len(ov["ranges"]) or ov["done"][i]:
            return
        if self.ema is not None and self._ema_active:
            raise RuntimeError("a training backward inside ema_weights(): the arena holds the averaged weights, leave the context first")
        lo, hi, ids = ov["ranges"][i]
        self._open_step()
        side = ov["stream"]
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._update_range(lo, hi, background=True)
            from . import autograd_ops
            autograd_ops.weights.refresh(owner=(id(self), i), param_ids=ids)
        ov["done"][i] = ov["used"] = True

    def step(self, grad_scale: float = 1.0, max_grad_norm=None):
        from . import autograd_ops
        autograd_ops.wgrad_queue.flush()               # normally empty: the backward pass flushes its grouped weight gradients itself
        a = self.arena
        if self.ema is not None and self._ema_active:
            raise RuntimeError("FusedAdam.step inside ema_weights(): the arena holds the averaged weights, leave the context first")
        if a.pending:
            raise RuntimeError(f"FusedAdam.step with {a.pending} micro-step(s) folded into the accumulator and not finalised: the arena "
                               "holds only the last micro-batch's gradient.  Call arena.accumulate(weight, final=True) after the last "
                               "backward (or arena.zero_grad() to drop the accumulation)")
        dev_mode = getattr(self, "dev_state", None) is not None
        ov = getattr(self, "_ov", None)
        if dev_mode:
            if max_grad_norm is not None and ov is not None:
                raise ValueError("backward-overlapped optimiser steps cannot be combined with grad_scale / max_grad_norm")
            self._set_clip(max_grad_norm)
            if self.dev_ls is not None and grad_scale != 1.0:      # the reducer's 1 / world -> the scaler record's base_scale (host write,
                self.sync_hyper(grad_scale)                        # only when it changes: never inside a capture, whose steps pass 1)
        if ov is not None and ov["used"]:
            # some ranges were updated during the backward: finish the others on this stream, then join
            if max_grad_norm is not None or grad_scale != 1.0:
                raise ValueError("backward-overlapped optimiser steps cannot be combined with grad_scale / max_grad_norm")
            from . import autograd_ops
            for i, (lo, hi, ids) in enumerate(ov["ranges"]):
                if not ov["done"][i]:
                    self._update_range(lo, hi)
                    autograd_ops.weights.refresh(owner=(id(self), i), param_ids=ids)
            for lo, hi in ov["rest"]:
                self._update_range(lo, hi)
            if ov["rest"] and ov["rest_ids"]:
                autograd_ops.weights.refresh(owner=(id(self), "rest"), param_ids=ov["rest_ids"])
            torch.cuda.current_stream().wait_stream(ov["stream"])
            ov["done"] = [False] * len(ov["ranges"])
            ov["used"] = False
            self._step_open = False
            if self.ema is not None:                   # on the main stream, behind the join: every range has its new values
                self._ema_update()
            return
        if dev_mode and self.dev_ls is not None:    # found-inf check, unscaled norm, hyper[3] = base_scale / S * coefficient, scale update
            check(lib.vmc_loss_scale_check(ptr(a.flat_grad), a.numel, ptr(self.dev_ls), ptr(self.dev_hyper),
                                           ptr(self.dev_clip) if max_grad_norm is not None else None, ptr(self.dev_state),
                                           ptr(self._ls_ws), self._ls_ws.numel(), stream()), "loss_scale_check")
        elif max_grad_norm is not None and dev_mode:  # the same, computed on the device: hyper[3] = base_scale * coefficient
            check(lib.vmc_grad_clip_dev(ptr(a.flat_grad), a.numel, ptr(self.dev_hyper), ptr(self.dev_clip), ptr(self._clip_ws),
                                        self._clip_ws.numel(), stream()), "grad_clip_dev")
        elif max_grad_norm is not None:            # torch.nn.utils.clip_grad_norm_ (train.py:105-106)
            grad_scale = clipped_grad_scale(float(a.grad_norm().item()), grad_scale, max_grad_norm)
        self._open_step()
        if dev_mode and self._fused_update():          # AdamW + refresh of the 16-bit copies in one pass over the masters
            self._step_open = False
            if self.ema is not None:
                self._ema_update()
            return
        self._update_range(0, a.numel, grad_scale)
        self._step_open = False
        invalidate_weight_copies(self)
        if self.ema is not None:
            self._ema_update()

    FUSED_CAST = os.environ.get("VMC_ADAM_FUSED_CAST", "1") != "0"      # builder A/B switch

    def _fused_update(self) -> bool:
        """Device-state mode: vmc_adam_cast_multi updates every matrix tile by tile and writes its 16-bit compute copies from the
        registers (one read of the masters instead of two), a second small launch covers the parameters without copies.  Needs all
        cached copies of this arena's parameters in ONE compute dtype; otherwise the two-kernel path runs."""
        if not self.FUSED_CAST:
            return False
        import numpy as np
        from . import autograd_ops
        from ._lib import dt
        a = self.arena
        ids = getattr(self, "_param_ids", None)
        if ids is None:
            ids = self._param_ids = frozenset(id(p) for p in a.params)
        tabs = autograd_ops.weights.tables(owner=id(self), param_ids=ids)
        if len(tabs) != 1:
            return False
        (dtype16, tab), = tabs.items()
        covered = tab[4]
        plan = getattr(self, "_fused_plan", None)
        if plan is None or plan[0] != covered:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("optimiser plan changed while a graph is being captured: run one eager step first")
            rest = [(o, p.numel()) for p, o in zip(a.params, a.offsets) if id(p) not in covered]
            rec = np.zeros((max(1, len(rest)), 2), dtype=np.int64)
            block0 = 0
            for i, (o, n) in enumerate(rest):
                rec[i, 0] = o
                rec[i, 1] = n | (block0 << 32)
                block0 += (n + 1023) // 1024
            plan = self._fused_plan = (covered, torch.from_numpy(rec).to(a.flat_param.device), len(rest), block0)
            self._old_plans = getattr(self, "_old_plans", []) + [plan[1]]      # a captured graph may still read an older table
        check(lib.vmc_adam_cast_multi_skip(ptr(tab[1]), tab[2], tab[3], ptr(plan[1]) if plan[2] else None, plan[2], plan[3], ptr(a.flat_param),
                                           ptr(a.flat_grad), ptr(self.m), ptr(self.v), ptr(self.dev_hyper), float(self.betas[0]),
                                           float(self.betas[1]), float(self.eps), float(self.weight_decay), int(self.decoupled), dt(dtype16),
                                           self._skip_ptr(), stream()), "adam_cast_multi")
        autograd_ops.weights.epoch += 1
        return True

    def state_dict(self):
        """With loss scaling on, ``step`` is the TRUE step count read from the device (one synchronising read: the host mirror counts
        attempts, skipped steps included) and ``loss_scale`` carries the scaler record (8 int32 words, vmc_loss_scale_state)."""
        sd = {"step": self.step_count, "m": self.m, "v": self.v, "lr": self.param_groups[0]["lr"]}
        if getattr(self, "dev_ls", None) is not None:
            sd["step"] = int(self.dev_state[0].item())
            sd["loss_scale"] = self.dev_ls.detach().cpu().clone()
        if self.ema is not None:
            sd["ema"], sd["ema_one_minus_decay"], sd["ema_warmup"] = self.ema, self._ema_w, self._ema_warmup
        return sd

    def load_state_dict(self, sd):
        """Layout {step, m, v, lr} over the flat arena (NOT torch.optim's per-parameter state: checkpoint.py says so)."""
        self.step_count = int(sd["step"])
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.param_groups[0]["lr"] = sd["lr"]
        if sd.get("ema") is not None:                         # the average and its weight; allocated here when it was not on yet
            if self.ema is None:
                self.ema, self._ema_active = torch.empty_like(self.arena.flat_param), False
            self.ema.copy_(sd["ema"])
            self._ema_w, self._ema_warmup = float(sd["ema_one_minus_decay"]), bool(sd["ema_warmup"])
        if getattr(self, "dev_state", None) is not None:      # device-state mode: the step count and lr the kernels read
            self.dev_state[0] = self.step_count
            if sd.get("loss_scale") is not None and self.dev_ls is not None:      # S, factors, interval, tracker, counters
                self.dev_ls.copy_(sd["loss_scale"].to(torch.int32))
            self._hyper_host = None
            self.sync_hyper()


def invalidate_weight_copies(optimizer=None):
    """The optimiser kernel wrote the fp32 masters behind autograd's version counters: the cached 16-bit compute copies of
    the parameters it owns are re-cast into their buffers in one launch (autograd_ops._WeightCache.refresh)."""
    from . import autograd_ops
    if optimizer is None:
        autograd_ops.weights.refresh()
        return
    ids = getattr(optimizer, "_param_ids", None)
    if ids is None:
        ids = optimizer._param_ids = frozenset(id(p) for p in optimizer.arena.params)
    autograd_ops.weights.refresh(owner=id(optimizer), param_ids=ids)


class CosineAnnealingLR:
    """Closed form of torch's CosineAnnealingLR(T_max, eta_min), stepped once per epoch (train_and_eval.py:162)."""

    def __init__(self, optimizer, T_max, eta_min=0.0):
        self.opt, self.T_max, self.eta_min = optimizer, T_max, eta_min
        self.base_lr = optimizer.param_groups[0]["lr"]
        self.last_epoch = 0

    def step(self):
        self.last_epoch += 1
        self.opt.param_groups[0]["lr"] = self.eta_min + (self.base_lr - self.eta_min) * (1 + math.cos(math.pi * self.last_epoch / self.T_max)) / 2

    def get_last_lr(self):
        return [self.opt.param_groups[0]["lr"]]

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "base_lr": self.base_lr}
