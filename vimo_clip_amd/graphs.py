"""hipGraph capture of launch-bound steps.

The libvmc entry points only enqueue kernels on the stream they are given (no allocation, no synchronisation;
include/vmc.h), so a whole TFAM forward — or a forward + backward + fused AdamW step — over fixed shapes can be
captured once and replayed as one graph launch.  At the reference's TFAM batch size (8 clips of 16x768 tokens) a
forward is ~90 kernels of a few microseconds each: replay removes the per-launch host cost that otherwise dominates.
"""
from __future__ import annotations

import gc

import torch


def pooled_stream(model):
    """Which token stream ``model`` (an AMO_CLIP) mean-pools: "rgb" (cross attention, rgb-only), "motion" (flow-only), or None for
    the two concatenation modes, which cannot be padded further (AMO_CLIP.pools_padded_tokens) and keep exact shapes."""
    if not getattr(model, "pools_padded_tokens", False):
        return None
    return "motion" if model.use_only_flow else "rgb"


def pad_to_bucket(rgb, mot, mask_rgb, mask_flow, bucket: int, pooled="rgb"):
    """Zero-pad a ragged TFAM batch to its length bucket: (rgb, mot, mask_rgb, mask_flow, n).

    RGB and motion tokens [B, T, D] are padded along T, each to its own next multiple of ``bucket``; the masks [B, T] (True / 1 =
    real token) get zeros on the new rows, and a mask that is None becomes all-true over the ORIGINAL length first -- otherwise
    the new rows would be attended to.  n is the original length of the ``pooled`` stream ("rgb" | "motion"), to be handed to
    ``AMO_CLIP.forward(..., pool_len=n)``: the added rows are then masked as keys, feed only their own rows as queries, stay out of
    the mean-pool and receive a zero gradient, so the padded batch gives the logits and gradients of the unpadded one and every
    batch whose lengths fall into the same buckets shares one captured graph.  ``bucket <= 1`` or ``pooled is None`` (the
    concatenation modes): everything is returned as it came, n = None."""
    if bucket <= 1 or pooled is None:
        return rgb, mot, mask_rgb, mask_flow, None

    def pad(x, T, fill_mask_like=None):
        if x is None:
            x = torch.ones(fill_mask_like.shape[:2], dtype=torch.bool, device=fill_mask_like.device)
        if x.shape[1] == T:
            return x
        return torch.nn.functional.pad(x, (0, 0) * (x.dim() - 2) + (0, T - x.shape[1]))      # zeros behind dim 1

    n = int(mot.shape[1] if pooled == "motion" else rgb.shape[1])
    Tr, Tf = -(-rgb.shape[1] // bucket) * bucket, -(-mot.shape[1] // bucket) * bucket
    return pad(rgb, Tr), pad(mot, Tf), pad(mask_rgb, Tr, rgb), pad(mask_flow, Tf, mot), n


def concat_mode(model):
    """Which concatenation an AMO_CLIP performs: "time" (``concat_dim = 1``: tokens), "feature" (``concat_dim = -1``: features, then
    ``projection_layer``), or None for the modes that pool one stream (``pooled_stream``)."""
    if getattr(model, "use_only_rgb", False) or getattr(model, "use_only_flow", False) or getattr(model, "use_cross_attention", True):
        return None
    return "time" if model.concat_dim == 1 else "feature"


def pad_concat_to_bucket(rgb, mot, mask_rgb, mask_flow, bucket: int, mode):
    """``pad_to_bucket`` for the two concatenation modes: (rgb, mot, mask_rgb, mask_flow, n_rgb, n_mot, T_out).

    Each stream is zero-padded to its own next multiple of ``bucket``, the masks get zeros on the new rows (a mask that is None
    becomes all-true over the ORIGINAL length first).  n_rgb / n_mot are the original lengths, to be handed to
    ``AMO_CLIP.forward(..., token_lens=(n_rgb, n_mot), concat_len=T_out)``, which rebuilds the concatenation with the real rows first
    so that the padded batch gives the logits and gradients of the unpadded one.  T_out is the padded length of the concatenated
    sequence: for "time" roundup(n_rgb - 1 + n_mot, bucket) -- the concatenated length is bucketed, not the sum of two rounded
    lengths, which keeps clips of up to 64 concatenated tokens on the fused chains; for "feature" the padded motion length.
    ``bucket <= 1`` or ``mode is None``: everything is returned as it came, n_rgb = n_mot = T_out = None."""
    if bucket <= 1 or mode is None:
        return rgb, mot, mask_rgb, mask_flow, None, None, None
    n_rgb, n_mot = int(rgb.shape[1]), int(mot.shape[1])
    rgb, mot, mask_rgb, mask_flow, _ = pad_to_bucket(rgb, mot, mask_rgb, mask_flow, bucket)
    T_out = -(-(n_rgb - 1 + n_mot) // bucket) * bucket if mode == "time" else int(mot.shape[1])
    return rgb, mot, mask_rgb, mask_flow, n_rgb, n_mot, T_out


class _PoolLens:
    """One-element int32 tensors of the pool lengths seen so far, per device: a replay copies one into the graph's static input, and
    no step pays a host-to-device transfer for a length it has seen before."""

    def __init__(self):
        self._t = {}

    def get(self, n, device):
        key = (int(n), str(device))
        t = self._t.get(key)
        if t is None:
            t = self._t[key] = torch.tensor([int(n)], dtype=torch.int32, device=device)
        return t


class GraphedCallable:
    """Captures ``fn(*static_inputs)`` once; ``__call__(*inputs)`` copies the inputs into the static buffers, replays
    the graph and returns the static outputs (valid until the next call)."""

    def __init__(self, fn, *example_inputs, warmup: int = 3):
        self.static_inputs = [x.clone() if torch.is_tensor(x) else x for x in example_inputs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up outside capture: lazy kernel attributes, caches, allocator
            for _ in range(warmup):
                fn(*self.static_inputs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # No cyclic garbage collection inside the capture: a collected cycle may own captured graphs of its own (a dropped trainer and
        # its GraphedTrainStep reference each other), and releasing their memory pools while a stream captures aborts the process.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(self.graph):
                self.static_outputs = fn(*self.static_inputs)
        finally:
            if gc_was_on:
                gc.enable()

    def __call__(self, *inputs):
        for dst, src in zip(self.static_inputs, inputs):
            if torch.is_tensor(dst) and dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.static_outputs

    def replay(self):
        self.graph.replay()
        return self.static_outputs


class GraphedTrainStep:
    """One training step (vmc_train_tick + forward + backward + fused Adam) per batch shape as a hipGraph replay.

    The optimiser must be in device-state mode (``FusedAdam.enable_device_state``): the step count, the bias corrections, the
    learning rate and the dropout seeds then live in device memory, so every captured launch has constant arguments and a
    replay IS the next step (host scalars would be frozen into the graph).  The warm-up run that precedes a
    capture is undone (parameters, Adam moments and the step state are restored), so capturing a new batch shape does not
    train on its example batch.

    Data parallel (``exchange`` given; replaces nn.DataParallel's per-step reduce_add, TFAM/train_and_eval.py:392): the step is
    TWO graphs with the gradient exchange between them -- ``step_fn`` = tick + forward + loss + backward (one graph per batch
    shape), then ``exchange()`` (the bucketed RCCL all-reduce or reduce-scatter + all-gather of parallel.GradientAllReducer, eager:
    collectives are not captured) whose return value (1 / world) goes to the optimiser's device-resident grad_scale, then
    ``opt_fn`` = [vmc_grad_clip_dev over the rank-summed arena when it passes ``max_grad_norm``, base_scale = 1 / world, or with
    ``FusedAdam.enable_loss_scaling`` vmc_loss_scale_check: every rank sees the same exchanged arena, so all skip together +] the fused
    AdamW + the refresh of the 16-bit copies (one graph, shape independent).  Gradient-ready hooks are
    silenced while capturing (a replay runs no Python, so the buckets go out after the backward graph, not during it).

    Ragged batches (``bucket > 1``): the first four inputs are taken as (rgb tokens, motion tokens, mask_rgb, mask_flow) and go
    through ``pad_to_bucket``; ``step_fn`` then receives the padded tensors, the remaining inputs and, last, ``pool_len`` -- a
    one-element int32 tensor holding the batch's own length, one more static input that is refreshed before every replay and that
    ``step_fn`` hands to ``AMO_CLIP.forward(pool_len=...)``.  The graph key uses the padded lengths, so one graph serves a whole
    bucket, exactly (see pad_to_bucket).  ``pooled``: the stream the model pools (``pooled_stream(model)``); None keeps exact
    shapes, as ``bucket = 1`` does.  Dropout masks are a function of the padded shape (element index ``row * N + col``): a
    bucketed step draws other masks than an unbucketed one, and the same masks as an eager step on the same padded tensors.

    Concatenation models (``concat`` = ``concat_mode(model)``, "time" | "feature", with ``bucket > 1``): the first four inputs go
    through ``pad_concat_to_bucket`` instead; ``step_fn`` receives the padded tensors, the remaining inputs, then the two length
    tensors n_rgb and n_mot (static inputs refreshed before every replay, for ``AMO_CLIP.forward(token_lens=...)``) and, last,
    the int T_out (``concat_len``), which is part of the graph key by value.

    ``extra_live``: further tensors that ``step_fn`` modifies in place and that a warm-up run must leave as it found them (the
    cursor and sums of a metrics.DeviceMetricLog appended to inside the step); saved and restored with the optimiser's."""

    def __init__(self, step_fn, optimizer, max_graphs: int = 16, exchange=None, opt_fn=None, graph_factory=None, bucket: int = 1,
                 pooled="rgb", extra_live=(), concat=None):
        if getattr(optimizer, "dev_state", None) is None:
            raise ValueError("GraphedTrainStep needs FusedAdam.enable_device_state()")
        if (exchange is None) != (opt_fn is None):
            raise ValueError("GraphedTrainStep: exchange and opt_fn come together (two-graph data-parallel step)")
        self.step_fn, self.opt, self.max_graphs = step_fn, optimizer, max_graphs
        self.exchange, self.opt_fn = exchange, opt_fn
        self._factory = graph_factory or GraphedCallable
        self._graphs = {}
        self._opt_graph = None
        self.bucket, self.pooled, self.concat = int(bucket), pooled, concat
        self._lens = _PoolLens()
        self.extra_live = tuple(extra_live)

    @property
    def n_graphs(self) -> int:
        """Step graphs captured so far (one per distinct input shape / value key)."""
        return len(self._graphs)

    @staticmethod
    def _key(inputs):
        return tuple((tuple(x.shape), x.dtype) if torch.is_tensor(x) else x for x in inputs)

    def captured(self, *inputs):
        """The captured step graph that ``__call__(*inputs)`` would replay (exact shapes: ``bucket = 1`` callers), None when that
        shape has not been captured.  For tools that replay a step without the host work around it."""
        return self._graphs.get(self._key(inputs))

    def _live(self):
        o, a = self.opt, self.opt.arena
        live = (a.flat_param, a.flat_grad, o.m, o.v, o.dev_state, o.dev_hyper)
        clip = getattr(o, "dev_clip", None)            # device-side gradient clipping in use: its norm / coefficient slots too
        live = live if clip is None else live + (clip,)
        ls = getattr(o, "dev_ls", None)                # loss scaling on: a warm-up leaves S, the tracker and the counters as it found them
        live = live if ls is None else live + (ls,)
        ema = getattr(o, "ema", None)                  # weight average on: a warm-up run's update is taken back with the parameters'
        live = live if ema is None else live + (ema,)
        return live + self.extra_live

    def _capture(self, fn, inputs):
        from . import autograd_ops
        o = self.opt
        live = self._live()
        saved = [t.clone() for t in live]
        count, host = o.step_count, getattr(o, "_hyper_host", None)
        hooks = list(autograd_ops.grad_ready_hooks)
        autograd_ops.grad_ready_hooks[:] = []          # no collective inside a warm-up or a capture
        try:
            g = self._factory(fn, *inputs, warmup=1)
        finally:
            autograd_ops.grad_ready_hooks[:] = hooks
        for t, s in zip(live, saved):
            t.copy_(s)
        o.step_count = count
        now = getattr(o, "_hyper_host", None)
        if now is not None and now != host:        # the warm-up moved a host-written slot (first clipped step, another max_grad_norm): kept, so written again
            o._hyper_host = None
            o.sync_hyper(now[1])
        autograd_ops.weights.refresh()          # the 16-bit compute copies follow the restored masters
        return g

    def __call__(self, *inputs):
        from . import autograd_ops
        if self.bucket > 1 and self.concat is not None:
            rgb, mot, mr, mf, nr, nm, T_out = pad_concat_to_bucket(*inputs[:4], self.bucket, self.concat)
            inputs = (rgb, mot, mr, mf) + tuple(inputs[4:]) + (self._lens.get(nr, rgb.device), self._lens.get(nm, rgb.device), T_out)
        elif self.bucket > 1 and self.pooled is not None:
            rgb, mot, mr, mf, n = pad_to_bucket(*inputs[:4], self.bucket, self.pooled)
            inputs = (rgb, mot, mr, mf) + tuple(inputs[4:]) + (self._lens.get(n, rgb.device),)
        key = self._key(inputs)
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) >= self.max_graphs:           # too many shapes: eager step (same device-state arithmetic)
                out = self.step_fn(*inputs)
                if self.exchange is not None:
                    self.opt.sync_hyper(grad_scale=self.exchange())
                    self.opt_fn()
                return out
            g = self._graphs[key] = self._capture(self.step_fn, inputs)
        if self.exchange is not None and self._opt_graph is None:
            self._opt_graph = self._capture(self.opt_fn, ())
        out = g(*inputs)
        if self.exchange is not None:
            self.opt.sync_hyper(grad_scale=self.exchange())    # host -> device only when the factor changes (1 / world: once)
            self._opt_graph()
        self.opt.step_count += 1                               # host mirror of the device step count
        # host mirror of what the replayed Adam + vmc_cast_weights_multi launches did: the masters and their 16-bit copies
        # changed without any Python running, so everything keyed on the weight epoch (TfamPack.pack_is_current, captured
        # evaluation forwards) must see a new epoch (the fused eval path scored stale packs after pure replays)
        autograd_ops.weights.epoch += 1
        return out
