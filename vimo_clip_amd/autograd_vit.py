"""Differentiable forward of the CLIP ViT on libvmc kernels (student fine-tuning path, train.py:95-104).

Same arithmetic as VisionTransformer._encode_patches, but every op is an autograd.Function from
autograd_ops so that ``loss.backward()`` runs the hand-written backward kernels (K8).  Activations are
kept in the compute dtype; the residual stream uses ``model.residual_dtype``.

``model.recompute = "block"`` keeps only the input stream of every residual block for the backward pass and recomputes the block
there (_BlockFn); ``saved_activation_bytes`` counts what either mode keeps.

``model.patch_dropout = p > 0`` (training with gradients only) keeps the class token and Kp = max(1, int(g^2 (1 - p))) randomly drawn
patch tokens of every frame: the patch GEMM, the tower and their backward run on Kp + 1 rows per frame (``patch_keep_for``).

``model.drop_path = p > 0`` (training with gradients only) is stochastic depth per frame: block l keeps K_l = max(1, int(F (1 - p_l)))
of the F frames, p_l = p l / max(1, L - 1); the block runs on the kept frames alone and its output is merged back into the stream
with the scale F / K_l (``drop_keep_for``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import autograd_ops as ag
from . import ops, synth


def _mix64(x: int) -> int:
    """synth._mix64 (the splitmix64 finaliser) on one Python int."""
    return int(synth._mix64(np.array([x & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0])


def patch_keep_for(model, F: int, device):
    """The keep set [F, Kp] int32 of this training forward, or None when nothing is dropped: ``model.patch_dropout`` is 0, the model
    is in eval mode, or no gradient is being recorded.  The seed is ``model.patch_dropout_seed_address`` verbatim when set (a device
    address with bit 63, e.g. FusedAdam.seed_address(i): a captured step then draws anew on every replay); otherwise the splitmix
    finaliser of ``model.patch_dropout_seed`` and the number of sets this model has drawn so far."""
    p = float(getattr(model, "patch_dropout", 0.0) or 0.0)
    if p <= 0.0 or not model.training or not torch.is_grad_enabled():
        return None
    if not p < 1.0:
        raise ValueError(f"VisionTransformer.patch_dropout must be in [0, 1), got {p}")
    g = model.input_resolution // model.patch_size
    seed = getattr(model, "patch_dropout_seed_address", None)
    if seed is None:
        calls = getattr(model, "_patch_dropout_calls", 0)
        model._patch_dropout_calls = calls + 1
        seed = _mix64(_mix64(int(getattr(model, "patch_dropout_seed", 0))) + calls) >> 1          # a value below 2^63
    return ops.patch_keep_sample(seed, F, g * g, ops.patch_keep_count(g * g, p), device)


DROP_PATH_SALT = 0xD509A7B1C0FFEE11      # keeps the drop-path stream apart from the patch-dropout stream of the same base seed


def drop_keep_for(model, F: int, device):
    """Per residual block None (the block runs on every frame, as it always did) or (keep int32 [K_l] ascending, slot int32 [F], s_l =
    F / K_l): the frames block l keeps in this training forward.  All None -- and nothing drawn -- when ``model.drop_path`` is 0, the
    model is in eval mode, or no gradient is being recorded; a block whose K_l equals F is None as well (block 0 always).  The seed
    is ``model.drop_path_seed_address`` verbatim when set (a device address with bit 63: a captured step draws anew on every replay);
    otherwise the splitmix finaliser of ``model.drop_path_seed`` and the number of forwards this model has drawn for so far.  The block
    index goes into the counter of the hash, so one seed serves every block of a forward."""
    L = len(model.transformer.resblocks)
    p = float(getattr(model, "drop_path", 0.0) or 0.0)
    if p <= 0.0 or not model.training or not torch.is_grad_enabled():
        return [None] * L
    if not p < 1.0:
        raise ValueError(f"VisionTransformer.drop_path must be in [0, 1), got {p}")
    counts = [ops.drop_path_keep_count(F, ops.drop_path_rate(p, l, L)) for l in range(L)]
    if all(K == F for K in counts):
        return [None] * L
    if F > ops.DROP_PATH_MAX_F:
        raise ValueError(f"drop path draws among at most {ops.DROP_PATH_MAX_F} frames per forward, got {F}: split the batch")
    seed = getattr(model, "drop_path_seed_address", None)
    if seed is None:
        calls = getattr(model, "_drop_path_calls", 0)
        model._drop_path_calls = calls + 1
        seed = _mix64(_mix64(int(getattr(model, "drop_path_seed", 0)) ^ DROP_PATH_SALT) + calls) >> 1          # a value below 2^63
    return [None if K == F else (*ops.drop_path_sample(seed, l, F, K, device), F / K) for l, K in enumerate(counts)]


def _given_drop_keep(model, drop_keep, F: int):
    """``drop_keep=``: a list of length L of None or an int32 device tensor [K_l] of ascending frame ids -> the triples of
    ``drop_keep_for`` (the inverse of every keep set is plain index plumbing, once per forward)."""
    L = len(model.transformer.resblocks)
    if not torch.is_grad_enabled() or not model.training:
        raise ValueError("drop_keep needs the training forward (train() mode with gradients enabled)")
    if not isinstance(drop_keep, (list, tuple)) or len(drop_keep) != L:
        raise ValueError(f"drop_keep must be a list of {L} entries (one per residual block), each None or an int32 tensor of frame ids")
    out = []
    for k in drop_keep:
        if k is None:
            out.append(None)
            continue
        if k.dtype != torch.int32 or k.dim() != 1 or not 1 <= k.numel() <= F or not k.is_contiguous():
            raise ValueError(f"a drop_keep entry must be a contiguous int32 vector of 1..{F} frame ids, got {k.dtype} {tuple(k.shape)}")
        slot = torch.full((F,), -1, dtype=torch.int32, device=k.device)
        slot[k.long().clamp(0, F - 1)] = torch.arange(k.numel(), dtype=torch.int32, device=k.device)
        out.append((k, slot, F / k.numel()))
    return out


def vit_tokens_train(model, x: torch.Tensor, wrap_quirk: bool = False, cls_only: bool = True, keep: torch.Tensor = None,
                     drop_keep=None):
    """x: u8 [F,3,R,R] frames or float pixel values.  Returns (the final residual stream, F, N, rows_are_cls).
    drop_keep: per block None or the frames it keeps (``_given_drop_keep``); None: ``drop_keep_for(model)`` decides (every block runs
    on every frame unless ``model.drop_path`` asks otherwise).
    keep: int32 [F, Kp] device tensor of ascending patch ids per frame: only those patches (and the class token) enter the tower and
    the N returned is Kp + 1; None: ``patch_keep_for(model)`` decides (nothing is dropped unless ``model.patch_dropout`` asks for it).
    cls_only: only x[:, 0] of the last block reaches ln_post, so its out_proj / ln_2 / MLP run on the F class rows (forward and,
    through autograd, backward: the dgrad / wgrad GEMMs of those four linears shrink by N as well); the stream returned is then
    [F, D].  The attention of the last block still sees every token (its K / V gradients flow to all rows)."""
    dt16, D, H = model.compute_dtype, model.width, model.heads
    recompute = getattr(model, "recompute", "none")
    if recompute not in RECOMPUTE_MODES:
        raise ValueError(f"VisionTransformer.recompute must be one of {RECOMPUTE_MODES}, got {recompute!r}")
    lora = getattr(model, "lora", None)              # lora.add_lora: the blocks' linears carry adapters
    if lora is not None:
        if recompute != "none":
            raise ValueError("LoRA adapters are not supported together with recompute='block'")
        lora.refresh(dt16)                           # 16-bit copies of the frozen weights and of every adapter (at most one launch)
    F = x.shape[0]
    g = model.input_resolution // model.patch_size
    N = g * g + 1
    if keep is None:
        keep = patch_keep_for(model, F, model.class_embedding.device)
    drop = drop_keep_for(model, F, model.class_embedding.device) if drop_keep is None else _given_drop_keep(model, drop_keep, F)
    with torch.no_grad():   # the input frames carry no gradient
        if x.dtype == torch.uint8:
            x, wrap_quirk = model.fit_frames_u8(x, wrap_quirk)
            patches = ops.preprocess_patches_u8(x, model.patch_size, dt16, wrap_quirk)
        else:
            patches = ops.patches_f32(x, model.patch_size, dt16)
        if keep is not None:                                                       # patch dropout: the GEMM sees the kept rows only
            patches = ops.gather_rows16(patches, keep, g * g)
            N = keep.shape[1] + 1
    xp = ag.linear(patches, model.conv1.weight)                                    # [F*g*g, D], or [F*Kp, D]
    if keep is None:
        xs = ag.AssembleTokensFn.apply(xp, model.class_embedding, model.positional_embedding, F, N, model.residual_dtype)
    else:
        xs = ag.AssembleTokensKeepFn.apply(xp, model.class_embedding, model.positional_embedding, keep, model.residual_dtype)
    xs = ag.layernorm(xs, model.ln_pre.weight, model.ln_pre.bias, dt16, out_f32=(model.residual_dtype == torch.float32))
    if model.residual_dtype != torch.float32:
        xs = ag.cast(xs, model.residual_dtype)
    blocks = list(model.transformer.resblocks)
    for i, blk in enumerate(blocks):
        cls = cls_only and i + 1 == len(blocks)
        sites = lora.blocks[i] if lora is not None else {}
        if drop[i] is None:
            xs = _block(model, blk, sites, xs, F, N, cls, recompute)
            continue
        # drop path: the block sees the K kept frames only; the stream of the others passes by, bit for bit
        keep_l, slot_l, s_l = drop[i]
        x_sub, xs = ag.FrameGatherFn.apply(xs, keep_l, slot_l)
        y_sub = _block(model, blk, sites, x_sub, keep_l.numel(), N, cls, recompute)
        if cls:
            xs = _ClsRowsFn.apply(xs, F, N)
        xs = ag.DropPathMergeFn.apply(xs, y_sub, keep_l, slot_l, s_l)
    return xs, F, N, cls_only


def _block(model, blk, sites, xs, F, N, cls, recompute):
    """One residual block on the F frames of xs [F*N, D]; cls: the last block under cls_only, which returns the F class rows."""
    dt16, H = model.compute_dtype, model.heads
    if recompute == "block":
        return _BlockFn.apply(xs, (F, N, H, dt16, model.residual_dtype == torch.float32, cls),
                              *(blk.get_parameter(name) for name in _BLOCK_PARAMS))
    h, xs = ag.layernorm(xs, blk.ln_1.weight, blk.ln_1.bias, dt16, passthrough=True)
    qkv = _linear(sites.get("attn.in_proj"), h, blk.attn.in_proj_weight, blk.attn.in_proj_bias)
    o = ag.SelfAttnPackedFn.apply(qkv, None, F, N, H)
    if cls:
        o, xs = _ClsRowsFn.apply(o, F, N), _ClsRowsFn.apply(xs, F, N)
    xs = _linear(sites.get("attn.out_proj"), o, blk.attn.out_proj.weight, blk.attn.out_proj.bias, res=xs,
                 out_f32=(model.residual_dtype == torch.float32))
    h, xs = ag.layernorm(xs, blk.ln_2.weight, blk.ln_2.bias, dt16, passthrough=True)
    u = _linear(sites.get("mlp.c_fc"), h, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, act=ops.ACT_QUICKGELU)
    return _linear(sites.get("mlp.c_proj"), u, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, res=xs,
                   out_f32=(model.residual_dtype == torch.float32))


def _linear(site, x, weight, bias, **kw):
    """ag.linear, or the adapted linear of lora.py where the block carries adapters on this weight."""
    if site is None:
        return ag.linear(x, weight, bias, **kw)
    from .lora import lora_linear
    return lora_linear(site, x, bias, **kw)


RECOMPUTE_MODES = ("none", "block")
_BLOCK_PARAMS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                 "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")


class _Ctx:
    """What a per-op Function's forward and backward use of their ``ctx``, without an autograd node behind it: _BlockFn runs the
    Functions' static methods itself, in the order the engine runs the nodes of the same block."""

    def __init__(self, *needs_input_grad):
        self.needs_input_grad = needs_input_grad
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _block_forward(xs, meta, params, keep):
    """One residual block through the same Function bodies, with the same arguments, as the loop of vit_tokens_train (the training
    launches: weight copies made with ``both=True``, the c_fc pre-activation written as a side output).  keep: return the contexts
    the backward needs; otherwise they die here, and with them everything but the block's output."""
    F, N, H, dt16, out_f32, cls = meta
    ln1_w, ln1_b, in_w, in_b, out_w, out_b, ln2_w, ln2_b, fc_w, fc_b, proj_w, proj_b = params
    c = {k: _Ctx(*need) for k, need in (("ln_1", (True,)), ("in_proj", (True,)), ("attn", (True,)), ("cls_o", (True,)), ("cls_x", (True,)),
                                        ("out_proj", (True, True, True, True)), ("ln_2", (True,)), ("c_fc", (True,)),
                                        ("c_proj", (True, True, True, True)))}
    h, xs = ag.LayerNormFn.forward(c["ln_1"], xs, ln1_w, ln1_b, dt16, True, False)
    qkv = ag.LinearFn.forward(c["in_proj"], h, in_w, in_b, None, ag.ACT_NONE, False)
    o = ag.SelfAttnPackedFn.forward(c["attn"], qkv, None, F, N, H)
    if cls:
        o, xs = _ClsRowsFn.forward(c["cls_o"], o, F, N), _ClsRowsFn.forward(c["cls_x"], xs, F, N)
    xs = ag.LinearFn.forward(c["out_proj"], o, out_w, out_b, xs, ag.ACT_NONE, out_f32)
    h, xs = ag.LayerNormFn.forward(c["ln_2"], xs, ln2_w, ln2_b, dt16, True, False)
    u = ag.LinearFn.forward(c["c_fc"], h, fc_w, fc_b, None, ops.ACT_QUICKGELU, False)
    xs = ag.LinearFn.forward(c["c_proj"], u, proj_w, proj_b, xs, ag.ACT_NONE, out_f32)
    return (xs, c) if keep else (xs, None)


class _BlockFn(torch.autograd.Function):
    """A residual block as ONE autograd node that saves its input stream only (``model.recompute = "block"``).  The backward runs the
    block's forward again from that input and then the backward bodies of the per-op Functions, in the engine's order for the same
    block: the kernels and their operands are those of the per-op path, so outputs and gradients are the same bits.  The weight
    gradients are parked in the surrounding pass's wgrad_queue (no nested engine pass) and leave at the end of the block, and the
    16-bit weight copies are the cached ones of the first forward (nothing has stepped in between)."""

    @staticmethod
    def forward(ctx, xs, meta, *params):
        ctx.save_for_backward(xs)
        ctx.meta, ctx.params = meta, params
        return _block_forward(xs, meta, params, keep=False)[0]

    @staticmethod
    def backward(ctx, dy):
        (xs,) = ctx.saved_tensors
        cls = ctx.meta[5]
        _, c = _block_forward(xs, ctx.meta, ctx.params, keep=True)
        g = [None] * 12                                 # gradients of _BLOCK_PARAMS that are not written into an arena slot
        du, g[10], g[11], dres = ag.LinearFn.backward(c.pop("c_proj"), dy)[:4]
        dh, g[8], g[9] = ag.LinearFn.backward(c.pop("c_fc"), du)[:3]
        dxs, g[6], g[7] = ag.LayerNormFn.backward(c.pop("ln_2"), dh, dres)[:3]
        do, g[4], g[5], dres = ag.LinearFn.backward(c.pop("out_proj"), dxs)[:4]
        if cls:
            dres = _ClsRowsFn.backward(c.pop("cls_x"), dres)[0]
            do = _ClsRowsFn.backward(c.pop("cls_o"), do)[0]
        dqkv = ag.SelfAttnPackedFn.backward(c.pop("attn"), do)[0]
        dh, g[2], g[3] = ag.LinearFn.backward(c.pop("in_proj"), dqkv)[:3]
        dx, g[0], g[1] = ag.LayerNormFn.backward(c.pop("ln_1"), dh, dres)[:3]
        # the parked weight-gradient problems hold this block's recomputed activations and their gradients (32 D bytes per row): they
        # leave now, as one group per block, so that nothing of a recomputed block outlives its backward.  A tile's arithmetic does
        # not depend on what shares its launch, so the gradients are the bits of the larger groups of the per-op path
        ag.wgrad_queue.flush()
        return (dx, None, *g)


def saved_activation_bytes(geometry, frames: int, recompute: str = "none", bytes16: int = 2, residual_bytes: int = 4,
                           cls_only: bool = True, tokens: int = None, drop_path: float = 0.0) -> int:
    """Bytes the residual blocks of the training forward keep for the backward pass (what the per-op Functions of autograd_ops
    hand to ``save_for_backward``; the patch GEMM, ln_pre, ln_post and the projection are not counted).
    geometry: a model name or (resolution, patch, width, layers, heads, output_dim).
    "none": per token row and block the residual stream at ln_1 and at ln_2, the two LayerNorm outputs, qkv, the attention output,
    the c_fc pre-activation and the QuickGELU output -- (2 r + 14 b) D bytes (36 D for fp32 / 16-bit) -- plus lse (4 H) and two
    (mean, rstd) pairs (16).  With cls_only the last block keeps everything after its attention for the F class rows only.
    "block": one input stream per block, r D bytes per row.  During the backward one recomputed block ("none" with one layer, the
    last block's class-row shortcut aside) is alive on top of that.
    tokens: token rows per frame instead of the geometry's g^2 + 1 (patch dropout: Kp + 1).
    drop_path: block l keeps what it keeps today for K_l = max(1, int(F (1 - p_l))) of the F frames, p_l = drop_path l / max(1, L - 1)
    (the gather and the merge around it keep two int32 vectors, not counted)."""
    if recompute not in RECOMPUTE_MODES:
        raise ValueError(f"recompute must be one of {RECOMPUTE_MODES}, got {recompute!r}")
    if isinstance(geometry, str):
        from .synth import vit_geometry
        geometry = vit_geometry(geometry)
    R, p, D, L, H, _E = geometry
    N = (R // p) ** 2 + 1
    if tokens is not None:
        if not 2 <= tokens <= N:
            raise ValueError(f"tokens must be in 2..{N} for this geometry, got {tokens}")
        N = tokens
    if not 0.0 <= float(drop_path) < 1.0:
        raise ValueError(f"drop_path must satisfy 0 <= p < 1, got {drop_path}")
    r, b = residual_bytes, bytes16
    kept = [ops.drop_path_keep_count(frames, ops.drop_path_rate(drop_path, l, L)) for l in range(L)]      # all `frames` at 0
    if recompute == "block":
        return sum(K * N * r * D for K in kept)
    attn_half = (r + 5 * b) * D + 4 * H + 8          # stream at ln_1, ln_1 output, qkv, attention output; lse; (mean, rstd)
    mlp_half = (r + 9 * b) * D + 8                   # stream at ln_2, ln_2 output, z, u; (mean, rstd)
    full = N * (attn_half + mlp_half)                # per frame
    if not cls_only:
        return sum(K * full for K in kept)
    # the last block: out_proj reads a gathered copy of the class rows of the attention output (one more 16-bit row), then F rows
    return sum(K * full for K in kept[:-1]) + kept[-1] * (N * attn_half + b * D + mlp_half)


class _ClsRowsFn(torch.autograd.Function):
    """Select the class-token rows x[f*N] (a strided gather is memory plumbing); the backward scatters the
    gradient back into a zero matrix."""

    @staticmethod
    def forward(ctx, xs, F, N):
        ctx.meta = (F, N, xs.shape[1], xs.dtype)
        return xs.view(F, N, -1)[:, 0].contiguous()

    @staticmethod
    def backward(ctx, dcls):
        F, N, D, dtype = ctx.meta
        dx = torch.zeros((F, N, D), dtype=dtype, device=dcls.device)
        dx[:, 0].copy_(dcls if dcls.dtype == dtype else (ops.cast32(dcls.contiguous()) if dtype == torch.float32
                                                          else ops.cast16(dcls.contiguous(), dtype)))
        return dx.view(F * N, D), None, None


class _ProjFn(torch.autograd.Function):
    """y = x @ proj  with proj stored [D, E] (OpenAI clip ``x @ self.proj``): linear with W = proj^T."""

    @staticmethod
    def forward(ctx, x16, proj):
        wT = ag.weights.get(proj, x16.dtype, transposed=True)                     # [E, D]
        ctx.save_for_backward(x16)
        ctx.proj = proj
        return ops.linear(x16, wT, out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, dy):
        (x16,) = ctx.saved_tensors
        proj = ctx.proj
        dt16 = x16.dtype
        M, D = x16.shape
        E = proj.shape[1]
        dy16 = ops.cast16(dy.contiguous(), dt16)
        w = ag.weights.get(proj, dt16, pad_k=(E % 64 != 0))                       # [D, Epad]
        dyp = dy16
        if w.shape[1] != E:
            dyp = torch.zeros((M, w.shape[1]), dtype=dt16, device=dy16.device)
            dyp[:, :E].copy_(dy16)
        dx = ops.linear(dyp, w)                                                    # [M,E] @ [D,E]^T -> [M,D]
        out = ag._grad_out(proj, (D, E))
        if D % 8 == 0 and E % 8 == 0:
            ops.wgrad_tn(x16, dy16, out)                                            # dproj[D,E] = x^T dy
        else:
            Mp = ag._pad64(M)
            xt = torch.zeros((D, Mp), dtype=dt16, device=x16.device)
            ag.check(ag.lib.vmc_transpose16(ag.ptr(x16), ag.ptr(xt), M, D, x16.stride(0), Mp, ag.stream()), "transpose16")
            dyt = torch.zeros((E, Mp), dtype=dt16, device=x16.device)
            ag.check(ag.lib.vmc_transpose16(ag.ptr(dy16), ag.ptr(dyt), M, E, dy16.stride(0), Mp, ag.stream()), "transpose16")
            ops.linear_wgrad(xt, dyt, out)
        return dx, ag._deliver(proj, out)


def vit_forward_train(model, x: torch.Tensor, wrap_quirk: bool = False, keep: torch.Tensor = None, drop_keep=None) -> torch.Tensor:
    """[F,3,R,R] -> [F,E] f32 embeddings, differentiable w.r.t. every ViT parameter.  keep, drop_keep: see vit_tokens_train."""
    xs, F, N, rows_are_cls = vit_tokens_train(model, x, wrap_quirk, cls_only=getattr(model, "cls_only_last_block", True), keep=keep,
                                              drop_keep=drop_keep)
    cls = xs if rows_are_cls else _ClsRowsFn.apply(xs, F, N)
    h = ag.layernorm(cls, model.ln_post.weight, model.ln_post.bias, model.compute_dtype)
    return _ProjFn.apply(h, model.proj)
