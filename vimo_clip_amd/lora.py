"""LoRA adapters on the linears of the CLIP ViT tower (parameter-efficient fine-tuning of the student).

``add_lora(vit, rank)`` freezes the tower and registers rank-r fp32 adapters A [r, K], B [N, r] beside the chosen linears;
``autograd_vit.vit_tokens_train`` then runs those linears through ``LoraLinearFn``:

    ts   = round16(s (x A16^T))                       vmc_lora_down_concat, which also copies x:  xcat = [x | ts | 0]      [M, K + 64 (+ 64)]
    y    = vmc_linear / vmc_linear_preact on xcat and Wcat = [W16 | B16 | 0]  [N, K + 64 (+ 64)]   (the adapter term is one more K tile;
                                                      both are zero-padded to a multiple of 128 columns: cat_width)
    dz   = round16(dy), then the activation backward                                             as LinearFn
    us   = round16(s (dz B16))                        vmc_lora_down_concat on dz and B16^T:       dzcat = [dz | us | 0]    [M, N + 64 (+ 64)]
    dx   = vmc_linear on dzcat and WcatT = [W16^T | A16^T | 0]  [K, N + 64 (+ 64)]
    dA   = us^T x,  dB = dz^T ts                      vmc_lora_wgrad_tn on column windows of the two concat buffers

with s = alpha / r.  No weight gradient of the frozen W is formed, the gradient arena (optim.GradArena, built AFTER add_lora) holds
adapters and heads only, and the optimiser, clipping, accumulation, the loss scale and the data-parallel reducer work unchanged.
``merge_lora`` folds W += s B A into the fp32 masters and removes the adapters: the model is back on the inference path with the
reference's ``state_dict`` keys.  There is no merged-forward mode: round16(W + s B A) loses small updates in bf16.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import autograd_ops as ag
from . import ops
from ._lib import check, dt, lib, ptr, stream

TAIL = ops.LORA_TAIL


def cat_width(k: int) -> int:
    """Columns of a concat buffer behind k operand columns: the 64-column adapter tail, then zeros up to a multiple of 128.  The zeros
    change no sum; gemm_route.h sends a K that is no multiple of 128 to the two-stage tile kernel (measured 135 us against 70-85 us
    for the 8-phase kernels on the ViT-B/32 linears), and K + 64 of a tower linear never is one."""
    return (k + TAIL + 127) // 128 * 128


def _concat(x, a16, site):
    """[x | round16(s x a16^T) | 0] with cat_width(K) columns: the kernel writes K + 64 of them, a strided fill the rest."""
    M, K = x.shape
    out = torch.empty((M, cat_width(K)), dtype=x.dtype, device=x.device)
    ops.lora_down_concat(x, a16, site.rank, site.scale, out=out)
    if out.shape[1] > K + TAIL:
        out[:, K + TAIL:].zero_()                    # memory plumbing: 128 bytes per row
    return out


TARGETS = ("attn", "mlp")
# target -> (site name, module path inside a block, weight attribute, bias attribute, A / B parameter names on that module)
_SITES = {
    "attn": (("attn.in_proj", "attn", "in_proj_weight", "in_proj_bias", "in_proj_lora_A", "in_proj_lora_B"),
             ("attn.out_proj", "attn.out_proj", "weight", "bias", "lora_A", "lora_B")),
    "mlp": (("mlp.c_fc", "mlp.c_fc", "weight", "bias", "lora_A", "lora_B"),
            ("mlp.c_proj", "mlp.c_proj", "weight", "bias", "lora_A", "lora_B")),
}


class LoraSite:
    """One adapted linear: the frozen weight, its adapters and the 16-bit operands the kernels read (built by LoraState.refresh)."""

    def __init__(self, name, module, w_attr, a_attr, b_attr, rank, scale):
        self.name, self.module, self.w_attr, self.a_attr, self.b_attr = name, module, w_attr, a_attr, b_attr
        self.rank, self.scale = rank, scale
        self.wcat = self.wcat_t = self.a16 = self.b16_t = None
        self.base_key = None

    weight = property(lambda self: getattr(self.module, self.w_attr))
    A = property(lambda self: getattr(self.module, self.a_attr))
    B = property(lambda self: getattr(self.module, self.b_attr))


class LoraState:
    """What ``add_lora`` leaves on the tower as ``vit.lora``: the sites per block and the 16-bit copies.

    Wcat / WcatT are cast once per version of the frozen weight.  Their 64-column tails and the stand-alone A16 / B16^T of ALL sites
    are re-cast in place by one vmc_cast_weights_multi launch whenever an adapter may have changed (its version counter, its
    storage, or autograd_ops.weights.epoch, which every optimiser step bumps).  The buffers keep their addresses."""

    def __init__(self, rank, alpha, targets):
        self.rank, self.alpha, self.targets = rank, alpha, tuple(targets)
        self.scale = alpha / rank
        self.blocks = []            # per residual block: {site name: LoraSite}
        self.restore = []           # (parameter, requires_grad before add_lora)
        self._dtype16 = None
        self._table = None          # (pointer key, device records, n, tiles)
        self._old_tables = []       # a captured graph may still read an older table
        self._fresh = None

    def sites(self):
        return [s for blk in self.blocks for s in blk.values()]

    def parameters(self):
        return [p for s in self.sites() for p in (s.A, s.B)]

    def refresh(self, dtype16):
        sites = self.sites()
        if self._dtype16 != dtype16:
            for s in sites:
                N, K = s.weight.shape
                dev = s.weight.device
                s.wcat = torch.zeros((N, cat_width(K)), dtype=dtype16, device=dev)
                s.wcat_t = torch.zeros((K, cat_width(N)), dtype=dtype16, device=dev)
                s.a16 = torch.zeros((s.rank, K), dtype=dtype16, device=dev)
                s.b16_t = torch.zeros((s.rank, N), dtype=dtype16, device=dev)
                s.base_key = None
            self._dtype16, self._table, self._fresh = dtype16, None, None
        for s in sites:
            w = s.weight
            key = (w._version, w.data_ptr())
            if s.base_key != key:
                N, K = w.shape
                check(lib.vmc_cast_weight(ptr(w.detach()), ptr(s.wcat), ptr(s.wcat_t), N, K, s.wcat.stride(0), s.wcat_t.stride(0), dt(dtype16),
                                          stream()), "cast_weight")
                s.base_key = key
        ptrs = tuple(p.data_ptr() for p in self.parameters())
        fresh = (ag.weights.epoch, ptrs, tuple(p._version for p in self.parameters()))
        if fresh == self._fresh:
            return
        if self._table is None or self._table[0] != ptrs:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LoRA copy table changed while a graph is being captured: run one eager step first")
            self._table = self._build_table(sites, ptrs)
            self._old_tables.append(self._table[1])
        check(lib.vmc_cast_weights_multi(ptr(self._table[1]), self._table[2], self._table[3], dt(dtype16), stream()), "cast_weights_multi")
        self._fresh = fresh

    @staticmethod
    def _build_table(sites, ptrs):
        """The records of vmc_cast_weights_multi (include/vmc.h): A [r, K] -> A16 and, transposed, the tail of WcatT; B [N, r] -> the
        tail of Wcat and, transposed, B16^T."""
        import numpy as np
        rec = np.zeros((2 * len(sites), 6), dtype=np.int64)
        tile0 = 0
        for i, s in enumerate(sites):
            N, K = s.weight.shape
            for j, (p, w16, w16_t) in enumerate(((s.A, s.a16, s.wcat_t[:, N:]), (s.B, s.wcat[:, K:], s.b16_t))):
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise TypeError(f"LoRA adapter {s.name}: adapters are contiguous float32 parameters")
                rows, cols = p.shape
                tx, ty = (cols + 63) // 64, (rows + 63) // 64
                rec[2 * i + j] = (p.data_ptr(), w16.data_ptr(), w16_t.data_ptr(), rows | (cols << 32), w16.stride(0) | (w16_t.stride(0) << 32),
                                  tile0 | (tx << 32))
                tile0 += tx * ty
        return ptrs, torch.from_numpy(rec).to(sites[0].weight.device), 2 * len(sites), tile0


def _module_at(block, path):
    m = block
    for part in path.split("."):
        m = getattr(m, part)
    return m


def add_lora(vit, rank: int, alpha: float = None, targets=("attn",), freeze_base: bool = True) -> LoraState:
    """Rank-`rank` adapters on the linears of every residual block of `vit` (a VisionTransformer).  targets: "attn" (in_proj and
    out_proj), "mlp" (c_fc and c_proj).  A: kaiming_uniform_(a = sqrt 5), B: zeros -- the adapted tower starts as the base tower.
    alpha: default 2 rank; the adapter term is scaled by alpha / rank.  freeze_base: requires_grad = False on every parameter of the
    tower (the adapted weights are frozen either way: LoraLinearFn forms no dW).  Build the GradArena after this call."""
    if getattr(vit, "lora", None) is not None:
        raise ValueError("add_lora: the tower already carries adapters (merge_lora first)")
    rank = int(rank)
    if rank < 8 or rank > TAIL or rank % 8:
        raise ValueError(f"add_lora: rank must be a multiple of 8 in 8..{TAIL}, got {rank}")
    targets = (targets,) if isinstance(targets, str) else tuple(targets)
    if not targets or any(t not in TARGETS for t in targets):
        raise ValueError(f"add_lora: targets must be drawn from {TARGETS}, got {targets}")
    if getattr(vit, "recompute", "none") != "none":
        raise ValueError("LoRA adapters are not supported together with recompute='block'")
    alpha = float(2 * rank if alpha is None else alpha)
    st = LoraState(rank, alpha, [t for t in TARGETS if t in targets])
    st.restore = [(p, p.requires_grad) for p in vit.parameters()]
    if freeze_base:
        for p in vit.parameters():
            p.requires_grad_(False)
    for blk in vit.transformer.resblocks:
        sites = {}
        for t in st.targets:
            for name, path, w_attr, _b, a_attr, b_attr in _SITES[t]:
                mod = _module_at(blk, path)
                w = getattr(mod, w_attr)
                N, K = w.shape
                if K % 64 or N % 64:
                    raise ValueError(f"add_lora: {name} is {N} x {K}; adapted linears need both multiples of 64")
                w.requires_grad_(False)
                A = nn.Parameter(torch.empty((rank, K), dtype=torch.float32, device=w.device))
                nn.init.kaiming_uniform_(A, a=math.sqrt(5))
                mod.register_parameter(a_attr, A)
                mod.register_parameter(b_attr, nn.Parameter(torch.zeros((N, rank), dtype=torch.float32, device=w.device)))
                sites[name] = LoraSite(name, mod, w_attr, a_attr, b_attr, rank, st.scale)
        st.blocks.append(sites)
    vit.lora = st
    return st


def merge_lora(vit) -> None:
    """W += s B A in the fp32 masters, on the device, then the adapters are removed and every ``requires_grad`` is what it was before
    ``add_lora``: the model has the reference's ``state_dict`` keys again and runs the unchanged inference path.  A one-off at
    checkpoint time (one fp32 GEMM per site through torch), not part of a step."""
    st = getattr(vit, "lora", None)
    if st is None:
        raise ValueError("merge_lora: the tower carries no adapters")
    with torch.no_grad():
        for s in st.sites():
            s.weight.addmm_(s.B.detach(), s.A.detach(), alpha=st.scale)
            delattr(s.module, s.a_attr)
            delattr(s.module, s.b_attr)
    for p, req in st.restore:
        p.requires_grad_(req)
    del vit.lora


def merged_state_dict(model) -> dict:
    """``model.state_dict()`` (clones) as ``merge_lora`` would leave it -- W + s B A in place of every adapted weight, no adapter
    keys -- without touching the live adapters: what a checkpoint written in the middle of training holds.  `model`: the tower or
    any module that contains towers (FlowStudentModel)."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for prefix, mod in model.named_modules():
        st = getattr(mod, "lora", None)
        if not isinstance(st, LoraState):
            continue
        pre = prefix + "." if prefix else ""
        names = {id(p): n for n, p in mod.named_parameters()}
        for s in st.sites():
            sd[pre + names[id(s.weight)]].addmm_(s.B.detach(), s.A.detach(), alpha=st.scale)
            del sd[pre + names[id(s.A)]], sd[pre + names[id(s.B)]]
    return sd


def lora_state_dict(vit) -> dict:
    """The adapters alone, under their ``state_dict`` names inside the tower, plus ``lora.rank`` / ``lora.alpha`` / ``lora.targets``."""
    st = getattr(vit, "lora", None)
    if st is None:
        raise ValueError("lora_state_dict: the tower carries no adapters")
    sd = {k: v.detach().clone() for k, v in vit.state_dict().items() if "lora_" in k}
    sd.update({"lora.rank": st.rank, "lora.alpha": st.alpha, "lora.targets": list(st.targets)})
    return sd


def load_lora_state_dict(vit, sd: dict) -> None:
    """Copy adapters saved by ``lora_state_dict`` into a tower that carries the same adapters (add_lora with the same rank / targets)."""
    st = getattr(vit, "lora", None)
    if st is None:
        raise ValueError("load_lora_state_dict: call add_lora first")
    if int(sd.get("lora.rank", st.rank)) != st.rank or list(sd.get("lora.targets", st.targets)) != list(st.targets):
        raise ValueError("load_lora_state_dict: rank / targets differ from the tower's adapters")
    own = {k: v for k, v in vit.named_parameters() if "lora_" in k}
    keys = {k for k in sd if not k.startswith("lora.")}
    if keys != set(own):
        raise KeyError(f"load_lora_state_dict: key mismatch: {sorted(keys ^ set(own))}")
    with torch.no_grad():
        for k, p in own.items():
            p.copy_(sd[k])
    if "lora.alpha" in sd and float(sd["lora.alpha"]) != st.alpha:
        st.alpha = float(sd["lora.alpha"])
        st.scale = st.alpha / st.rank
        for s in st.sites():
            s.scale = st.scale


# ------------------------------------------------------------------------------------------------
# the adapted linear
# ------------------------------------------------------------------------------------------------
class LoraLinearFn(torch.autograd.Function):
    """y = act(x W^T + s (x A^T) B^T + b) (+ res) with W frozen: LinearFn's role for a linear that carries adapters.  A and B are
    inputs so that the node lives where x itself needs no gradient (the first block of a frozen tower).  Saves xcat in place of x."""

    @staticmethod
    def forward(ctx, x, A, B, bias, res, act, out_f32, site, inference):
        dt16 = x.dtype
        weight = site.weight
        N, K = weight.shape
        if x.shape[1] != K:
            raise ValueError(f"LoraLinearFn: x has {x.shape[1]} columns, weight needs {K}")
        xcat = _concat(x, site.a16, site)
        b = bias.detach() if bias is not None else None
        z = None
        if act != ag.ACT_NONE:
            if res is not None:
                raise ValueError("LoraLinearFn: activation and residual are not combined on this path")
            if inference:
                return ops.linear(xcat, site.wcat, bias=b, act=act, out_dtype=torch.float32 if out_f32 else dt16)
            if act == ops.ACT_RELU:
                z = y = ops.linear(xcat, site.wcat, bias=b, act=act)
            else:
                z = torch.empty((x.shape[0], N), dtype=dt16, device=x.device)
                y = ops.linear(xcat, site.wcat, bias=b, act=act, z_out=z)
            if out_f32:
                y = ops.cast32(y)
        else:
            y = ops.linear(xcat, site.wcat, bias=b, res=res, out_dtype=torch.float32 if out_f32 else dt16)
        if inference:
            return y
        ctx.save_for_backward(xcat, z)
        ctx.site, ctx.A, ctx.B, ctx.bias, ctx.act = site, A, B, bias, act
        ctx.has_res = res is not None
        ctx.res_dtype = res.dtype if res is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        xcat, z = ctx.saved_tensors
        site, A, B, bias, act = ctx.site, ctx.A, ctx.B, ctx.bias, ctx.act
        dt16 = xcat.dtype
        N, K = site.weight.shape
        r = site.rank
        dy = dy.contiguous()
        dy16 = ops.cast16(dy, dt16)
        dz = ops.act_bwd(z, dy16, act) if act != ag.ACT_NONE else dy16
        dres = None
        if ctx.has_res and ctx.needs_input_grad[4]:
            dres = dy if dy.dtype == ctx.res_dtype else (ops.cast32(dy) if ctx.res_dtype == torch.float32 else dy16)
        dzcat = _concat(dz, site.b16_t, site)                                             # [dz | us | 0]
        dx = ops.linear(dzcat, site.wcat_t) if ctx.needs_input_grad[0] else None          # dz W16 + us A16
        dA = dB = db = None
        if A.requires_grad:
            dA = ops.lora_wgrad_tn(dzcat[:, N:N + r], xcat[:, :K], ag._grad_out(A, (r, K)))
        if B.requires_grad:
            dB = ops.lora_wgrad_tn(xcat[:, K:K + r], dzcat[:, :N], ag._grad_out(B, (N, r)), transpose_out=True)
        if bias is not None and bias.requires_grad:
            db = ops.colsum(dz)
        return dx, ag._deliver(A, dA), ag._deliver(B, dB), ag._deliver(bias, db), dres, None, None, None, None


def lora_linear(site: LoraSite, x, bias=None, res=None, act=ag.ACT_NONE, out_f32=False):
    return LoraLinearFn.apply(x, site.A, site.B, bias, res, act, out_f32, site, not torch.is_grad_enabled())
