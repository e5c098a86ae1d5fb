"""Float64 reference, designed-rounding model, inputs and case list for ONE TRAINING STEP of the student: the ViT tower through
autograd_vit.vit_forward_train and the heads of FlowStudentModel._heads (autograd_ops' Functions over the libvmc kernels).  No GPU
code: torch and numpy on the CPU.  tests/test_student_step_refs_host.py checks everything in here on the CPU (against the oracle and
attention_refs, the conditions on the inputs, the measure on itself and ten mutants); tests/test_gpu_student_step_parity.py compares
what the backward pass leaves in the gradient arena (or in ``.grad``).

``step_ref64`` is one step in float64 autograd with the upstream gradients GIVEN (the loss is no part of it), on the values the
kernels see: 16-bit compute copies of the weight matrices widened, fp32 biases / LayerNorm parameters / class and positional
embeddings, u8 frames.  ``step_model16`` is the same graph with the roundings the path is designed to make (DESIGN.md §5.4 lists
each with its line in the code; none is taken from kernel output).  The measure, the rounding carriers ``_RoundFwd`` / ``_RoundGrad``,
the ``Policy`` that owns them and the ReLU calibration are tfam_chain_refs' (DESIGN.md §5.3); the attention is attention_refs'.

Two levels.  *tower*: frames -> embeddings E [F, E] with upstream dE; outputs E and the gradient of every VisionTransformer
parameter.  *student*: frames -> (emb, emb_distill, logits) with upstream (d emb, d emb_distill, d logits); adds the gradients of
residual_mlp.fc1 / fc2 and classification_head.0 / .2.  Gradient tensors are named "g." + the parameter's name inside
VisionTransformer ("g.transformer.resblocks.0.attn.in_proj_bias") or inside FlowStudentModel for the heads ("g.residual_mlp.fc1.weight").
"""
import functools

import numpy as np
import torch

import attention_refs as AR
import tfam_chain_refs as TC
from attention_refs import R_MAX, R_RMS, VAC_MAX, VAC_RMS      # noqa: F401  (the measure's constants: imported, never restated)
from oracle.vit import CLIP_MEAN, CLIP_STD
from tfam_chain_refs import Policy, failures, measure, measure_all, tensor_names, vacuity      # noqa: F401
from train_kernel_refs import BF16, EPS32, F16, F32

F64 = torch.float64
WIDTH, HEADS, LAYERS = 128, 2, 2
ALPHA = float(np.float32(0.1))            # ResidualMLP.alpha as vmc_axpby_f32 receives it (a C float)
BLOCK_PARAMS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
HEAD_PARAMS = ("residual_mlp.fc1.weight", "residual_mlp.fc1.bias", "residual_mlp.fc2.weight", "residual_mlp.fc2.bias",
               "classification_head.0.weight", "classification_head.0.bias", "classification_head.2.weight", "classification_head.2.bias")
MUTANTS = ("cls_grad_one_frame", "pos_grad_no_cls_row", "ln_no_dpass", "cls_scatter_drops_kv", "in_proj_bias_last_tile",
           "quickgelu_grad_at_u", "conv1_grad_pad_cols", "proj_grad_transposed", "pool_div", "fork_one_branch")
# the case each mutant of the float32 evaluation must fail: conv1_grad_pad_cols needs a padded K (3 p^2 = 48), proj_grad_transposed
# D != E, the last two the heads
MUTANT_CASE = {"cls_grad_one_frame": "a", "pos_grad_no_cls_row": "a", "ln_no_dpass": "b", "cls_scatter_drops_kv": "c",
               "in_proj_bias_last_tile": "b", "quickgelu_grad_at_u": "a", "conv1_grad_pad_cols": "d", "proj_grad_transposed": "d",
               "pool_div": "s1", "fork_one_branch": "s2"}
# Upstream gradients = N(0, 1) times this power of two.  f16: chosen (on the CPU, from model16 alone) so that no stored 16-bit
# gradient exceeds 2^14 and fewer than 1 % of the non-zero elements of any of them are f16-subnormal; the host test asserts both.
UP_SCALE = {BF16: 1.0, F16: 2.0 ** 9}


# ---------------------------------------------------------------------------------------------- cases
def _case(name, R, p, E, F, level="tower", cls_only=True, arena=True, B=0, T=0, C=0, seed=0):
    """parks_stream / parks_conv1: the weight gradients of the linears on all F N token rows / of the patch GEMM on its F (N - 1)
    rows leave through autograd_ops.wgrad_queue as a grouped launch (LinearFn.backward: an arena slot, an unpadded K, and
    ops.wgrad_group_ok -- whole 128-row pairs, at least 256 rows); everything else takes the per-linear launch."""
    g = R // p
    N, K = g * g + 1, 3 * p * p
    whole = lambda rows: arena and rows >= 256 and rows % 128 == 0
    return dict(name=name, level=level, R=R, p=p, E=E, F=F, N=N, K=K, cls_only=cls_only, arena=arena, B=B, T=T, C=C, seed=seed,
                parks_stream=whole(F * N), parks_conv1=whole(F * (N - 1)) and K % 64 == 0)


CASES = [
    _case("a", 64, 16, 64, 3, seed=1),
    _case("b", 56, 8, 64, 3, seed=2),
    _case("c", 64, 8, 64, 3, seed=3),
    _case("d", 56, 4, 96, 3, seed=4),
    _case("e", 64, 4, 64, 3, seed=5),
    _case("f", 96, 4, 96, 2, seed=6),
    _case("g", 64, 16, 64, 3, cls_only=False, seed=1),
    _case("h", 56, 8, 64, 3, arena=False, seed=2),
    _case("i", 56, 8, 64, 64, seed=9),               # case b's geometry at 64 frames: 3200 = 25 x 128 token rows
    _case("s1", 64, 16, 64, 4, level="student", B=2, T=2, C=140, seed=7),
    _case("s2", 64, 8, 64, 4, level="student", B=2, T=2, C=10, seed=15),
]
BY_NAME = {c["name"]: c for c in CASES}


def param_shapes(c):
    """name -> shape of every parameter of the case, under the names of VisionTransformer (and of FlowStudentModel for the heads)."""
    D, E, N, p = WIDTH, c["E"], c["N"], c["p"]
    s = {"conv1.weight": (D, 3, p, p), "class_embedding": (D,), "positional_embedding": (N, D), "ln_pre.weight": (D,), "ln_pre.bias": (D,)}
    for i in range(LAYERS):
        pre = f"transformer.resblocks.{i}."
        for n, sh in zip(BLOCK_PARAMS, ((D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,))):
            s[pre + n] = sh
    s.update({"ln_post.weight": (D,), "ln_post.bias": (D,), "proj": (D, E)})
    if c["level"] == "student":
        for n, sh in zip(HEAD_PARAMS, ((E, E), (E,), (E, E), (E,), (E // 2, E), (E // 2,), (c["C"], E // 2), (c["C"],))):
            s[n] = sh
    return s


def is_matrix(name):
    """Parameters the GEMMs read through a 16-bit compute copy (autograd_ops.weights.get)."""
    return name == "proj" or (name.endswith("weight") and ".ln_" not in name and not name.startswith("ln_"))


def _fan_in(name, shape):
    return shape[0] if name == "proj" else int(np.prod(shape[1:]))


@functools.lru_cache(maxsize=None)
def make_inputs(name, dtype):
    """Everything one step reads: fp32 masters, their 16-bit copies, u8 frames, upstream gradients.  Matrices N(0, 1) / sqrt(K),
    biases N(0, 1) / 4, LayerNorm 1 + N / 4 and N / 4, class / positional embeddings N(0, 1): LayerNorm outputs and
    pre-activations of order one everywhere.

    The q and k rows of every in_proj are then scaled by ``stress`` (the idea of synth.vit_state_dict), stepped up until the float64
    forward shows an attention that is not trivially uniform (median over rows of the largest probability >= 4 / N in every
    block), and -- student level -- classification_head.0's bias is moved off the ReLU edge (tfam_chain_refs._relu_gap_bias)."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(9000 + c["seed"])
    rn = lambda *s, scale=1.0, shift=0.0: torch.randn(*s, generator=g) * scale + shift
    p = {}
    for n, sh in param_shapes(c).items():
        if is_matrix(n):
            # classification_head.0 sees B = 2 pooled rows that differ by a third of their size (the class token's row is mostly the
            # class and positional embeddings, the same in every frame): eight times the scale, so that the two pre-activations of a
            # column lie far enough apart for the ReLU gap below
            p[n] = rn(*sh, scale=(8.0 if n == "classification_head.0.weight" else 1.0) * _fan_in(n, sh) ** -0.5)
        elif n.endswith("ln_1.weight") or n.endswith("ln_2.weight") or n in ("ln_pre.weight", "ln_post.weight"):
            p[n] = rn(*sh, scale=0.25, shift=1.0)
        elif n in ("class_embedding", "positional_embedding"):
            p[n] = rn(*sh)
        else:
            p[n] = rn(*sh, scale=0.25)
    inp = dict(case=c, dtype=dtype, p32=p)
    inp["frames"] = torch.randint(0, 256, (c["F"], 3, c["R"], c["R"]), generator=g, dtype=torch.int64).to(torch.uint8)
    s = UP_SCALE[dtype]
    if c["level"] == "tower":
        inp["up"] = {"E": rn(c["F"], c["E"]) * s}
    else:
        inp["up"] = {"emb": rn(c["F"], c["E"]) * s, "emb_distill": rn(c["F"], c["E"]) * s, "logits": rn(c["B"], c["C"]) * s}
    base = {n: v.clone() for n, v in p.items() if n.endswith("in_proj_weight")}
    for stress in (1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 4.0):
        for n, v in base.items():
            p[n] = torch.cat([v[:2 * WIDTH] * stress, v[2 * WIDTH:]])
        inp["w16"] = {n: v.to(dtype) for n, v in p.items() if is_matrix(n)}
        with torch.no_grad():
            probe = run_step(inp, Policy(), probe=True)
        if min(probe["attn_peak"]) >= 4.0 / c["N"]:
            break
    inp["stress"], inp["attn_peak"] = stress, probe["attn_peak"]
    if c["level"] == "student":
        b, margin = TC._relu_gap_bias(probe["head_z0"], p["classification_head.0.bias"].to(F64))
        p["classification_head.0.bias"] = b
        inp["relu_margin"] = margin
    return inp


# ---------------------------------------------------------------------------------------------- pieces of the graph
def _r16(x, dtype):
    return x.to(F32).to(dtype).to(x.dtype)


def patch_rows(frames_u8, p, pol, wrap=True):
    """u8 frames [F, 3, R, R] -> the patch GEMM's A operand [F g g, 3 p p], column (c p + dy) p + dx (elementwise.hip, `at`).
    The reference: ((v / 255) - mean) / std in float64.  The model: the kernel's own fp32 expression (v / 255 - mean) * (1 / std)
    rounded to the compute dtype -- the training path takes vmc_preprocess_patches_u8, not the split-precision operands."""
    v = frames_u8.to(torch.int64)
    if wrap:
        v = (256 - v) % 256                       # the float -> PIL wrap quirk, v -> (256 - v) mod 256
    if pol.dtype is None:
        mean, std = (torch.tensor(t, dtype=F64).view(1, 3, 1, 1) for t in (CLIP_MEAN, CLIP_STD))
        pix = (v.to(F64) / 255.0 - mean) / std
    else:
        mean, std = (torch.tensor(t, dtype=F32).view(1, 3, 1, 1) for t in (CLIP_MEAN, CLIP_STD))
        pix = ((v.to(F32) / 255.0 - mean) * (1.0 / std)).to(pol.dtype).to(F64)
    F, _, R, _ = pix.shape
    g = R // p
    return pix.reshape(F, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(F * g * g, 3 * p * p).to(pol.compute)


def _quickgelu(z):
    return z * torch.sigmoid(1.702 * z)


def _quickgelu_grad(z):
    s = torch.sigmoid(1.702 * z)
    return s * (1.0 + 1.702 * z * (1.0 - s))


_ACT = {"quickgelu": (_quickgelu, _quickgelu_grad), "gelu": (torch.nn.functional.gelu, TC._gelu_grad),
        "relu": (torch.relu, lambda y: (y > 0).to(y.dtype))}


class _ActSaved(torch.autograd.Function):
    """y = round16(act(z)) on the fp32 accumulator (gemm_common.h: bias, the z16 side store, apply_act, the store); the backward is
    vmc_act_bwd on round16(dy) and the SAVED 16-bit tensor -- z16 = round16(z) for QuickGELU / GELU, the fused output y itself for
    ReLU -- stored 16-bit.  at_u (mutant quickgelu_grad_at_u): the derivative taken at the activation's output."""

    @staticmethod
    def forward(ctx, z, pol, kind, tag, at_u):
        y = _r16(_ACT[kind][0](z), pol.dtype)
        ctx.save_for_backward(y if (kind == "relu" or at_u) else _r16(z, pol.dtype))
        ctx.args = (pol, kind, tag)
        return y

    @staticmethod
    def backward(ctx, g):
        (saved,) = ctx.saved_tensors
        pol, kind, tag = ctx.args
        g16 = _r16(g, pol.dtype)
        pol.note(tag + ".dy16", g16)
        d = _r16(g16 * _ACT[kind][1](saved), pol.dtype)
        pol.note(tag + ".dz16", d)
        return d, None, None, None, None


class _VitAttn(torch.autograd.Function):
    """vmc_attention_vit_fwd (out 16-bit, lse fp32; attention_refs.vit_forward: the in-LDS family at every token count, streamed
    kernel included) paired with vmc_attention_bwd on the saved out / lse (the family attention_refs.bwd_family_of gives the kernel
    attn_route.h picks for this N).  rows_keep (mutant cls_scatter_drops_kv): dqkv survives on these rows only."""

    @staticmethod
    def forward(ctx, qkv, pol, F, N, rows_keep):
        D = WIDTH
        q, k, v = (qkv[:, i * D:(i + 1) * D].detach().to(F64) for i in range(3))
        shape = (F, HEADS, N, N, 64)
        r = AR.vit_forward(q, k, v, shape, pol.dtype)
        ctx.save_for_backward(q, k, v, r["out"], r["lse"])
        ctx.args = (pol, shape, rows_keep, qkv.dtype)
        return r["out"].to(qkv.dtype)

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, lse = ctx.saved_tensors
        pol, shape, rows_keep, cd = ctx.args
        N = shape[2]
        fam = AR.bwd_family_of({"bwd": AR.route_bwd(N, N, 64)[0]})
        r = AR._attn(q, k, v, None, g.to(F64), None, shape, dtype=pol.dtype, fam=fam, out_lse=(out, lse.to(F32)))
        dqkv = torch.cat([r["dq"], r["dk"], r["dv"]], 1)
        pol.note("attn.dqkv", dqkv)
        if rows_keep is not None:
            dqkv = dqkv * rows_keep[:, None]
        return dqkv.to(cd), None, None, None, None


class _ScaleGrad(torch.autograd.Function):
    """Identity whose gradient is scaled (mutant pool_div)."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def attn_plain(qkv, F, N):
    D = WIDTH
    return TC._attn_plain(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], None, None, (F, HEADS, N, N, 64))


# ---------------------------------------------------------------------------------------------- the step
def run_step(inp, pol, probe=False):
    """One step under `pol` (tfam_chain_refs.Policy: dtype None = the float64 reference; mutant = one of MUTANTS).  Returns float64
    tensors {"E" | "emb", "emb_distill", "logits", "g.<parameter>"} and, for the reference, "floor".  probe (make_inputs only):
    forward alone, returns the attention peaks and the bias-free pre-activation of classification_head.0."""
    c = inp["case"]
    F, N, p, E, D, K = c["F"], c["N"], c["p"], c["E"], WIDTH, c["K"]
    cd, mut, ref = pol.compute, pol.mutant, pol.dtype is None
    student = c["level"] == "student"
    leaves, absrec, peaks, extra = {}, [], [], {}

    def leaf(name):
        if name not in leaves:
            src = inp["w16"][name] if name in inp["w16"] else inp["p32"][name]
            leaves[name] = src.to(F64).to(cd).clone().requires_grad_(True)
        return leaves[name]

    def lin(x, wname, bname=None, b_override=None):
        W = leaf(wname)
        W = W.t() if wname == "proj" else W.reshape(W.shape[0], -1)
        y = x @ W.t()
        if bname is not None:
            y = y + (leaf(bname) if b_override is None else b_override)
        if ref and y.requires_grad:
            y.register_hook(lambda g, x=x.detach(), k=(wname, bname): absrec.append((k, g.abs(), x.abs())))
        return y

    def act(z, kind, tag, at_u=False):
        if ref:
            return _ACT[kind][0](z)
        return _ActSaved.apply(z, pol, kind, tag, at_u)

    def ln(x, name):
        return TC._layer_norm(x, leaf(name + ".weight"), leaf(name + ".bias"), pol)

    # ---- patch GEMM (16-bit output), token assembly into the fp32 stream, ln_pre (fp32 output)
    xp = pol.g(pol.r(lin(patch_rows(inp["frames"], p, pol), "conv1.weight")), "dxp16")
    cls, pos = leaf("class_embedding"), leaf("positional_embedding")
    cls_rows = cls.expand(F, 1, D)
    if mut == "cls_grad_one_frame":
        cls_rows = torch.cat([cls.detach().expand(1, 1, D), cls.expand(F - 1, 1, D)])
    pos_rows = torch.cat([pos[:1].detach(), pos[1:]]) if mut == "pos_grad_no_cls_row" else pos
    xs = (torch.cat([cls_rows, xp.reshape(F, N - 1, D)], 1) + pos_rows).reshape(F * N, D)
    if ref and xs.requires_grad:
        xs.register_hook(lambda g: extra.__setitem__("abs_dpos", g.abs().reshape(F, N, D).sum(0)))
    xs = ln(xs, "ln_pre")
    # ---- residual blocks
    for i in range(LAYERS):
        pre, last = f"transformer.resblocks.{i}.", i + 1 == LAYERS
        h = pol.g(pol.r(ln(xs, pre + "ln_1")), pre + "dh1_16")
        b_in = None
        if mut == "in_proj_bias_last_tile" and i == 0:
            b = leaf(pre + "attn.in_proj_bias")
            b_in = torch.cat([b[:-16], b[-16:].detach()])
        qkv = pol.r(lin(h, pre + "attn.in_proj_weight", pre + "attn.in_proj_bias", b_override=b_in))
        if ref or probe:
            with torch.no_grad():
                q, k = (qkv[:, j * D:(j + 1) * D].reshape(F, N, HEADS, 64).transpose(1, 2) for j in (0, 1))
                peaks.append(float(torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1).max(-1).values.median()))
        if ref:
            o = attn_plain(qkv, F, N)
        else:
            keep = None
            if mut == "cls_scatter_drops_kv" and last:
                keep = (torch.arange(F * N) % N == 0).to(F64)
            o = pol.g(_VitAttn.apply(qkv, pol, F, N, keep), pre + "do16")
        if last and c["cls_only"]:                 # _ClsRowsFn: the class rows of the attention output and of the stream
            o, xs = o.reshape(F, N, D)[:, 0], xs.reshape(F, N, D)[:, 0]
        xs = xs + pol.g(lin(o, pre + "attn.out_proj.weight", pre + "attn.out_proj.bias"), pre + "dy_out16")
        h = pol.g(pol.r(ln(xs, pre + "ln_2")), pre + "dh2_16")
        u = act(lin(h, pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias"), "quickgelu", pre + "c_fc", at_u=(mut == "quickgelu_grad_at_u"))
        res = xs.detach() if (mut == "ln_no_dpass" and i == 0) else xs
        xs = res + pol.g(lin(u, pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias"), pre + "dy_proj16")
    if not c["cls_only"]:
        xs = xs.reshape(F, N, D)[:, 0]
    h = pol.g(pol.r(ln(xs, "ln_post")), "dh_post16")
    emb = pol.g(lin(h, "proj"), "dE16")             # _ProjFn: fp32 output; round16(dE) is the dgrad operand and the wgrad dY
    outs = {}
    if not student:
        outs["E"] = emb
    else:
        B, T, C = c["B"], c["T"], c["C"]
        e_mlp = emb.detach() if mut == "fork_one_branch" else emb
        x16 = pol.g(pol.r(e_mlp), "dx_fc1_16")                                            # CastFn, both ways
        hh = act(lin(x16, "residual_mlp.fc1.weight", "residual_mlp.fc1.bias"), "gelu", "fc1")
        m = pol.g(lin(hh, "residual_mlp.fc2.weight", "residual_mlp.fc2.bias"), "dm16")
        outs["emb"], outs["emb_distill"] = emb, e_mlp + ALPHA * m
        pooled = emb.reshape(B, T, E).sum(1) * (1.0 / T)
        if mut == "pool_div":
            pooled = _ScaleGrad.apply(pooled, 1.0 / B)
        pooled = pol.g(pol.r(pooled), "dpooled16")
        if probe:
            return {"attn_peak": peaks, "head_z0": pooled @ leaf("classification_head.0.weight").t()}
        z = lin(pooled, "classification_head.0.weight", "classification_head.0.bias")
        extra["relu_negative_share"] = float((z.detach() < 0).double().mean())
        extra["relu_min_abs"] = float(z.detach().abs().min())
        hr = act(z, "relu", "head0")
        outs["logits"] = pol.g(lin(hr, "classification_head.2.weight", "classification_head.2.bias"), "dlogits16")
    if probe:
        return {"attn_peak": peaks}
    names = list(outs)
    torch.autograd.backward([outs[n] for n in names], [inp["up"][n].to(F64).to(cd) for n in names])
    out = {n: outs[n].detach().to(F64) for n in names}
    for name in param_shapes(c):
        t = leaf(name)
        out["g." + name] = (t.grad if t.grad is not None else torch.zeros_like(t)).to(F64).reshape(param_shapes(c)[name])
    if mut == "conv1_grad_pad_cols" and K % 64:
        # the crop of the K-padded weight gradient [D, kpad] taken at the pad's width instead of at column 0
        gw, pad = out["g.conv1.weight"].reshape(D, K), (K + 63) // 64 * 64 - K
        out["g.conv1.weight"] = torch.cat([gw[:, pad:], torch.zeros(D, pad, dtype=F64)], 1).reshape(D, 3, p, p)
    if mut == "proj_grad_transposed":
        out["g.proj"] = out["g.proj"].t().contiguous().view(D, E)
    out.update(extra)
    out["attn_peak"] = peaks
    if ref:
        out["floor"] = _floors(out, absrec)
    return out


def _floors(out, absrec):
    """2^-23 of the largest sum of absolute values behind an element: |dY|^T |X| for a weight gradient, sum |dY| for a bias gradient,
    the frame sum of |dx| for the class / positional embeddings, the largest element for everything else."""
    fl = {}
    for (wname, bname), g, x in absrec:
        gw = float((g.t() @ x).max())
        fl["g." + wname] = max(fl.get("g." + wname, 0.0), EPS32 * gw)
        if bname is not None:
            fl["g." + bname] = max(fl.get("g." + bname, 0.0), EPS32 * float(g.sum(0).max()))
    fl["g.positional_embedding"] = EPS32 * float(out["abs_dpos"].max())
    fl["g.class_embedding"] = EPS32 * float(out["abs_dpos"][0].max())
    for k in tensor_names(out):
        if k not in fl and k != "abs_dpos":
            fl[k] = EPS32 * float(out[k].abs().max())
    del out["abs_dpos"]
    return fl


@functools.lru_cache(maxsize=None)
def step_ref64(name, dtype):
    return run_step(make_inputs(name, dtype), Policy())


@functools.lru_cache(maxsize=None)
def step_model16(name, dtype):
    pol = Policy(dtype)
    out = run_step(make_inputs(name, dtype), pol)
    out["stored"] = dict(pol.stored)
    return out


def step_eval32(name, dtype, bug=None):
    """model16 evaluated in float32 with round-to-nearest stores (attention_refs' model inside the attentions stays float64): what a
    faithful implementation computes -- the measure's self-test -- or one of the MUTANTS of it."""
    return run_step(make_inputs(name, dtype), Policy(dtype, compute=F32, mutant=bug))


def check(got, r64, m16):
    """The measure over every tensor of `got`; returns (measurements, failure messages naming the tensor, both ratios and the first
    offending index)."""
    ms = measure_all(got, r64, m16)
    bad = []
    for m in ms:
        if m["ok"]:
            continue
        d = (got[m["name"]].detach().to("cpu").to(F64) - r64[m["name"]]).abs()
        over = torch.nonzero(~torch.isfinite(d) | (d > R_MAX * m["e_max"]))
        idx = tuple(over[0].tolist()) if len(over) else tuple(torch.nonzero(d == d.max())[0].tolist())
        bad.append(f"{m['name']}: rms ratio {m['ratio_rms']:.2f} (<= {R_RMS}), max ratio {m['ratio_max']:.2f} (<= {R_MAX}), "
                   f"finite {m['finite']}, first offending index {idx}")
    return ms, bad
