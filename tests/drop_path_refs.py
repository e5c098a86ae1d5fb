"""CPU references for stochastic depth that skips dropped frames (vimo_clip_amd/csrc/drop_path.hip, include/vmc.h).
No GPU code: numpy and torch on the CPU.

Part one: the sampler's reference (patch_dropout_ref's, with the block in the counter), float64 restatements of the four data
kernels written from the header's definitions, and the bounds their outputs are held to, derived here and never from kernel output.

Part two: one training step WITH drop path -- the float64 step and its designed-rounding model.  It is the graph of
student_step_refs.run_step (restated, since that file does not change; its pieces -- make_inputs, patch_rows, _VitAttn, attn_plain,
_ActSaved, Policy, the measure and its constants -- are imported, never restated) in which a dropping block runs on the kept frames
only and the stream behind it is x_in + mask s (Block(x_in) - x_in); x_in is the class rows in a cls_only last block.  The stream is
fp32, so the model adds no 16-bit rounding point; it takes c = fl32(1 - s) and s = fl32(F / K) as the kernels receive them, the
reference the exact F / K.  tests/test_drop_path_host.py checks everything in here on the CPU."""
import functools

import numpy as np
import torch

import patch_dropout_ref as PR
import student_step_refs as S
import tfam_chain_refs as TC
from student_step_refs import (ALPHA, BY_NAME, HEADS, LAYERS, R_MAX, R_RMS, VAC_MAX, VAC_RMS, WIDTH, Policy, _ActSaved,      # noqa: F401
                               _VitAttn, attn_plain, check, make_inputs, measure_all, param_shapes, patch_rows, tensor_names, vacuity)
from train_kernel_refs import BF16, EPS32, F16, F32

F64 = torch.float64


# ============================================================================================== part one: the kernels
def keep_count(F, p, block, layers):
    """K_l = max(1, int(F (1 - p_l))), p_l = p l / max(1, L - 1) -- written out, not imported from the package."""
    return max(1, int(F * (1.0 - p * block / max(1, layers - 1))))


def sample(seed, block, F, K):
    """(keep int32 [K] ascending, slot int32 [F]): the K frames with the smallest (hash32(seed, block F + f), f).
    patch_dropout_ref.keep_sample draws "frame" b of a [b + 1, F] grid with the counter b F + f: row `block` of it is this draw."""
    keep = PR.keep_sample(seed, block + 1, F, K)[block]
    return keep, slots(keep, F)


def slots(keep, F):
    slot = np.full(F, -1, dtype=np.int32)
    slot[np.asarray(keep)] = np.arange(len(keep), dtype=np.int32)
    return slot


def scales(F, K):
    """(c, s) as the kernels receive them: s = fl32(F / K), c = fl32(1 - F / K) (ops.drop_path_merge rounds each once from float64)."""
    s = F / K
    return float(np.float32(1.0 - s)), float(np.float32(s))


def gather(src, keep):
    """src torch [F, row] -> [K, row]: bit copies."""
    return src[torch.as_tensor(np.asarray(keep), dtype=torch.long)]


def merge(x, y, slot, c, s):
    """(out float64 [F, row], mag float64 [F, row], kept bool [F]): out[f] = c x[f] + s y[slot[f]] for a kept frame, x[f] for a dropped
    one, on the stored values widened; mag = |c x| + |s y| on the kept rows (what the fp32 bound scales with), 0 on the others."""
    slot_t = torch.as_tensor(np.asarray(slot), dtype=torch.long)
    kept = slot_t >= 0
    x64, y64 = x.to(F64), y.to(F64)
    out, mag = x64.clone(), torch.zeros_like(x64)
    out[kept] = c * x64[kept] + s * y64[slot_t[kept]]
    mag[kept] = (c * x64[kept]).abs() + (s * y64[slot_t[kept]]).abs()
    return out, mag, kept


def scatter_add(dpass, dsub, slot):
    """dx[f] = dpass[f] + dsub[slot[f]] (kept) or dpass[f] (dropped): merge with c = s = 1."""
    return merge(dpass, dsub, slot, 1.0, 1.0)


def merge_bwd(dout, keep, slot, c, s):
    """(dx float64 [F, row], dx_mag, kept, dy float64 [K, row], dy_mag): dx[f] = c dout[f] (kept; a one-term "sum") or dout[f];
    dy[j] = s dout[keep[j]]."""
    slot_t = torch.as_tensor(np.asarray(slot), dtype=torch.long)
    kept = slot_t >= 0
    d64 = dout.to(F64)
    dx, mag = d64.clone(), torch.zeros_like(d64)
    dx[kept] = c * d64[kept]
    mag[kept] = dx[kept].abs()
    dy = s * d64[torch.as_tensor(np.asarray(keep), dtype=torch.long)]
    return dx, mag, kept, dy, dy.abs()


# The bound of a kept row.  The kernel forms fl(fl(c x) + fl(s y)) in fp32 with round-to-nearest: with |d_i| <= 2^-24,
# fl(c x) = c x (1 + d1), fl(s y) = s y (1 + d2), the sum (a + b)(1 + d3), so the error is at most
#     2^-24 (|c x| + |s y|) + 2^-24 |a + b| <= 2^-23 (|c x| + |s y|) (1 + 2^-24).
# A fused multiply-add has one rounding fewer and stays inside it; one product alone (merge_bwd) or one sum alone (scatter_add,
# c = s = 1: the products are exact) too.  KAPPA = 1 + 2^-20 covers the second-order term with room; FP32_TINY (the smallest normal
# float, times the three operations) covers results in the subnormal range whether the device keeps or flushes them.  Where the store
# is 16-bit it rounds once more: half an ulp, u |v| with u = 2^-8 (bf16) / 2^-11 (f16) on the normal range and half the subnormal
# spacing (2^-134 / 2^-25) below it; |v| is taken with the fp32 error on top, so the bound never leans on the value it judges.
KAPPA = 1.0 + 2.0 ** -20
FP32_TINY = 3 * 2.0 ** -126
HALF_ULP = {F32: (0.0, 0.0), BF16: (2.0 ** -8, 2.0 ** -134), F16: (2.0 ** -11, 2.0 ** -25)}


def kept_bound(value64, mag, dtype):
    """Elementwise bound for a kept row whose exact value is value64 and whose two terms have magnitudes summing to mag."""
    fp32 = KAPPA * 2.0 ** -23 * mag + FP32_TINY
    u, sub = HALF_ULP[dtype]
    return fp32 + u * (value64.abs() + fp32) + sub


# ============================================================================================== part two: the step
def _dcase(name, base, drop, **over):
    """A case of student_step_refs (its geometry, weights, frames and upstream gradients: make_inputs(base)) with explicit keep sets:
    drop[l] = None (block l runs on every frame and is not wrapped) or the ascending frame ids it keeps."""
    c = dict(BY_NAME[base], **over)
    assert len(drop) == LAYERS and all(d is None or (list(d) == sorted(set(d)) and 0 <= d[0] and d[-1] < c["F"]) for d in drop)
    return dict(name=name, base=base, drop=tuple(None if d is None else tuple(d) for d in drop), cls_only=c["cls_only"], level=c["level"],
                F=c["F"], N=c["N"])


CASES = [
    # F = 3: frame 0 is kept by block 0 only, frame 1 by block 1 only, frame 2 by both
    _dcase("dp_a", "a", [(0, 2), (1, 2)]),
    _dcase("dp_g", "g", [(0, 2), (1, 2)]),                                        # the same, not cls_only
    # F = 64: block 0 keeps all (not wrapped: 3200 rows, the grouped weight-gradient launch), block 1 keeps 48 frames (2400 rows,
    # no multiple of 128: per-linear launches) -- both weight-gradient paths in one backward
    _dcase("dp_i", "i", [None, tuple(f for f in range(64) if f % 4 != 1)]),
    _dcase("dp_s1", "s1", [(0, 1, 3), (2, 3)]),                                   # student level, B = 2, T = 2
]
DBY_NAME = {c["name"]: c for c in CASES}

MUTANTS = ("dy_sub_unscaled", "direct_unscaled", "gather_bwd_overwrites", "keep_shifted", "dropped_rows_scaled", "merge_token_rows")
# merge_token_rows needs a cls_only last block; the others are run where frames differ in what they keep
MUTANT_CASE = {"dy_sub_unscaled": "dp_a", "direct_unscaled": "dp_g", "gather_bwd_overwrites": "dp_g", "keep_shifted": "dp_a",
               "dropped_rows_scaled": "dp_s1", "merge_token_rows": "dp_a"}


def run_step(name, dtype, pol, bug=None):
    """One step of case `name` under `pol` (Policy: dtype None = the float64 reference), student_step_refs.run_step's graph with
    drop path.  bug: one of MUTANTS.  Returns float64 tensors {"E" | "emb", "emb_distill", "logits", "g.<parameter>"} and, for the
    reference, "floor"."""
    dc = DBY_NAME[name]
    inp = make_inputs(dc["base"], dtype)
    c = inp["case"]
    F, N, p, E, D, K = c["F"], c["N"], c["p"], c["E"], WIDTH, c["K"]
    cd, ref = pol.compute, pol.dtype is None
    student = c["level"] == "student"
    leaves, absrec, peaks, extra = {}, [], [], {}

    def leaf(n):
        if n not in leaves:
            src = inp["w16"][n] if n in inp["w16"] else inp["p32"][n]
            leaves[n] = src.to(F64).to(cd).clone().requires_grad_(True)
        return leaves[n]

    def lin(x, wname, bname=None):
        W = leaf(wname)
        W = W.t() if wname == "proj" else W.reshape(W.shape[0], -1)
        y = x @ W.t()
        if bname is not None:
            y = y + leaf(bname)
        if ref and y.requires_grad:
            y.register_hook(lambda g, x=x.detach(), k=(wname, bname): absrec.append((k, g.abs(), x.abs())))
        return y

    def act(z, kind, tag):
        return S._ACT[kind][0](z) if ref else _ActSaved.apply(z, pol, kind, tag, False)

    def ln(x, n):
        return TC._layer_norm(x, leaf(n + ".weight"), leaf(n + ".bias"), pol)

    def block(xs, i, Fb, cls):
        """student_step_refs.run_step's loop body on Fb frames."""
        pre = f"transformer.resblocks.{i}."
        h = pol.g(pol.r(ln(xs, pre + "ln_1")), pre + "dh1_16")
        qkv = pol.r(lin(h, pre + "attn.in_proj_weight", pre + "attn.in_proj_bias"))
        with torch.no_grad():
            q, k = (qkv[:, j * D:(j + 1) * D].reshape(Fb, N, HEADS, 64).transpose(1, 2) for j in (0, 1))
            peaks.append(float(torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1).max(-1).values.median()))
        o = attn_plain(qkv, Fb, N) if ref else pol.g(_VitAttn.apply(qkv, pol, Fb, N, None), pre + "do16")
        if cls:
            o, xs = o.reshape(Fb, N, D)[:, 0], xs.reshape(Fb, N, D)[:, 0]
        xs = xs + pol.g(lin(o, pre + "attn.out_proj.weight", pre + "attn.out_proj.bias"), pre + "dy_out16")
        h = pol.g(pol.r(ln(xs, pre + "ln_2")), pre + "dh2_16")
        u = act(lin(h, pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias"), "quickgelu", pre + "c_fc")
        return xs + pol.g(lin(u, pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias"), pre + "dy_proj16")

    # ---- patch GEMM, token assembly, ln_pre: as student_step_refs.run_step
    xp = pol.g(pol.r(lin(patch_rows(inp["frames"], p, pol), "conv1.weight")), "dxp16")
    cls_e, pos = leaf("class_embedding"), leaf("positional_embedding")
    xs = (torch.cat([cls_e.expand(F, 1, D), xp.reshape(F, N - 1, D)], 1) + pos).reshape(F * N, D)
    if ref and xs.requires_grad:
        xs.register_hook(lambda g: extra.__setitem__("abs_dpos", g.abs().reshape(F, N, D).sum(0)))
    xs = ln(xs, "ln_pre")
    # ---- residual blocks
    for i in range(LAYERS):
        cls = i + 1 == LAYERS and c["cls_only"]
        kept = dc["drop"][i]
        if kept is None:
            xs = block(xs, i, F, cls)
            continue
        Kf, n = len(kept), 1 if cls else N
        idx = torch.tensor(kept, dtype=torch.long)
        cc, s = (1.0 - F / Kf, F / Kf) if ref else scales(F, Kf)
        y = block(xs.reshape(F, N * D)[idx].reshape(Kf * N, D), i, Kf, cls)                  # FrameGatherFn, then the block on K frames
        if cls:                                                                              # x_in: the class rows of the stream
            base = xs[:F] if bug == "merge_token_rows" else xs.reshape(F, N, D)[:, 0]
        else:
            base = xs
        base = base.reshape(F, n * D)
        xk = base[idx].detach() if bug == "gather_bwd_overwrites" else base[idx]
        direct, branch = cc * xk, s * y.reshape(Kf, n * D)
        if bug == "direct_unscaled":
            direct = S._ScaleGrad.apply(direct, 1.0 / cc)
        if bug == "dy_sub_unscaled":
            branch = S._ScaleGrad.apply(branch, 1.0 / s)
        where = (idx + 1) % F if bug == "keep_shifted" else idx
        out = cc * base if bug == "dropped_rows_scaled" else base
        xs = out.index_copy(0, where, direct + branch).reshape(F * n, D)                     # DropPathMergeFn
    if not c["cls_only"]:
        xs = xs.reshape(F, N, D)[:, 0]
    h = pol.g(pol.r(ln(xs, "ln_post")), "dh_post16")
    emb = pol.g(lin(h, "proj"), "dE16")
    outs = {}
    if not student:
        outs["E"] = emb
    else:
        B, T = c["B"], c["T"]
        x16 = pol.g(pol.r(emb), "dx_fc1_16")
        hh = act(lin(x16, "residual_mlp.fc1.weight", "residual_mlp.fc1.bias"), "gelu", "fc1")
        m = pol.g(lin(hh, "residual_mlp.fc2.weight", "residual_mlp.fc2.bias"), "dm16")
        outs["emb"], outs["emb_distill"] = emb, emb + ALPHA * m
        pooled = pol.g(pol.r(emb.reshape(B, T, E).sum(1) * (1.0 / T)), "dpooled16")
        z = lin(pooled, "classification_head.0.weight", "classification_head.0.bias")
        extra["relu_negative_share"] = float((z.detach() < 0).double().mean())
        extra["relu_min_abs"] = float(z.detach().abs().min())
        hr = act(z, "relu", "head0")
        outs["logits"] = pol.g(lin(hr, "classification_head.2.weight", "classification_head.2.bias"), "dlogits16")
    names = list(outs)
    torch.autograd.backward([outs[n] for n in names], [inp["up"][n].to(F64).to(cd) for n in names])
    out = {n: outs[n].detach().to(F64) for n in names}
    shapes = param_shapes(c)
    for n in shapes:
        t = leaf(n)
        out["g." + n] = (t.grad if t.grad is not None else torch.zeros_like(t)).to(F64).reshape(shapes[n])
    out.update(extra)
    out["attn_peak"] = peaks
    if ref:
        out["floor"] = S._floors(out, absrec)
    return out


@functools.lru_cache(maxsize=None)
def step_ref64(name, dtype):
    return run_step(name, dtype, Policy())


@functools.lru_cache(maxsize=None)
def step_model16(name, dtype):
    pol = Policy(dtype)
    out = run_step(name, dtype, pol)
    out["stored"] = dict(pol.stored)
    return out


def step_eval32(name, dtype, bug=None):
    """model16 evaluated in float32: what a faithful implementation computes, or one of the MUTANTS of it."""
    return run_step(name, dtype, Policy(dtype, compute=F32), bug=bug)
