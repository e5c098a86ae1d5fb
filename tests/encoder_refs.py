"""Float64 reference, designed-rounding model, inputs, case list and mutants for the INFERENCE forward of the CLIP ViT encoder:
VisionTransformer._encode_patches with _patches / patch_operands / _encode_chunks around it (vimo_clip_amd/clip_vit.py) -- the path
bench.py measures, the extractor runs and FlowStudentModel's teacher runs.  No GPU code: torch and numpy on the CPU.
tests/test_encoder_refs_host.py checks everything in here on the CPU (against the oracle and attention_refs, the routes of every
case, the conditions on the inputs, the measure on itself and twelve mutants); tests/test_gpu_encoder_parity.py compares what the
path returns and what its ``trace=`` hook records.

``forward_ref64`` is the forward in float64 on the values the kernels see: 16-bit compute copies of the block weights and of
``proj`` widened, fp32 biases / LayerNorm parameters / class and positional embeddings, u8 pixels (through the wrap quirk where the
case asks for it).  Its patch embedding is sum_k ((v / 255 - mean_c) / std_c) conv1[n, k] with the fp32 MASTER conv1: the
split-precision patch GEMM claims fp32 accuracy against exactly that.  ``forward_model16`` is the same graph with the roundings the
path is designed to make (DESIGN.md §5.5 lists each with its line in the code; none is taken from kernel output).  The measure, the
rounding carrier ``_RoundFwd`` and the ``Policy`` that owns it are tfam_chain_refs' (DESIGN.md §5.3); the attention is
attention_refs'; QuickGELU and the plain patch operand are student_step_refs'.

Tensors: the stream after ln_pre and after every residual add that the ``trace=`` hook records ("ln_pre", "blk{i}.attn",
"blk{i}.mlp"; [F N, D]) and the embeddings "E" [F, E].  "E_trace" is E again (the embeddings of the ``trace=`` run, which takes the
full last-block attention instead of the class query), "E_cls" (case h) E of the run with the last block on the class rows, "E_gray"
(case k) E of encode_gray_u8: different launches of the same function, so one reference and one model serve them.
"""
import functools

import numpy as np
import torch

import attention_refs as AR
import tfam_chain_refs as TC
from attention_refs import FAM_LDS, route_vit, vit_forward      # noqa: F401
from oracle.vit import CLIP_MEAN, CLIP_STD
from student_step_refs import _quickgelu, patch_rows
from tfam_chain_refs import R_MAX, R_RMS, VAC_MAX, VAC_RMS, Policy, _RoundFwd, failures, measure, measure_all, vacuity      # noqa: F401
from train_kernel_refs import BF16, EPS32, F16, F32

F64 = torch.float64
ALPHA_U8 = float(np.float32(1.0 / 255.0))          # patch_operands' alpha as vmc_linear receives it (a C float)
BLOCK_PARAMS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
MUTANTS = ("patch_lo_dropped", "patch_mean_not_in_bias", "alpha_on_product_only", "pos_row_shift", "wrap_255_minus_v",
           "f32_split_hi_only", "cls_kv_offset", "ln_post_without_mlp", "defer_drops_branch0", "gelu_erf_for_quickgelu",
           "gray_one_channel", "chunk_last_frame_repeated")
# (case, tensor) each mutant of the float32 evaluation must fail
MUTANT_CASE = {"patch_lo_dropped": ("a", "ln_pre"), "patch_mean_not_in_bias": ("a", "ln_pre"), "alpha_on_product_only": ("b", "ln_pre"),
               "pos_row_shift": ("b", "ln_pre"), "wrap_255_minus_v": ("c", "ln_pre"), "f32_split_hi_only": ("d", "ln_pre"),
               "cls_kv_offset": ("e", "E"), "ln_post_without_mlp": ("a", "E"), "defer_drops_branch0": ("h", "E"),
               "gelu_erf_for_quickgelu": ("g", "blk0.mlp"), "gray_one_channel": ("k", "ln_pre"), "chunk_last_frame_repeated": ("m", "E")}


# ---------------------------------------------------------------------------------------------- cases
def _case(name, F, R, p, D=256, H=4, E=64, L=2, source="u8", wrap=False, exact=True, cls_only=True, cls_query=True, defer=False,
          res16=False, frame_chunk=256, seed=0):
    """source: "u8" (encode_frames_u8), "pix" (encode_pixel_values on the normalised fp32 pixels), "gray" (encode_gray_u8 of one
    plane AND encode_frames_u8 of the plane given three times).  mode: the patch layout _patches picks.  fused: the residual adds
    go through vmc_add_layernorm_fwd (clip_vit.py: `fused = xf32 and D % 256 == 0 and self.fuse_add_ln`)."""
    g = R // p
    K = 3 * p * p
    mode = ("f32_split" if source == "pix" else "u8_exact") if exact else "plain"
    return dict(name=name, F=F, R=R, p=p, D=D, H=H, E=E, L=L, N=g * g + 1, K=K, kpad=(K + 63) // 64 * 64, source=source, wrap=wrap,
                exact=exact, mode=mode, cls_only=cls_only, cls_query=cls_query, defer=defer, res16=res16, frame_chunk=frame_chunk,
                fused=(not res16) and D % 256 == 0, seed=seed)


CASES = [
    _case("a", 3, 64, 16, seed=1),
    _case("b", 3, 56, 8, seed=2),
    _case("c", 3, 64, 8, wrap=True, seed=3),
    _case("d", 3, 56, 4, source="pix", seed=4),
    _case("e", 3, 64, 4, seed=5),
    _case("f", 2, 96, 4, seed=6),
    _case("g", 3, 64, 16, D=128, H=2, seed=7),
    _case("h", 3, 56, 8, defer=True, cls_only=False, seed=2),      # case b's inputs; "E_cls": the run with cls_only back on
    _case("i", 3, 64, 16, cls_only=False, cls_query=False, seed=9),
    _case("j", 2, 64, 16, D=768, H=12, seed=10),
    _case("k", 3, 64, 8, source="gray", exact=False, seed=11),
    _case("l", 256, 64, 8, seed=12),
    _case("m", 5, 64, 16, frame_chunk=2, seed=13),
    _case("r1", 3, 64, 16, res16=True, seed=14),
    _case("r2", 3, 64, 8, D=128, H=2, res16=True, seed=15),
]
BY_NAME = {c["name"]: c for c in CASES}


def stage_names(c):
    """What the ``trace=`` hook of _encode_patches records for the case: ln_pre, every residual add of the ordinary blocks, and of
    the last block its attention add when it runs on all rows, its MLP add only when that is written to the stream (unfused)."""
    names = ["ln_pre"]
    for i in range(c["L"]):
        last = i + 1 == c["L"]
        if last and c["cls_only"]:
            break
        names.append(f"blk{i}.attn")
        if not (last and c["fused"]):
            names.append(f"blk{i}.mlp")
    return names


def output_names(c):
    extra = {"h": ["E_cls"], "k": ["E_gray"]}.get(c["name"], [])
    return stage_names(c) + ["E", "E_trace"] + extra


def param_shapes(c):
    D, E, N, p = c["D"], c["E"], c["N"], c["p"]
    s = {"conv1.weight": (D, 3, p, p), "class_embedding": (D,), "positional_embedding": (N, D), "ln_pre.weight": (D,), "ln_pre.bias": (D,)}
    for i in range(c["L"]):
        pre = f"transformer.resblocks.{i}."
        for n, sh in zip(BLOCK_PARAMS, ((D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,))):
            s[pre + n] = sh
    s.update({"ln_post.weight": (D,), "ln_post.bias": (D,), "proj": (D, E)})
    return s


def is_matrix(name):
    """Parameters the GEMMs read through a 16-bit compute copy (autograd_ops.weights.get); conv1 has its own operands."""
    return name == "proj" or (name.endswith("weight") and "ln_" not in name and name != "conv1.weight")


def _fan_in(name, shape):
    return shape[0] if name == "proj" else int(np.prod(shape[1:]))


@functools.lru_cache(maxsize=None)
def make_inputs(name, dtype):
    """Everything the forward reads: fp32 masters, the 16-bit copies of the matrices, u8 frames (case k: one plane).  Matrices
    N(0, 1) / sqrt(K), biases N(0, 1) / 4, LayerNorm 1 + N / 4 and N / 4, class / positional embeddings N(0, 1).  The q and k rows
    of every in_proj are then scaled by ``stress``, stepped up until the float64 forward shows an attention that is not trivially
    uniform (median over rows of the largest probability >= 4 / N in every block), as student_step_refs does."""
    c = BY_NAME[name]
    D = c["D"]
    g = torch.Generator().manual_seed(4000 + c["seed"])
    rn = lambda *s, scale=1.0, shift=0.0: torch.randn(*s, generator=g) * scale + shift
    p = {}
    for n, sh in param_shapes(c).items():
        if is_matrix(n) or n == "conv1.weight":
            p[n] = rn(*sh, scale=_fan_in(n, sh) ** -0.5)
        elif n.endswith("ln_1.weight") or n.endswith("ln_2.weight") or n in ("ln_pre.weight", "ln_post.weight"):
            p[n] = rn(*sh, scale=0.25, shift=1.0)
        elif n in ("class_embedding", "positional_embedding"):
            p[n] = rn(*sh)
        else:
            p[n] = rn(*sh, scale=0.25)
    inp = dict(case=c, dtype=dtype, p32=p)
    ch = 1 if c["source"] == "gray" else 3
    inp["frames"] = torch.randint(0, 256, (c["F"], ch, c["R"], c["R"]), generator=g, dtype=torch.int64).to(torch.uint8)
    base = {n: v.clone() for n, v in p.items() if n.endswith("in_proj_weight")}
    for stress in (1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 4.0):
        for n, v in base.items():
            p[n] = torch.cat([v[:2 * D] * stress, v[2 * D:]])
        inp["w16"] = {n: v.to(dtype) for n, v in p.items() if is_matrix(n)}
        peaks = run_forward(inp, Policy(), probe=True)["attn_peak"]
        if min(peaks) >= 4.0 / c["N"]:
            break
    inp["stress"] = stress
    return inp


def frames_rgb(inp):
    """The case's frames as [F, 3, R, R] u8 (a grey plane given three times)."""
    fr = inp["frames"]
    return fr.expand(-1, 3, -1, -1).contiguous() if fr.shape[1] == 1 else fr


def pixel_values(inp):
    """What encode_pixel_values receives (case d): the oracle's normalisation in fp32."""
    from oracle.vit import normalize_u8
    return normalize_u8(frames_rgb(inp))


# ---------------------------------------------------------------------------------------------- the patch embedding
def _rows(pix, p):
    """[F, 3, R, R] -> [F g g, 3 p p], column (c p + dy) p + dx (elementwise.hip, `at`): patch_rows' layout."""
    F, _, R, _ = pix.shape
    g = R // p
    return pix.reshape(F, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(F * g * g, 3 * p * p)


def _split16(w32, dtype):
    """patch_operands' `split`: fp32 -> (hi, lo) 16-bit halves, as fp32 values."""
    hi = w32.to(dtype)
    return hi.float(), (w32 - hi.float()).to(dtype).float()


def patch_embed(inp, pol, frames):
    """[F (N - 1), D]: the patch GEMM's alpha (acc + bias'), before the positional rows; and, for the reference, |A| |W|^T."""
    c, cd, mut = inp["case"], pol.compute, pol.mutant
    D, p, K = c["D"], c["p"], c["K"]
    w32 = inp["p32"]["conv1.weight"].float()
    if pol.dtype is None:
        A = patch_rows(frames, p, pol, wrap=c["wrap"])
        W = w32.reshape(D, K).to(F64)
        return A @ W.t(), A.abs() @ W.abs().t()
    dt = pol.dtype
    if c["mode"] == "plain":
        A = patch_rows(frames, p, pol, wrap=c["wrap"])
        if mut == "gray_one_channel":              # the plane lands in channel slice 0 only
            A = torch.cat([A[:, :p * p], torch.zeros_like(A[:, p * p:])], 1)
        return A @ w32.reshape(D, K).to(dt).to(F64).to(cd).t(), None
    if c["mode"] == "f32_split":
        x32 = _rows(pixel_values(inp), p)                                  # vmc_patches_f32_split reads the fp32 pixels
        x_hi, x_lo = _split16(x32, dt)
        w_hi, w_lo = _split16(w32.reshape(D, K), dt)
        x_hi, x_lo, w_hi, w_lo = (t.to(F64).to(cd) for t in (x_hi, x_lo, w_hi, w_lo))
        if mut == "f32_split_hi_only":
            return x_hi @ w_hi.t(), None
        return (x_hi + x_lo) @ w_hi.t() + x_hi @ w_lo.t(), None            # [x_hi | x_lo | x_hi] . [W_hi | W_hi | W_lo]
    # u8_exact: raw pixels as exact integers against [W'_hi | W'_lo], W' = conv1 / std in fp32; bias' and alpha in the epilogue
    v = frames.to(torch.int64)
    if c["wrap"]:
        v = (255 - v) if mut == "wrap_255_minus_v" else (256 - v) % 256
    V = _rows(v.to(F64), p).to(cd)
    w2 = w32.reshape(D, 3, p * p)
    istd = torch.tensor([1.0 / s for s in CLIP_STD]).view(1, 3, 1)         # fp32, as patch_operands builds it
    mean = torch.tensor(CLIP_MEAN).view(1, 3, 1)
    hi, lo = _split16((w2 * istd).reshape(D, K), dt)
    if mut == "patch_lo_dropped":
        lo = torch.zeros_like(lo)
    bias = (-255.0 * (w2.double() * (mean.double() * istd.double())).sum(dim=(1, 2))).float()
    if mut == "patch_mean_not_in_bias":
        bias = torch.zeros_like(bias)
    acc = V @ hi.to(F64).to(cd).t() + V @ lo.to(F64).to(cd).t()
    alpha = torch.tensor(ALPHA_U8, dtype=F64).to(cd)
    if mut == "alpha_on_product_only":
        return alpha * acc + bias.to(F64).to(cd), None
    return alpha * (acc + bias.to(F64).to(cd)), None


# ---------------------------------------------------------------------------------------------- the forward
def run_forward(inp, pol, probe=False):
    """The forward under `pol` (tfam_chain_refs.Policy: dtype None = the float64 reference, which runs every block on every row;
    mutant = one of MUTANTS).  Returns float64 tensors by name and, for the reference, "floor" and "attn_peak".  probe (make_inputs
    only): the attention peaks alone."""
    c = inp["case"]
    F, N, D, H, L, p = c["F"], c["N"], c["D"], c["H"], c["L"], c["p"]
    cd, mut, ref = pol.compute, pol.mutant, pol.dtype is None
    fused = c["fused"] and not ref
    P = lambda n: inp["p32"][n].to(F64).to(cd)
    W = lambda n: inp["w16"][n].to(F64).to(cd)
    r16 = pol.r
    st = r16 if (c["res16"] and not ref) else (lambda t: t)              # a store into the residual stream
    ln = lambda t, name: TC._layer_norm(t, P(name + ".weight"), P(name + ".bias"), pol)
    out, peaks = {}, []

    frames = frames_rgb(inp)
    if mut == "chunk_last_frame_repeated":
        frames = torch.cat([frames[:-1], frames[-2:-1]])
    tok, absacc = patch_embed(inp, pol, frames)
    pos, cls = P("positional_embedding"), P("class_embedding")
    pos_patch = pos[:N - 1] if mut == "pos_row_shift" else pos[1:]
    x = torch.cat([st(cls + pos[0]).expand(F, 1, D), st(tok.reshape(F, N - 1, D) + pos_patch)], 1).reshape(F * N, D)
    if ref:
        # one fp32 rounding of the largest sum of absolute values behind a patch token, through ln_pre's scale rstd gamma
        yc = x - x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt((yc * yc).mean(-1, keepdim=True) + TC.LN_EPS)
        acc_rows = torch.cat([torch.zeros(F, 1, dtype=F64), absacc.max(-1).values.reshape(F, N - 1)], 1).reshape(F * N, 1)
        patch_floor = EPS32 * float((acc_rows * rstd).max()) * float(P("ln_pre.weight").abs().max())
    x = st(ln(x, "ln_pre"))
    out["ln_pre"] = x
    for i in range(L):
        pre, last = f"transformer.resblocks.{i}.", i + 1 == L
        cls_rows = last and c["cls_only"] and not ref                    # the last block on the F class rows
        h = r16(ln(x, pre + "ln_1"))
        qkv = r16(h @ W(pre + "attn.in_proj_weight").t() + P(pre + "attn.in_proj_bias"))
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        if ref or probe:
            qh, kh = (t.reshape(F, N, H, 64).transpose(1, 2) for t in (q, k))
            peaks.append(float(torch.softmax(qh @ kh.transpose(-1, -2) / 8.0, -1).max(-1).values.median()))
        if cls_rows:
            q = q.reshape(F, N, D)[:, 0]
            if mut == "cls_kv_offset":
                k = v
        NQ = 1 if cls_rows else N
        o = vit_forward(q.to(F64), k.to(F64), v.to(F64), (F, H, NQ, N, 64), pol.dtype)["out"].to(cd)
        xr = x.reshape(F, N, D)[:, 0] if cls_rows else x
        x_in = xr
        y = o @ W(pre + "attn.out_proj.weight").t() + P(pre + "attn.out_proj.bias")
        xr = xr + r16(y) if fused else st(xr + y)
        if not cls_rows:
            out[f"blk{i}.attn"] = xr
        h = r16(ln(xr, pre + "ln_2"))
        z = h @ W(pre + "mlp.c_fc.weight").t() + P(pre + "mlp.c_fc.bias")
        act = torch.nn.functional.gelu if (mut == "gelu_erf_for_quickgelu" and i == 0) else _quickgelu
        u = r16(act(z))
        y = u @ W(pre + "mlp.c_proj.weight").t() + P(pre + "mlp.c_proj.bias")
        x_attn = xr
        xr = xr + r16(y) if fused else st(xr + y)
        if not cls_rows:
            out[f"blk{i}.mlp"] = xr
        if last:
            if mut == "ln_post_without_mlp":
                xr = x_attn
            if mut == "defer_drops_branch0" and c["defer"]:
                xr = x_in + r16(y)                                           # (x + branch0) + m without branch0
        x = xr
    if probe:
        return {"attn_peak": peaks}
    xc = x if x.shape[0] == F else x.reshape(F, N, D)[:, 0]
    hp = r16(ln(xc, "ln_post"))
    out["E"] = hp @ W("proj")
    out = {n: t.detach().to(F64) for n, t in out.items()}
    names = output_names(c)
    for alias in names:
        if alias.startswith("E_"):
            out[alias] = out["E"]
    if not ref:
        return {n: out[n] for n in names}
    out["attn_peak"] = peaks
    fl = {n: 8.0 * EPS32 * float(t.abs().max()) for n, t in out.items() if isinstance(t, torch.Tensor)}
    fl["ln_pre"] = max(fl["ln_pre"], patch_floor)
    out["floor"] = fl
    out["patch_floor"] = patch_floor
    return out


@functools.lru_cache(maxsize=None)
def forward_ref64(name, dtype):
    with torch.no_grad():
        return run_forward(make_inputs(name, dtype), Policy())


@functools.lru_cache(maxsize=None)
def forward_model16(name, dtype):
    with torch.no_grad():
        return run_forward(make_inputs(name, dtype), Policy(dtype))


def forward_eval32(name, dtype, bug=None):
    """model16 evaluated in float32 with round-to-nearest stores (attention_refs' model inside the attentions stays float64): what a
    faithful implementation computes -- the measure's self-test -- or one of the MUTANTS of it."""
    with torch.no_grad():
        return run_forward(make_inputs(name, dtype), Policy(dtype, compute=F32, mutant=bug))


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


# ---------------------------------------------------------------------------------------------- the GEMM calls of the shipped path
def gemm_calls(c, dt):
    """(what, line of tests/host/gemm_route_dump.cpp) of every vmc_linear call the case's shipped forward makes on one chunk of
    F frames, read off VisionTransformer._encode_patches."""
    F, N, D, E, L = min(c["F"], c["frame_chunk"]), c["N"], c["D"], c["E"], c["L"]
    code = {F32: 0, BF16: 1, F16: 2}
    d16, sdt = code[dt], code[dt] if c["res16"] else 0
    calls = []

    def add(what, M, Nn, K, lda=None, ldc=None, ldres=0, act=0, bias=1, res=0, od=None, rd=0, org=0, rrm=0):
        f = [M, Nn, K, K if lda is None else lda, K, Nn if ldc is None else ldc, ldres, 0, act, bias, res, 0, d16 if od is None else od, rd, org,
             rrm, d16, 1, 0, 0, 4, 0]
        calls.append((what, "linear " + " ".join(str(v) for v in f)))

    parts = {"u8_exact": 2, "f32_split": 3, "plain": 1}[c["mode"]]
    add("patch", F * (N - 1), D, parts * c["kpad"], ldres=D, bias=int(c["mode"] == "u8_exact"), res=1, od=sdt, rd=0, org=N - 1, rrm=N - 1)
    for i in range(L):
        last = i + 1 == L
        rows_only = last and c["cls_only"]
        M, ld = (F, N * D) if rows_only else (F * N, D)
        if rows_only and c["cls_query"]:
            add(f"blk{i}.kv", F * N, 2 * D, D)
            add(f"blk{i}.q_cls", F, D, D, lda=N * D)
            lda_o = D
        else:
            add(f"blk{i}.in_proj", F * N, 3 * D, D)
            lda_o = ld
        if c["fused"]:
            add(f"blk{i}.out_proj", M, D, D, lda=lda_o)
            add(f"blk{i}.c_fc", M, 4 * D, D, act=1)
            add(f"blk{i}.c_proj", M, D, 4 * D)
        else:
            add(f"blk{i}.out_proj", M, D, D, lda=lda_o, ldc=ld, ldres=ld, res=1, od=sdt, rd=sdt)
            add(f"blk{i}.c_fc", M, 4 * D, D, act=1)
            add(f"blk{i}.c_proj", M, D, 4 * D, ldc=ld, ldres=ld, res=1, od=sdt, rd=sdt)
    add("proj", F, E, D, bias=0, od=0)
    return calls
