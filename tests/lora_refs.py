"""Float64 references, designed-rounding model, measures, case lists and mutants for the LoRA adapters (vimo_clip_amd/csrc/lora.hip,
vimo_clip_amd/lora.py).  No GPU code: torch on the CPU.  tests/test_lora_refs_host.py checks everything in here on the
CPU; tests/test_gpu_lora_kernels.py and tests/test_gpu_lora_step.py compare what the kernels and the training step return.

Kernels: the yardstick of gemm_refs (imported): r64 is the operation in float64 on the values the kernel sees, the same expression in
float32 on the CPU gives e32; the 16-bit ``ts`` columns of vmc_lora_down_concat are held to the interval rule (measure16), the fp32
adapter gradients of vmc_lora_wgrad_tn to measure32.

Adapted linear and training step: the measure of DESIGN.md §5.3 / §5.4 (tfam_chain_refs.measure, imported) between a float64 reference
(nothing rounds: float64 autograd of x (W + s B A)^T) and the model with the roundings the path is designed to make:

    ts = round16(s (x A16^T))      z = x W16^T + ts B16^T + b            (one fp32 accumulation: the adapter term is one more K tile)
    dz = round16(dy) [then the activation backward, stored 16-bit]       us = round16(s (dz B16))
    dx = dz W16 + us A16           dA = us^T x        dB = dz^T ts       (s lives inside us and ts)
"""
import functools

import torch

import student_step_refs as ST
import tfam_chain_refs as TC
from gemm_refs import E32_MAX, SHARE_MIN, interval16, measure16, measure32, pinned_share, trunc16      # noqa: F401
from student_step_refs import Policy, measure, vacuity                                                 # noqa: F401
from tfam_chain_refs import _RoundFwd, _RoundGrad                                                      # noqa: F401
from train_kernel_refs import BF16, DT16, DT_NAME, EPS32, F16, F32, e32_of, randn

F64 = torch.float64
TAIL = 64                     # columns of the adapter term in a concat buffer


# ---------------------------------------------------------------------------------------------- kernel cases
def _down(M, K, r, s):
    return dict(kind="down", name=f"{M}x{K}-r{r}", M=M, K=K, r=r, s=s)


def _wg(M, r, C, purpose):
    return dict(kind="wgrad", name=f"{M}x{r}x{C}", M=M, r=r, C=C, purpose=purpose)


# ragged row tiles, a padded rank, the widest rank and the deepest K of the towers
DOWN_CASES = [_down(80, 128, 16, 2.0), _down(200, 512, 8, 4.0), _down(330, 1024, 32, 0.5), _down(136, 4096, 64, 0.25)]
# (slices, tokens per slice) of lora_route.h's plan is pinned by tests/host/test_lora_route.cpp
WGRAD_CASES = [_wg(65, 64, 64, "one slice"), _wg(1100, 16, 136, "ragged slices, ragged C"), _wg(2500, 8, 520, "padded rank")]
DOWN_MUTANTS = ("s_twice", "tail_not_zeroed", "trunc16")


def case_id(c, dt):
    return f"{c['name']}-{DT_NAME[dt]}"


@functools.lru_cache(maxsize=None)
def down_inputs(name, dt):
    """x [M, K] N(0, 1) and the adapter a16 [r, K] N(0, 1) / sqrt(K), both 16-bit."""
    c = {d["name"]: d for d in DOWN_CASES}[name]
    seed = (c["M"] * 31 + c["K"]) * 17 + c["r"]
    return randn((c["M"], c["K"]), seed + 1, dt), randn((c["r"], c["K"]), seed + 2, dt, c["K"] ** -0.5)


def down_ref(x, a16, s, dtype=F64):
    """ts [M, r] = s (x a16^T) evaluated in `dtype` (before the 16-bit store)."""
    return (x.to(dtype) @ a16.to(dtype).t()) * s


@functools.lru_cache(maxsize=None)
def down_prepared(name, dt):
    c = {d["name"]: d for d in DOWN_CASES}[name]
    x, a = down_inputs(name, dt)
    r64, r32 = down_ref(x, a, c["s"]), down_ref(x, a, c["s"], F32)
    e32 = e32_of(r32, r64)
    ends = interval16(r64, e32, dt)
    return dict(x=x, a=a, r64=r64, r32=r32, e32=e32, ends=ends, pinned=pinned_share(*ends))


def down_concat_model(c, dt, mutant=None):
    """The [M, K + 64] buffer a faithful kernel leaves (float32 sum, one rounding to nearest), or a DOWN_MUTANT of it."""
    P = down_prepared(c["name"], dt)
    v32 = P["r32"] * (c["s"] if mutant == "s_twice" else 1.0)
    ts = trunc16(v32, dt) if mutant == "trunc16" else v32.to(dt)
    tail = torch.zeros((c["M"], TAIL - c["r"]), dtype=dt)
    if mutant == "tail_not_zeroed":
        tail = torch.full_like(tail, 2.0 ** -20)         # what an uninitialised buffer might hold: tiny, finite, not zero
    return torch.cat([P["x"], ts, tail], 1)


def check_down(c, dt, out, x_bits=None):
    """Every condition on the [M, K + 64] result of vmc_lora_down_concat (`out` on the CPU; x_bits: what the first K columns must
    hold, default the case's x).  Returns (figures of the interval rule, list of failures)."""
    P = down_prepared(c["name"], dt)
    K, r = c["K"], c["r"]
    bad = []
    want = P["x"] if x_bits is None else x_bits
    if not torch.equal(out[:, :K].view(torch.int16), want.view(torch.int16)):
        bad.append("the copied columns differ from x")
    if not bool((out[:, K + r:].view(torch.int16) == 0).all()):
        bad.append("tail columns beyond r are not exactly zero")
    m = measure16(out[:, K:K + r].contiguous(), P["r64"], P["e32"], dt, P["ends"])
    if not m["ok"]:
        bad.append(f"ts: {m['bad']} elements outside the interval (ratio {m['ratio']:.2f})")
    return m, bad


@functools.lru_cache(maxsize=None)
def wgrad_prepared(name, dt):
    """t [M, r] (the rank-r activations or gradients) and x [M, C], both N(0, 1) 16-bit; out = t^T x."""
    c = {d["name"]: d for d in WGRAD_CASES}[name]
    seed = (c["M"] * 31 + c["r"]) * 17 + c["C"]
    t, x = randn((c["M"], c["r"]), seed + 1, dt), randn((c["M"], c["C"]), seed + 2, dt)
    r64, r32 = t.to(F64).t() @ x.to(F64), t.to(F32).t() @ x.to(F32)
    return dict(t=t, x=x, r64=r64, r32=r32, e32=e32_of(r32, r64))


# ---------------------------------------------------------------------------------------------- the adapted linear
LINEAR_MUTANTS = ("s_twice", "s_missing_dA", "dB_untransposed", "us_unrounded_dy")


def _r16(v, pol):
    return v if pol.dtype is None else v.to(F32).to(pol.dtype).to(v.dtype)


class LoraLinearRef(torch.autograd.Function):
    """z = x W^T + ts B^T (+ b) with the roundings of the module docstring under `pol` (dtype None: none of them, i.e. the reference).
    round_dy: this function rounds the incoming gradient itself, dz = round16(dy) (a linear without activation); otherwise the
    caller's activation backward has stored dz 16-bit already."""

    @staticmethod
    def forward(ctx, x, W, A, B, bias, pol, s, round_dy, tag):
        mut = pol.mutant
        ts = _r16((x @ A.t()) * (s * s if mut == "s_twice" else s), pol)
        z = x @ W.t() + ts @ B.t()
        if bias is not None:
            z = z + bias
        ctx.save_for_backward(x, W, A, B, ts)
        ctx.args = (pol, s, round_dy, tag, bias is not None)
        return z

    @staticmethod
    def backward(ctx, dy):
        x, W, A, B, ts = ctx.saved_tensors
        pol, s, round_dy, tag, has_bias = ctx.args
        mut = pol.mutant
        dz = _r16(dy, pol) if round_dy else dy
        if round_dy and pol.dtype is not None:
            pol.note(tag + ".dz16", dz)
        us = _r16(((dy if mut == "us_unrounded_dy" else dz) @ B) * s, pol)
        dx = dz @ W + us @ A
        dA = us.t() @ x
        if mut == "s_missing_dA":
            dA = dA / s
        dB = dz.t() @ ts
        if mut == "dB_untransposed":
            dB = dB.t().contiguous().view(dB.shape)
        if pol.dtype is None:      # the reference: sums of absolute values behind the adapter gradients (the measure's floors)
            pol.stored.setdefault("_abs", {})[tag] = (us.abs().t() @ x.abs(), dz.abs().t() @ ts.abs(), dz.abs().sum(0))
        else:                      # the operands of the backward vmc_lora_down_concat and its stored result (us_check)
            pol.stored.setdefault("_us", {})[tag] = (dz.detach(), B.detach(), us.detach())
        return dx, None, dA, dB, (dz.sum(0) if has_bias else None), None, None, None, None


LINEAR_SHAPES = [dict(name="attn", M=85, N=128, K=128, r=8, alpha=16.0), dict(name="mlp", M=40, N=128, K=512, r=16, alpha=32.0)]


@functools.lru_cache(maxsize=None)
def linear_inputs(name, dt):
    c = {d["name"]: d for d in LINEAR_SHAPES}[name]
    M, N, K, r = c["M"], c["N"], c["K"], c["r"]
    seed = 4000 + M + N + K + r
    return dict(case=c, dtype=dt, s=c["alpha"] / r, x=randn((M, K), seed + 1, dt), W=randn((N, K), seed + 2, dt, K ** -0.5),
                A=randn((r, K), seed + 3, dt, K ** -0.5), B=randn((N, r), seed + 4, dt, r ** -0.5), b=randn((N,), seed + 5, F32, 0.25),
                dy=randn((M, N), seed + 6, F32))


def run_linear(inp, pol):
    """One adapted linear forward + backward under `pol`: {"y", "dx", "dA", "dB", "db"} in float64, plus "floor" for the reference."""
    cd = pol.compute
    leaves = {k: inp[k].to(F64).to(cd).clone().requires_grad_(True) for k in ("x", "A", "B", "b")}
    W = inp["W"].to(F64).to(cd)
    y = LoraLinearRef.apply(leaves["x"], W, leaves["A"], leaves["B"], leaves["b"], pol, inp["s"], True, "lin")
    y.backward(inp["dy"].to(F64).to(cd))
    out = {"y": _r16(y.detach(), pol).to(F64), "dx": _r16(leaves["x"].grad, pol).to(F64), "dA": leaves["A"].grad.to(F64),
           "dB": leaves["B"].grad.to(F64), "db": leaves["b"].grad.to(F64)}
    if pol.dtype is None:
        absA, absB, absb = pol.stored["_abs"]["lin"]
        out["floor"] = {"dA": EPS32 * float(absA.max()), "dB": EPS32 * float(absB.max()), "db": EPS32 * float(absb.max()),
                        "y": EPS32 * float(out["y"].abs().max()), "dx": EPS32 * float(out["dx"].abs().max())}
    return out


def linear_plain64(inp):
    """float64 autograd of x (W + s B A)^T + b: what the adapted linear is, with no concat, no tail and no rounding."""
    lv = {k: inp[k].to(F64).clone().requires_grad_(True) for k in ("x", "A", "B", "b")}
    y = lv["x"] @ (inp["W"].to(F64) + inp["s"] * (lv["B"] @ lv["A"])).t() + lv["b"]
    y.backward(inp["dy"].to(F64))
    return {"y": y.detach(), "dx": lv["x"].grad, "dA": lv["A"].grad, "dB": lv["B"].grad, "db": lv["b"].grad}


@functools.lru_cache(maxsize=None)
def linear_ref64(name, dt):
    return run_linear(linear_inputs(name, dt), Policy())


@functools.lru_cache(maxsize=None)
def linear_model16(name, dt):
    return run_linear(linear_inputs(name, dt), Policy(dt))


def linear_eval32(name, dt, mutant=None):
    return run_linear(linear_inputs(name, dt), Policy(dt, compute=F32, mutant=mutant))


def us_check(name, dt, mutant=None):
    """The interval rule on ``us``, the 16-bit output of the backward vmc_lora_down_concat, of a float32 evaluation (or a mutant of
    it): the kernel's operands are dz = round16(dy) and B16, so r64 = s (dz B16) -- the check that tells a ``us`` built from the
    unrounded dy from the designed one, which the step-level measure cannot (an unrounded dy is closer to the reference, not
    farther).  Returns gemm_refs.measure16's figures."""
    inp = linear_inputs(name, dt)
    pol = Policy(dt, compute=F32, mutant=mutant)
    run_linear(inp, pol)
    dz, B, us = pol.stored["_us"]["lin"]
    dz16 = inp["dy"].to(dt)                                       # the designed operand, whatever the evaluation used
    assert torch.equal(dz.to(dt).view(torch.int16), dz16.view(torch.int16))
    r64, r32 = (dz16.to(F64) @ B.to(F64)) * inp["s"], (dz16.to(F32) @ B.to(F32)) * inp["s"]
    return measure16(us.to(dt), r64, e32_of(r32, r64), dt)


# ---------------------------------------------------------------------------------------------- the student step with adapters
# FlowStudentModel(lora_rank = r) on the tiny geometries: frames -> (emb, emb_distill, logits) with the upstream gradients given
# (the method of DESIGN.md §5.4 and of student_step_refs.run_step, whose pieces are imported).  The tower is frozen: the tensors are
# the three outputs, "g.<adapter>" under the adapter's name inside VisionTransformer, and "g.<head parameter>".
SITE_OF = {"attn": (("attn.in_proj_weight", "attn.in_proj_lora_A", "attn.in_proj_lora_B"),
                    ("attn.out_proj.weight", "attn.out_proj.lora_A", "attn.out_proj.lora_B")),
           "mlp": (("mlp.c_fc.weight", "mlp.c_fc.lora_A", "mlp.c_fc.lora_B"), ("mlp.c_proj.weight", "mlp.c_proj.lora_A", "mlp.c_proj.lora_B"))}


def _step(name, geom, R, p, L, E, F, B, T, C, rank, targets, seed):
    g = R // p
    return dict(name=name, geometry=geom, R=R, p=p, L=L, E=E, F=F, N=g * g + 1, K=3 * p * p, B=B, T=T, C=C, rank=rank, alpha=2.0 * rank,
                targets=tuple(targets), seed=seed, cls_only=True, level="student")


STEP_CASES = [
    _step("t32-r8-attn", "ViT-tiny/32", 64, 32, 2, 64, 6, 2, 3, 140, 8, ("attn",), 107),
    _step("t32-r16-attn+mlp", "ViT-tiny/32", 64, 32, 2, 64, 6, 2, 3, 140, 16, ("attn", "mlp"), 68),
    _step("t14-r16-attn", "ViT-tiny/14", 56, 14, 3, 96, 5, 5, 1, 10, 16, ("attn",), 33),
    _step("t14-r8-attn+mlp", "ViT-tiny/14", 56, 14, 3, 96, 5, 5, 1, 10, 8, ("attn", "mlp"), 34),
]
STEP_BY_NAME = {c["name"]: c for c in STEP_CASES}
# Upstream gradients = N(0, 1) times this power of two.  f16: chosen (on the CPU, from step_model16 alone) so that no stored 16-bit
# gradient exceeds 2^14 and fewer than 1 % of the non-zero elements of any of them are f16-subnormal; the host test asserts both.
UP_SCALE = {BF16: 1.0, F16: 2.0 ** 8}
# the case each mutant of the float32 evaluation of the step must fail (us_unrounded_dy is told apart by us_check alone: see there)
STEP_MUTANT_CASE = {"s_twice": "t32-r8-attn", "s_missing_dA": "t32-r16-attn+mlp", "dB_untransposed": "t14-r16-attn"}


def step_param_shapes(c):
    """Every base parameter of the case (VisionTransformer's names; the heads under FlowStudentModel's) -> shape."""
    D, E, N, p = ST.WIDTH, c["E"], c["N"], c["p"]
    s = {"conv1.weight": (D, 3, p, p), "class_embedding": (D,), "positional_embedding": (N, D), "ln_pre.weight": (D,), "ln_pre.bias": (D,)}
    for i in range(c["L"]):
        for n, sh in zip(ST.BLOCK_PARAMS, ((D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,))):
            s[f"transformer.resblocks.{i}.{n}"] = sh
    s.update({"ln_post.weight": (D,), "ln_post.bias": (D,), "proj": (D, E)})
    for n, sh in zip(ST.HEAD_PARAMS, ((E, E), (E,), (E, E), (E,), (E // 2, E), (E // 2,), (c["C"], E // 2), (c["C"],))):
        s[n] = sh
    return s


def adapter_names(c):
    """[(weight name, A name, B name)] of every adapted linear, inside VisionTransformer."""
    return [tuple(f"transformer.resblocks.{i}.{n}" for n in trip) for i in range(c["L"]) for t in c["targets"] for trip in SITE_OF[t]]


@functools.lru_cache(maxsize=None)
def step_inputs(name, dtype, fresh=False):
    """As student_step_refs.make_inputs (same distributions, the same attention stress and ReLU calibration), plus the adapters:
    A N(0, 1) / sqrt(K), B N(0, 1) / (4 sqrt(r)) -- with s = 2 the adapter term is about half the base weight's -- or B = 0 (fresh)."""
    c = STEP_BY_NAME[name]
    g = torch.Generator().manual_seed(7000 + c["seed"])
    rn = lambda *s, scale=1.0, shift=0.0: torch.randn(*s, generator=g) * scale + shift
    p = {}
    for n, sh in step_param_shapes(c).items():
        if ST.is_matrix(n):
            p[n] = rn(*sh, scale=(8.0 if n == "classification_head.0.weight" else 1.0) * ST._fan_in(n, sh) ** -0.5)
        elif n.endswith("ln_1.weight") or n.endswith("ln_2.weight") or n in ("ln_pre.weight", "ln_post.weight"):
            p[n] = rn(*sh, scale=0.25, shift=1.0)
        elif n in ("class_embedding", "positional_embedding"):
            p[n] = rn(*sh)
        else:
            p[n] = rn(*sh, scale=0.25)
    ad = {}
    for wn, an, bn in adapter_names(c):
        N_, K_ = p[wn].shape
        ad[an] = rn(c["rank"], K_, scale=K_ ** -0.5)
        ad[bn] = rn(N_, c["rank"], scale=0.25 * c["rank"] ** -0.5) * (0.0 if fresh else 1.0)
    inp = dict(case=c, dtype=dtype, p32=p, ad32=ad, s=c["alpha"] / c["rank"])
    inp["frames"] = torch.randint(0, 256, (c["F"], 3, c["R"], c["R"]), generator=g, dtype=torch.int64).to(torch.uint8)
    sc = UP_SCALE[dtype]
    inp["up"] = {"emb": rn(c["F"], c["E"]) * sc, "emb_distill": rn(c["F"], c["E"]) * sc, "logits": rn(c["B"], c["C"]) * sc}
    base = {n: v.clone() for n, v in p.items() if n.endswith("in_proj_weight")}
    for stress in (1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 4.0):
        for n, v in base.items():
            p[n] = torch.cat([v[:2 * ST.WIDTH] * stress, v[2 * ST.WIDTH:]])
        inp["w16"] = {n: v.to(dtype) for n, v in p.items() if ST.is_matrix(n)}
        inp["ad16"] = {n: v.to(dtype) for n, v in ad.items()}
        with torch.no_grad():
            probe = run_lora_step(inp, Policy(), probe=True)
        if min(probe["attn_peak"]) >= 4.0 / c["N"]:
            break
    inp["stress"], inp["attn_peak"] = stress, probe["attn_peak"]
    b, margin = TC._relu_gap_bias(probe["head_z0"], p["classification_head.0.bias"].to(F64))
    p["classification_head.0.bias"] = b
    inp["relu_margin"] = margin
    return inp


def run_lora_step(inp, pol, probe=False, adapters=True):
    """One step under `pol` (dtype None: the float64 reference; mutant: one of LINEAR_MUTANTS).  adapters=False: the base model's
    forward (what a freshly initialised adapter, B = 0, must reproduce).  Returns float64 tensors and, for the reference, "floor"."""
    c = inp["case"]
    F, N, p, E, D, L = c["F"], c["N"], c["p"], c["E"], ST.WIDTH, c["L"]
    cd, ref = pol.compute, pol.dtype is None
    leaves, absrec, peaks, extra = {}, [], [], {}
    sites = {wn: (an, bn) for wn, an, bn in adapter_names(c)} if adapters else {}

    def const(name):
        src = inp["w16"][name] if name in inp["w16"] else inp["p32"][name]
        return src.to(F64).to(cd)

    def leaf(name):
        if name not in leaves:
            src = inp["ad16"][name] if name in inp["ad16"] else (inp["w16"][name] if name in inp["w16"] else inp["p32"][name])
            leaves[name] = src.to(F64).to(cd).clone().requires_grad_(True)
        return leaves[name]

    def head_lin(x, wname, bname):
        W = leaf(wname)
        y = x @ W.t() + leaf(bname)
        if ref and y.requires_grad:
            y.register_hook(lambda g, x=x.detach(), k=(wname, bname): absrec.append((k, g.abs(), x.abs())))
        return y

    def tower_lin(x, wname, bname, round_dy):
        """A linear of a block: adapted where the case says so (the rounding of dy is then LoraLinearRef's), frozen otherwise."""
        W = const(wname)
        b = const(bname)
        if wname in sites:
            an, bn = sites[wname]
            return LoraLinearRef.apply(x, W, leaf(an), leaf(bn), b, pol, inp["s"], round_dy, wname)
        y = x @ W.t() + b
        return pol.g(y, wname + ".dy16") if round_dy else y

    def act(z, kind, tag):
        return ST._ACT[kind][0](z) if ref else ST._ActSaved.apply(z, pol, kind, tag, False)

    def ln(x, name):
        return TC._layer_norm(x, const(name + ".weight"), const(name + ".bias"), pol)

    xp = pol.r(ST.patch_rows(inp["frames"], p, pol) @ const("conv1.weight").reshape(D, -1).t())
    xs = (torch.cat([const("class_embedding").expand(F, 1, D), xp.reshape(F, N - 1, D)], 1) + const("positional_embedding")).reshape(F * N, D)
    xs = ln(xs, "ln_pre")
    for i in range(L):
        pre, last = f"transformer.resblocks.{i}.", i + 1 == L
        h = pol.g(pol.r(ln(xs, pre + "ln_1")), pre + "dh1_16")
        # (the attention backward stores dqkv 16-bit itself: LinearFn's cast of it is the identity)
        qkv = pol.r(tower_lin(h, pre + "attn.in_proj_weight", pre + "attn.in_proj_bias", False))
        if ref or probe:
            with torch.no_grad():
                q, k = (qkv[:, j * D:(j + 1) * D].reshape(F, N, ST.HEADS, 64).transpose(1, 2) for j in (0, 1))
                peaks.append(float(torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1).max(-1).values.median()))
        o = ST.attn_plain(qkv, F, N) if ref else pol.g(ST._VitAttn.apply(qkv, pol, F, N, None), pre + "do16")
        if last:
            o, xs = o.reshape(F, N, D)[:, 0], xs.reshape(F, N, D)[:, 0]
        xs = xs + tower_lin(o, pre + "attn.out_proj.weight", pre + "attn.out_proj.bias", True)
        h = pol.g(pol.r(ln(xs, pre + "ln_2")), pre + "dh2_16")
        u = act(tower_lin(h, pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias", False), "quickgelu", pre + "c_fc")
        xs = xs + tower_lin(u, pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias", True)
    h = pol.g(pol.r(ln(xs, "ln_post")), "dh_post16")
    emb = pol.g(h @ const("proj"), "dE16")
    B, T, C = c["B"], c["T"], c["C"]
    x16 = pol.g(pol.r(emb), "dx_fc1_16")
    hh = act(head_lin(x16, "residual_mlp.fc1.weight", "residual_mlp.fc1.bias"), "gelu", "fc1")
    m = pol.g(head_lin(hh, "residual_mlp.fc2.weight", "residual_mlp.fc2.bias"), "dm16")
    outs = {"emb": emb, "emb_distill": emb + ST.ALPHA * m}
    pooled = pol.g(pol.r(emb.reshape(B, T, E).sum(1) * (1.0 / T)), "dpooled16")
    if probe:
        return {"attn_peak": peaks, "head_z0": pooled @ leaf("classification_head.0.weight").t()}
    z = head_lin(pooled, "classification_head.0.weight", "classification_head.0.bias")
    extra["relu_negative_share"] = float((z.detach() < 0).double().mean())
    extra["relu_min_abs"] = float(z.detach().abs().min())
    outs["logits"] = pol.g(head_lin(act(z, "relu", "head0"), "classification_head.2.weight", "classification_head.2.bias"), "dlogits16")
    names = list(outs)
    live = [n for n in names if outs[n].requires_grad]           # without adapters nothing trains in front of emb
    torch.autograd.backward([outs[n] for n in live], [inp["up"][n].to(F64).to(cd) for n in live])
    out = {n: outs[n].detach().to(F64) for n in names}
    for name in list(inp["ad16"] if adapters else ()) + list(ST.HEAD_PARAMS):
        t = leaf(name)
        out["g." + name] = (t.grad if t.grad is not None else torch.zeros_like(t)).to(F64)
    out.update(extra)
    out["attn_peak"] = peaks
    if ref:
        fl = {}
        for (wname, bname), g_, x_ in absrec:
            fl["g." + wname] = max(fl.get("g." + wname, 0.0), EPS32 * float((g_.t() @ x_).max()))
            fl["g." + bname] = max(fl.get("g." + bname, 0.0), EPS32 * float(g_.sum(0).max()))
        for wn, (an, bn) in sites.items():
            absA, absB, _ = pol.stored["_abs"][wn]
            fl["g." + an], fl["g." + bn] = EPS32 * float(absA.max()), EPS32 * float(absB.max())
        for k in ST.tensor_names(out):
            fl.setdefault(k, EPS32 * float(out[k].abs().max()))
        out["floor"] = fl
    return out


@functools.lru_cache(maxsize=None)
def step_ref64(name, dtype, fresh=False, adapters=True):
    pol = Policy()
    out = run_lora_step(step_inputs(name, dtype, fresh), pol, adapters=adapters)
    return out


@functools.lru_cache(maxsize=None)
def step_model16(name, dtype, fresh=False, adapters=True):
    pol = Policy(dtype)
    out = run_lora_step(step_inputs(name, dtype, fresh), pol, adapters=adapters)
    out["stored"] = {k: v for k, v in pol.stored.items() if not k.startswith("_")}
    return out


def step_eval32(name, dtype, mutant=None):
    return run_lora_step(step_inputs(name, dtype), Policy(dtype, compute=F32, mutant=mutant))
