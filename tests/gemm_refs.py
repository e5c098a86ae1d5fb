"""Float64 references, measures, input makers and case lists for the GEMM family (vmc_linear / _preact / _variant, vmc_linear_splitk_f32,
vmc_linear_wgrad_tn / _bias_tn / _tn_group).  No GPU code: torch on the CPU only.  tests/test_gemm_refs_host.py checks the references,
the route of every case (tests/host/gemm_route_dump.cpp on gemm_route.h) and the measure itself; tests/test_gpu_gemm_parity.py
compares the HIP kernels with them.  The yardstick and its margin are train_kernel_refs' (DESIGN 5): every reference takes the values
the kernel sees (16-bit-rounded operands, f32 bias, the residual as stored), r64 evaluates the operation in float64, the same
function in float32 on the CPU gives e32 = max|r32 - r64| / max|r64|.

  f32 outputs:     max|got - r64| / max|r64| <= MARGIN max(e32, 2^-23)
  16-bit outputs:  round16(r64 - B) <= got <= round16(r64 + B) elementwise,  B = MARGIN max(e32, 2^-23) max|r64|
                   round16: torch's cast (nearest-even, monotone).  A kernel whose fp32 value before the store lies within B of r64
                   and which rounds that value once, to nearest, passes; where the two ends coincide the output is pinned to the bit.
                   A case is only meaningful while most elements are pinned: SHARE_MIN, asserted on the CPU from the reference alone.
"""
from collections import OrderedDict

import torch

import train_kernel_refs as R
from train_kernel_refs import BF16, DT16, DT_NAME, E32_MAX, EPS32, F16, F32, MARGIN, bound32, e32_of, padded  # noqa: F401  (re-exported)

F64 = torch.float64
SHARE_MIN = {BF16: 0.9, F16: 0.6}
MAX_MACS = 2e10
ACT_NAME = ("none", "qgelu", "gelu", "relu")


# ---------------------------------------------------------------------------------------------- references
def row_maps(M, out_row_group=0, res_row_mod=0):
    """orow / rrow of include/vmc.h for the GEMM rows 0 .. M-1."""
    m = torch.arange(M)
    orow = m + m // out_row_group + 1 if out_row_group else m
    rrow = m % res_row_mod if res_row_mod else orow
    return orow, rrow


def linear_ref64(a, w, bias=None, res=None, act=0, alpha=1.0, out_row_group=0, res_row_mod=0, dtype=F64, prod=None):
    """Z = A W^T + bias and C = alpha act(Z) + res[rrow], both [M, N] in GEMM row order (row m belongs at output row orow[m]),
    evaluated in `dtype`.  prod: A W^T in `dtype`, where it is shared between epilogues."""
    z = (a.to(dtype) @ w.to(dtype).t()) if prod is None else prod
    if bias is not None:
        z = z + bias.to(dtype)
    orow, rrow = row_maps(z.shape[0], out_row_group, res_row_mod)
    c = R.act_ref(z, act, dtype)
    if float(alpha) != 1.0:
        c = c * float(alpha)
    if res is not None:
        c = c + res.to(dtype)[rrow]
    return {"C": c, "Z": z, "orow": orow}


def wgrad_ref64(dy, x, dtype=F64):
    """dW [N, K] = dY^T X and dbias [N] = column sums of dY."""
    dy = dy.to(dtype)
    return {"C": dy.t() @ x.to(dtype), "dbias": dy.sum(0)}


# ---------------------------------------------------------------------------------------------- measures
def measure32(got, r64, e32):
    """f32 output: err = max|got - r64| / max|r64| against MARGIN max(e32, 2^-23)."""
    err = R.max_rel(got, r64)
    ratio = err / max(e32, EPS32)
    return dict(err=err, e32=e32, ratio=ratio, ok=bool(ratio <= MARGIN) and bool(torch.isfinite(got).all()))


def interval16(r64, e32, dtype):
    """(lo, hi) in `dtype`: the roundings of r64 -+ B."""
    B = bound32(e32) * r64.abs().max().item()
    return (r64 - B).to(dtype), (r64 + B).to(dtype)


def pinned_share(lo, hi):
    return (lo.view(torch.int16) == hi.view(torch.int16)).double().mean().item()


def measure16(got, r64, e32, dtype, ends=None):
    """16-bit output under the interval rule.  bad: elements outside [lo, hi] (NaN counts); ratio: the smallest b with
    round16(r64 - b) <= got <= round16(r64 + b) everywhere, estimated from the rounding cell of got, over max(e32, 2^-23) max|r64|
    (reported, not asserted)."""
    lo, hi = ends if ends is not None else interval16(r64, e32, dtype)
    g = got.detach().to("cpu")
    assert g.dtype is dtype and g.shape == r64.shape
    g64 = g.to(F64)
    inside = (g64 >= lo.to(F64)) & (g64 <= hi.to(F64))
    bad = int((~inside).sum())
    half = R.ulp(g64, dtype) / 2
    need = torch.clamp(torch.maximum(g64 - half - r64, r64 - g64 - half), min=0.0)
    need = torch.nan_to_num(need, nan=float("inf")).max().item()
    s = r64.abs().max().item()
    return dict(bad=bad, share_bad=bad / g.numel(), pinned=pinned_share(lo, hi), e32=e32, ratio=need / (s * max(e32, EPS32)), ok=bad == 0)


def trunc16(v32, dtype):
    """A 16-bit store that truncates toward zero instead of rounding to nearest (a mutant for the self-test of the measure)."""
    t = v32.to(dtype)
    over = t.to(F64).abs() > v32.to(F64).abs()
    return torch.where(over, (t.view(torch.int16) - 1).view(dtype), t)


# ---------------------------------------------------------------------------------------------- cases
def _lin(name, M, N, K, plan, act=0, bias=True, res=None, out="16", alpha=1.0, z=False, pad=None, org=0, rrm=0, variant=None, env=None,
         dts=DT16, sub=False):
    """One vmc_linear call.  plan: what gemm_route_dump prints for it.  res: None, "f32" or "16"; out: "f32" or "16".
    pad: leading dimensions as increments over K (lda, ldw) / N (ldc, ldres, ldz).  variant: vmc_linear_variant's.
    env: (name, value) of a VMC_GEMM_* switch, read once per process.  sub: the A operand scaled into the f16 subnormals."""
    p = dict(lda=0, ldw=0, ldc=0, ldres=0, ldz=0)
    p.update(pad or {})
    return dict(kind="linear", name=name, M=M, N=N, K=K, plan=plan, act=act, bias=bias, res=res, out=out, alpha=alpha, z=z, pad=p, org=org,
                rrm=rrm, variant=variant, env=env, dts=tuple(dts), sub=sub)


EPI_PAD = dict(lda=8, ldw=16, ldres=12, ldz=4)


def _epilogue_matrix(tag, M, N, K, plan):
    """Every activation x residual kind x output type, with and without Z, at ldc = N + 4 and N + 8, alpha = 0.75, every leading dimension
    padded.  The cases of one (act, res, out) are adjacent: they share one reference."""
    cs = []
    for act in range(4):
        for res in (None, "f32", "16"):
            for out in ("f32", "16"):
                for z in (False, True):
                    for ldc in (4, 8):
                        nm = f"{tag}-{ACT_NAME[act]}-res{res or '0'}-out{out}{'-z' if z else ''}-ldc+{ldc}"
                        cs.append(_lin(nm, M, N, K, plan, act=act, res=res, out=out, alpha=0.75, z=z, pad=dict(EPI_PAD, ldc=ldc)))
    return cs


# the smallest shapes that reach each kernel of gemm_route.h (asserted through the dump by the host test)
LINEAR_CASES = [
    _lin("cfg2-n4", 333, 204, 128, "1 TILE 2 0 333"),                    # N % 8 == 4: the 8-wide stores are off
    _lin("cfg2-k9", 300, 140, 576, "1 TILE 2 0 300", act=1),             # nine K tiles: no U grouping
    _lin("cfg3", 300, 140, 512, "1 TILE 3 0 300", act=1),
    _lin("cfg6", 130, 260, 1088, "1 TILE 6 0 130", res="f32", out="f32"),
    _lin("cfg7", 130, 260, 1024, "1 TILE 7 0 130", act=3),
    _lin("cfg1", 1100, 1800, 192, "1 TILE 1 0 1100", act=2, z=True),
    _lin("cfg0-k64", 3850, 3076, 64, "1 TILE 0 0 3850", act=1),
    _lin("cfg0-twostage", 3850, 3076, 256, "1 TILE 0 0 3850", variant=0, res="16"),
    _lin("g8", 3900, 4096, 256, "1 G8 0 0 3900", act=1, z=True),
    _lin("g8-band", 4100, 2304, 256, "1 G8 0 0 4100", alpha=0.75),       # 129 .. 191 tiles of 256 x 256
    _lin("g8p-bias", 3072, 4096, 256, "1 G8P 0 0 3072", alpha=0.75),
    _lin("g8p-nobias", 3072, 4096, 256, "1 G8P 1 0 3072", alpha=0.75, bias=False),
    _lin("g8p-qgelu", 3072, 4096, 256, "1 G8P 2 0 3072", act=1),
    _lin("g8p-qgelu-z", 3072, 4096, 256, "1 G8P 3 0 3072", act=1, z=True),
    _lin("g8p-relu", 3072, 4096, 256, "1 G8P 4 0 3072", act=3),
    _lin("g8p32-bias", 3072, 4096, 256, "1 G8P 5 0 3072", variant=5),
    _lin("g8p32-nobias", 3072, 4096, 256, "1 G8P 6 0 3072", variant=5, bias=False),
    _lin("g8p32-qgelu", 3072, 4096, 256, "1 G8P 7 0 3072", variant=5, act=1),
    _lin("g8p-two-tiles-bias", 8192, 4096, 384, "1 G8P 0 0 8192"),       # 512 tiles: two per workgroup
    _lin("g8p-two-tiles-qgelu", 8192, 4096, 384, "1 G8P 2 0 8192", act=1),
    _lin("tail-split", 4300, 4096, 256, "2 G8P 0 0 4096 TILE 2 4096 204"),
    # out_row_group / res_row_mod: patch rows -> token rows, positional-embedding broadcast
    _lin("rows-3x16", 48, 128, 64, "1 TILE 2 0 48", bias=False, res="f32", out="f32", org=16, rrm=16),
    _lin("rows-5x49", 245, 772, 192, "1 TILE 2 0 245", res="f32", out="f32", org=49, rrm=49, pad=dict(lda=8, ldc=4, ldres=12)),
    _lin("rows-5x49-16", 245, 772, 192, "1 TILE 2 0 245", res="16", out="16", org=49, rrm=49, pad=dict(ldw=16, ldc=8)),
    _lin("resmod-245", 245, 772, 192, "1 TILE 2 0 245", res="f32", out="16", rrm=49, act=1, alpha=0.75),
    # f16 operands in the subnormal range: A (the dY of an input-gradient GEMM) scaled by 2^-16, no bias, f32 out
    _lin("subnormal-a", 333, 204, 128, "1 TILE 2 0 333", bias=False, out="f32", dts=(F16,), sub=True),
]
EPI_SMALL = _epilogue_matrix("epi", 333, 204, 128, "1 TILE 2 0 333")
EPI_G8 = _epilogue_matrix("epi-g8", 3900, 4096, 256, "1 G8 0 0 3900")

# switches read once per process: each runs in a child process of its own
ENV_CASES = [
    _lin("u2-cfg4", 300, 140, 512, "1 TILE 4 0 300", act=1, env=("VMC_GEMM_U", "2")),
    _lin("u2-cfg8", 130, 260, 1024, "1 TILE 8 0 130", act=3, env=("VMC_GEMM_U", "2")),
    _lin("ks-cfg5", 700, 900, 1024, "1 TILE 5 0 700", act=1, env=("VMC_GEMM_KS", "1")),
    _lin("ks-cfg9", 130, 260, 1024, "1 TILE 9 0 130", res="f32", out="f32", env=("VMC_GEMM_KS", "1")),
]
for _v in range(1, 12):
    ENV_CASES.append(_lin(f"sweep-{_v}", 300, 260, 192, f"1 TILE {(-1, 10, 11, 12, 13, 2, 1, 14, 15, 16, 17, 18)[_v]} 0 300",
                          env=("VMC_GEMM_CFG", str(_v))))
ENV_SETTINGS = list(OrderedDict.fromkeys(c["env"] for c in ENV_CASES))


def _sk(name, M, N, K, plan, pad=(0, 0), dts=DT16, sub=False):
    """vmc_linear_splitk_f32.  plan: slices, K tiles per slice, K tiles of the last slice."""
    return dict(kind="splitk", name=name, M=M, N=N, K=K, plan=plan, pad=pad, dts=tuple(dts), sub=sub)


SPLITK_CASES = [
    _sk("one-slice", 64, 144, 192, (1, 3, 3)),
    _sk("ragged-last", 64, 144, 1088, (4, 5, 2), pad=(8, 16)),
    _sk("130x260", 130, 260, 4096, (16, 4, 4)),
    _sk("512x512", 512, 512, 8192, (32, 4, 4)),
    _sk("subnormal-a", 64, 144, 1088, (4, 5, 2), dts=(F16,), sub=True),
]


def _tn(name, M, N, K, plan, win=(0, 0), dts=DT16, sub=False):
    """vmc_linear_wgrad_tn and _bias_tn (each case runs both).  plan: kernel, token slices, 128-token pairs per slice.
    win: dY / X are column windows of tensors (lddy, ldx) = (N + win[0], K + win[1]) wide whose other columns hold NaN."""
    return dict(kind="tn", name=name, M=M, N=N, K=K, plan=plan, win=win, dts=tuple(dts), sub=sub)


TN_CASES = [
    _tn("77", 77, 144, 200, ("TN128", 1, 0)),
    _tn("1000-window", 1000, 264, 136, ("TN128", 4, 0), win=(24, 16)),
    _tn("4099", 4099, 520, 264, ("TN128", 13, 0)),
    _tn("tn256", 10880, 1032, 776, ("TN256", 11, 8)),       # the fewest tokens the 256 x 256 kernel takes at 5 x 4 ragged tiles
    _tn("subnormal-dy", 1000, 264, 136, ("TN128", 4, 0), dts=(F16,), sub=True),
]
# vmc_linear_wgrad_tn_group: one launch of four problems (M, N, K, dbias, (lddy - N, ldx - K))
GROUP_PROBLEMS = [(256, 64, 40, False, (0, 0)), (2560, 520, 264, True, (0, 0)), (1024, 1000, 264, False, (24, 16)), (512, 776, 1032, True, (0, 0))]

GROUP_CASES = [dict(_tn(f"group-{_M}x{_N}x{_K}", _M, _N, _K, ("TN_GROUP", 1, 0), _w), dbias=_b) for _M, _N, _K, _b, _w in GROUP_PROBLEMS]

ALL_CASES = LINEAR_CASES + EPI_SMALL + EPI_G8 + ENV_CASES + SPLITK_CASES + TN_CASES


def case_id(c, dt):
    return f"{c['name']}-{DT_NAME[dt]}"


def flat(cases):
    """(case, dtype) pairs, dtype outermost within runs of one shape so that neighbours share a product."""
    out = []
    i = 0
    while i < len(cases):
        j = i
        while j < len(cases) and (cases[j]["M"], cases[j]["N"], cases[j]["K"]) == (cases[i]["M"], cases[i]["N"], cases[i]["K"]):
            j += 1
        for dt in DT16:
            out += [(c, dt) for c in cases[i:j] if dt in c["dts"]]
        i = j
    return out


def macs(c):
    return c["M"] * c["N"] * c["K"]


def dump_line(c, dt):
    """The line of tests/host/gemm_route_dump.cpp that describes the case as the GPU test issues it."""
    M, N, K = c["M"], c["N"], c["K"]
    code = {F32: 0, BF16: 1, F16: 2}
    if c["kind"] == "linear":
        p, env = c["pad"], dict([c["env"]] if c["env"] else [])
        f = [M, N, K, K + p["lda"], K + p["ldw"], N + p["ldc"], (N + p["ldres"]) if c["res"] else 0, (N + p["ldz"]) if c["z"] else 0, c["act"],
             int(c["bias"]), int(c["res"] is not None), int(c["z"]), code[F32 if c["out"] == "f32" else dt],
             code[F32 if c["res"] == "f32" else dt] if c["res"] else 0, c["org"], c["rrm"], code[dt], 1 if c["variant"] is None else c["variant"],
             int(env.get("VMC_GEMM_CFG", 0)), int(env.get("VMC_GEMM_KS", 0)), int(env.get("VMC_GEMM_U", 4)), 0]
        return "linear " + " ".join(str(v) for v in f)
    if c["kind"] == "splitk":
        return f"splitk {M} {N} {K}"
    return f"tn {M} {N} {K} {N + c['win'][0]} {K + c['win'][1]}"


def plan_text(c):
    return c["plan"] if isinstance(c["plan"], str) else " ".join(str(v) for v in c["plan"])


# ---------------------------------------------------------------------------------------------- inputs and shared references
SUB_SCALE = 2.0 ** -16


def _seed(c):
    return (c["M"] * 31 + c["N"]) * 17 + c["K"]


def operands(c, dt):
    """The two 16-bit operands: N(0,1) activations (dY for the TN kernels), K^-1/2-scaled weights (N(0,1) X for the TN kernels)."""
    s = _seed(c) + (500 if c["sub"] else 0)
    M, N, K = c["M"], c["N"], c["K"]
    if c["kind"] == "tn":
        return R.randn((M, N), s + 1, dt, SUB_SCALE if c["sub"] else 1.0), R.randn((M, K), s + 2, dt)
    return R.randn((M, K), s + 1, dt, SUB_SCALE if c["sub"] else 1.0), R.randn((N, K), s + 2, dt, K ** -0.5)


_PROD = OrderedDict()       # (kind, M, N, K, dt, sub) -> operands, A W^T (or dY^T X and colsum dY) in f64 and f32; the two most recent only (up to 400 MB each)
_EPI = OrderedDict()        # the reference of one (product, epilogue): shared by the cases that differ in Z / ldc / kernel variant only


def product(c, dt):
    key = (c["kind"] == "tn", c["M"], c["N"], c["K"], dt, c["sub"])
    if key not in _PROD:
        a, b = operands(c, dt)
        if c["kind"] == "tn":
            p = dict(a=a, b=b, p64=wgrad_ref64(a, b), p32=wgrad_ref64(a, b, F32))
        else:
            p = dict(a=a, b=b, p64=a.to(F64) @ b.to(F64).t(), p32=a.to(F32) @ b.to(F32).t())
        _PROD[key] = p
        while len(_PROD) > 2:
            _PROD.popitem(last=False)
    return _PROD[key]


def clear():
    _PROD.clear()
    _EPI.clear()


def epilogue_inputs(c, dt):
    """bias [N] f32 (N(0,1)) and the residual as stored (N(0,1); [res rows, N]: res_row_mod rows where that applies, else one per output row)."""
    s = _seed(c)
    M, N = c["M"], c["N"]
    out_rows = M + M // c["org"] if c["org"] else M
    # an activation without a residual leaves ReLU's zeros and GELU's small negative values, which no bound of this kind pins: there the
    # bias is 2.5 + N(0,1) / 2, so that about one pre-activation in a hundred is negative and the rest of the output stays pinned
    shifted = c["act"] != 0 and c["res"] is None
    bias = R.randn((N,), s + 3, F32, 0.5 if shifted else 1.0, 2.5 if shifted else 0.0) if c["bias"] else None
    res = None
    if c["res"]:
        res = R.randn((c["rrm"] or out_rows, N), s + 4, F32 if c["res"] == "f32" else dt)
    return bias, res, out_rows


def prepare(c, dt):
    """Everything a comparison needs for one case: operands, epilogue inputs, r64 / e32 per output and, for 16-bit outputs, the two
    ends of the interval."""
    assert macs(c) <= MAX_MACS
    P = product(c, dt)
    if c["kind"] == "linear":
        key = (c["M"], c["N"], c["K"], dt, c["sub"], c["act"], c["bias"], c["res"], c["out"], c["alpha"], c["org"], c["rrm"])
    else:
        key = (c["kind"], c["M"], c["N"], c["K"], dt, c["sub"])
    if key in _EPI:
        return _EPI[key]
    out = dict(a=P["a"], b=P["b"], outs={})
    if c["kind"] == "linear":
        bias, res, out_rows = epilogue_inputs(c, dt)
        kw = dict(bias=bias, res=res, act=c["act"], alpha=c["alpha"], out_row_group=c["org"], res_row_mod=c["rrm"])
        r64 = linear_ref64(None, None, prod=P["p64"], **kw)
        r32 = linear_ref64(None, None, prod=P["p32"], dtype=F32, **kw)
        out.update(bias=bias, res=res, out_rows=out_rows, orow=r64["orow"])
        names = [("C", F32 if c["out"] == "f32" else dt)] + ([] if c["org"] else [("Z", dt)])
    elif c["kind"] == "splitk":
        r64, r32 = {"C": P["p64"]}, {"C": P["p32"]}
        names = [("C", F32)]
    else:
        r64, r32 = P["p64"], P["p32"]
        names = [("C", F32), ("dbias", F32)]
    for n, odt in names:
        e32 = e32_of(r32[n], r64[n])
        o = dict(r64=r64[n], r32=r32[n], e32=e32, dtype=odt)
        if odt is not F32:
            o["ends"] = interval16(r64[n], e32, odt)
            o["pinned"] = pinned_share(*o["ends"])
        out["outs"][n] = o
    _EPI[key] = out
    while len(_EPI) > 2:
        _EPI.popitem(last=False)
    return out


def judge(got, o):
    """The rule for one output (got on the CPU, in the output's dtype and the reference's row order)."""
    if o["dtype"] is F32:
        return measure32(got, o["r64"], o["e32"])
    return measure16(got, o["r64"], o["e32"], o["dtype"], o["ends"])
