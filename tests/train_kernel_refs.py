"""Plain references, error measures and case lists for the small training-path kernels (LayerNorm forward / backward family,
activations, adds, casts, dropout).  No GPU code: torch and numpy on the CPU only.  tests/test_train_kernel_refs_host.py
checks the references themselves; tests/test_gpu_train_kernels.py compares the HIP kernels with them.

Every reference takes the values the kernel sees (inputs already rounded to their storage dtype) and evaluates the
operation in float64 (``r64``).  The same function evaluated in float32 (``r32``, plain torch on the CPU, never the kernel) is the
yardstick ``e32 = max|r32 - r64| / max|r64|``: what a sequential fp32 evaluation of the operation loses on these inputs.

  fp32 outputs:    max|got - r64| / max|r64| <= MARGIN * max(e32, 2^-23)
  16-bit outputs:  |got - r64| <= ulp16(r64) + MARGIN * max(e32, 2^-23) * max|r64|      (elementwise)
  elementwise kernels with 16-bit output (activations, add, casts, dropout): |got - r64| <= ulp16(r64)

MARGIN = 8 is not measured: it covers what the GPU legitimately does differently from a sequential fp32 evaluation (64-lane
butterfly, 4-wave LDS sum, up to 512 partials, FMA contraction, rsqrt / exp / rcp at 1-2 ulp), none of which grows faster with the
size than the CPU's own sum.  A yardstick above E32_MAX = 2^-18 would make the bound vacuous, so every case must stay below it.
"""
import math

import numpy as np
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT16 = (BF16, F16)
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}

EPS32 = 2.0 ** -23
MARGIN = 8.0
E32_MAX = 2.0 ** -18
LN_EPS = 1e-5

_MANT = {BF16: 7, F16: 10, F32: 23}
_EMIN = {BF16: -126, F16: -14, F32: -126}


# ---------------------------------------------------------------------------------------------- error measures
def widen(t):
    """The values a kernel sees, as float64 on the CPU."""
    return t.detach().to("cpu").to(torch.float64)


def ulp(r64, dtype):
    """Spacing of `dtype` at the magnitude of each element of the float64 tensor r64, floored at the subnormal spacing."""
    a = r64.detach().abs().to(torch.float64)
    _, e = torch.frexp(a)                           # a = m 2^e, m in [0.5, 1): the binade of a starts at 2^(e-1)
    e = torch.where(a > 0, e - 1, torch.full_like(e, _EMIN[dtype])).clamp(min=_EMIN[dtype], max=1023)
    return torch.ldexp(torch.ones_like(a), e - _MANT[dtype])


def ulp16(r64, dtype):
    assert dtype in DT16
    return ulp(r64, dtype)


def smallest_normal(dtype):
    return 2.0 ** _EMIN[dtype]


def max_rel(a, r64):
    """max|a - r64| / max|r64|  (the absolute maximum where the reference is identically zero)."""
    r64 = r64.to(torch.float64)
    d = (a.detach().to("cpu").to(torch.float64) - r64).abs().max().item()
    s = r64.abs().max().item()
    return d / s if s > 0 else d


def e32_of(r32, r64):
    return max_rel(r32, r64)


def bound32(e32):
    return MARGIN * max(e32, EPS32)


def excess16(got, r64, e32, dtype, elementwise=False):
    """max over the elements of |got - r64| / allowed: <= 1 passes.  `elementwise` drops the fp32 term."""
    r64 = r64.to(torch.float64)
    allow = ulp16(r64, dtype)
    if not elementwise:
        allow = allow + bound32(e32) * r64.abs().max().item()
    return ((got.detach().to("cpu").to(torch.float64) - r64).abs() / allow).max().item()


def ulps_off(got, r64, dtype):
    """max|got - r64| in units of the spacing of `dtype` at r64."""
    r64 = r64.to(torch.float64)
    return ((got.detach().to("cpu").to(torch.float64) - r64).abs() / ulp(r64, dtype)).max().item()


# ---------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, dtype=F32, scale=1.0, shift=0.0):
    """Deterministic normal values, rounded to their storage dtype."""
    return (torch.randn(shape, generator=_gen(seed)) * scale + shift).to(dtype)


def padded(t, ld, fill):
    """t [rows, D] inside a [rows, ld] buffer whose gap columns hold `fill`; returns (buffer, view of the first D columns)."""
    rows, D = t.shape
    buf = torch.full((rows, ld), fill, dtype=t.dtype)
    buf[:, :D] = t
    return buf, buf[:, :D]


# ---------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd_ref(x, gamma, beta, eps=LN_EPS, dtype=torch.float64):
    """y, mean, rstd of LayerNorm over the last axis (biased variance), evaluated in `dtype`."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1) + eps)
    return {"y": xc * rstd[:, None] * gamma + beta, "mean": mean, "rstd": rstd}


def ln_stats_f32(x, eps=LN_EPS):
    """mean / rstd of the rows of x, computed in float64 and rounded to f32: statistics that do not depend on a forward kernel."""
    r = ln_fwd_ref(x, torch.ones(x.shape[-1]), torch.zeros(x.shape[-1]), eps)
    return r["mean"].to(F32), r["rstd"].to(F32)


def ln_bwd_autograd(dy, x, gamma, add=None, dy2=None, eps=LN_EPS, dtype=torch.float64):
    """dx (+ add), dgamma, dbeta of LayerNorm for the incoming gradient dy (+ dy2): torch.autograd through layer_norm in `dtype`."""
    xr = x.to(dtype).clone().requires_grad_(True)
    g = gamma.to(dtype).clone().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (xr.shape[-1],), g, b, eps)
    dyt = dy.to(dtype) if dy2 is None else dy.to(dtype) + dy2.to(dtype)
    y.backward(dyt)
    dx = xr.grad if add is None else xr.grad + add.to(dtype)
    return {"dx": dx.detach(), "dgamma": g.grad.detach(), "dbeta": b.grad.detach()}


def ln_bwd_formula(dy, x, gamma, add=None, dy2=None, eps=LN_EPS, dtype=torch.float64):
    """The same three gradients from the closed form the kernels implement:
    dx = rstd (g w - mean(g w) - xhat mean(g w xhat)),  dgamma = sum_rows g xhat,  dbeta = sum_rows g."""
    x, w = x.to(dtype), gamma.to(dtype)
    g = dy.to(dtype) if dy2 is None else dy.to(dtype) + dy2.to(dtype)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xh = xc * rstd
    gw = g * w
    dx = rstd * (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True))
    if add is not None:
        dx = dx + add.to(dtype)
    return {"dx": dx, "dgamma": (g * xh).sum(0), "dbeta": g.sum(0)}


# LayerNorm backward cases.  api: "bwd" (vmc_layernorm_bwd), "bwd2" (vmc_layernorm_bwd2).  dy / x / dx: "32" or "16".
# pad: ldx = D + pad.  The reduce kernel sees P = ceil(rows / 4) partial rows (at most 512).
def _lnb(rows, D, dt16, api="bwd", dy="16", x="32", dx="32", pad=0, add=False, dy2=False, shift=0.0, stats="f64"):
    return dict(rows=rows, D=D, dt16=dt16, api=api, dy=dy, x=x, dx=dx, pad=pad, add=add, dy2=dy2, shift=shift, stats=stats)


def ln_bwd_case_id(c):
    s = f"{c['api']}-{c['rows']}x{c['D']}-{DT_NAME[c['dt16']]}-dy{c['dy']}-x{c['x']}-dx{c['dx']}"
    for k in ("add", "dy2"):
        if c[k]:
            s += "-" + k
    if c["pad"]:
        s += f"-ldx+{c['pad']}"
    if c["shift"]:
        s += "-shift"
    if c["stats"] != "f64":
        s += "-fwdstats"
    return s


LN_BWD_D = (4, 260, 512, 516, 768, 772, 1024, 1028, 2048)       # every NCH at its upper edge and just past the previous one
LN_BWD_P_ROWS = (3, 7, 62, 65, 195, 256, 257)                   # D = 260: P = 1, 2, 16, 17, 49, 64, 65
LN_BWD_CASES = []
for _i, _D in enumerate(LN_BWD_D):
    for _dt in DT16:      # 9 rows: three blocks, the last with one row; both entry points over the sweep
        LN_BWD_CASES.append(_lnb(9, _D, _dt, api="bwd2" if (_i + (_dt is F16)) % 2 else "bwd", dy2=bool((_i + (_dt is F16)) % 2)))
for _i, _r in enumerate(LN_BWD_P_ROWS):
    for _dt in DT16:
        LN_BWD_CASES.append(_lnb(_r, 260, _dt, api="bwd2", dy2=True, dx="16" if _i % 2 else "32", add=bool(_i % 2)))
LN_BWD_CASES += [
    _lnb(1, 4, BF16), _lnb(1, 4, F16), _lnb(1, 1028, BF16, dx="16"), _lnb(3, 2048, F16, api="bwd2", dy2=True),
    # P = 512: every wave takes 2 (2053 rows: 5 waves take 3) or 3 (4100 rows: 4 waves take 3) rows -- the prefetch runs,
    # and some waves own no further row
    _lnb(2053, 772, BF16, api="bwd2", dy2=True, add=True), _lnb(2053, 772, F16, dx="16", add=True),
    _lnb(4100, 260, F16, api="bwd2", dy2=True), _lnb(4100, 1028, BF16, x="16", pad=8),
    _lnb(2053, 2048, BF16, add=True), _lnb(2049, 2048, F16, api="bwd2", dy2=True, dx="16"),
    # statistics taken from vmc_layernorm_fwd(save_stats) instead of float64: pins the pair
    _lnb(65, 516, BF16, stats="fwd"), _lnb(65, 772, F16, x="16", pad=8, stats="fwd"),
    _lnb(65, 516, BF16, shift=30.0), _lnb(65, 516, F16, api="bwd2", dy2=True, shift=30.0),
]
# dtype mixes at one mid-size shape: each of dy / x (ldx = D + 8) / dx in both widths, add and dy2 present and absent
for _dt in DT16:
    LN_BWD_CASES += [
        _lnb(65, 516, _dt, dy="32", x="32", dx="32", pad=8),
        _lnb(65, 516, _dt, dy="32", x="16", dx="16", pad=8, add=True),
        _lnb(65, 516, _dt, dy="16", x="16", dx="32", pad=8, add=True, api="bwd2", dy2=True),
        _lnb(65, 516, _dt, dy="32", x="32", dx="16", pad=8, api="bwd2", dy2=True),
        _lnb(65, 516, _dt, dy="16", x="32", dx="16", pad=8, api="bwd2", dy2=True, add=True),
        _lnb(65, 516, _dt, dy="16", x="16", dx="16", pad=8),
    ]


def ln_bwd_inputs(c, seed=0):
    """CPU tensors of one LayerNorm backward case, each in its storage dtype: x = 2 randn (+ shift), dy = randn, gamma = 1 + randn / 2."""
    rows, D, dt = c["rows"], c["D"], c["dt16"]
    s = 1000 * seed + rows * 7 + D
    t = {"x": randn((rows, D), s + 1, F32 if c["x"] == "32" else dt, 2.0, c["shift"]),
         "dy": randn((rows, D), s + 2, F32 if c["dy"] == "32" else dt),
         "gamma": randn((D,), s + 3, F32, 0.5, 1.0),
         "dy2": randn((rows, D), s + 4, dt) if c["dy2"] else None,
         "add": randn((rows, D), s + 5, F32 if c["dx"] == "32" else dt) if c["add"] else None}
    return t


def ln_bwd_refs(t, dtype):
    return ln_bwd_autograd(t["dy"], t["x"], t["gamma"], add=t["add"], dy2=t["dy2"], dtype=dtype)


# LayerNorm forward (vmc_layernorm_fwd): (rows, D, dt16, x width, outputs)
LN_FWD_D = (4, 260, 516, 772, 1028, 2048, 2052, 4096)
LN_FWD_CASES = []
for _i, _D in enumerate(LN_FWD_D):
    for _dt in DT16:
        LN_FWD_CASES.append(dict(rows=5, D=_D, dt16=_dt, x="32", out="both"))
        LN_FWD_CASES.append(dict(rows=5, D=_D, dt16=_dt, x="16", out="y16" if (_i + (_dt is F16)) % 2 else "y32"))
LN_FWD_CASES += [dict(rows=16387, D=260, dt16=BF16, x="16", out="both"), dict(rows=16387, D=260, dt16=F16, x="32", out="both")]


def ln_fwd_case_id(c):
    return f"{c['rows']}x{c['D']}-{DT_NAME[c['dt16']]}-x{c['x']}-{c['out']}"


def ln_fwd_inputs(c):
    """x = 1 + 2 randn: the row means are an output, and a mean near zero would have no relative accuracy in any arithmetic."""
    rows, D = c["rows"], c["D"]
    s = rows * 11 + D
    return {"x": randn((rows, D), s + 1, F32 if c["x"] == "32" else c["dt16"], 2.0, 1.0),
            "gamma": randn((D,), s + 2, F32, 0.5, 1.0), "beta": randn((D,), s + 3, F32, 0.5)}


# fused residual add + LayerNorm (vmc_add_layernorm_fwd / vmc_add2_layernorm_fwd)
ADD_LN_SHAPES = [(r, D) for D in (256, 512, 768, 1024, 1280, 1536, 1792, 2048) for r in (1, 5)] + [(8195, 256)]


def add_ln_inputs(rows, D, dt16, two):
    s = rows * 13 + D + (5 if two else 0)
    return {"x": randn((rows, D), s + 1, F32, 2.0, 1.0), "b": randn((rows, D), s + 2, dt16),
            "b0": randn((rows, D), s + 3, dt16) if two else None,
            "gamma": randn((D,), s + 4, F32, 0.5, 1.0), "beta": randn((D,), s + 5, F32, 0.5)}


def add_ln_sum_f32(t):
    """The fp32 residual stream the kernel leaves: (x + b0) + b, single IEEE adds in that order."""
    s = t["x"].clone()
    if t["b0"] is not None:
        s = s + t["b0"].to(F32)
    return s + t["b"].to(F32)


# post-norm tail with dropout (vmc_postnorm_dropout_fwd) and its backward (vmc_postnorm_bwd)
POSTNORM_SHAPES = [(r, D) for D in (256, 512, 768, 1024, 1280, 1536, 1792, 2048) for r in (1, 7)] + [(8195, 256)]
POSTNORM_DROPS = (((0.0, 0), (0.0, 0)), ((0.3, 1234567), (0.0, 0)), ((0.1, 987654321), (0.2, 55555)))
# (rows, D, dy in f32, dy2 present): both widths of dy, with and without the second gradient
POSTNORM_BWD_CASES = [(7, 256, True, True), (65, 768, False, False), (2053, 512, False, True), (9, 2048, True, False)]
POSTNORM_MASK_CASE = (67, 768, False, False)        # the case that ties the backward's mask to the canonical one


def drops_id(d):
    return "p" + "-".join(str(p) for (p, _) in d)


def postnorm_inputs(rows, D, dt16):
    """x and the branch share their sign (positive in even rows, negative in odd ones): x + branch F never cancels, so a bound in
    ulps of the sum is meaningful, and the row means -- an output -- stay away from zero."""
    s = rows * 17 + D
    sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
    return {"x": ((randn((rows, D), s + 1, F32, 2.0).abs() + 0.5) * sign).to(F32), "b": (randn((rows, D), s + 2).abs() * sign).to(dt16),
            "gamma": randn((D,), s + 3, F32, 0.5, 1.0), "beta": randn((D,), s + 4, F32, 0.5)}


def postnorm_bwd_inputs(rows, D, dt16, dy_f32, dy2):
    s = rows * 19 + D
    return {"sum": randn((rows, D), s + 1, F32, 2.0), "dy": randn((rows, D), s + 2, F32 if dy_f32 else dt16),
            "dy2": randn((rows, D), s + 3, dt16) if dy2 else None, "gamma": randn((D,), s + 4, F32, 0.5, 1.0)}


# ---------------------------------------------------------------------------------------------- activations
ACTS = (0, 1, 2, 3)                      # none, QuickGELU, GELU (erf), ReLU  (include/vmc.h)
ACT_N = (1, 7, 8, 1003, 8 * 4096 * 256 + 13)
ACT_PLANTED = (0.0, -0.0, 1e-3, -1e-3, 8.0, -8.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4)


def act_ref(x, act, dtype=torch.float64):
    x = x.to(dtype)
    if act == 1:
        return x * torch.sigmoid(1.702 * x)
    if act == 2:
        return 0.5 * x * torch.erfc(-x * math.sqrt(0.5))       # = x Phi(x), without the cancellation of 1 + erf in the left tail
    if act == 3:
        return torch.relu(x)
    return x.clone()


def act_grad_ref(x, act, dtype=torch.float64):
    """Closed-form derivative."""
    x = x.to(dtype)
    if act == 1:
        s = torch.sigmoid(1.702 * x)
        return s * (1.0 + 1.702 * x * (1.0 - s))
    if act == 2:
        return 0.5 * torch.erfc(-x * math.sqrt(0.5)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == 3:
        return (x > 0).to(dtype)
    return torch.ones_like(x)


def act_inputs(n, dtype, seed=0):
    """x = 3 randn with the planted values at the front (vector body) and, again, at the end (scalar tail when n % 8 != 0)."""
    x = randn((n,), 31 + n % 1000 + seed, F32, 3.0)
    p = torch.tensor(ACT_PLANTED)
    if n >= 8 + 2 * len(p):
        x[:len(p)] = p
        x[-len(p):] = p.flip(0)      # reversed: the last n % 8 elements (the tail) hold 0, -0, 1e-3, ...
    elif n >= 2:
        x[:min(n, len(p))] = p[:min(n, len(p))]
    return x.to(dtype)


# ---------------------------------------------------------------------------------------------- casts
CAST_N = (1, 3, 4, 1001, 4 * 4096 * 256 + 3)


def cast_specials_f32(dtype):
    """f32 values whose rounding to `dtype` is delicate: exact ties in both directions, the largest finite value, overflow,
    infinities, NaN, 16-bit subnormals, f32 subnormals."""
    m = _MANT[dtype]
    h = 2.0 ** -(m + 1)                                    # half a 16-bit ulp at 1.0
    big = float(torch.finfo(dtype).max)
    sub = 2.0 ** (_EMIN[dtype] - m)                        # smallest 16-bit subnormal
    vals = [1.0 + h, 1.0 + 3 * h, -(1.0 + h), -(1.0 + 3 * h),             # ties: to even goes down, then up
            1.0 + h + 2.0 ** -23, 1.0 + h - 2.0 ** -24,                    # just past / just short of a tie
            big, -big, 70000.0, -70000.0, float("inf"), float("-inf"), float("nan"),
            sub, 3 * sub, sub / 2, 1.5 * sub, 2.5 * sub, -sub / 2, smallest_normal(dtype) - sub, smallest_normal(dtype),
            0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149]
    if dtype is F16:
        vals += [65504.0 + 15.9, 65504.0 + 16.0, 65520.0 - 1e-2]           # below / at the tie between the largest finite value and inf
    else:
        vals += [3.3961775292304e38, 3.4e38]                                 # bf16: past the tie between max and inf (still finite f32)
    return torch.tensor(vals, dtype=F32)


def cast_inputs_f32(n, dtype):
    x = randn((n,), 41 + n % 1000, F32, 3.0)
    p = cast_specials_f32(dtype)
    if n >= 8 + 2 * len(p):
        x[:len(p)] = p
        x[-len(p):] = p.flip(0)
    else:
        x[:min(n, len(p))] = p[-min(n, len(p)):]
    return x


def cast_inputs_16(n, dtype):
    """Every kind of 16-bit pattern: random bits (NaNs, infinities, subnormals included) with the special values planted."""
    bits = torch.randint(0, 65536, (n,), generator=_gen(43 + n % 1000), dtype=torch.int32)
    special = torch.tensor([0x0000, 0x8000, 0x0001, 0x8001, 0x7C00, 0xFC00, 0x7F80, 0xFF80, 0x7E00, 0x7FC0, 0x7BFF, 0x7F7F, 0x03FF, 0x007F],
                           dtype=torch.int32)
    if n >= 8 + 2 * len(special):
        bits[:len(special)] = special
        bits[-len(special):] = special.flip(0)
    else:
        bits[:min(n, len(special))] = special[:min(n, len(special))]
    return torch.from_numpy(bits.numpy().astype(np.uint16).view(np.int16).copy()).view(dtype)


def same_bits(a, b):
    """Bitwise equality of two tensors of one dtype, except that any NaN matches any NaN."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
    iv = torch.int32 if a.dtype is F32 else torch.int16
    return bool((((a.view(iv) == b.view(iv)) | (torch.isnan(a) & torch.isnan(b)))).all())


# ---------------------------------------------------------------------------------------------- dropout
DROP_N = 1 << 20
# vmc_cast_dropout2 launches at most 8192 x 256 threads of 8 elements: 300 threads take a second pass of the body, 5 elements are left to the tail
CAST_DROPOUT2_N = 8 * 8192 * 256 + 8 * 300 + 5
DROP_P = (0.1, 0.3)


def drop_scale_f64(p):
    """1 / (1 - p) for the f32 value of p the kernel receives."""
    return 1.0 / (1.0 - float(np.float32(p)))


def drop_share_tolerance(p, n):
    """5 standard deviations of the dropped share of n independent draws."""
    return 5.0 * math.sqrt(p * (1.0 - p) / n)
