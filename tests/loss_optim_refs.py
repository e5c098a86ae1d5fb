"""Plain references, inputs and case lists for the kernels that finish a training step: the three losses, the Adam family with
vmc_train_tick, vmc_sumsq, the sinusoidal positional encoding, vmc_colsum, vmc_transpose16 and vmc_cast_weight.  No GPU code: torch
and numpy on the CPU only.  tests/test_loss_optim_refs_host.py checks the references themselves; tests/test_gpu_loss_optim_kernels.py
compares the HIP kernels with them.

The rule is the one of tests/train_kernel_refs.py: every reference takes the values the kernel sees and evaluates in float64
(``r64``); the same function in float32 on the CPU is the yardstick ``e32``; fp32 outputs must satisfy
``max|got - r64| / max|r64| <= MARGIN max(e32, 2^-23)`` and every case has ``e32 <= 2^-18``.  vmc_sumsq adds its workgroup partials with
fp32 atomics and gets the term sumsq_allow derives for that on top.  Four outputs would hide an error under the plain rule and get an
element-wise bound, derived here and not tuned:

  BCE gradient, targets in {0, 1}:  |got - r64| <= 8 2^-23 |r64| + 2^-126 / n
      Each element is one product of a sigmoid and a weight, a handful of roundings and one exp: relative to the element itself.
      A term below the smallest normal float may be flushed before it is divided by n, which is the absolute floor.
  cross-entropy loss of one row:    |got - r64| <= 8 2^-23 (|r64| + log C)
      The row's loss is ysum log(se) - sum_c y_c (x_c - m) with se in [1, C]: roundings relative to log(se) <= log C and to the loss,
      never to the largest logit m.
  Adam update d = p_new - p_old:    |d - d64| <= ulp32(p_new) + 8 max(e32_d, 2^-23) max|d64|
      p_new is rounded once to fp32 (the first term); everything else is the plain rule applied to the update, so that a relative error
      of the update is visible although it is 1e-3 of the parameter.
  positional encoding:              |got - r64| <= 4 a + 2^-23 |r64| + 2^-22,   a = 2^-23 (1 + |d_even c|) t div
      a is what an fp32 angle t div carries from the roundings of c = -ln(1e4) / D, of d_even c, of expf and of t div; sin and cos have
      slope <= 1, the add to x rounds once at the size of the result, and 2^-22 covers sinf / cosf themselves (|pe| <= 1).
"""
import functools
import math

import numpy as np
import torch

from oracle import student as oracle_student
from train_kernel_refs import (BF16, DT_NAME, E32_MAX, EPS32, F16, F32, MARGIN, bound32, cast_inputs_16, e32_of, max_rel, randn,  # noqa: F401
                               same_bits, ulp, widen)

F64 = torch.float64
TINY32 = 2.0 ** -126
M64 = (1 << 64) - 1


def f32v(x):
    """The float32 value of a Python number, as a Python float (what a kernel receives for a float argument)."""
    return float(np.float32(x))


def rel_scalar(got, r64, floor=0.0):
    """|got - r64| / max(|r64|, floor) of two scalars."""
    got, r64 = float(got), float(r64)
    d = abs(got - r64)
    s = max(abs(r64), floor)
    return d / s if s > 0 else d


# ---------------------------------------------------------------------------------------------- distillation loss
DISTILL_ROWS = (1, 3, 4, 5, 30)                 # four rows per workgroup
DISTILL_E = (5, 64, 65, 768, 1000)
DISTILL_LAYOUTS = ("dense", "slice", "per-row")
DISTILL_CASES = [(mode, rows, E) for mode in ("cosine", "mse") for rows in DISTILL_ROWS for E in DISTILL_E]
DISTILL_EPS = 1e-5


def distill_ref(s, t, mode, dtype=F64):
    """loss and d loss / d student of oracle.student.distillation_loss, autograd in `dtype`."""
    sr = s.to(dtype).clone().requires_grad_(True)
    loss = oracle_student.distillation_loss(sr, t.to(dtype), mode)
    loss.backward()
    return {"loss": loss.detach(), "ds": sr.grad.detach()}


def distill_inputs(rows, E, seed=0):
    s = randn((rows, E), 7000 + 31 * rows + E + seed)
    t = randn((rows, E), 8000 + 31 * rows + E + seed) * 0.5 + 0.25 * s          # cosine around 0.4: clear of both clamp edges
    return s, t.to(F32)


def distill_clip_len(rows):
    """T of the `[:, :-1]` layout: the largest divisor of rows that is at most 5."""
    return max(d for d in range(1, 6) if rows % d == 0)


def distill_teacher_buffer(t, layout):
    """(buffer, rows_per_clip, teacher_clip_stride in elements) holding the teacher rows `t` in one of the three layouts.  Rows and gaps the
    kernel must not read hold NaN."""
    rows, E = t.shape
    if layout == "dense":
        return t.clone(), rows, rows * E
    if layout == "slice":                       # teacher[:, :-1] of a [clips, T + 1, E] tensor
        T = distill_clip_len(rows)
        buf = torch.full((rows // T, T + 1, E), float("nan"))
        buf[:, :T] = t.view(rows // T, T, E)
        return buf, T, (T + 1) * E
    buf = torch.full((rows, 2 * E + 3), float("nan"))       # one row per clip, clips 2 E + 3 elements apart
    buf[:, :E] = t
    return buf, 1, 2 * E + 3


def distill_degenerate_inputs(E=65):
    """Two row sets for the cosine mode.  "unit": zero teacher row, s = t, s = -t among ordinary rows (gradients of size 1 / rows; the
    three planted rows have gradient exactly 0).  "tiny": zero student row and |s| = 1e-6 < eps among ordinary rows: the norm clamp holds
    the student norm at eps, the gradient is t / (eps |t| rows) and nothing flows through the norm."""
    s, t = distill_inputs(6, E, seed=5)
    unit_s, unit_t = s.clone(), t.clone()
    unit_t[1] = 0.0
    unit_s[2] = unit_t[2]
    unit_s[3] = -unit_t[3]
    tiny_s, tiny_t = s.clone(), t.clone()
    tiny_s[1] = 0.0
    d = tiny_t[4] + 0.5 * tiny_s[4]                 # direction with a cosine near 0.8 to the teacher row
    tiny_s[4] = (d.double() / d.double().norm() * 1e-6).to(F32)
    return {"unit": (unit_s, unit_t, (1, 2, 3)), "tiny": (tiny_s, tiny_t, ())}     # (student, teacher, rows whose gradient is exactly 0)


# ---------------------------------------------------------------------------------------------- BCE with logits
BCE_N = (1, 255, 257, 1120, 8192, 8193, 16384, 16385, 71680)
BCE_PW = (-1.0, 0.0, 9.0)                       # negative: no pos_weight
BCE_TAILS = (9.0, 13.0, 17.0, 30.0, 100.0, 1e4)
BCE_CASES = [(n, pw, soft) for n in BCE_N for pw in BCE_PW for soft in (False, True)]
BCE_SINGLE_WG_MAX = 8192
BCE_BLOCKS = 64


def bce_planted():
    """(logits, hard targets) of the planted tails: +-9 ... +-1e4, each with target 0 and target 1."""
    xs, ys = [], []
    for a in BCE_TAILS:
        for sgn in (1.0, -1.0):
            for y in (0.0, 1.0):
                xs.append(sgn * a)
                ys.append(y)
    return torch.tensor(xs), torch.tensor(ys)


@functools.lru_cache(maxsize=None)
def bce_inputs(n, soft):
    """logits = 3 randn, targets multi-hot (about one in five) or soft (0.1 / 0.9); the planted tails at the front and, reversed, at the end."""
    x = randn((n,), 9100 + n % 977, F32, 3.0)
    hot = torch.rand((n,), generator=torch.Generator().manual_seed(9200 + n % 977)) < 0.2
    px, py = bce_planted()
    k = len(px)
    y = hot.to(F32)
    if n >= 2 * k + 8:
        x[:k], x[-k:] = px, px.flip(0)
        y[:k], y[-k:] = py, py.flip(0)
    if n == 1:
        x = x.abs()       # a lone negative logit with target 0 is x + log1p(e^x) - x in the loss formula itself: fp32 yardstick 1.5e-5
    if soft:
        y = y * 0.8 + 0.1
    return x, y.to(F32)


def bce_w(y, pw):
    return torch.ones_like(y) if pw < 0 else f32v(pw) * y + 1.0


def bce_grad_stable(x, y, pw, dtype=F64):
    """d mean-loss / d x = [(1 - y) sigma(x) - w y sigma(-x)] / n: no cancellation in either confident tail."""
    x, y = x.to(dtype), y.to(dtype)
    w = bce_w(y, pw)
    return ((1.0 - y) * torch.sigmoid(x) - w * y * torch.sigmoid(-x)) / x.numel()


def bce_grad_cancelling(x, y, pw, dtype=F32):
    """The formula the kernel used before: (1 - y) - lw (1 - sigma(x)).  Only for the CPU proof that the bound rejects it."""
    x, y = x.to(dtype), y.to(dtype)
    lw = 1.0 + (bce_w(y, pw) - 1.0) * y
    sig = 1.0 / (1.0 + torch.exp(-x))
    return ((1.0 - y) - lw * (1.0 - sig)) / x.numel()


def bce_loss(x, y, pw, dtype=F64):
    """oracle.student.classification_loss with every term in `dtype` (the oracle rounds its weights to float32)."""
    x, y = x.to(dtype), y.to(dtype)
    lw = 1.0 + (bce_w(y, pw) - 1.0) * y
    return ((1.0 - y) * x + lw * (torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0))).mean()


def bce_ref(x, y, pw, dtype=F64):
    """mean loss and its gradient (the stable closed form), in `dtype`."""
    return {"loss": bce_loss(x, y, pw, dtype), "dx": bce_grad_stable(x, y, pw, dtype)}


def bce_grad_allow(r64, n):
    """Element-wise allowance of the gradient for targets in {0, 1}."""
    return MARGIN * EPS32 * r64.abs() + TINY32 / n


# ---------------------------------------------------------------------------------------------- cross entropy
CE_ROWS = (1, 3, 4, 5, 37)
CE_C = (1, 2, 63, 64, 65, 140, 1000)
CE_KINDS = ("index", "onehot", "soft")
CE_LOGITS = ("spike", "equal")
CE_CASES = [(rows, C, kind) for rows in CE_ROWS for C in CE_C for kind in CE_KINDS]
# one confident row: (x_t, gap to the runner-up); the other classes sit 80 below the target
CE_CONFIDENT = [(xt, gap, C, kind) for xt in (80.0, 8.0) for gap in (11.5, 5.0) for C in (2, 3, 140) for kind in ("index", "onehot")]


@functools.lru_cache(maxsize=None)
def ce_inputs(rows, C, kind, logits="spike"):
    """(logits, index targets or None, probability targets or None).  "spike": 5 randn with one logit of the first row at 80.  Soft rows
    are a softmax scaled by 1, 0.5, 2, ... so that most rows do not sum to 1 (the kernel's ysum factor)."""
    s = 9300 + 41 * rows + C
    x = randn((rows, C), s, F32, 5.0)
    if logits == "spike":
        x[0, C // 2] = 80.0
    else:
        x = torch.full((rows, C), 2.5)
    idx = torch.randint(0, C, (rows,), generator=torch.Generator().manual_seed(s + 1), dtype=torch.int64)
    if kind == "index":
        return x, idx, None
    if kind == "onehot":
        return x, None, torch.nn.functional.one_hot(idx, C).to(F32)
    y = torch.softmax(randn((rows, C), s + 2), 1) * torch.tensor([1.0, 0.5, 2.0])[torch.arange(rows) % 3][:, None]
    return x, None, y.to(F32)


def ce_confident_inputs(xt, gap, C, kind):
    x = torch.full((1, C), xt - 80.0)
    x[0, 0], x[0, 1] = xt, xt - gap
    idx = torch.zeros(1, dtype=torch.int64)
    return (x, idx, None) if kind == "index" else (x, None, torch.nn.functional.one_hot(idx, C).to(F32))


def ce_ref(x, tidx, tprob, dtype=F64):
    """Row losses, their mean and d mean / d x of nn.CrossEntropyLoss in `dtype`, through log_softmax (torch's own route):
    l_r = -sum_c y_c log_softmax(x)_c,  grad = (softmax(x) sum(y) - y) / rows."""
    x = x.to(dtype)
    y = torch.nn.functional.one_hot(tidx, x.shape[1]).to(dtype) if tprob is None else tprob.to(dtype)
    row = -(y * torch.log_softmax(x, 1)).sum(1)
    dx = (torch.softmax(x, 1) * y.sum(1, keepdim=True) - y) / x.shape[0]
    return {"rows": row, "loss": row.mean(), "dx": dx}


def ce_row_stable32(x, y):
    """fp32 evaluation of ysum log(se) - sum_c y_c (x_c - m) for one row."""
    x, y = x.to(F32), y.to(F32)
    m = x.max()
    return y.sum() * torch.log(torch.exp(x - m).sum()) - (y * (x - m)).sum()


def ce_row_cancelling32(x, y):
    """fp32 evaluation of the formula the kernel used before: ysum (m + log se) - sum_c y_c x_c."""
    x, y = x.to(F32), y.to(F32)
    m = x.max()
    return y.sum() * (m + torch.log(torch.exp(x - m).sum())) - (y * x).sum()


def ce_row_allow(r64, C):
    return MARGIN * EPS32 * (abs(float(r64)) + math.log(C))


# ---------------------------------------------------------------------------------------------- Adam
ADAM_MODES = ((1, 0.1), (0, 0.1), (0, 0.0), (1, 0.0))        # (decoupled, weight decay)
ADAM_GSCALE = (1.0, 0.25)
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_N = (1, 3, 4, 5, 1023, 4099)
ADAM_BG_N = (2048, 2049, 2051, 3076, 6151)      # max_workgroups = 1: a trip is 2 x 256 float4
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 3e-3, 0.9, 0.999, 1e-8
ADAM_PLANTED = 4


def adam_host_scalars(step, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2):
    """(step_size, inv_sqrt_bc2) as vmc_adam_step forms them: from the float arguments, in double, rounded to float."""
    bc1 = 1.0 - f32v(b1) ** step
    bc2 = 1.0 - f32v(b2) ** step
    return f32v(f32v(lr) / bc1), f32v(1.0 / math.sqrt(bc2))


@functools.lru_cache(maxsize=None)
def adam_inputs(n):
    """p, g, m, v with the planted elements: g = 0 with m = v = 0; a subnormal v under a tiny gradient; g = -1e15; p = 0.  For n < 12 they
    follow one ordinary element, otherwise they open the tensor and, reversed, close it (the scalar tail when n % 4 != 0)."""
    p, g = randn((n,), 9500 + n), randn((n,), 9501 + n, scale=0.3)
    m, v = randn((n,), 9502 + n, scale=0.1), (randn((n,), 9503 + n, scale=0.2) ** 2).to(F32)

    def plant(i, kind):
        if kind == 0:
            g[i] = m[i] = v[i] = 0.0
        elif kind == 1:
            g[i], m[i], v[i] = 1e-21, 1e-21, 1e-40
        elif kind == 2:
            g[i] = -1e15
        else:
            p[i] = 0.0
    if n >= 12:
        for k in range(ADAM_PLANTED):
            plant(k, k)
            plant(n - 1 - k, k)
    else:
        for k in range(min(ADAM_PLANTED, n - 1)):
            plant(1 + k, k)
    return p, g, m, v


def adam_zero_grad_index(n):
    """Index of the planted element with g = m = v = 0, or None."""
    return 0 if n >= 12 else (1 if n >= 2 else None)


def adam_ref(p, g, m, v, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, gscale, dtype=F64):
    """One Adam / AdamW element update in `dtype` from the fp32 scalars the kernel gets.  Returns the update d = p_new - p_old (decay term
    plus step, never formed through p), p_new, m and v."""
    c = lambda s: torch.tensor(f32v(s), dtype=dtype)            # noqa: E731
    lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, gscale = (c(s) for s in (lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, gscale))
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    gr = g * gscale
    if decoupled:
        decay = -(lr * wd) * p
    else:
        gr = gr + wd * p
        decay = torch.zeros_like(p)
    m1 = b1 * m + (1.0 - b1) * gr
    v1 = b2 * v + (1.0 - b2) * gr * gr
    d = decay - step_size * m1 / (torch.sqrt(v1) * inv_sqrt_bc2 + eps)
    return {"d": d, "p": p + d, "m": m1, "v": v1}


def adam_excess(p_got, p_old, r64, r32):
    """(max over the elements of |d - d64| / allowed, e32_d) with d = p_got - p_old formed in float64."""
    d = widen(p_got) - widen(p_old)
    e32 = e32_of(r32["d"], r64["d"])
    allow = ulp(widen(p_got), F32) + bound32(e32) * r64["d"].abs().max().item()
    return ((d - r64["d"]).abs() / allow).max().item(), e32


def adam_split_rel(got, r64, big):
    """The plain measure over the ordinary elements and, on their own, over the elements of the 1e15 gradient (which would otherwise set
    max|r64| for everything): the larger of the two."""
    got, r64 = widen(got), r64.to(F64)
    out = max_rel(got[~big], r64[~big]) if bool((~big).any()) else 0.0
    if bool(big.any()):
        out = max(out, ((got[big] - r64[big]).abs() / r64[big].abs()).max().item())
    return out


# ---------------------------------------------------------------------------------------------- vmc_train_tick
TICK_SEEDS = (0, 1, 8, 300)                     # 300: more seeds than threads
TICK_BASE_SEED = 0x1E3779B97F4A7C15


def tick_hyper(lr, t, b1=ADAM_B1, b2=ADAM_B2):
    """hyper[1], hyper[2] after the tick that makes the step count t: the double formulas, not yet rounded."""
    return f32v(lr) / (1.0 - f32v(b1) ** t), 1.0 / math.sqrt(1.0 - f32v(b2) ** t)


def tick_seed(base, t, i):
    """The splitmix of (base seed, step count, call site) in Python integers; bit 63 is always clear."""
    x = (base ^ ((t * 0x9E3779B97F4A7C15 + i * 0xD1B54A32D192ED03) & M64)) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x & ~(1 << 63) & M64


# ---------------------------------------------------------------------------------------------- vmc_sumsq
SUMSQ_N = (1, 255, 257, 262144, 262147)         # 1024 workgroups x 256 threads: the last two reach the grid cap and the second trip
SUMSQ_PRESET = (0.0, 3.5)


SUMSQ_BLOCK, SUMSQ_GRID_CAP = 256, 1024


def sumsq_input(n):
    """randn; the elements past the grid cap (the second grid-stride trip) are 100, so that a lost second trip is a tenth of the result."""
    x = randn((n,), 9600 + n % 1000)
    x[SUMSQ_BLOCK * SUMSQ_GRID_CAP:] = 100.0
    return x


def sumsq_ref(x, preset, dtype=F64):
    x = x.to(dtype)
    return (x * x).sum() + torch.tensor(preset, dtype=dtype)


def sumsq_atomic_adds(n):
    """Workgroups of vmc_sumsq: each adds its partial to `out` with one fp32 atomic, in no fixed order."""
    return min(-(-n // SUMSQ_BLOCK), SUMSQ_GRID_CAP)


def sumsq_allow(e32, n):
    """Relative allowance of vmc_sumsq.  The plain rule covers a workgroup's own partial (64-lane butterfly, 4-wave LDS sum).  The partials
    then reach `out` through P sequential fp32 adds in arbitrary order; every term is >= 0, so the running total never exceeds the result
    and each add rounds by at most 2^-24 of the result: P 2^-24 on top, a worst case that holds for every order (6.1e-5 at the cap of 1024
    workgroups, nothing to speak of for one or two).  A lost workgroup (about 1 / P of the result) or a lost second trip stays far outside."""
    return bound32(e32) + sumsq_atomic_adds(n) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- positional encoding
PE_SHAPES = ((1, 1, 2), (2, 40, 512), (2, 300, 64), (1, 2500, 768))
PE_HOST_SHAPES = ((40, 512), (2500, 512), (2500, 768), (4000, 64))
LN1E4 = math.log(10000.0)


def pe_table64(T, D):
    """pe[t, 2k] = sin(t w_k), pe[t, 2k + 1] = cos(t w_k), w_k = 10000^(-2k / D), in float64."""
    t = torch.arange(T, dtype=F64)[:, None]
    w = torch.exp(torch.arange(0, D, 2, dtype=F64) * (-LN1E4 / D))
    pe = torch.zeros(T, D, dtype=F64)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(t * w), torch.cos(t * w)
    return pe


def pe_table32(T, D, own_frequency=False):
    """The model's own float32 table (TFAM positional encoding as PyTorch builds it).  own_frequency: the mutant in which the odd column
    uses its own index for the frequency."""
    t = torch.arange(T, dtype=F32)[:, None]
    c = -LN1E4 / D
    w = torch.exp(torch.arange(0, D, 2).float() * c)
    pe = torch.zeros(T, D)
    pe[:, 0::2] = torch.sin(t * w)
    pe[:, 1::2] = torch.cos(t * (torch.exp(torch.arange(1, D, 2).float() * c) if own_frequency else w))
    return pe


def pe_allow(T, D, r64):
    """Element-wise allowance for x + pe of shape [..., T, D]."""
    d_even = (torch.arange(D) // 2 * 2).to(F64)
    c = LN1E4 / D
    a = EPS32 * (1.0 + d_even * c)[None, :] * torch.arange(T, dtype=F64)[:, None] * torch.exp(-d_even * c)[None, :]
    return 4.0 * a + EPS32 * r64.abs() + 2.0 ** -22


# ---------------------------------------------------------------------------------------------- column sums, transpose, weight casts
COLSUM_M = (1, 3, 127, 128, 129, 1030, 8197)    # slabs = clamp(M / 128, 1, 64): 1, 1, 1, 1, 1, 8, 64 with a short last slab
COLSUM_N = (4, 140, 252, 260, 768)              # 256 columns per block: 260 and 768 take more than one
COLSUM_CASES = [(M, N) for M in COLSUM_M for N in COLSUM_N]
COLSUM_PAD = 8


def colsum_slabs(M):
    return min(max(M // 128, 1), 64)


@functools.lru_cache(maxsize=4)
def colsum_input(M, N):
    return randn((M, N), 9700 + M + N, F32, 1.0, 0.25)


def colsum_ref(x, dtype=F64):
    return x.to(dtype).sum(0)


T16_SHAPES = ((1, 1), (1, 77), (203, 1), (64, 64), (65, 63), (33, 130))


def kpad(k):
    return (k + 63) // 64 * 64
