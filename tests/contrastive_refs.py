"""Plain references, inputs, case lists and bounds for the contrastive (symmetric InfoNCE) distillation mode: the three kernels of
vimo_clip_amd/csrc/contrastive.hip (vmc_contrastive_prep / _softmax / _norm_bwd) and the composed loss of
vimo_clip_amd.losses.distillation_loss(mode="contrastive").  No GPU code: torch and numpy on the CPU only.
tests/test_contrastive_refs_host.py checks the references themselves; tests/test_gpu_contrastive_kernels.py, _loss.py and _step.py
compare the HIP code with them.

The rule is the one of tests/train_kernel_refs.py: a reference takes the values the kernel sees and evaluates in float64 (``r64``); the
same function in float32 on the CPU is the yardstick ``e32``; fp32 outputs satisfy ``max|got - r64| / max|r64| <= MARGIN max(e32, 2^-23)``
("the plain rule"), 16-bit outputs ``|got - r64| <= ulp16(r64) + MARGIN max(e32, 2^-23) max|r64|``, and every case has e32 <= 2^-18.
What the plain rule would hide gets a bound of its own, derived here and not tuned:

  inv_s                    the rows whose norm the clamp holds have inv_s = 1 / eps = 1e5, four orders above the others: the plain rule is
                           applied to the free rows alone, and a clamp row must equal fl(1 / fl(1e-5)) to one rounding (2^-23 relative).
  softmax loss             |got - r64| <= 8 2^-23 (|r64| + log M).  A row's term is log(sum) - (z_ii - m) with sum in [1, M]: roundings
                           relative to log M and to the loss, never to the size of the logits (the cross-entropy bound of
                           tests/loss_optim_refs.py).
  dz16                     |got - round16(r64)| <= ulp16(r64): the fp32 value in front of the store is far closer to r64 than a 16-bit
                           spacing, so it rounds to round16(r64) or to its neighbour.
  composed loss            |got - r64| <= 2 e_z + 8 2^-23 (|r64| + log M),  e_z = MARGIN max(e32_z, 2^-23) max|z64|:
                           e_z is the plain rule for the logits GEMM (fp32 accumulation of products of 16-bit numbers); a log-sum-exp
                           moves by at most the largest change of its arguments, and so does z_ii.
  composed ds              elementwise |got - r64| <= N(a) + MARGIN max(e32_n, 2^-23) max|ds64| with, per element of du,
                             a = F |v16| / (2 M tau)                     a one-ulp16 flip of dz16 entries, see below
                               + (2 e_z + e_p) (P |v16|) / (2 M tau)     the logits' error carried through the softmax
                               + MARGIN max(e32_du, 2^-23) max|du64|     the plain rule for the gradient GEMM.
                           P_ij = p_row_ij + p_col_ij (|dz_ii| on the diagonal): exp(z - lse) changes by the relative amount 2 e_z when
                           every logit moves by e_z, plus e_p = MARGIN 2^-23 max(1, max|lse|) for the fp32 log-sum-exp and exp themselves.
                           F_ij = ulp16(dz64_ij) where dz64_ij lies within P_ij (2 e_z + e_p) of a rounding tie and 0 elsewhere: only
                           there can the kernel's fp32 value round to the other neighbour.  F |v16| <= ulp16(2) sum_j |v16_j|_inf.
                           N carries a through the backward of the normalisation: N(a)_ik = inv_s_i (a_ik + |u_ik| sum_k' |u_ik'| a_ik')
                           on free rows, a_ik / eps on clamp rows.  e32_n is the yardstick of that backward alone.

The operands' own rounding is part of the definition, so the inputs are made *decided* (``decide``): every element of u = s / max(|s|, eps)
and of v lies further than MARGIN 2^-23 |u| from a rounding tie of both 16-bit types, which is more than an fp32 evaluation of u can
be off.  The kernel's u16 and v16 are then the reference's bit for bit, and no bound has to pay for an operand that rounds the other way.
"""
import functools
import math

import torch

from train_kernel_refs import (BF16, DT16, DT_NAME, E32_MAX, EPS32, F16, F32, MARGIN, bound32, e32_of, excess16, max_rel, randn,  # noqa: F401
                               ulp, ulp16, widen)

F64 = torch.float64
EPS = float(torch.tensor(1e-5, dtype=F32))          # the clamp as the kernels hold it
TAU = 0.07
MAX_ROWS = 16384
GUARD = 8
LOSS_FLOOR = 0.05


def pad64(M):
    return (M + 63) // 64 * 64


def round16(x, dtype16):
    """The 16-bit rounding of the definition, back in float64."""
    return x.to(F32).to(dtype16).to(F64)


# ---------------------------------------------------------------------------------------------- prep
PREP_M = (1, 2, 63, 64, 65, 130)
PREP_E = (64, 192, 512, 768)
PREP_LAYOUTS = ("dense", "slice")


def clip_len(rows):
    """T of the `[:, :-1]` layout: the largest divisor of rows that is at most 5."""
    return max(d for d in range(1, 6) if rows % d == 0)


def tie_distance(x, dtype16):
    """Distance of every element of the float64 tensor x to the nearest value that `dtype16` rounds either way."""
    return ulp(x, dtype16) / 2 - (x - x.to(dtype16).to(F64)).abs()


def undecided(s):
    """Elements of the rows s whose normalised value lies within MARGIN 2^-23 of a rounding tie of bf16 or f16."""
    u = prep_rows(s)[0]
    bad = torch.zeros_like(u, dtype=torch.bool)
    for d in DT16:
        bad |= tie_distance(u, d) <= MARGIN * EPS32 * u.abs()
    return bad


def decide(s):
    """s (fp32 [M, E]) with the few elements that `undecided` names moved by 2^-13 of themselves, until none is left."""
    s = s.clone()
    for it in range(40):
        bad = undecided(s)
        if not bad.any():
            return s
        sign = torch.where(torch.arange(s.numel()).view(s.shape) % 2 == 0, 1.0, -1.0)      # alternating: the norm hardly moves
        s = torch.where(bad, s * (1.0 + sign * 2.0 ** -13), s).to(F32)
    raise AssertionError("decide: did not converge")


def prep_rows(x, dtype=F64):
    """(x / max(|x|, eps), 1 / max(|x|, eps)) of the rows of x, evaluated in `dtype`."""
    x = x.to(dtype)
    inv = 1.0 / torch.sqrt((x * x).sum(-1)).clamp(min=EPS)
    return x * inv[:, None], inv


def prep_ref(s, t, dtype=F64):
    u, inv_s = prep_rows(s, dtype)
    v, inv_t = prep_rows(t, dtype)
    return {"u": u, "v": v, "inv_s": inv_s, "inv_t": inv_t}


def clamp_rows(s):
    return torch.sqrt((s.to(F64) ** 2).sum(-1)) <= EPS


@functools.lru_cache(maxsize=None)
def prep_inputs(M, E):
    """(student, teacher) fp32 [M, E], decided.  Planted among ordinary rows where there is room: a row of norm 1e-7 (student row 1),
    a zero student row (row 2) and a zero teacher row (row 3)."""
    t = randn((M, E), 5100 + 7 * M + E)
    s = 0.5 * t + randn((M, E), 5200 + 7 * M + E)
    if M >= 2:
        s[1] = s[1] / s[1].double().norm().float() * 1e-7
    if M >= 63:
        s[2] = 0.0
        t[3] = 0.0
    return decide(s.to(F32)), decide(t.to(F32))


def teacher_buffer(t, layout):
    """(buffer, rows_per_clip, clip stride in elements) holding the teacher rows in one layout; what must not be read holds NaN."""
    rows, E = t.shape
    if layout == "dense":
        return t.clone(), rows, rows * E
    T = clip_len(rows)
    buf = torch.full((rows // T, T + 1, E), float("nan"))
    buf[:, :T] = t.view(rows // T, T, E)
    return buf, T, (T + 1) * E


# ---------------------------------------------------------------------------------------------- softmax
SOFTMAX_M = (1, 2, 5, 64, 65, 130, 257)


def softmax_clip_rows(M):
    return sorted({0, 1, 2, 5, M})


SOFTMAX_CASES = [(M, T, "tau") for M in SOFTMAX_M for T in softmax_clip_rows(M)] + [(130, 5, "80"), (257, 0, "80")]


def valid_mask(M, T):
    """V[i, j]: clip(j) != clip(i) or j == i, clip(i) = i // T; T == 0: every pair."""
    if T == 0:
        return torch.ones(M, M, dtype=torch.bool)
    c = torch.arange(M) // T
    return (c[:, None] != c[None, :]) | torch.eye(M, dtype=torch.bool)


@functools.lru_cache(maxsize=None)
def softmax_inputs(M, kind):
    """z fp32 [M, M].  "tau": cosines around 0 with the diagonal around 0.45, over tau -- what the chain produces.  "80": logits spread
    over [-80, 80]: every third diagonal entry at 80, at least 18 above its row and column (p_ii next to 1, dz_ii a difference of numbers
    near 2), every third at -80."""
    if kind == "tau":
        c = (randn((M, M), 6100 + M, F32, 0.12) + torch.eye(M) * 0.45).clamp(-1.0, 1.0)
        return (c / TAU).to(F32)
    z = randn((M, M), 6200 + M, F32, 30.0).clamp(-80.0, 62.0)
    i = torch.arange(M)
    z[i, i] = torch.where(i % 3 == 0, torch.tensor(80.0), torch.where(i % 3 == 1, torch.tensor(-80.0), z[i, i]))
    return z.to(F32)


def softmax_ref(z, T, dtype=F64):
    """Masked row / column log-sum-exp, loss, top-1 count, dz (unrounded) and P = p_row + p_col of the logits z [M, M]."""
    z = z.to(dtype)
    M = z.shape[0]
    V = valid_mask(M, T)
    zm = z.masked_fill(~V, float("-inf"))
    lse_row, lse_col = torch.logsumexp(zm, 1), torch.logsumexp(zm, 0)
    d = z.diagonal()
    loss = ((lse_row - d) + (lse_col - d)).sum() / (2 * M)
    P = torch.exp(zm - lse_row[:, None]) + torch.exp(zm - lse_col[None, :])
    dz = P - 2.0 * torch.eye(M, dtype=dtype)
    top1 = int((d[:, None] >= zm).all(1).sum())
    return {"lse_row": lse_row, "lse_col": lse_col, "loss": loss, "dz": dz, "P": P, "top1": top1, "valid": V}


def softmax_loss_allow(r64, M):
    return MARGIN * EPS32 * (abs(float(r64)) + math.log(M))


def dz16_excess(got16, dz64, dtype16):
    """max |got - round16(r64)| / ulp16(r64): <= 1 passes."""
    return ((got16.to(F64) - round16(dz64, dtype16)).abs() / ulp16(dz64, dtype16)).max().item()


# ---------------------------------------------------------------------------------------------- norm_bwd
NORM_BWD_CASES = [(1, 64), (5, 192), (65, 512), (130, 768)]


def norm_bwd_ref(du, s, dtype=F64):
    """ds = inv_s (du - u (u . du)) where |s| > eps, du / eps where the clamp holds the norm."""
    du = du.to(dtype)
    u, inv = prep_rows(s, dtype)
    free = ~clamp_rows(s)
    ds = inv[:, None] * (du - u * (u * du).sum(-1, keepdim=True))
    return torch.where(free[:, None], ds, du / EPS)


@functools.lru_cache(maxsize=None)
def norm_bwd_inputs(M, E):
    s, _ = prep_inputs(M, E) if (M in PREP_M and E in PREP_E) else (randn((M, E), 5300 + M + E), None)
    s = s.clone()
    if M >= 5:
        s[1] = s[1] / s[1].double().norm().float() * 1e-7
        s[2] = 0.0
    du = randn((M, E), 5400 + M + E, F32, 1e-3)
    return s, du


# ---------------------------------------------------------------------------------------------- the composed loss
LOSS_SHAPES = ((3, 5, 64), (4, 29, 512), (5, 13, 768), (1, 65, 64))
FLOOR_ONLY_SHAPES = ((2, 1, 64),)              # loss around 1e-4: only in the checks with an absolute floor


@functools.lru_cache(maxsize=None)
def loss_inputs(B, T, E):
    """(student [B, T, E], teacher buffer [B, T + 1, E]): student = 0.5 teacher + noise, both decided; the teacher is the buffer's
    [:, :-1] slice and the last frame of every clip holds NaN."""
    t = decide(randn((B * T, E), 7100 + 31 * B + 7 * T + E))
    s = decide((0.5 * t + randn((B * T, E), 7200 + 31 * B + 7 * T + E)).to(F32))
    buf = torch.full((B, T + 1, E), float("nan"))
    buf[:, :T] = t.view(B, T, E)
    return s.view(B, T, E), buf


def loss_exact(s, t, T, tau=TAU, dtype=F64, dtype16=None, mask=True):
    """The float64 model of the issue on rows s, t [M, E] with clips of T rows: loss, top1 and the hand-derived gradient, with the
    intermediates the bounds need.  dtype16 None: no rounding anywhere (the model that is compared with autograd); bf16 / f16: u, v and
    dz are rounded to it, which is the definition of the mode."""
    M, E = s.shape
    rnd = (lambda x: x) if dtype16 is None else (lambda x: round16(x, dtype16).to(dtype))
    p = prep_ref(s, t, dtype)
    u16, v16 = rnd(p["u"]), rnd(p["v"])
    z = (u16 @ v16.t()) / tau
    sm = softmax_ref(z, T if mask else 0, dtype)
    dz16 = rnd(sm["dz"])
    du = (dz16 @ v16) / (2 * M * tau)
    free = ~clamp_rows(s)
    u, inv = p["u"], p["inv_s"]
    ds = torch.where(free[:, None], inv[:, None] * (du - u * (u * du).sum(-1, keepdim=True)), du / EPS)
    return {"loss": sm["loss"], "ds": ds, "top1": sm["top1"], "u": u, "inv_s": inv, "u16": u16, "v16": v16, "z": z, "dz": sm["dz"],
            "dz16": dz16, "du": du, "P": sm["P"], "lse_row": sm["lse_row"], "lse_col": sm["lse_col"], "free": free}


def loss_ref(s, t, T, dtype16, tau=TAU, mask=True):
    """The composed reference with both roundings, float64."""
    return loss_exact(s, t, T, tau, F64, dtype16, mask)


def loss_autograd(s, t, T, tau=TAU, mask=True):
    """torch autograd of the logsumexp form in float64, no rounding: (loss, d loss / d s)."""
    sr = s.to(F64).clone().requires_grad_(True)
    u = sr / sr.norm(dim=-1, keepdim=True).clamp(min=EPS)
    tt = t.to(F64)
    v = tt / tt.norm(dim=-1, keepdim=True).clamp(min=EPS)
    z = u @ v.t() / tau
    M = z.shape[0]
    zm = z.masked_fill(~valid_mask(M, T if mask else 0), float("-inf"))
    d = z.diagonal()
    loss = ((torch.logsumexp(zm, 1) - d) + (torch.logsumexp(zm, 0) - d)).sum() / (2 * M)
    loss.backward()
    return loss.detach(), sr.grad.detach()


def norm_bwd_carry(a, r):
    """N(a) of the docstring: an elementwise bound a on du carried to ds."""
    u, inv = r["u"].abs(), r["inv_s"]
    free_rows = inv[:, None] * (a + u * (u * a).sum(-1, keepdim=True))
    return torch.where(r["free"][:, None], free_rows, a / EPS)


def loss_bounds(s, t, T, dtype16, tau=TAU, mask=True):
    """(reference, allowance of the loss, elementwise allowance of ds, yardsticks) of the composed chain."""
    r = loss_ref(s, t, T, dtype16, tau, mask)
    M = s.shape[0]
    u32, v32 = r["u16"].to(F32), r["v16"].to(F32)
    e32_z = e32_of((u32 @ v32.t()) / F32_of(tau), r["z"])
    e_z = bound32(e32_z) * r["z"].abs().max().item()
    lse_max = max(r["lse_row"].abs().max().item(), r["lse_col"].abs().max().item(), 1.0)
    rel = 2 * e_z + MARGIN * EPS32 * lse_max
    eye = torch.eye(M, dtype=torch.bool)
    P = torch.where(eye, r["dz"].abs(), r["P"])
    flips = torch.where(tie_distance(r["dz"], dtype16) <= P * rel, ulp16(r["dz"], dtype16), torch.zeros_like(P))
    va = r["v16"].abs()
    k = 1.0 / (2 * M * tau)
    e32_du = e32_of((r["dz16"].to(F32) @ v32) * F32_of(k), r["du"])
    a = (flips @ va) * k + rel * (P @ va) * k + bound32(e32_du) * r["du"].abs().max().item()
    e32_n = e32_of(norm_bwd_ref(r["du"].to(F32), s, F32), norm_bwd_ref(r["du"].to(F32), s, F64))
    allow_ds = norm_bwd_carry(a, r) + bound32(e32_n) * r["ds"].abs().max().item()
    allow_loss = 2 * e_z + softmax_loss_allow(r["loss"], M)
    margin = top1_margin(r["z"], r["valid"] if "valid" in r else valid_mask(M, T if mask else 0))
    return r, allow_loss, allow_ds, {"e32_z": e32_z, "e32_du": e32_du, "e32_n": e32_n, "e_z": e_z, "flips": int((flips > 0).sum()),
                                     "top1_margin": margin}


def F32_of(x):
    return float(torch.tensor(x, dtype=F32))


def top1_margin(z, V):
    """min_i |z_ii - max over the valid j != i of z_ij|: above 2 e_z the top-1 count of the chain is decided."""
    M = z.shape[0]
    off = z.masked_fill(~V | torch.eye(M, dtype=torch.bool), float("-inf")).max(1).values
    gap = (z.diagonal() - off).abs()
    return gap[torch.isfinite(gap)].min().item() if torch.isfinite(gap).any() else float("inf")
