"""CPU: the references of tests/loss_optim_refs.py are themselves right (against torch's own float64 functions and the committed
oracle), every case the GPU tests run has an fp32 yardstick small enough for its bound to mean something, and the element-wise bounds
can be met by a stable fp32 evaluation while rejecting the cancelling formulas and the positional-encoding mutant."""
import math

import numpy as np
import pytest
import torch

import loss_optim_refs as R
from oracle import student as oracle_student

F32, F64 = R.F32, R.F64


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


# ---------------------------------------------------------------------------------------------- distillation
@pytest.mark.parametrize("mode,rows,E", R.DISTILL_CASES)
def test_distill_cases_have_a_usable_yardstick(mode, rows, E):
    s, t = R.distill_inputs(rows, E)
    r64, r32 = R.distill_ref(s, t, mode), R.distill_ref(s, t, mode, F32)
    assert R.rel_scalar(r32["loss"], r64["loss"], 1.0 if mode == "cosine" else 0.0) <= R.E32_MAX
    assert R.e32_of(r32["ds"], r64["ds"]) <= R.E32_MAX
    if mode == "cosine":            # clear of the clamp edges: every row passes its gradient
        cos = torch.nn.functional.cosine_similarity(s.double(), t.double(), dim=-1)
        assert bool((cos.abs() < 0.999).all()) and bool((r64["ds"].abs().amax(1) > 0).all())
    for layout in R.DISTILL_LAYOUTS:
        buf, rpc, stride = R.distill_teacher_buffer(t, layout)
        flat = buf.reshape(-1)
        back = torch.stack([flat[(r // rpc) * stride + (r % rpc) * E:][:E] for r in range(rows)])
        assert torch.equal(back, t)


def test_distill_degenerate_rows_are_what_they_claim():
    eps = R.DISTILL_EPS
    for name, (s, t, zero_rows) in R.distill_degenerate_inputs().items():
        r64, r32 = R.distill_ref(s, t, "cosine"), R.distill_ref(s, t, "cosine", F32)
        assert R.e32_of(r32["ds"], r64["ds"]) <= R.E32_MAX and R.rel_scalar(r32["loss"], r64["loss"], 1.0) <= R.E32_MAX
        for r in zero_rows:
            assert bool((r64["ds"][r] == 0).all())
        sn, tn = s.double().norm(dim=1), t.double().norm(dim=1)
        c_raw = (s.double() * t.double()).sum(1) / (sn.clamp(min=eps) * tn.clamp(min=eps))
        edge = torch.minimum((c_raw - (1 - eps)).abs(), (c_raw + (1 - eps)).abs())
        assert bool((edge > 5e-6).all()), name                    # the pass / block decision is not a rounding matter
        assert bool(((sn - eps).abs() > 0.5 * eps).all())
        if name == "tiny":
            assert sn[1] == 0 and abs(sn[4].item() - 1e-6) < 1e-9 and 0.5 < (c_raw[4] * eps / 1e-6).item() < 0.95
            # gradient of the rows held by the norm clamp: -t / (eps |t| rows), nothing through the norm
            for r in (1, 4):
                assert _close(r64["ds"][r], -t[r].double() / (eps * tn[r] * s.shape[0]), 1e-9)


# ---------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize("pw", R.BCE_PW)
@pytest.mark.parametrize("soft", [False, True])
def test_bce_reference_equals_torch_and_the_oracle(pw, soft):
    x, y = R.bce_inputs(1120, soft)
    r = R.bce_ref(x, y, pw)
    w = R.bce_w(y.double(), pw)
    xr = x.double().clone().requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(xr, y.double(), pos_weight=w)
    loss.backward()
    assert _close(r["loss"], loss.detach())
    mid = x.abs() <= 9                                     # float64 autograd itself cancels further out
    assert _close(r["dx"][mid], xr.grad[mid], 1e-11)
    o = oracle_student.classification_loss(x.double(), y, None if pw < 0 else pw)     # the oracle rounds its weights to float32
    assert R.rel_scalar(o, r["loss"]) <= 2.0 ** -22
    # both tails of the closed form against exact values
    px, py = R.bce_planted()
    g = R.bce_grad_stable(px, py, pw) * len(px)
    for xi, yi, gi in zip(px.tolist(), py.tolist(), g.tolist()):
        wi = 1.0 if pw < 0 else pw * yi + 1.0
        want = (1 - yi) / (1 + math.exp(-xi) if xi > -700 else math.inf) if yi == 0 else -wi / (1 + math.exp(xi) if xi < 700 else math.inf)
        assert abs(gi - want) <= 1e-14 * abs(want), (xi, yi)


@pytest.mark.parametrize("n,pw,soft", R.BCE_CASES)
def test_bce_cases_have_a_usable_yardstick(n, pw, soft):
    x, y = R.bce_inputs(n, soft)
    r64, r32 = R.bce_ref(x, y, pw), R.bce_ref(x, y, pw, F32)
    assert R.rel_scalar(r32["loss"], r64["loss"]) <= R.E32_MAX
    assert R.e32_of(r32["dx"], r64["dx"]) <= R.E32_MAX
    if n >= 64:
        for sgn in (1.0, -1.0):
            for a in R.BCE_TAILS:
                assert ((x == sgn * a) & (y == y.min())).sum() >= 2 and ((x == sgn * a) & (y == y.max())).sum() >= 2


@pytest.mark.parametrize("pw", R.BCE_PW)
def test_bce_gradient_bound_admits_the_stable_formula_and_rejects_the_cancelling_one(pw):
    """fp32 on the CPU, hard targets, planted tails: sigma evaluated without cancellation stays inside the element-wise bound; the former
    (1 - y) - lw (1 - sigma) leaves it by orders of magnitude."""
    x, y = R.bce_inputs(255, False)
    n = x.numel()
    r64 = R.bce_grad_stable(x, y, pw)
    allow = R.bce_grad_allow(r64, n)

    def sig32(z):
        e = torch.exp(-z.abs())
        return torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    w = R.bce_w(y, pw)
    stable = ((1.0 - y) * sig32(x) - (w * y) * sig32(-x)) * np.float32(1.0 / n)
    assert stable.dtype is F32
    ex_stable = ((stable.double() - r64).abs() / allow).max().item()
    ex_cancel = ((R.bce_grad_cancelling(x, y, pw).double() - r64).abs() / allow).max().item()
    print(f"pw {pw}: stable {ex_stable:.3f}, cancelling {ex_cancel:.3e} of the allowed error")
    assert ex_stable <= 1.0 < 100.0 < ex_cancel
    # the cancelling formula at y = 1: relative errors far above 8 x 2^-23 at x = 9 and 13, and a gradient of exactly 0 from x = 17
    xs, ys = torch.tensor([9.0, 13.0, 17.0]), torch.ones(3)
    c, e = R.bce_grad_cancelling(xs, ys, -1.0).double(), R.bce_grad_stable(xs, ys, -1.0)
    rel = ((c - e) / e).abs().tolist()
    assert rel[0] > 1e-5 and rel[1] > 1e-4 and c[2].item() == 0.0 and e[2].item() < 0


# ---------------------------------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("rows,C,kind", R.CE_CASES)
def test_ce_reference_equals_torch_and_the_oracle_and_has_a_usable_yardstick(rows, C, kind):
    for logits in R.CE_LOGITS:
        x, idx, prob = R.ce_inputs(rows, C, kind, logits)
        r64, r32 = R.ce_ref(x, idx, prob), R.ce_ref(x, idx, prob, F32)
        xr = x.double().clone().requires_grad_(True)
        tgt = idx if prob is None else prob.double()
        loss = torch.nn.functional.cross_entropy(xr, tgt)
        loss.backward()
        assert _close(r64["loss"], loss.detach()) and _close(r64["dx"], xr.grad)
        assert _close(r64["loss"], oracle_student.cross_entropy_loss(x.double(), tgt), 1e-11)
        assert R.rel_scalar(r32["loss"], r64["loss"]) <= R.E32_MAX
        assert R.e32_of(r32["dx"], r64["dx"]) <= R.E32_MAX
        if kind == "soft" and rows >= 3:
            assert abs(prob[1].sum().item() - 0.5) < 1e-5 and abs(prob[2].sum().item() - 2.0) < 1e-5


@pytest.mark.parametrize("xt,gap,C,kind", R.CE_CONFIDENT)
def test_ce_row_bound_admits_the_stable_formula(xt, gap, C, kind):
    x, idx, prob = R.ce_confident_inputs(xt, gap, C, kind)
    r64 = R.ce_ref(x, idx, prob)["loss"].item()
    y = torch.nn.functional.one_hot(idx, C)[0].float() if prob is None else prob[0]
    assert abs(r64 - math.log1p(math.exp(-gap) + (C - 2) * math.exp(-80.0))) <= 1e-12 * r64
    got = R.ce_row_stable32(x[0], y).item()
    lsm = R.ce_ref(x, idx, prob, F32)["loss"].item()
    assert abs(got - r64) <= R.ce_row_allow(r64, C) and abs(lsm - r64) <= R.ce_row_allow(r64, C)


def test_ce_row_bound_rejects_the_cancelling_formula():
    """Logits [80, 80 - 11.5, 0], target 0: the former ysum (m + log se) - yx rounds the loss of 1.013e-5 at the size of m = 80 and gives
    7.63e-6; the bound is relative to log C."""
    x, idx, prob = R.ce_confident_inputs(80.0, 11.5, 3, "onehot")
    r64 = R.ce_ref(x, idx, prob)["loss"].item()
    got = R.ce_row_cancelling32(x[0], prob[0]).item()
    print(f"r64 {r64:.4e}, cancelling fp32 {got:.4e}, allowed {R.ce_row_allow(r64, 3):.3e}")
    assert abs(r64 - 1.013e-5) < 1e-8 and abs(got - 7.63e-6) < 1e-8
    assert abs(got - r64) > 2 * R.ce_row_allow(r64, 3)


# ---------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("decoupled,wd", R.ADAM_MODES)
@pytest.mark.parametrize("step", [1, 3])
def test_adam_reference_equals_torch_optim_and_the_oracle(decoupled, wd, step):
    p, g, m, v = R.adam_inputs(1023)
    lr, b1, b2, eps = (R.f32v(s) for s in (R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS))
    wdv = R.f32v(wd)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    r = R.adam_ref(p, g, m, v, lr, b1, b2, eps, wd, decoupled, lr / bc1, 1.0 / math.sqrt(bc2), 1.0)
    q = torch.nn.Parameter(p.double().clone())
    q.grad = g.double().clone()
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdv)
    opt.state[q] = {"step": torch.tensor(float(step - 1), dtype=F64), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    opt.step()
    st = opt.state[q]
    assert _close(r["m"], st["exp_avg"]) and _close(r["v"], st["exp_avg_sq"])
    # the reference rounds step_size and inv_sqrt_bc2 to fp32 as the kernel's caller does: two roundings of 2^-24 on the update
    dt = q.detach() - p.double()
    assert (r["d"] - dt).abs().max().item() <= 2.0 ** -22 * dt.abs().max().item()
    op, om, ov = oracle_student.adam_step(p.double(), g.double(), m.double(), v.double(), step, lr, b1, b2, eps, wdv, bool(decoupled))
    assert _close(q.detach(), op) and _close(r["m"], om) and _close(r["v"], ov)


@pytest.mark.parametrize("n", R.ADAM_N + R.ADAM_BG_N)
def test_adam_cases_have_a_usable_yardstick(n):
    p, g, m, v = R.adam_inputs(n)
    for decoupled, wd in R.ADAM_MODES:
        for gs in R.ADAM_GSCALE:
            for step in R.ADAM_STEPS:
                ss, ib = R.adam_host_scalars(step)
                a = (p, g, m, v, R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS, wd, decoupled, ss, ib, gs)
                r64, r32 = R.adam_ref(*a), R.adam_ref(*a, dtype=F32)
                assert all(bool(torch.isfinite(r32[k]).all()) for k in r32)
                if r64["d"].abs().max() > 0:
                    assert R.e32_of(r32["d"], r64["d"]) <= R.E32_MAX
                big = g.abs() > 1e10
                assert R.adam_split_rel(r32["m"], r64["m"], big) <= R.E32_MAX and R.adam_split_rel(r32["v"], r64["v"], big) <= R.E32_MAX
                # the update stands clear of the spacing of p: the bound's first term does not swallow it
                assert n < 12 or r64["d"].abs().max().item() > 100 * R.ulp(r64["p"], F32).max().item()
    z = R.adam_zero_grad_index(n)
    if z is not None:
        assert g[z] == 0 and m[z] == 0 and v[z] == 0 and p[z] != 0
    if n >= 12:
        assert v[1] == np.float32(1e-40) and 0 < v[1] < R.TINY32 and g[2] == -1e15 and p[3] == 0 and p[n - 4] == 0 and g[n - 3] == -1e15


def test_adam_host_scalars_and_tick_formulas():
    ss, ib = R.adam_host_scalars(1)
    assert ss == R.f32v(R.f32v(3e-3) / (1.0 - R.f32v(0.9))) and abs(ib - 1 / math.sqrt(1 - R.f32v(0.999))) < 1e-5
    assert R.adam_host_scalars(100000) == (R.f32v(3e-3), 1.0)
    h1, h2 = R.tick_hyper(3e-3, 2)
    assert abs(h1 - 3e-3 / 0.19) < 1e-8 and abs(h2 - 1 / math.sqrt(1 - 0.999 ** 2)) < 1e-3
    seeds = [R.tick_seed(R.TICK_BASE_SEED, t, i) for t in (1, 2) for i in range(300)]
    assert len(set(seeds)) == 600 and all(0 <= s < (1 << 63) for s in seeds)
    # the finaliser is splitmix64's: its first output for state 0 is the published 0xE220A8397B1DCDAF
    assert R.tick_seed(0, 1, 0) == 0xE220A8397B1DCDAF & ~(1 << 63)


# ---------------------------------------------------------------------------------------------- sumsq, colsum, positional encoding
@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sumsq_cases_have_a_usable_yardstick_and_the_atomics_term_hides_no_lost_partial(n):
    x = R.sumsq_input(n)
    sq = x.double() ** 2
    P = R.sumsq_atomic_adds(n)
    assert P == {1: 1, 255: 1, 257: 2, 262144: 1024, 262147: 1024}[n]
    for preset in R.SUMSQ_PRESET:
        r64 = R.sumsq_ref(x, preset).item()
        e32 = R.rel_scalar(R.sumsq_ref(x, preset, F32), r64)
        assert e32 <= R.E32_MAX
        allow = R.sumsq_allow(e32, n) * r64
        if P > 1:           # the smallest share any one workgroup holds, and the second trip, are far outside the allowance
            first = sq[:P * R.SUMSQ_BLOCK]
            first = torch.cat([first, torch.zeros(P * R.SUMSQ_BLOCK - first.numel(), dtype=F64)]).view(-1, P, R.SUMSQ_BLOCK) if n < P * R.SUMSQ_BLOCK \
                else first.view(1, P, R.SUMSQ_BLOCK)
            assert first.sum((0, 2)).min().item() > 4 * allow
        if n > R.SUMSQ_BLOCK * R.SUMSQ_GRID_CAP:
            assert sq[R.SUMSQ_BLOCK * R.SUMSQ_GRID_CAP:].sum().item() > 100 * allow


@pytest.mark.parametrize("M,N", R.COLSUM_CASES)
def test_colsum_cases_have_a_usable_yardstick(M, N):
    x = R.colsum_input(M, N)
    for dt in (F32, R.BF16, R.F16):
        xs = x.to(dt)
        assert R.e32_of(R.colsum_ref(xs, F32), R.colsum_ref(xs)) <= R.E32_MAX
    assert R.colsum_slabs(M) == {1: 1, 3: 1, 127: 1, 128: 1, 129: 1, 1030: 8, 8197: 64}[M]


@pytest.mark.parametrize("T,D", R.PE_HOST_SHAPES)
def test_positional_encoding_bound_admits_the_fp32_table_and_rejects_the_own_frequency_mutant(T, D):
    r64 = R.pe_table64(T, D)
    allow = R.pe_allow(T, D, r64)
    own = ((R.pe_table32(T, D).double() - r64).abs() / allow).max().item()
    mut = ((R.pe_table32(T, D, own_frequency=True).double() - r64).abs() / allow).max().item()
    print(f"({T}, {D}): fp32 table {own:.3f}, own-frequency mutant {mut:.3e} of the allowed error")
    assert own <= 1.0 < mut
    assert r64[0, 0::2].abs().max() == 0 and bool((r64[0, 1::2] == 1).all())
    assert abs(r64[min(T, 5) - 1, D - 1].item() - math.cos((min(T, 5) - 1) * 10000.0 ** (-(D - 2) / D))) < 1e-12
