"""GPU: the kernels that finish a training step -- distillation, BCE and cross-entropy losses, the Adam family with vmc_train_tick,
vmc_sumsq, the sinusoidal positional encoding, vmc_colsum, vmc_transpose16, vmc_cast_weight -- each against a float64 CPU reference of
the same operation (tests/loss_optim_refs.py), called through the C ABI (vimo_clip_amd._lib).

fp32 outputs must satisfy  max|got - r64| / max|r64| <= 8 max(e32, 2^-23)  with e32 the error of a float32 CPU evaluation of the same
reference on the same inputs; scalar losses the same (denominator max(|r64|, 1) for the cosine loss); exact operations are bit-equal to
the CPU.  The BCE gradient, the loss of a single cross-entropy row, the Adam update and the positional encoding have element-wise
bounds of their own, derived in tests/loss_optim_refs.py.  With VMC_LOSS_OPTIM_PARITY_JSON=<path> the measured figures of every case are
written there, one line each (profiles/loss_optim_parity.jsonl keeps the worst line per kernel and output of such a file)."""
import json
import os

import numpy as np
import pytest
import torch

import loss_optim_refs as R
import train_kernel_refs as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16
DT16 = [BF16, F16]
DT16_IDS = ["bf16", "f16"]
E_ARG, E_ALIGN, E_DTYPE = -1, -2, -4
NAN = float("nan")
SENTINEL = 12345.0
LR, B1, B2, EPS = R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS

L = None            # vimo_clip_amd._lib, loaded by the module fixture
_REC = []


@pytest.fixture(scope="module", autouse=True)
def _lib_module():
    global L
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vimo_clip_amd import _lib
    L = _lib
    yield
    out = os.environ.get("VMC_LOSS_OPTIM_PARITY_JSON", "")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps({"margin": R.MARGIN, "floor": R.EPS32}) + "\n")          # then one line per case
            f.writelines(json.dumps(r) + "\n" for r in _REC)


def rec(kernel, case, output, err, e32, ratio, allowed, unit):
    """ratio / allowed <= 1 passes; `unit` says what the ratio is."""
    print(f"{kernel} {case} {output}: err {err:.3e}, e32 {e32:.3e}, {ratio:.3f} of {allowed:g} ({unit})")
    _REC.append({"kernel": kernel, "case": case, "output": output, "err": err, "e32": e32, "ratio": ratio, "allowed": allowed, "unit": unit})


def ck_vec(kernel, case, output, got, r64, r32):
    """fp32 vector: max|got - r64| / max|r64| <= 8 max(e32, 2^-23)."""
    e32 = R.e32_of(r32, r64)
    assert e32 <= R.E32_MAX
    assert bool(torch.isfinite(got).all()), f"{kernel} {case} {output}: not finite"
    err = R.max_rel(got, r64)
    rec(kernel, case, output, err, e32, err / max(e32, R.EPS32), R.MARGIN, "err / max(e32, 2^-23)")
    assert err <= R.bound32(e32), f"{kernel} {case} {output}: {err:.3e} > {R.bound32(e32):.3e} (e32 {e32:.3e})"


def ck_scalar(kernel, case, output, got, r64, r32, floor=0.0):
    """scalar: |got - r64| / max(|r64|, floor) <= 8 max(e32, 2^-23)."""
    e32 = R.rel_scalar(r32, r64, floor)
    assert e32 <= R.E32_MAX
    got = float(got)
    assert np.isfinite(got), f"{kernel} {case} {output}: {got}"
    err = R.rel_scalar(got, r64, floor)
    rec(kernel, case, output, err, e32, err / max(e32, R.EPS32), R.MARGIN, "err / max(e32, 2^-23)")
    assert err <= R.bound32(e32), f"{kernel} {case} {output}: {err:.3e} > {R.bound32(e32):.3e} (e32 {e32:.3e})"


def ck_elem(kernel, case, output, got, r64, allow, unit):
    """element-wise: |got - r64| <= allow for every element."""
    assert bool(torch.isfinite(got).all()), f"{kernel} {case} {output}: not finite"
    d = (R.widen(got) - r64).abs()
    ex = (d / allow).max().item()
    rec(kernel, case, output, d.max().item(), 0.0, ex, 1.0, unit)
    assert ex <= 1.0, f"{kernel} {case} {output}: {ex:.3f} x the allowed error"


def dev(t):
    return None if t is None else t.to(DEV)


def empty(shape, dtype=F32):
    """An output buffer the kernel has to overwrite: NaN everywhere."""
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def sync():
    torch.cuda.synchronize()


def call(name, *args):
    return getattr(L.lib, name)(*args)


def ok(name, *args):
    L.check(call(name, *args), name)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype is F32 else torch.int16)


# ================================================================================================ distillation loss
def _distill(s, tbuf, rows, E, rpc, stride, cosine, with_grad):
    s_d, t_d = dev(s), dev(tbuf)
    loss, ds = empty((1,)), (empty((rows, E)) if with_grad else None)
    wsb = call("vmc_loss_workspace_bytes", rows)
    assert wsb == rows * 4
    ws = empty((rows,))
    ok("vmc_distill_loss", L.ptr(s_d), L.ptr(t_d), L.ptr(loss), L.ptr(ds), rows, E, rpc, stride, int(cosine), L.ptr(ws), wsb, L.stream())
    sync()
    assert torch.equal(s_d.cpu(), s)
    return loss.cpu().item(), (ds.cpu() if with_grad else None)


@pytest.mark.parametrize("mode,rows,E", R.DISTILL_CASES)
def test_distill_loss(mode, rows, E):
    """vmc_distill_loss, both modes, against float64 autograd through oracle.student.distillation_loss: every teacher layout (the rows and
    gaps it must skip hold NaN), with the gradient and without."""
    s, t = R.distill_inputs(rows, E)
    r64, r32 = R.distill_ref(s, t, mode), R.distill_ref(s, t, mode, F32)
    floor = 1.0 if mode == "cosine" else 0.0
    for layout in R.DISTILL_LAYOUTS:
        buf, rpc, stride = R.distill_teacher_buffer(t, layout)
        for with_grad in (True, False):
            cid = f"{mode}-{rows}x{E}-{layout}{'' if with_grad else '-nograd'}"
            loss, ds = _distill(s, buf, rows, E, rpc, stride, mode == "cosine", with_grad)
            ck_scalar("vmc_distill_loss", cid, "loss", loss, r64["loss"], r32["loss"], floor)
            if with_grad:
                ck_vec("vmc_distill_loss", cid, "dstudent", ds, r64["ds"], r32["ds"])


@pytest.mark.parametrize("name", ["unit", "tiny"])
def test_distill_loss_degenerate_rows(name):
    """Cosine mode: zero teacher row, s = t and s = -t (gradient exactly 0: dot = 0, or the clamp of the cosine blocks it); zero student
    row and |s| = 1e-6 < eps (the norm clamp holds |s| at eps and passes nothing through the norm)."""
    s, t, zero_rows = R.distill_degenerate_inputs()[name]
    rows, E = s.shape
    r64, r32 = R.distill_ref(s, t, "cosine"), R.distill_ref(s, t, "cosine", F32)
    loss, ds = _distill(s, t, rows, E, rows, rows * E, True, True)
    ck_scalar("vmc_distill_loss", f"cosine-degenerate-{name}", "loss", loss, r64["loss"], r32["loss"], 1.0)
    ck_vec("vmc_distill_loss", f"cosine-degenerate-{name}", "dstudent", ds, r64["ds"], r32["ds"])
    for r in zero_rows:
        assert bool((ds[r] == 0).all()), r
    if name == "tiny":      # the two clamped rows on their own, so that neither hides behind the other
        for r in (1, 4):
            ck_vec("vmc_distill_loss", f"cosine-degenerate-tiny-row{r}", "dstudent", ds[r], r64["ds"][r], r32["ds"][r])


# ================================================================================================ BCE with logits
def _bce(x, y, pw, with_grad):
    n = x.numel()
    x_d, y_d = dev(x), dev(y)
    loss, dx = empty((1,)), (empty((n,)) if with_grad else None)
    ws = empty((R.BCE_BLOCKS,))
    ok("vmc_bce_loss", L.ptr(x_d), L.ptr(y_d), L.ptr(loss), L.ptr(dx), n, pw, L.ptr(ws), R.BCE_BLOCKS * 4, L.stream())
    sync()
    ws = ws.cpu()
    if n <= R.BCE_SINGLE_WG_MAX:
        assert bool(torch.isnan(ws).all()), "the single-workgroup path touched the workspace"
    else:
        blocks = min(-(-n // 256), R.BCE_BLOCKS)
        assert bool(torch.isfinite(ws[:blocks]).all()) and bool(torch.isnan(ws[blocks:]).all())
    return loss.cpu().item(), (dx.cpu() if with_grad else None)


@pytest.mark.parametrize("n,pw,soft", R.BCE_CASES, ids=lambda v: str(v))
def test_bce_loss(n, pw, soft):
    """vmc_bce_loss: the single-workgroup path (n <= 8192, the workspace stays untouched), the two-pass path, its 64-block cap and second
    grid-stride trip.  Hard targets: every gradient element within 8 x 2^-23 of itself (+ 2^-126 / n), both confident tails planted, and
    its sign right out to |x| = 1e4.  Soft targets cancel between the two terms for real: max-relative rule."""
    x, y = R.bce_inputs(n, soft)
    r64, r32 = R.bce_ref(x, y, pw), R.bce_ref(x, y, pw, F32)
    cid = f"n{n}-pw{pw:g}-{'soft' if soft else 'hard'}"
    for with_grad in (True, False):
        loss, dx = _bce(x, y, pw, with_grad)
        ck_scalar("vmc_bce_loss", cid + ("" if with_grad else "-nograd"), "loss", loss, r64["loss"], r32["loss"])
        if not with_grad:
            continue
        if soft:
            ck_vec("vmc_bce_loss", cid, "dlogits", dx, r64["dx"], r32["dx"])
        else:
            assert R.e32_of(r32["dx"], r64["dx"]) <= R.E32_MAX
            ck_elem("vmc_bce_loss", cid, "dlogits", dx, r64["dx"], R.bce_grad_allow(r64["dx"], n), "of 8 2^-23 |r64| + 2^-126 / n, element-wise")
            assert bool((dx[y == 1] <= 0).all()) and bool((dx[y == 0] >= 0).all())
            far = x.abs() >= 100                                   # vanishing side of the far tails: nothing above the floor
            gone = far & (r64["dx"].abs() * n < R.TINY32)
            if n >= 64:
                assert int(gone.sum()) == 8
            assert bool((dx[gone].double().abs() <= R.bce_grad_allow(r64["dx"], n)[gone]).all())


# ================================================================================================ cross entropy
def _ce(x, idx, prob, with_grad):
    rows, C = x.shape
    x_d, i_d, p_d = dev(x), dev(idx), dev(prob)
    loss, dx = empty((1,)), (empty((rows, C)) if with_grad else None)
    ws = empty((rows,))
    ok("vmc_cross_entropy_loss", L.ptr(x_d), L.ptr(i_d), L.ptr(p_d), L.ptr(loss), L.ptr(dx), rows, C, L.ptr(ws), rows * 4, L.stream())
    sync()
    return loss.cpu().item(), (dx.cpu() if with_grad else None)


@pytest.mark.parametrize("rows,C,kind", R.CE_CASES)
def test_cross_entropy_loss(rows, C, kind):
    """vmc_cross_entropy_loss against float64 log_softmax: index targets, float one-hot rows, soft rows whose sums are 1, 0.5 and 2; logits
    5 randn with an 80 spike, and all-equal logits; with the gradient and without.  rows = 1: the scalar is the row's loss and must be
    within 8 x 2^-23 (|r64| + log C)."""
    for logits in R.CE_LOGITS:
        x, idx, prob = R.ce_inputs(rows, C, kind, logits)
        r64, r32 = R.ce_ref(x, idx, prob), R.ce_ref(x, idx, prob, F32)
        cid = f"{rows}x{C}-{kind}-{logits}"
        for with_grad in (True, False):
            loss, dx = _ce(x, idx, prob, with_grad)
            tag = cid + ("" if with_grad else "-nograd")
            if rows == 1:
                allow = R.ce_row_allow(r64["loss"], C)
                err = abs(loss - r64["loss"].item())
                rec("vmc_cross_entropy_loss", tag, "row loss", err, 0.0, err / allow if allow > 0 else err, 1.0, "of 8 2^-23 (|r64| + log C)")
                assert np.isfinite(loss) and err <= allow, (loss, r64["loss"].item(), allow)
            else:
                ck_scalar("vmc_cross_entropy_loss", tag, "loss", loss, r64["loss"], r32["loss"])
            if with_grad:
                ck_vec("vmc_cross_entropy_loss", cid, "dlogits", dx, r64["dx"], r32["dx"])


@pytest.mark.parametrize("xt,gap,C,kind", R.CE_CONFIDENT)
def test_cross_entropy_confident_row(xt, gap, C, kind):
    """One confident row, logits [x_t, x_t - gap, x_t - 80, ...], target 0: the loss log(1 + e^-gap) is 1.0e-5 (gap 11.5) or 6.7e-3
    (gap 5) whatever x_t is, and must not be rounded at the size of x_t."""
    x, idx, prob = R.ce_confident_inputs(xt, gap, C, kind)
    r64 = R.ce_ref(x, idx, prob)["loss"].item()
    allow = R.ce_row_allow(r64, C)
    for with_grad in (True, False):      # the gradient of such a row is p_t - 1 with torch's own cancellation: not judged here
        loss, _ = _ce(x, idx, prob, with_grad)
        err = abs(loss - r64)
        rec("vmc_cross_entropy_loss", f"confident-xt{xt:g}-gap{gap:g}-C{C}-{kind}{'' if with_grad else '-nograd'}", "row loss", err, 0.0,
            err / allow, 1.0, "of 8 2^-23 (|r64| + log C)")
        assert np.isfinite(loss) and err <= allow, (loss, r64, allow)


def test_cross_entropy_error_codes():
    x, idx, prob = (dev(t) for t in (torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 8)))
    loss, ws = empty((1,)), empty((4,))
    p = L.ptr

    def ce(i, q, wsb=16):
        return call("vmc_cross_entropy_loss", p(x), i, q, p(loss), None, 4, 8, p(ws), wsb, L.stream())
    assert ce(p(idx), p(prob)) == E_ARG and ce(None, None) == E_ARG and ce(p(idx), None, 15) == E_ARG
    assert ce(p(idx), None) == 0 and ce(None, p(prob)) == 0
    sync()


# ================================================================================================ Adam
ADAM_GUARD = 8


def _adam_call(api, t, mode, gs, step, max_wg=1):
    """One update through `api` from the inputs t = (p, g, m, v); each buffer carries a guard of 8 sentinels behind its n elements."""
    n = t[0].numel()
    decoupled, wd = mode
    p, g, m, v = (dev(torch.cat([x, torch.full((ADAM_GUARD,), SENTINEL)])) for x in t)
    ss, ib = R.adam_host_scalars(step)
    if api == "host":
        ok("vmc_adam_step", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, LR, B1, B2, EPS, wd, decoupled, step, gs, L.stream())
    else:
        hyper = torch.tensor([LR, ss, ib, gs], dtype=F32, device=DEV)      # the four floats vmc_adam_step passes by value
        if api == "dev":
            ok("vmc_adam_step_dev", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, L.ptr(hyper), B1, B2, EPS, wd, decoupled, L.stream())
        else:
            ok("vmc_adam_step_dev_bg", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, L.ptr(hyper), B1, B2, EPS, wd, decoupled, max_wg, L.stream())
    sync()
    out = []
    for buf, x in zip((p, g, m, v), t):
        buf = buf.cpu()
        assert bool((buf[n:] == SENTINEL).all()), "wrote past the end"
        out.append(buf[:n])
    assert torch.equal(out[1], t[1])
    return out[0], out[2], out[3]


def _adam_check(kernel, cid, t, got, mode, gs, step):
    """The update d = p_new - p_old element-wise, m and v under the plain rule (the 1e15 gradient on its own), the planted elements."""
    p, g, m, v = t
    n = p.numel()
    decoupled, wd = mode
    ss, ib = R.adam_host_scalars(step)
    a = (p, g, m, v, LR, B1, B2, EPS, wd, decoupled, ss, ib, gs)
    r64, r32 = R.adam_ref(*a), R.adam_ref(*a, dtype=F32)
    pg, mg, vg = got
    assert all(bool(torch.isfinite(x).all()) for x in got), f"{kernel} {cid}: not finite"
    ex, e32 = R.adam_excess(pg, p, r64, r32)
    assert e32 <= R.E32_MAX
    rec(kernel, cid, "update", ex, e32, ex, 1.0, "of ulp32(p) + 8 max(e32_d, 2^-23) max|d64|, element-wise")
    assert ex <= 1.0, f"{kernel} {cid} update: {ex:.3f} x the allowed error"
    big = g.abs() > 1e10
    for name, gk in (("m", mg), ("v", vg)):
        e = R.adam_split_rel(r32[name], r64[name], big)
        err = R.adam_split_rel(gk, r64[name], big)
        assert e <= R.E32_MAX
        rec(kernel, cid, name, err, e, err / max(e, R.EPS32), R.MARGIN, "err / max(e32, 2^-23)")
        assert err <= R.bound32(e), f"{kernel} {cid} {name}: {err:.3e} > {R.bound32(e):.3e}"
    z = R.adam_zero_grad_index(n)
    if z is not None and not (wd != 0 and not decoupled):        # g = m = v = 0: p moves by the decoupled decay alone, bit for bit
        want = np.float32(p[z].item()) * (np.float32(1.0) - np.float32(LR) * np.float32(wd)) if decoupled else np.float32(p[z].item())
        assert pg[z].item() == float(want) and mg[z].item() == 0.0 and vg[z].item() == 0.0


@pytest.mark.parametrize("decoupled,wd", R.ADAM_MODES)
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_step(n, decoupled, wd):
    """vmc_adam_step (default launch) against float64, one update at a time from identical inputs: AdamW, L2, no decay; grad_scale 1 and
    0.25; steps 1, 2, 1000, 100000; sizes with and without a scalar tail.  vmc_adam_step_dev with the same four floats written by the host
    gives the same bits."""
    t = R.adam_inputs(n)
    for gs in R.ADAM_GSCALE:
        for step in R.ADAM_STEPS:
            cid = f"n{n}-dec{decoupled}-wd{wd:g}-gs{gs:g}-t{step}"
            got = _adam_call("host", t, (decoupled, wd), gs, step)
            _adam_check("vmc_adam_step", cid, t, got, (decoupled, wd), gs, step)
            got_dev = _adam_call("dev", t, (decoupled, wd), gs, step)
            for a, b in zip(got, got_dev):
                assert torch.equal(bits(a), bits(b)), cid


@pytest.mark.parametrize("decoupled,wd", R.ADAM_MODES)
@pytest.mark.parametrize("n", R.ADAM_BG_N)
def test_adam_step_dev_bg_one_workgroup(n, decoupled, wd):
    """vmc_adam_step_dev_bg with max_workgroups = 1 against float64: a trip is 2048 elements, so these sizes reach the full trip, the
    scalar tail, the half trip (only the first float4 of a thread's pair exists) and the third trip.  vmc_adam_step_dev (default grid) on
    the same inputs against float64 too."""
    t = R.adam_inputs(n)
    for gs, step in ((1.0, 2), (0.25, 1000)):
        cid = f"n{n}-dec{decoupled}-wd{wd:g}-gs{gs:g}-t{step}"
        _adam_check("vmc_adam_step_dev_bg", cid, t, _adam_call("bg", t, (decoupled, wd), gs, step, max_wg=1), (decoupled, wd), gs, step)
        _adam_check("vmc_adam_step_dev", cid, t, _adam_call("dev", t, (decoupled, wd), gs, step), (decoupled, wd), gs, step)


def test_adam_error_codes():
    b = torch.zeros(64, device=DEV)
    h = torch.zeros(8, device=DEV)
    p, off = L.ptr(b), L.ptr(b) + 4

    def host(pp=p, n=16, step=1):
        return call("vmc_adam_step", pp, p, p, p, n, LR, B1, B2, EPS, 0.0, 1, step, 1.0, L.stream())

    def bg(pp=p, hh=L.ptr(h), n=16, wg=1):
        return call("vmc_adam_step_dev_bg", pp, p, p, p, n, hh, B1, B2, EPS, 0.0, 1, wg, L.stream())
    assert host(pp=off) == E_ALIGN and host(n=0) == E_ARG and host(step=0) == E_ARG
    assert bg(pp=off) == E_ALIGN and bg(hh=L.ptr(h) + 4) == E_ALIGN and bg(n=0) == E_ARG and bg(wg=0) == E_ARG
    assert call("vmc_adam_step_dev", off, p, p, p, 16, L.ptr(h), B1, B2, EPS, 0.0, 1, L.stream()) == E_ALIGN
    sync()
    assert bool((b == 0).all())


# ================================================================================================ vmc_train_tick
TICK_GUARD = 4
I64_SENTINEL = -0x0123456789ABCDEF


@pytest.mark.parametrize("n_seeds", R.TICK_SEEDS)
def test_train_tick(n_seeds):
    """Step count exact; hyper[1] = lr / (1 - b1^t) and hyper[2] = 1 / sqrt(1 - b2^t) within one fp32 ulp of the double formulas;
    hyper[0] and hyper[3] untouched; the seeds bit-equal to the mix in Python integers with bit 63 clear; nothing written behind them."""
    for t0, ticks in ((0, 1), (0, 2), (0, 5), (999, 1)):
        state = torch.full((2 + n_seeds + TICK_GUARD,), I64_SENTINEL, dtype=torch.int64)
        state[0], state[1] = t0, R.TICK_BASE_SEED
        hyper = torch.tensor([LR, 111.0, 222.0, 0.25], dtype=F32)
        s_d, h_d = dev(state), dev(hyper)
        for _ in range(ticks):
            ok("vmc_train_tick", L.ptr(s_d), L.ptr(h_d), B1, B2, n_seeds, L.stream())
        sync()
        s, h = s_d.cpu(), h_d.cpu()
        t = t0 + ticks
        assert s[0].item() == t and s[1].item() == R.TICK_BASE_SEED
        assert torch.equal(bits(h[[0, 3]]), bits(hyper[[0, 3]]))
        for k, want in zip((1, 2), R.tick_hyper(LR, t)):
            off = abs(h[k].double().item() - want) / R.ulp(torch.tensor(want, dtype=F64), F32).item()
            rec("vmc_train_tick", f"seeds{n_seeds}-t{t}", f"hyper[{k}]", off, 0.0, off, 1.0, "fp32 ulp of the double formula")
            assert off <= 1.0, (k, h[k].item(), want)
        assert s[2:2 + n_seeds].tolist() == [R.tick_seed(R.TICK_BASE_SEED, t, i) for i in range(n_seeds)]
        assert bool((s[2 + n_seeds:] == I64_SENTINEL).all())
    assert call("vmc_train_tick", None, L.ptr(h_d), B1, B2, 1, L.stream()) == E_ARG
    assert call("vmc_train_tick", L.ptr(s_d), L.ptr(h_d), B1, B2, -1, L.stream()) == E_ARG


# ================================================================================================ vmc_sumsq
@pytest.mark.parametrize("preset", R.SUMSQ_PRESET)
@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sumsq(n, preset):
    """vmc_sumsq accumulates into `out`.  The workgroup sums are added with fp32 atomics, so the bits may differ from call to call and the
    allowance carries P 2^-24 for the P adds on top of the plain rule (loss_optim_refs.sumsq_allow)."""
    x = R.sumsq_input(n)
    x_d = dev(torch.cat([x, torch.full((4,), NAN)]))               # the kernel must not read past n
    out = torch.full((1,), preset, device=DEV)
    ok("vmc_sumsq", L.ptr(x_d), n, L.ptr(out), L.stream())
    sync()
    got, r64 = out.cpu().item(), R.sumsq_ref(x, preset).item()
    e32 = R.rel_scalar(R.sumsq_ref(x, preset, F32), r64)
    assert e32 <= R.E32_MAX and np.isfinite(got)
    err, allow = R.rel_scalar(got, r64), R.sumsq_allow(e32, n)
    rec("vmc_sumsq", f"n{n}-preset{preset:g}", "out", err, e32, err / allow, 1.0, "of 8 max(e32, 2^-23) + P 2^-24")
    assert err <= allow, f"vmc_sumsq n{n} preset {preset}: {err:.3e} > {allow:.3e} (e32 {e32:.3e})"


# ================================================================================================ positional encoding
@pytest.mark.parametrize("B,T,D", R.PE_SHAPES)
def test_add_sinusoidal_pe(B, T, D):
    """In place on x = randn, broadcast over B: every element within 4 a + 2^-23 |r64| + 2^-22 of x + pe64 (a: what an fp32 angle carries)."""
    x = R.randn((B, T, D), 9800 + T + D)
    x_d = dev(x.clone())
    ok("vmc_add_sinusoidal_pe", L.ptr(x_d), B, T, D, L.stream())
    sync()
    r64 = x.double() + R.pe_table64(T, D)[None]
    ck_elem("vmc_add_sinusoidal_pe", f"{B}x{T}x{D}", "x", x_d.cpu(), r64, R.pe_allow(T, D, r64), "of 4 a + 2^-23 |r64| + 2^-22, element-wise")


def test_add_sinusoidal_pe_rejects_odd_width():
    x = torch.zeros(2, 3, 5, device=DEV)
    assert call("vmc_add_sinusoidal_pe", L.ptr(x), 2, 3, 5, L.stream()) == E_ARG
    assert call("vmc_add_sinusoidal_pe", None, 2, 3, 4, L.stream()) == E_ARG
    sync()
    assert bool((x == 0).all())


# ================================================================================================ column sums
@pytest.mark.parametrize("M,N", R.COLSUM_CASES)
def test_colsum(M, N):
    """vmc_colsum against the float64 column sums of the stored values: f32 / bf16 / f16 input, ld_in = N and N + 8 with NaN in the gap
    columns, workspace and output NaN-filled; slab boundaries (M / 128, at most 64, a short last slab) and more than one column block."""
    x = R.colsum_input(M, N)
    slabs = R.colsum_slabs(M)
    wsb = call("vmc_colsum_workspace_bytes", M, N)
    assert wsb == slabs * N * 4
    for dt in (F32, BF16, F16):
        xs = x.to(dt)
        r64, r32 = R.colsum_ref(xs), R.colsum_ref(xs, F32)
        for ld in (N, N + R.COLSUM_PAD):
            buf, _ = TR.padded(xs, ld, NAN)
            b_d, out, ws = dev(buf), empty((N,)), empty((slabs * N,))
            ok("vmc_colsum", L.ptr(b_d), L.ptr(out), M, N, ld, L.dt(dt), L.ptr(ws), wsb, L.stream())
            sync()
            ck_vec("vmc_colsum", f"{M}x{N}-{R.DT_NAME[dt]}-ld{ld}", "out", out.cpu(), r64, r32)


def test_colsum_error_codes():
    x, out, ws = torch.zeros(4, 16, device=DEV), empty((8,)), empty((64,))
    p = L.ptr
    assert call("vmc_colsum", p(x), p(out), 4, 6, 6, L.F32, p(ws), 256, L.stream()) == E_ALIGN       # N % 4
    assert call("vmc_colsum", p(x), p(out), 4, 8, 10, L.F32, p(ws), 256, L.stream()) == E_ALIGN      # ld_in % 4
    assert call("vmc_colsum", p(x), p(out), 4, 8, 4, L.F32, p(ws), 256, L.stream()) == E_ARG         # ld_in < N
    assert call("vmc_colsum", p(x), p(out), 4, 8, 8, L.F32, p(ws), 8 * 4 - 1, L.stream()) == E_ARG   # short workspace
    assert call("vmc_colsum", p(x), p(out), 4, 8, 8, 7, p(ws), 8 * 4, L.stream()) == E_DTYPE         # in_dtype not f32 / bf16 / f16
    assert call("vmc_colsum", p(x), p(out), 4, 8, 8, L.F32, p(ws), 8 * 4, L.stream()) == 0
    sync()


# ================================================================================================ transpose, weight casts
PATTERN16 = 0x5A5A


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("rows,cols", R.T16_SHAPES)
def test_transpose16(rows, cols, dt16):
    """Every kind of 16-bit pattern, ld_in = cols + 3 and ld_out = rows + 5: the transpose bit for bit, the gap columns of the output
    untouched."""
    src = R.cast_inputs_16(rows * cols, dt16).view(rows, cols)
    buf = torch.full((rows, cols + 3), 1.0, dtype=dt16)
    buf[:, :cols] = src
    out0 = torch.full((cols, rows + 5), PATTERN16, dtype=torch.int16)
    b_d, o_d = dev(buf), dev(out0)
    ok("vmc_transpose16", L.ptr(b_d), L.ptr(o_d), rows, cols, cols + 3, rows + 5, L.stream())
    sync()
    want = out0.clone()
    want[:, :rows] = bits(src).t()
    assert torch.equal(o_d.cpu(), want)
    assert call("vmc_transpose16", L.ptr(b_d), L.ptr(o_d), rows, cols, cols - 1, rows, L.stream()) == E_ARG
    assert call("vmc_transpose16", L.ptr(b_d), L.ptr(o_d), rows, cols, cols, rows - 1, L.stream()) == E_ARG


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("rows,cols", R.T16_SHAPES + ((68, 132),))
def test_cast_weight(rows, cols, dt16):
    """vmc_cast_weight: the plain copy, the copy padded to a multiple of 64 columns, the transposed (padded) copy alone and both in one
    launch -- bit-equal to the CPU cast (ties, overflow, subnormals, infinities planted; any NaN matches any NaN), pad columns exactly 0.
    64 x 64 and 68 x 132 (six tiles, ragged edges both ways) take the 4-wide path, the other shapes the scalar one."""
    w = TR.cast_inputs_f32(rows * cols, dt16).view(rows, cols).contiguous()
    ref = w.to(dt16)
    w_d = dev(w)

    def expect(r, ld):
        e = torch.zeros(r.shape[0], ld, dtype=dt16)
        e[:, :r.shape[1]] = r
        return e

    def run(ld, ldt):
        o = torch.zeros(rows, ld, dtype=dt16, device=DEV) if ld else None
        ot = torch.zeros(cols, ldt, dtype=dt16, device=DEV) if ldt else None
        ok("vmc_cast_weight", L.ptr(w_d), L.ptr(o), L.ptr(ot), rows, cols, ld, ldt, L.dt(dt16), L.stream())
        sync()
        if ld:
            assert R.same_bits(o, expect(ref, ld)) and bool((o[:, cols:].cpu().view(torch.int16) == 0).all())
        if ldt:
            assert R.same_bits(ot, expect(ref.t(), ldt)) and bool((ot[:, rows:].cpu().view(torch.int16) == 0).all())
    run(cols, 0)                          # plain
    run(R.kpad(cols), 0)                  # pad_k
    run(0, rows)                          # transposed
    run(0, R.kpad(rows))                  # transposed, padded
    run(R.kpad(cols), R.kpad(rows))       # both copies in one launch
    assert torch.equal(w_d.cpu().view(torch.int32), w.view(torch.int32))
    o = torch.zeros(rows, cols, dtype=dt16, device=DEV)
    assert call("vmc_cast_weight", L.ptr(w_d), None, None, rows, cols, cols, rows, L.dt(dt16), L.stream()) == E_ARG
    assert call("vmc_cast_weight", L.ptr(w_d), L.ptr(o), None, rows, cols, cols - 1, 0, L.dt(dt16), L.stream()) == E_ARG
