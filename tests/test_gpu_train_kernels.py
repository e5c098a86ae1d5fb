"""GPU: the small training-path kernels -- LayerNorm backward family, fused LayerNorm forwards, activations, adds, casts, token
assembly, dropout -- each against a float64 CPU reference of the same operation (tests/train_kernel_refs.py), called through the
C ABI (vimo_clip_amd._lib) so that ldx, add, dy2 and the NULL outputs are reachable.

fp32 outputs must satisfy  max|got - r64| / max|r64| <= 8 max(e32, 2^-23)  with e32 the error of a float32 CPU evaluation of the
same reference on the same inputs; 16-bit outputs  |got - r64| <= ulp16(r64) + that bound x max|r64|  elementwise; purely
elementwise kernels one ulp of their output type.  With VMC_TRAIN_PARITY_JSON=<path> the measured figures of every case are written
there (the case lines of profiles/train_kernel_parity.jsonl were made that way)."""
import json
import os

import numpy as np
import pytest
import torch

import train_kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = R.F32, R.BF16, R.F16
DT16 = [BF16, F16]
DT16_IDS = ["bf16", "f16"]
E_ARG, E_ALIGN, E_SHAPE, E_DTYPE = -1, -2, -3, -4
EPS = R.LN_EPS
SENTINEL = 12345.0

L = None            # vimo_clip_amd._lib, loaded by the module fixture
_REC = []


@pytest.fixture(scope="module", autouse=True)
def _lib_module():
    global L
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vimo_clip_amd import _lib
    L = _lib
    yield
    out = os.environ.get("VMC_TRAIN_PARITY_JSON", "")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps({"margin": R.MARGIN, "floor": R.EPS32}) + "\n")          # then one line per case
            f.writelines(json.dumps(r) + "\n" for r in _REC)


def rec(kernel, case, output, err, e32, bound, unit):
    print(f"{kernel} {case} {output}: err {err:.3e} {unit}, e32 {e32:.3e}, bound {bound:.3e}")
    _REC.append({"kernel": kernel, "case": case, "output": output, "err": err, "e32": e32, "unit": unit,
                 "err_over_yardstick": err / max(e32, R.EPS32) if unit == "rel" else None, "bound": bound})


def ck32(kernel, case, output, got, r64, r32):
    """fp32 output: max|got - r64| / max|r64| <= 8 max(e32, 2^-23)."""
    e32 = R.e32_of(r32, r64)
    assert e32 <= R.E32_MAX
    err = R.max_rel(got, r64)
    rec(kernel, case, output, err, e32, R.bound32(e32), "rel")
    assert err <= R.bound32(e32), f"{kernel} {case} {output}: {err:.3e} > {R.bound32(e32):.3e} (e32 {e32:.3e})"


def ck16(kernel, case, output, got, r64, r32, dtype):
    """16-bit output: |got - r64| <= ulp16(r64) + 8 max(e32, 2^-23) max|r64| for every element."""
    assert got.dtype is dtype
    e32 = R.e32_of(r32, r64)
    assert e32 <= R.E32_MAX
    ex = R.excess16(got, r64, e32, dtype)
    rec(kernel, case, output, ex, e32, 1.0, "of allowed (ulp16 + fp32 bound)")
    assert ex <= 1.0, f"{kernel} {case} {output}: {ex:.3f} x the allowed error"


def ck_ulp(kernel, case, output, got, r64, dtype, ulps=1.0):
    """elementwise kernels: every element within `ulps` spacings of the output type at the float64 value."""
    assert got.dtype is dtype
    off = R.ulps_off(got, r64, dtype)
    rec(kernel, case, output, off, 0.0, ulps, "ulp " + R.DT_NAME[dtype])
    assert off <= ulps, f"{kernel} {case} {output}: {off:.3f} ulp"


def dev(t):
    return None if t is None else t.to(DEV)


def empty(shape, dtype):
    """An output buffer the kernel has to overwrite: NaN everywhere."""
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def sync():
    torch.cuda.synchronize()


def call(name, *args):
    return getattr(L.lib, name)(*args)


def ok(name, *args):
    L.check(call(name, *args), name)


# ================================================================================================ LayerNorm backward
def _ln_fwd(x_d, gamma, beta, rows, D, ld, dt16, y16=None, y32=None, mean=None, rstd=None):
    ok("vmc_layernorm_fwd", L.ptr(x_d), L.ptr(gamma), L.ptr(beta), L.ptr(y16), L.ptr(y32), L.ptr(mean), L.ptr(rstd), rows, D, ld, EPS,
       L.dt(x_d), L.dt(dt16), L.stream())


def _ln_bwd_launch(c, t, x_d, mean, rstd):
    rows, D, dt16 = c["rows"], c["D"], c["dt16"]
    dy, dy2, add, gamma = dev(t["dy"]), dev(t["dy2"]), dev(t["add"]), dev(t["gamma"])
    dx = empty((rows, D), F32 if c["dx"] == "32" else dt16)
    dg, db = empty((D,), F32), empty((D,), F32)
    wsb = call("vmc_layernorm_bwd_workspace_bytes", rows, D)
    assert wsb == min(-(-rows // 4), 512) * 2 * D * 4
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    tail = (rows, D, D + c["pad"], L.dt(dy), L.dt(x_d), L.dt(dx), L.dt(dt16), L.ptr(ws), wsb, L.stream())
    if c["api"] == "bwd":
        assert dy2 is None
        ok("vmc_layernorm_bwd", L.ptr(dy), L.ptr(x_d), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(add), L.ptr(dx), L.ptr(dg), L.ptr(db), *tail)
    else:
        ok("vmc_layernorm_bwd2", L.ptr(dy), L.ptr(dy2), L.ptr(x_d), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(add), L.ptr(dx), L.ptr(dg),
           L.ptr(db), *tail)
    sync()
    return dx, dg, db


@pytest.mark.parametrize("case", R.LN_BWD_CASES, ids=R.ln_bwd_case_id)
def test_layernorm_bwd(case):
    """vmc_layernorm_bwd / vmc_layernorm_bwd2 against float64 autograd through layer_norm (dy_total = dy + dy2, dx_ref = dx + add).
    mean / rstd come from float64 (rounded to f32) unless the case takes them from vmc_layernorm_fwd."""
    c, cid = case, R.ln_bwd_case_id(case)
    rows, D, dt16 = c["rows"], c["D"], c["dt16"]
    t = R.ln_bwd_inputs(c)
    xbuf, _ = R.padded(t["x"], D + c["pad"], SENTINEL)
    x_d = dev(xbuf)
    if c["stats"] == "fwd":
        mean, rstd = empty((rows,), F32), empty((rows,), F32)
        _ln_fwd(x_d, dev(t["gamma"]), dev(torch.zeros(D)), rows, D, D + c["pad"], dt16, y16=empty((rows, D), dt16), mean=mean, rstd=rstd)
    else:
        mean, rstd = (dev(s) for s in R.ln_stats_f32(t["x"]))
    dx, dg, db = _ln_bwd_launch(c, t, x_d, mean, rstd)
    r64, r32 = R.ln_bwd_refs(t, torch.float64), R.ln_bwd_refs(t, torch.float32)
    assert torch.equal(x_d.cpu(), xbuf)
    kernel = "vmc_layernorm_" + c["api"]
    if c["dx"] == "32":
        ck32(kernel, cid, "dx", dx, r64["dx"], r32["dx"])
    else:
        ck16(kernel, cid, "dx", dx, r64["dx"], r32["dx"], dt16)
    ck32(kernel, cid, "dgamma", dg, r64["dgamma"], r32["dgamma"])
    ck32(kernel, cid, "dbeta", db, r64["dbeta"], r32["dbeta"])


def _factors(rows, D, dt16, drops):
    """The factor tensor F the forward applies to the branch: vmc_postnorm_dropout_fwd on x = 0, branch = 1, read from sum_out."""
    (p1, s1), (p2, s2) = drops
    x0, b1 = torch.zeros(rows, D, device=DEV), torch.ones(rows, D, device=DEV, dtype=dt16)
    g, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    F, y16 = empty((rows, D), F32), empty((rows, D), dt16)
    ok("vmc_postnorm_dropout_fwd", L.ptr(x0), L.ptr(b1), L.ptr(g), L.ptr(b), L.ptr(F), None, L.ptr(y16), None, None, rows, D,
       EPS, p1, s1, p2, s2, L.dt(dt16), L.stream())
    sync()
    return F.cpu()


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("drops", R.POSTNORM_DROPS, ids=R.drops_id)
@pytest.mark.parametrize("rows,D,dy_f32,with_dy2", R.POSTNORM_BWD_CASES)
def test_postnorm_bwd(rows, D, dy_f32, with_dy2, drops, dt16):
    """vmc_postnorm_bwd: dsum, dgamma, dbeta against float64 autograd (the drops do not enter them); dbranch16 against r64 F with F read
    from the forward; exactly zero where F is, nonzero where F is not and the value is a normal number of the type."""
    (p1, s1), (p2, s2) = drops
    cid = f"{rows}x{D}-{R.DT_NAME[dt16]}-{R.drops_id(drops)}-dy{'32' if dy_f32 else '16'}{'-dy2' if with_dy2 else ''}"
    t = R.postnorm_bwd_inputs(rows, D, dt16, dy_f32, with_dy2)
    F = _factors(rows, D, dt16, drops)
    mean, rstd = (dev(s) for s in R.ln_stats_f32(t["sum"]))
    dsum, dbr = empty((rows, D), F32), empty((rows, D), dt16)
    dg, db = empty((D,), F32), empty((D,), F32)
    wsb = call("vmc_layernorm_bwd_workspace_bytes", rows, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dy, dy2, ssum, gamma = dev(t["dy"]), dev(t["dy2"]), dev(t["sum"]), dev(t["gamma"])
    ok("vmc_postnorm_bwd", L.ptr(dy), L.ptr(dy2), L.ptr(ssum), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(dsum), L.ptr(dbr),
       L.ptr(dg), L.ptr(db), rows, D, L.dt(dy), p1, s1, p2, s2, L.dt(dt16), L.ptr(ws), wsb, L.stream())
    sync()
    r64 = R.ln_bwd_autograd(t["dy"], t["sum"], t["gamma"], dy2=t["dy2"])
    r32 = R.ln_bwd_autograd(t["dy"], t["sum"], t["gamma"], dy2=t["dy2"], dtype=torch.float32)
    ck32("vmc_postnorm_bwd", cid, "dsum", dsum, r64["dx"], r32["dx"])
    ck32("vmc_postnorm_bwd", cid, "dgamma", dg, r64["dgamma"], r32["dgamma"])       # same reference for every drop setting
    ck32("vmc_postnorm_bwd", cid, "dbeta", db, r64["dbeta"], r32["dbeta"])
    want = r64["dx"] * F.double()
    ck16("vmc_postnorm_bwd", cid, "dbranch16", dbr, want, r32["dx"].double() * F.double(), dt16)
    got = dbr.cpu().double()
    assert bool((got[F == 0] == 0).all())
    live = (F != 0) & (want.abs() > R.smallest_normal(dt16))
    assert bool((got[live] != 0).all())
    if p1 > 0:
        share = (F == 0).double().mean().item()
        assert 0 < share < 1 and (rows * D < 4096 or abs(share - (1 - (1 - p1) * (1 - p2))) < 0.05)
    else:
        assert bool((F == 1).all())


def test_layernorm_bwd_error_codes():
    """Rejected before any launch: unsupported D, ldx < D, a workspace one byte short, a misaligned dbranch16, p2 without p1."""
    rows, D = 8, 256
    z = torch.zeros(rows, 2064, device=DEV)
    v = torch.zeros(2064, device=DEV)
    h = torch.zeros(rows * 2064 + 8, device=DEV, dtype=BF16)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    p = L.ptr

    def bwd(D=D, ldx=None, wsb=None):
        wsb = call("vmc_layernorm_bwd_workspace_bytes", rows, D) if wsb is None else wsb
        return call("vmc_layernorm_bwd", p(h), p(z), p(v), p(v), p(v), None, p(z), p(v), p(v), rows, D, D if ldx is None else ldx, L.BF16, L.F32, L.F32,
                    L.BF16, p(ws), wsb, L.stream())

    def pn(dbr=h.data_ptr(), p1=0.0, p2=0.0, D=D, wsb=None):
        wsb = call("vmc_layernorm_bwd_workspace_bytes", rows, D) if wsb is None else wsb
        return call("vmc_postnorm_bwd", p(h), None, p(z), p(v), p(v), p(v), p(z), dbr, p(v), p(v), rows, D, L.BF16, p1, 1, p2, 2, L.BF16, p(ws), wsb,
                    L.stream())

    assert bwd(D=2052) == E_SHAPE and bwd(D=254) == E_SHAPE and pn(D=2052) == E_SHAPE
    assert bwd(ldx=D - 4) == E_ALIGN and bwd(ldx=D + 2) == E_ALIGN
    need = call("vmc_layernorm_bwd_workspace_bytes", rows, D)
    assert need == 2 * 2 * D * 4 and bwd(wsb=need - 1) == E_ARG and pn(wsb=need - 1) == E_ARG
    assert pn(dbr=h.data_ptr() + 2) == E_ALIGN
    assert pn(p1=0.0, p2=0.2) == E_ARG and pn(p1=1.0) == E_ARG
    assert call("vmc_layernorm_fwd", p(z), p(v), p(v), p(h), None, None, None, rows, 4100, 4100, EPS, L.F32, L.BF16, L.stream()) == E_SHAPE
    sync()
    assert bool((z == 0).all()) and bool((v == 0).all())          # nothing ran


def test_layernorm_fwd_error_codes():
    """The forward LayerNorms, rejected before any launch: a D that is no multiple of 256 or above 2048 (above 4096 for the plain
    forward), ldx < D, an unknown 16-bit type, add+LayerNorm without y16, a second dropout without the first."""
    rows, D, W = 4, 256, 4104                                      # buffers W wide: no D below would leave them if it did launch
    x = torch.zeros(rows, W, device=DEV)
    v = torch.zeros(W, device=DEV)
    h = torch.zeros(rows, W, device=DEV, dtype=BF16)
    y16, y32, st = empty((rows, W), BF16), empty((rows, W), F32), empty((rows,), F32)
    p, S = L.ptr, L.stream

    def add(D=D, ldx=None, y=y16, dt=None):
        return call("vmc_add_layernorm_fwd", p(x), p(h), p(v), p(v), p(y), rows, D, D if ldx is None else ldx, D, EPS, 1, L.BF16 if dt is None else dt, S())

    def add2(D=D, ldx=None, y=y16, dt=None):
        return call("vmc_add2_layernorm_fwd", p(x), p(h), p(h), p(v), p(v), p(y), rows, D, D if ldx is None else ldx, D, D, EPS, 1,
                    L.BF16 if dt is None else dt, S())

    def pn(D=D, p1=0.0, p2=0.0, dt=None):
        return call("vmc_postnorm_dropout_fwd", p(x), p(h), p(v), p(v), None, p(y32), p(y16), p(st), p(st), rows, D, EPS, p1, 1, p2, 2,
                    L.BF16 if dt is None else dt, S())

    def pn0(D=D, dt=None):
        return call("vmc_postnorm_fwd", p(x), p(h), p(v), p(v), None, p(y32), p(y16), p(st), p(st), rows, D, EPS, L.BF16 if dt is None else dt, S())

    def ln(D=D, ldx=None, dt=None):
        return call("vmc_layernorm_fwd", p(x), p(v), p(v), p(y16), p(y32), p(st), p(st), rows, D, D if ldx is None else ldx, EPS, L.F32,
                    L.BF16 if dt is None else dt, S())

    for bad in (260, 2304):
        assert add(D=bad) == E_SHAPE and add2(D=bad) == E_SHAPE and pn(D=bad) == E_SHAPE and pn0(D=bad) == E_SHAPE
    assert ln(D=4100) == E_SHAPE and ln(D=258) == E_SHAPE
    assert add(ldx=D - 4) == E_ALIGN and add2(ldx=D - 4) == E_ALIGN and ln(ldx=D - 4) == E_ALIGN
    assert add(dt=7) == E_DTYPE and add2(dt=7) == E_DTYPE and pn(dt=7) == E_DTYPE and pn0(dt=7) == E_DTYPE and ln(dt=7) == E_DTYPE
    assert add(y=None) == E_ARG and add2(y=None) == E_ARG
    assert pn(p1=0.0, p2=0.2) == E_ARG and pn(p1=1.0) == E_ARG
    assert add(D=260, ldx=256, dt=7) == E_SHAPE and add(ldx=D - 4, dt=7) == E_ALIGN        # the order of the checks: shape, stride, type
    sync()
    for t in (y16, y32, st):
        assert bool(t.isnan().all())                               # nothing ran
    assert bool((x == 0).all())


# ================================================================================================ LayerNorm forwards
@pytest.mark.parametrize("case", R.LN_FWD_CASES, ids=R.ln_fwd_case_id)
def test_layernorm_fwd(case):
    """vmc_layernorm_fwd: y16 / y32 / mean / rstd against float64, x f32 and 16-bit with ldx = D + 8, every NCH instantiation, and
    16387 rows (more than 2048 blocks x 4 waves: waves take a second and a third row through the prefetch)."""
    c, cid = case, R.ln_fwd_case_id(case)
    rows, D, dt16 = c["rows"], c["D"], c["dt16"]
    t = R.ln_fwd_inputs(c)
    xbuf, _ = R.padded(t["x"], D + 8, SENTINEL)
    x_d = dev(xbuf)
    y16 = empty((rows, D), dt16) if c["out"] in ("both", "y16") else None
    y32 = empty((rows, D), F32) if c["out"] in ("both", "y32") else None
    mean, rstd = empty((rows,), F32), empty((rows,), F32)
    _ln_fwd(x_d, dev(t["gamma"]), dev(t["beta"]), rows, D, D + 8, dt16, y16=y16, y32=y32, mean=mean, rstd=rstd)
    sync()
    r64 = R.ln_fwd_ref(t["x"], t["gamma"], t["beta"])
    r32 = R.ln_fwd_ref(t["x"], t["gamma"], t["beta"], dtype=torch.float32)
    assert torch.equal(x_d.cpu(), xbuf)
    if y32 is not None:
        ck32("vmc_layernorm_fwd", cid, "y32", y32, r64["y"], r32["y"])
    if y16 is not None:
        ck16("vmc_layernorm_fwd", cid, "y16", y16, r64["y"], r32["y"], dt16)
    ck32("vmc_layernorm_fwd", cid, "mean", mean, r64["mean"], r32["mean"])
    ck32("vmc_layernorm_fwd", cid, "rstd", rstd, r64["rstd"], r32["rstd"])


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("two", [False, True], ids=["add", "add2"])
@pytest.mark.parametrize("rows,D", R.ADD_LN_SHAPES)
def test_add_layernorm_fwd(rows, D, two, dt16):
    """vmc_add_layernorm_fwd / vmc_add2_layernorm_fwd with ldx, ldb, ldb0 = D + 8: the residual stream becomes the fp32 sum
    (x + b0) + b bit for bit (write_x = 1) or stays untouched (write_x = 0), the gaps keep their sentinel, y16 = LN of that sum."""
    kernel = "vmc_add2_layernorm_fwd" if two else "vmc_add_layernorm_fwd"
    cid = f"{rows}x{D}-{R.DT_NAME[dt16]}"
    t = R.add_ln_inputs(rows, D, dt16, two)
    ld = D + 8
    xbuf, _ = R.padded(t["x"], ld, SENTINEL)
    bbuf, _ = R.padded(t["b"], ld, 7.0)
    b0buf = R.padded(t["b0"], ld, 9.0)[0] if two else None
    s32 = R.add_ln_sum_f32(t)
    r64 = R.ln_fwd_ref(s32, t["gamma"], t["beta"])
    r32 = R.ln_fwd_ref(s32, t["gamma"], t["beta"], dtype=torch.float32)
    gamma, beta = dev(t["gamma"]), dev(t["beta"])
    for write_x in (1, 0):
        x_d, b_d, b0_d = dev(xbuf), dev(bbuf), dev(b0buf)
        y16 = empty((rows, D), dt16)
        if two:
            ok(kernel, L.ptr(x_d), L.ptr(b0_d), L.ptr(b_d), L.ptr(gamma), L.ptr(beta), L.ptr(y16), rows, D, ld, ld, ld, EPS, write_x, L.dt(dt16), L.stream())
        else:
            ok(kernel, L.ptr(x_d), L.ptr(b_d), L.ptr(gamma), L.ptr(beta), L.ptr(y16), rows, D, ld, ld, EPS, write_x, L.dt(dt16), L.stream())
        sync()
        x_after = x_d.cpu()
        want_x = xbuf.clone()
        if write_x:
            want_x[:, :D] = s32
        assert R.same_bits(x_after, want_x), f"{kernel} {cid} write_x={write_x}: residual stream"
        assert torch.equal(b_d.cpu(), bbuf) and (not two or torch.equal(b0_d.cpu(), b0buf))
        ck16(kernel, f"{cid}-write_x{write_x}", "y16", y16, r64["y"], r32["y"], dt16)


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("drops", R.POSTNORM_DROPS, ids=R.drops_id)
@pytest.mark.parametrize("rows,D", R.POSTNORM_SHAPES)
def test_postnorm_dropout_fwd(rows, D, drops, dt16):
    """vmc_postnorm_dropout_fwd: sum_out within 4 fp32 ulps of x + b F (F read from the kernel on x = 0, b = 1; the kernel multiplies
    the two factors in sequence), y32 / y16 / mean / rstd against float64 LayerNorm of that sum; the same with the optional outputs
    absent."""
    (p1, s1), (p2, s2) = drops
    cid = f"{rows}x{D}-{R.DT_NAME[dt16]}-{R.drops_id(drops)}"
    t = R.postnorm_inputs(rows, D, dt16)
    F = _factors(rows, D, dt16, drops)
    f1 = np.float32(1.0) / (np.float32(1.0) - np.float32(p1)) if p1 > 0 else np.float32(1.0)
    f2 = np.float32(1.0) / (np.float32(1.0) - np.float32(p2)) if p2 > 0 else np.float32(1.0)
    assert set(F.unique().tolist()) <= {0.0, float(np.float32(f1 * f2))}      # the f32 quotient(s) 1 / (1 - p), multiplied in sequence
    s64 = t["x"].double() + t["b"].double() * F.double()
    r64 = R.ln_fwd_ref(s64, t["gamma"], t["beta"])
    r32 = R.ln_fwd_ref(s64.float(), t["gamma"], t["beta"], dtype=torch.float32)
    x, b, gamma, beta = dev(t["x"]), dev(t["b"]), dev(t["gamma"]), dev(t["beta"])

    def run(sum_out, y32, y16, mean, rstd):
        ok("vmc_postnorm_dropout_fwd", L.ptr(x), L.ptr(b), L.ptr(gamma), L.ptr(beta), L.ptr(sum_out), L.ptr(y32), L.ptr(y16), L.ptr(mean),
           L.ptr(rstd), rows, D, EPS, p1, s1, p2, s2, L.dt(dt16), L.stream())
        sync()

    so, y32, y16, mean, rstd = empty((rows, D), F32), empty((rows, D), F32), empty((rows, D), dt16), empty((rows,), F32), empty((rows,), F32)
    run(so, y32, y16, mean, rstd)
    off = R.ulps_off(so, s64, F32)
    rec("vmc_postnorm_dropout_fwd", cid, "sum_out", off, 0.0, 4.0, "ulp f32")
    assert off <= 4.0, f"sum_out {off:.2f} ulp"
    assert bool((so.cpu()[F == 0] == t["x"][F == 0]).all())                 # a dropped branch element leaves x exactly
    ck32("vmc_postnorm_dropout_fwd", cid, "y32", y32, r64["y"], r32["y"])
    ck16("vmc_postnorm_dropout_fwd", cid, "y16", y16, r64["y"], r32["y"], dt16)
    ck32("vmc_postnorm_dropout_fwd", cid, "mean", mean, r64["mean"], r32["mean"])
    ck32("vmc_postnorm_dropout_fwd", cid, "rstd", rstd, r64["rstd"], r32["rstd"])
    # optional outputs absent: only y32, then only y16
    y32b = empty((rows, D), F32)
    run(None, y32b, None, None, None)
    ck32("vmc_postnorm_dropout_fwd", cid + "-only-y32", "y32", y32b, r64["y"], r32["y"])
    y16b = empty((rows, D), dt16)
    run(None, None, y16b, None, None)
    ck16("vmc_postnorm_dropout_fwd", cid + "-only-y16", "y16", y16b, r64["y"], r32["y"], dt16)
    assert torch.equal(x.cpu(), t["x"]) and R.same_bits(b.cpu(), t["b"])


# ================================================================================================ activations
@pytest.fixture(scope="module")
def act_big():
    """Inputs of the grid-stride case, built once: 8 x 4096 x 256 + 13 elements, so the loop takes a second pass and ends in the tail."""
    n = R.ACT_N[-1]
    return {dt: (R.act_inputs(n, dt), R.randn((n,), 77, dt)) for dt in DT16}


def _act_io(n, dt16, act_big):
    if n == R.ACT_N[-1]:
        return act_big[dt16]
    return R.act_inputs(n, dt16), R.randn((n,), 77 + n, dt16)


def _act_fwd(x, act, dt16):
    x_d, y = dev(x), empty(tuple(x.shape), dt16)
    ok("vmc_act_fwd", L.ptr(x_d), L.ptr(y), x.numel(), act, L.dt(dt16), L.stream())
    sync()
    return y.cpu()


def _act_bwd(x, dy, act, dt16):
    x_d, dy_d, dx = dev(x), dev(dy), empty(tuple(x.shape), dt16)
    ok("vmc_act_bwd", L.ptr(x_d), L.ptr(dy_d), L.ptr(dx), x.numel(), act, L.dt(dt16), L.stream())
    sync()
    return dx.cpu()


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("n", R.ACT_N)
@pytest.mark.parametrize("act", R.ACTS, ids=["none", "quickgelu", "gelu", "relu"])
def test_act_fwd(act, n, dt16, act_big):
    """vmc_act_fwd: every element within one ulp of the output type of the float64 activation."""
    x, _ = _act_io(n, dt16, act_big)
    y = _act_fwd(x, act, dt16)
    ck_ulp("vmc_act_fwd", f"act{act}-n{n}-{R.DT_NAME[dt16]}", "y", y, R.act_ref(x, act), dt16)
    if act == 0:
        assert R.same_bits(y, x)
    if act == 3:
        assert torch.equal(y, torch.relu(x))


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("n", R.ACT_N)
@pytest.mark.parametrize("act", R.ACTS, ids=["none", "quickgelu", "gelu", "relu"])
def test_act_bwd(act, n, dt16, act_big):
    """vmc_act_bwd: dx = dy act'(x) within one ulp of the output type of the float64 closed form; saturation is exact."""
    x, dy = _act_io(n, dt16, act_big)
    dx = _act_bwd(x, dy, act, dt16)
    ck_ulp("vmc_act_bwd", f"act{act}-n{n}-{R.DT_NAME[dt16]}", "dx", dx, dy.double() * R.act_grad_ref(x, act), dt16)
    xf = x.float()
    if act == 3:            # relu' is 0 or 1, and 0 at 0
        assert torch.equal(dx[xf > 0], dy[xf > 0]) and bool((dx[xf <= 0] == 0).all())
    if act in (1, 2):       # gelu' and quickgelu' at +-100 (and beyond): dy and 0
        assert torch.equal(dx[xf >= 100], dy[xf >= 100]) and bool((dx[xf <= -100] == 0).all())
    if act == 0:
        assert R.same_bits(dx, dy)


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("act", R.ACTS, ids=["none", "quickgelu", "gelu", "relu"])
def test_act_vector_body_and_scalar_tail_agree(act, dt16):
    """The planted values go through the 8-wide body (front of a 1003-element array) and through the scalar tail (arrays of 7): same
    bits -- and both are within one ulp of float64."""
    planted = torch.tensor(R.ACT_PLANTED).to(dt16)
    body_x = R.act_inputs(1003, dt16)
    dy_body = R.randn((1003,), 5, dt16)
    assert R.same_bits(body_x[:12], planted)
    yb, db = _act_fwd(body_x, act, dt16), _act_bwd(body_x, dy_body, act, dt16)
    for lo in (0, 5):
        xt, dyt = planted[lo:lo + 7].clone(), dy_body[lo:lo + 7].clone()
        yt, dt_ = _act_fwd(xt, act, dt16), _act_bwd(xt, dyt, act, dt16)
        ck_ulp("vmc_act_fwd", f"act{act}-tail{lo}-{R.DT_NAME[dt16]}", "y", yt, R.act_ref(xt, act), dt16)
        ck_ulp("vmc_act_bwd", f"act{act}-tail{lo}-{R.DT_NAME[dt16]}", "dx", dt_, dyt.double() * R.act_grad_ref(xt, act), dt16)
        assert R.same_bits(yt, yb[lo:lo + 7]) and R.same_bits(dt_, db[lo:lo + 7])


# ================================================================================================ add, axpby, scale
@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("n", [1, 1001, 4096 * 256 + 77])
def test_add_all_dtype_mixes(n, dt16):
    """vmc_add for the eight mixes of a / b / y width: the float64 sum rounded once -- exact for f32 y, within one ulp16 otherwise."""
    for mix in range(8):
        da, db_, dy_ = (F32 if mix & 1 else dt16), (F32 if mix & 2 else dt16), (F32 if mix & 4 else dt16)
        a, b = R.randn((n,), 51 + mix, da, 3.0), R.randn((n,), 61 + mix, db_, 3.0)
        a_d, b_d, y = dev(a), dev(b), empty((n,), dy_)
        ok("vmc_add", L.ptr(a_d), L.ptr(b_d), L.ptr(y), n, L.dt(da), L.dt(db_), L.dt(dy_), L.dt(dt16), L.stream())
        sync()
        r64 = a.double() + b.double()
        cid = f"n{n}-{R.DT_NAME[da]}+{R.DT_NAME[db_]}->{R.DT_NAME[dy_]}"
        if dy_ is F32:
            assert torch.equal(y.cpu(), r64.float()), cid           # a + b in float64 is exact; one rounding to f32
            rec("vmc_add", cid, "y", 0.0, 0.0, 0.0, "exact")
        else:
            ck_ulp("vmc_add", cid, "y", y.cpu(), r64, dt16)


@pytest.mark.parametrize("n", [1, 1001, 4096 * 256 + 77])
def test_axpby_f32_and_scale_by_device_scalar(n):
    """vmc_axpby_f32 within 2 fp32 ulps of the float64 value (alpha a, beta b and the sum each round; the calls of the autograd layer
    -- (1, alpha) and (alpha, 0) with a = b -- included) on operands of one sign, where ulps of the result mean something, and within 2
    ulps of the larger product where the two terms cancel; vmc_scale_by_device_scalar exact against the fp32 product."""
    a, b = R.randn((n,), 71, F32, 3.0).abs() + 0.25, R.randn((n,), 72, F32, 3.0).abs() + 0.25      # one sign: the sum does not cancel
    a_d, b_d = dev(a), dev(b)
    for (alpha, beta, same) in ((1.0, 0.37, False), (0.37, 0.0, True), (1.25, 0.8, False), (-0.61, 0.0, True)):
        bb, bb_d = (a, a_d) if same else (b, b_d)
        y = empty((n,), F32)
        ok("vmc_axpby_f32", L.ptr(a_d), L.ptr(bb_d), L.ptr(y), n, alpha, beta, L.stream())
        sync()
        r64 = float(np.float32(alpha)) * a.double() + float(np.float32(beta)) * bb.double()
        off = R.ulps_off(y, r64, F32)
        rec("vmc_axpby_f32", f"n{n}-alpha{alpha}-beta{beta}", "y", off, 0.0, 2.0, "ulp f32")
        assert off <= 2.0
    # opposite signs: the sum cancels, so the roundings of alpha a and beta b (half an ulp of the larger product each) no longer scale
    # with the result: within 2 fp32 ulps at the magnitude of the larger of the two products and the result
    nb_d = dev(-b)
    y = empty((n,), F32)
    ok("vmc_axpby_f32", L.ptr(a_d), L.ptr(nb_d), L.ptr(y), n, 1.25, 0.8, L.stream())
    sync()
    pa, pb = float(np.float32(1.25)) * a.double(), float(np.float32(0.8)) * -b.double()
    scale = torch.maximum(torch.maximum(pa.abs(), pb.abs()), (pa + pb).abs())
    off = ((y.cpu().double() - (pa + pb)).abs() / R.ulp(scale, F32)).max().item()
    rec("vmc_axpby_f32", f"n{n}-alpha1.25-beta0.8-cancelling", "y", off, 0.0, 2.0, "ulp f32 of the larger product")
    assert off <= 2.0
    x = R.randn((n,), 73, F32, 3.0)
    for s in (0.125, 1.0 / 3.0, -7.3):
        sc = torch.tensor([s], dtype=F32)
        x_d, sc_d, y = dev(x), dev(sc), empty((n,), F32)
        ok("vmc_scale_by_device_scalar", L.ptr(x_d), L.ptr(y), n, L.ptr(sc_d), L.stream())
        sync()
        want = (x.double() * sc.double()).float()              # the f32 product: one rounding of the exact product
        assert torch.equal(y.cpu(), want) and torch.equal(want, x * sc)
    rec("vmc_scale_by_device_scalar", f"n{n}", "y", 0.0, 0.0, 0.0, "exact")


# ================================================================================================ casts
@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_f32_to_16(n, dt16):
    """vmc_cast_f32_to_16 against tensor.to(dtype) on the CPU, bit for bit (any NaN for NaN): ties both ways, the largest finite
    value, overflow to inf, infinities, NaN, 16-bit and f32 subnormals, in the 4-wide body and in the tail; float64 beside it:
    every finite result is the nearest value of the type."""
    x = R.cast_inputs_f32(n, dt16)
    x_d, y = dev(x), torch.zeros(n, dtype=dt16, device=DEV)
    ok("vmc_cast_f32_to_16", L.ptr(x_d), L.ptr(y), n, L.dt(dt16), L.stream())
    sync()
    y = y.cpu()
    want = x.to(dt16)
    assert bool((torch.isnan(y) == torch.isnan(x)).all())
    fin = torch.isfinite(want)
    r64 = x.double()
    assert bool(((y.double() - r64).abs()[fin] <= R.ulp16(r64, dt16)[fin] / 2).all())         # round to nearest
    rec("vmc_cast_f32_to_16", f"n{n}-{R.DT_NAME[dt16]}", "y", 0.0, 0.0, 0.0, "bits of the CPU cast")
    assert R.same_bits(y, want), f"first difference at {int((y.view(torch.int16) != want.view(torch.int16)).nonzero()[0])}"


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_16_to_f32(n, dt16):
    """vmc_cast_16_to_f32 against tensor.to(float32) on the CPU (and float64: widening is exact), every kind of bit pattern."""
    x = R.cast_inputs_16(n, dt16)
    x_d, y = dev(x), torch.zeros(n, dtype=F32, device=DEV)
    ok("vmc_cast_16_to_f32", L.ptr(x_d), L.ptr(y), n, L.dt(dt16), L.stream())
    sync()
    y = y.cpu()
    assert bool((torch.isnan(y) == torch.isnan(x)).all())
    ok_ = ~torch.isnan(x)
    assert torch.equal(y.double()[ok_], x.double()[ok_])
    assert R.same_bits(y, x.to(F32))
    rec("vmc_cast_16_to_f32", f"n{n}-{R.DT_NAME[dt16]}", "y", 0.0, 0.0, 0.0, "exact")


# ================================================================================================ token assembly, class rows
@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("x_f32", [True, False], ids=["x32", "x16"])
@pytest.mark.parametrize("Fr,N,D", [(3, 5, 64), (2, 50, 768)])
def test_assemble_tokens(Fr, N, D, x_f32, dt16):
    """vmc_assemble_tokens against cat(cls, xp) + pos in float64."""
    xp, cls, pos = R.randn((Fr * (N - 1), D), 81, dt16), R.randn((D,), 82), R.randn((N, D), 83)
    x = empty((Fr, N, D), F32 if x_f32 else dt16)
    xp_d, cls_d, pos_d = dev(xp), dev(cls), dev(pos)
    ok("vmc_assemble_tokens", L.ptr(xp_d), L.ptr(cls_d), L.ptr(pos_d), L.ptr(x), Fr, N, D, L.dt(x), L.dt(dt16), L.stream())
    sync()
    r64 = torch.cat([cls.double().expand(Fr, 1, D), xp.double().view(Fr, N - 1, D)], 1) + pos.double()
    cid = f"{Fr}x{N}x{D}-{R.DT_NAME[dt16]}-{'x32' if x_f32 else 'x16'}"
    if x_f32:
        assert torch.equal(x.cpu(), r64.float()), cid          # one f32 add of two values exact in float64
        rec("vmc_assemble_tokens", cid, "x", 0.0, 0.0, 0.0, "exact")
    else:
        ck_ulp("vmc_assemble_tokens", cid, "x", x.cpu(), r64, dt16)


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("x_f32", [True, False], ids=["x32", "x16"])
def test_set_class_rows(x_f32, dt16):
    """vmc_set_class_rows with row_stride = N D: row 0 of every frame becomes a + b (float64 beside it), every other row keeps its sentinel."""
    Fr, N, D = 3, 5, 68
    a, b = R.randn((D,), 91), R.randn((D,), 92)
    xdt = F32 if x_f32 else dt16
    x = torch.full((Fr, N, D), 3.0, dtype=xdt, device=DEV)
    a_d, b_d = dev(a), dev(b)
    ok("vmc_set_class_rows", L.ptr(x), L.ptr(a_d), L.ptr(b_d), Fr, D, N * D, L.dt(xdt), L.dt(dt16), L.stream())
    sync()
    x = x.cpu()
    r64 = (a.double() + b.double()).expand(Fr, D)
    cid = f"{R.DT_NAME[dt16]}-{'x32' if x_f32 else 'x16'}"
    if x_f32:
        assert torch.equal(x[:, 0], r64.float())
        rec("vmc_set_class_rows", cid, "x", 0.0, 0.0, 0.0, "exact")
    else:
        ck_ulp("vmc_set_class_rows", cid, "x", x[:, 0].contiguous(), r64, dt16)
    assert bool((x[:, 1:] == 3.0).all())
    assert call("vmc_set_class_rows", None, L.ptr(a_d), L.ptr(b_d), Fr, D, N * D, L.dt(xdt), L.dt(dt16), L.stream()) == E_ARG
    x_d = torch.full((Fr, N, D), 3.0, dtype=xdt, device=DEV)
    assert call("vmc_set_class_rows", L.ptr(x_d), L.ptr(a_d), L.ptr(b_d), Fr, D, N * D, L.dt(xdt), L.F32, L.stream()) == E_DTYPE
    sync()
    assert bool((x_d == 3.0).all())                      # a dtype16 that is no 16-bit type launches nothing


# ================================================================================================ dropout masks
def _dropout(x, p, seed, dt16):
    x_d = x if x.is_cuda else dev(x)
    y = torch.empty_like(x_d)
    ok("vmc_dropout", L.ptr(x_d), L.ptr(y), x.numel(), p, seed, L.dt(x), L.dt(dt16), L.stream())
    sync()
    return y.cpu()


def _K(n, p, seed):
    """The canonical mask: vmc_dropout on f32 ones (0 where dropped, the f32 quotient 1 / (1 - p) where kept)."""
    return _dropout(torch.ones(n, device=DEV), p, seed, BF16)


def _cast_dropout2(x_d, n, p1, s1, p2, s2, dt16, y=None):
    y = torch.zeros(n, dtype=dt16, device=DEV) if y is None else y
    ok("vmc_cast_dropout2", L.ptr(x_d), L.ptr(y), n, p1, s1, p2, s2, L.dt(dt16), L.stream())
    sync()
    return y.cpu()


def _kept_check(kernel, cid, got, x, K_list, ps, dtype):
    """got = x through the masks K_list: zero exactly where a mask is zero, x / ((1 - p1)(1 - p2)) within one ulp of `dtype` elsewhere."""
    keep = torch.ones(x.numel(), dtype=torch.bool)
    scale = 1.0
    for K, p in zip(K_list, ps):
        keep &= K != 0
        scale *= R.drop_scale_f64(p)
    got = got.cpu()
    assert bool((got[~keep] == 0).all()), f"{kernel} {cid}: a dropped element is not zero"
    nz = keep & (x.double().abs() * scale > R.smallest_normal(dtype))
    assert bool((got[nz] != 0).all()), f"{kernel} {cid}: a kept element is zero"
    ck_ulp(kernel, cid, "kept", got[keep], x.double()[keep] * scale, dtype)


@pytest.mark.parametrize("p", R.DROP_P)
def test_dropout_canonical_mask(p):
    """K = vmc_dropout on f32 ones: drop share within 5 sigma of p, same seed same mask, other seed other mask, p = 0 identity, a seed
    passed by address (bit 63 | address of a uint64 on the device) = the same value passed plainly, kept value = 1 / (1 - p)."""
    n, seed = R.DROP_N, 20240611
    K = _K(n, p, seed)
    sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert set(K.unique().tolist()) == {0.0, float(sc)}
    share = (K == 0).double().mean().item()
    rec("vmc_dropout", f"K-p{p}", "drop share", abs(share - p), 0.0, R.drop_share_tolerance(p, n), "abs")
    assert abs(share - p) <= R.drop_share_tolerance(p, n)
    ck_ulp("vmc_dropout", f"K-p{p}", "kept", K[K != 0], torch.full((int((K != 0).sum()),), R.drop_scale_f64(p), dtype=torch.float64), F32)
    assert torch.equal(_K(n, p, seed), K)
    other = _K(n, p, seed + 1)
    agree = ((other == 0) == (K == 0)).double().mean().item()
    assert abs(agree - (p * p + (1 - p) * (1 - p))) < 0.01          # independent masks agree where both drop or both keep
    x = R.randn((n,), 5)
    assert torch.equal(_dropout(x, 0.0, seed, BF16), x)
    cell = torch.tensor([seed], dtype=torch.int64, device=DEV)
    assert torch.equal(_K(n, p, (1 << 63) | cell.data_ptr()), K)
    # f32 data through the mask: zero where K is, x / (1 - p) within one f32 ulp plus the rounding of the quotient elsewhere
    y = _dropout(x, p, seed, BF16)
    assert bool((y[K == 0] == 0).all()) and torch.equal(y[K != 0], (x * float(sc))[K != 0])


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("p", R.DROP_P)
def test_dropout_16bit_paths_share_the_canonical_mask(p, dt16):
    """vmc_dropout on 16-bit data, 8-wide (aligned, n % 8 == 0, more elements than one pass of the grid) and scalar (n = 1003; an aligned
    length offset by one element): the mask of K on the same flat index, kept values x / (1 - p) within one ulp."""
    seed = 777
    n8 = 8 * 8192 * 256 + 8
    K = _K(n8, p, seed)
    x = R.randn((n8 + 1,), 6, dt16, 2.0)
    cid = f"p{p}-{R.DT_NAME[dt16]}"
    _kept_check("vmc_dropout", cid + "-8wide", _dropout(x[:n8].contiguous(), p, seed, dt16), x[:n8], [K], [p], dt16)
    _kept_check("vmc_dropout", cid + "-n1003", _dropout(x[:1003].contiguous(), p, seed, dt16), x[:1003], [K[:1003]], [p], dt16)
    xd = dev(x[:4097].contiguous())
    off = xd[1:]                                   # 4096 elements starting 2 bytes past a 16-byte boundary: the scalar kernel
    assert off.data_ptr() % 16 == 2
    y = torch.zeros(4097, dtype=dt16, device=DEV)
    ok("vmc_dropout", L.ptr(off), y.data_ptr() + 2, 4096, p, seed, L.dt(dt16), L.dt(dt16), L.stream())
    sync()
    assert y[0].item() == 0
    _kept_check("vmc_dropout", cid + "-offset", y[1:].cpu(), x[1:4097], [K[:4096]], [p], dt16)


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("two", [False, True], ids=["one-seed", "two-seeds"])
def test_cast_dropout2_shares_the_canonical_masks(two, dt16):
    """vmc_cast_dropout2 (f32 -> 16-bit through one or two masks) reproduces K of each seed on the same flat index: 8-wide body of which
    300 threads take a second pass, then a 5-element scalar tail; n = 1003, and a 4-byte-offset input (unaligned fallback); kept values x / ((1 - p1)(1 - p2)) within
    one ulp against float64."""
    (p1, s1), (p2, s2) = ((0.1, 424242), (0.2, 171717)) if two else ((0.3, 424242), (0.0, 0))
    n = R.CAST_DROPOUT2_N
    K1 = _K(n, p1, s1)
    Ks, ps = ([K1, _K(n, p2, s2)], [p1, p2]) if two else ([K1], [p1])
    if two:
        assert not torch.equal(Ks[0] == 0, Ks[1] == 0)
    x = R.randn((n + 1,), 8, F32, 2.0)
    xd = dev(x)
    cid = f"{'two' if two else 'one'}-{R.DT_NAME[dt16]}"
    _kept_check("vmc_cast_dropout2", cid + "-big", _cast_dropout2(xd, n, p1, s1, p2, s2, dt16), x[:n], Ks, ps, dt16)
    _kept_check("vmc_cast_dropout2", cid + "-n1003", _cast_dropout2(xd, 1003, p1, s1, p2, s2, dt16), x[:1003], [k[:1003] for k in Ks], ps, dt16)
    off = xd[1:4098]
    assert off.data_ptr() % 16 == 4
    _kept_check("vmc_cast_dropout2", cid + "-offset", _cast_dropout2(off, 4097, p1, s1, p2, s2, dt16), x[1:4098], [k[:4097] for k in Ks], ps, dt16)


@pytest.mark.parametrize("dt16", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("drops", R.POSTNORM_DROPS[1:], ids=R.drops_id)
def test_postnorm_masks_are_the_canonical_masks(drops, dt16):
    """The factor tensor of vmc_postnorm_dropout_fwd (to which the forward and backward tests tie their outputs) is the product of the
    canonical masks K of its seeds on the same flat index, and vmc_postnorm_bwd drops exactly there."""
    (p1, s1), (p2, s2) = drops
    rows, D, dy_f32, with_dy2 = R.POSTNORM_MASK_CASE
    assert not with_dy2
    F = _factors(rows, D, dt16, drops).flatten()
    K = _K(rows * D, p1, s1)
    if p2 > 0:
        K = K * _K(rows * D, p2, s2)           # f32 product of the two quotients, as the kernel forms it
    assert torch.equal(F, K)
    t = R.postnorm_bwd_inputs(rows, D, dt16, dy_f32, with_dy2)
    mean, rstd = (dev(s) for s in R.ln_stats_f32(t["sum"]))
    dsum, dbr, dg, db = empty((rows, D), F32), empty((rows, D), dt16), empty((D,), F32), empty((D,), F32)
    wsb = call("vmc_layernorm_bwd_workspace_bytes", rows, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dy, ssum, gamma = dev(t["dy"]), dev(t["sum"]), dev(t["gamma"])
    ok("vmc_postnorm_bwd", L.ptr(dy), None, L.ptr(ssum), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(dsum), L.ptr(dbr),
       L.ptr(dg), L.ptr(db), rows, D, L.dt(dy), p1, s1, p2, s2, L.dt(dt16), L.ptr(ws), wsb, L.stream())
    sync()
    r64 = R.ln_bwd_autograd(t["dy"], t["sum"], t["gamma"])["dx"].flatten()
    got = dbr.cpu().flatten().double()
    assert bool((got[K == 0] == 0).all())
    assert bool((got[(K != 0) & (r64.abs() * K.double() > R.smallest_normal(dt16))] != 0).all())
