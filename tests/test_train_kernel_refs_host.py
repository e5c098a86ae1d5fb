"""CPU: the references of tests/train_kernel_refs.py are themselves right (closed forms against float64 autograd, ulp16 against
torch.nextafter), and every case the GPU tests run has an fp32 yardstick small enough for its bound to mean something."""
import math

import numpy as np
import pytest
import torch

import train_kernel_refs as R


def _close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("rows,D", [(1, 4), (3, 260), (9, 516), (33, 772)])
@pytest.mark.parametrize("extras", [False, True])
def test_layernorm_backward_formula_equals_float64_autograd(rows, D, extras):
    x, dy, gamma = R.randn((rows, D), 1, scale=2.0, shift=30.0 if extras else 0.0), R.randn((rows, D), 2), R.randn((D,), 3, scale=0.5, shift=1.0)
    add = R.randn((rows, D), 4) if extras else None
    dy2 = R.randn((rows, D), 5, R.BF16) if extras else None
    a = R.ln_bwd_autograd(dy, x, gamma, add=add, dy2=dy2)
    f = R.ln_bwd_formula(dy, x, gamma, add=add, dy2=dy2)
    for k in ("dx", "dgamma", "dbeta"):
        assert a[k].dtype == torch.float64 and _close(f[k], a[k]), k


def test_layernorm_forward_reference_equals_torch_layer_norm():
    x, g, b = R.randn((7, 516), 1, scale=2.0), R.randn((516,), 2, scale=0.5, shift=1.0), R.randn((516,), 3)
    r = R.ln_fwd_ref(x, g, b)
    y = torch.nn.functional.layer_norm(x.double(), (516,), g.double(), b.double(), R.LN_EPS)
    assert _close(r["y"], y)
    m32, r32 = R.ln_stats_f32(x)
    assert m32.dtype == torch.float32 and R.max_rel(m32, r["mean"]) <= 2.0 ** -24 and R.max_rel(r32, r["rstd"]) <= 2.0 ** -24


@pytest.mark.parametrize("act", [1, 2, 3])
def test_activation_derivative_equals_float64_autograd(act):
    x = torch.cat([R.randn((4096,), 7, scale=3.0).double(), torch.tensor([1e-3, -1e-3, 8.0, -8.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4]).double()])
    xr = x.clone().requires_grad_(True)
    R.act_ref(xr, act).sum().backward()
    assert _close(R.act_grad_ref(x, act), xr.grad)
    if act == 2:       # the erfc form is torch's own GELU away from the left tail, and keeps its relative accuracy inside it
        m = x > -3
        assert _close(R.act_ref(x, 2)[m], torch.nn.functional.gelu(x)[m])
        assert abs(R.act_ref(torch.tensor([-8.0]), 2).item() / (-8.0 * 6.220960574271785e-16) - 1.0) < 1e-12     # -8 Phi(-8)
    # saturation of the closed forms themselves: below every output type's smallest subnormal at -100, one at +100
    big = torch.tensor([100.0, -100.0, 1e4, -1e4], dtype=torch.float64)
    assert torch.equal(R.act_grad_ref(big, act).float().abs(), torch.tensor([1.0, 0.0, 1.0, 0.0]))
    assert R.act_grad_ref(torch.zeros(1), 3).item() == 0.0


@pytest.mark.parametrize("dtype", R.DT16, ids=["bf16", "f16"])
def test_ulp16_is_the_gap_to_the_next_value(dtype):
    bits = np.arange(0, 0x7C00 if dtype is R.F16 else 0x7F80, dtype=np.int16)      # every finite non-negative value
    v = torch.from_numpy(bits.copy()).view(dtype)
    nxt = torch.nextafter(v, torch.full_like(v, float("inf")))
    gap = nxt.double() - v.double()
    fin = torch.isfinite(nxt)
    assert torch.equal(R.ulp16(v.double(), dtype)[fin], gap[fin])
    assert torch.equal(R.ulp16(-v.double(), dtype)[fin], gap[fin])
    # between two representable values the spacing is that of the lower one; zero and below the subnormals: the subnormal spacing
    mid = v.double() + gap / 2
    assert torch.equal(R.ulp16(mid, dtype)[fin], gap[fin])
    tiny = float(torch.nextafter(torch.zeros(1, dtype=dtype), torch.ones(1, dtype=dtype)).double())
    assert R.ulp16(torch.tensor([0.0, tiny / 4]), dtype).tolist() == [tiny, tiny]
    assert R.smallest_normal(dtype) == float(torch.finfo(dtype).tiny)


def test_error_measures():
    r = torch.tensor([1.0, -4.0], dtype=torch.float64)
    assert R.max_rel(torch.tensor([1.0, -4.0 + 2.0 ** -20]), r) == 2.0 ** -22
    assert R.bound32(0.0) == 8 * 2.0 ** -23 and R.bound32(2.0 ** -20) == 2.0 ** -17
    got = torch.tensor([1.0 + 2.0 ** -7, -4.0], dtype=torch.float64)
    assert R.excess16(got, r, 0.0, R.BF16, elementwise=True) == 1.0          # one bf16 ulp at 1.0
    assert R.excess16(got, r, 0.0, R.BF16) < 1.0
    assert R.ulps_off(torch.tensor([1.0 + 2.0 ** -22]), torch.tensor([1.0], dtype=torch.float64), R.F32) == 2.0


def _assert_yardstick(r64, r32, what):
    for k in r64:
        e = R.e32_of(r32[k], r64[k])
        assert e <= R.E32_MAX, f"{what} {k}: e32 = {e:.3g} > 2^-18"


@pytest.mark.parametrize("case", R.LN_BWD_CASES, ids=R.ln_bwd_case_id)
def test_layernorm_backward_cases_have_a_small_fp32_yardstick(case):
    t = R.ln_bwd_inputs(case)
    _assert_yardstick(R.ln_bwd_refs(t, torch.float64), R.ln_bwd_refs(t, torch.float32), R.ln_bwd_case_id(case))


def test_layernorm_backward_case_list_covers_the_branches_of_the_kernels():
    cs = R.LN_BWD_CASES
    assert {c["D"] for c in cs} >= set(R.LN_BWD_D) and set(R.LN_BWD_D) == {4, 260, 512, 516, 768, 772, 1024, 1028, 2048}
    P = {-(-c["rows"] // 4) for c in cs if c["D"] == 260}
    assert P >= {1, 2, 16, 17, 49, 64, 65}
    assert {2053, 4100, 1, 3} <= {c["rows"] for c in cs}
    assert all(c["rows"] <= 2053 for c in cs if c["D"] == 2048)
    for dt in R.DT16:
        for key, vals in (("dy", ("16", "32")), ("x", ("16", "32")), ("dx", ("16", "32")), ("add", (False, True)), ("dy2", (False, True)),
                          ("api", ("bwd", "bwd2"))):
            assert {c[key] for c in cs if c["dt16"] is dt} >= set(vals), (dt, key)
    assert any(c["stats"] == "fwd" for c in cs) and any(c["shift"] for c in cs) and any(c["pad"] == 8 and c["x"] == "16" for c in cs)


@pytest.mark.parametrize("case", R.LN_FWD_CASES, ids=R.ln_fwd_case_id)
def test_layernorm_forward_cases_have_a_small_fp32_yardstick(case):
    t = R.ln_fwd_inputs(case)
    _assert_yardstick(R.ln_fwd_ref(t["x"], t["gamma"], t["beta"]), R.ln_fwd_ref(t["x"], t["gamma"], t["beta"], dtype=torch.float32),
                      R.ln_fwd_case_id(case))


@pytest.mark.parametrize("rows,D", R.ADD_LN_SHAPES)
@pytest.mark.parametrize("two", [False, True], ids=["add", "add2"])
def test_add_layernorm_cases_have_a_small_fp32_yardstick(rows, D, two):
    for dt in R.DT16:
        t = R.add_ln_inputs(rows, D, dt, two)
        s = R.add_ln_sum_f32(t)
        assert s.dtype == torch.float32
        _assert_yardstick(R.ln_fwd_ref(s, t["gamma"], t["beta"]), R.ln_fwd_ref(s, t["gamma"], t["beta"], dtype=torch.float32), f"{rows}x{D}")


@pytest.mark.parametrize("rows,D", R.POSTNORM_SHAPES)
def test_postnorm_forward_cases_have_a_small_fp32_yardstick(rows, D):
    for dt in R.DT16:
        t = R.postnorm_inputs(rows, D, dt)
        assert bool(((t["x"] >= 0) == (t["b"].float() >= 0)).all())          # no cancellation in x + branch F for any F >= 0
        for F in (1.0, float(np.float32(1.0 / 0.7)), float(np.float32(1 / 0.9) * np.float32(1 / 0.8))):
            s = t["x"].double() + t["b"].double() * F
            _assert_yardstick(R.ln_fwd_ref(s, t["gamma"], t["beta"]), R.ln_fwd_ref(s.float(), t["gamma"], t["beta"], dtype=torch.float32),
                              f"{rows}x{D}")


@pytest.mark.parametrize("rows,D,dy_f32,dy2", R.POSTNORM_BWD_CASES + [R.POSTNORM_MASK_CASE])
def test_postnorm_backward_cases_have_a_small_fp32_yardstick(rows, D, dy_f32, dy2):
    for dt in R.DT16:
        t = R.postnorm_bwd_inputs(rows, D, dt, dy_f32, dy2)
        assert (t["dy"].dtype is torch.float32) == dy_f32 and (t["dy2"] is not None) == dy2
        r64 = R.ln_bwd_autograd(t["dy"], t["sum"], t["gamma"], dy2=t["dy2"])
        r32 = R.ln_bwd_autograd(t["dy"], t["sum"], t["gamma"], dy2=t["dy2"], dtype=torch.float32)
        _assert_yardstick(r64, r32, f"{rows}x{D}")


def test_postnorm_backward_and_cast_dropout2_case_lists_cover_the_branches():
    assert {c[2] for c in R.POSTNORM_BWD_CASES} == {True, False} and {c[3] for c in R.POSTNORM_BWD_CASES} == {True, False}
    assert not R.POSTNORM_MASK_CASE[2]
    n8, threads = R.CAST_DROPOUT2_N // 8, 8192 * 256            # glue.hip: grid_for((n + 7) / 8, 256, 256 * 32) blocks of 256
    assert -(-R.CAST_DROPOUT2_N // 8) > threads and n8 - threads >= 256 and R.CAST_DROPOUT2_N % 8 == 5


def test_input_builders_plant_their_special_values():
    for dt in R.DT16:
        x = R.act_inputs(1003, dt)
        p = torch.tensor(R.ACT_PLANTED).to(dt)
        assert R.same_bits(x[:12], p) and R.same_bits(x[-12:], p.flip(0))       # signed zeros kept
        c = R.cast_inputs_f32(1001, dt)
        s = R.cast_specials_f32(dt)
        assert R.same_bits(c[:len(s)], s) and R.same_bits(c[-len(s):], s.flip(0))
        assert torch.isnan(c).sum() == 2 and torch.isinf(c).sum() == 4
        lo = c.to(dt)
        assert lo[0].item() == 1.0 and lo[1].double().item() == 1.0 + 4 * 2.0 ** -(R._MANT[dt] + 1)      # ties go to even
        h = R.cast_inputs_16(1001, dt)
        assert h.dtype is dt and torch.isnan(h).any() and torch.isinf(h).any()
    assert R.same_bits(torch.tensor([0.0, float("nan")]), torch.tensor([0.0, float("nan")]))
    assert not R.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))


@pytest.mark.parametrize("p", R.DROP_P)
def test_fp32_dropout_scale_is_within_one_ulp(p):
    """The kernels scale kept values by the f32 quotient 1 / (1 - p): on ones, that is within one f32 ulp of the exact quotient."""
    sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    r = torch.tensor([R.drop_scale_f64(p)], dtype=torch.float64)
    assert R.ulps_off(torch.tensor([float(sc)], dtype=torch.float64), r, R.F32) <= 1.0
    assert R.drop_share_tolerance(p, R.DROP_N) == 5 * math.sqrt(p * (1 - p) / 2 ** 20)
