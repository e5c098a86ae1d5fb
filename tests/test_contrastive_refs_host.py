"""CPU: the references of tests/contrastive_refs.py are what they claim to be -- the unrounded float64 model equals torch autograd of the
logsumexp form, the mask means what the definition says, the degenerate inputs behave, every case keeps its fp32 yardstick below
2^-18 and its loss above the floor, the inputs are decided -- and the public function's argument errors fire before anything is
launched.  No GPU."""
import math

import pytest
import torch

import contrastive_refs as R
from contrastive_refs import BF16, DT16, E32_MAX, EPS32, F16, F32, F64, MARGIN


def _rows(B, T, E):
    s, buf = R.loss_inputs(B, T, E)
    return s.view(B * T, E), buf[:, :T].reshape(B * T, E)


@pytest.mark.parametrize("shape", R.LOSS_SHAPES + R.FLOOR_ONLY_SHAPES)
@pytest.mark.parametrize("mask", [True, False])
def test_unrounded_model_equals_autograd_of_the_logsumexp_form(shape, mask):
    B, T, E = shape
    s, t = _rows(B, T, E)
    r = R.loss_exact(s, t, T, mask=mask)
    loss, ds = R.loss_autograd(s, t, T, mask=mask)
    floor = max(ds.abs().max().item(), 1e-300)
    assert abs(float(r["loss"]) - float(loss)) <= 1e-10 * max(abs(float(loss)), 1.0)
    assert (r["ds"] - ds).abs().max().item() <= 1e-10 * floor, (shape, mask)


def test_mask_keeps_the_diagonal_and_drops_the_rest_of_the_clip():
    V = R.valid_mask(6, 2)
    assert V.diagonal().all() and not V[0, 1] and not V[3, 2] and V[0, 2] and V[5, 0]
    assert int(V.sum()) == 6 * 6 - 6 * 1
    assert R.valid_mask(6, 0).all() and torch.equal(R.valid_mask(6, 1), R.valid_mask(6, 0))
    assert torch.equal(R.valid_mask(5, 5), torch.eye(5, dtype=torch.bool))
    V = R.valid_mask(7, 5)                                         # a last clip that is not full
    assert not V[5, 6] and V[4, 5] and not V[0, 4]
    # a masked logit does not reach the loss: changing it changes nothing
    z = R.softmax_inputs(5, "tau").clone()
    a = R.softmax_ref(z, 2)
    z[0, 1], z[3, 2] = 50.0, -50.0
    b = R.softmax_ref(z, 2)
    assert float(a["loss"]) == float(b["loss"]) and torch.equal(a["dz"], b["dz"]) and b["dz"][0, 1] == 0 and b["dz"][3, 2] == 0


@pytest.mark.parametrize("dtype16", [None, BF16, F16])
def test_one_clip_gives_zero_loss_and_zero_gradient(dtype16):
    s, t = _rows(1, 65, 64)
    r = R.loss_exact(s, t, 65, dtype16=dtype16)
    assert float(r["loss"]) == 0.0 and not r["ds"].any() and r["top1"] == 65
    assert float(R.loss_exact(s, t, 65, dtype16=dtype16, mask=False)["loss"]) > R.LOSS_FLOOR


def test_zero_and_tiny_student_rows_give_a_finite_large_gradient():
    s, t = _rows(3, 5, 64)
    s = s.clone()
    s[1] = 0.0
    s[4] = s[4] / s[4].double().norm().float() * 1e-7
    r = R.loss_exact(s, t, 5)
    loss, ds = R.loss_autograd(s, t, 5)
    assert torch.isfinite(r["ds"]).all() and math.isfinite(float(r["loss"]))
    assert (r["ds"] - ds).abs().max().item() <= 1e-10 * ds.abs().max().item()
    assert r["ds"][1].abs().max().item() > 100 * r["ds"][0].abs().max().item()          # du / eps
    assert list(R.clamp_rows(s).nonzero().flatten()) == [1, 4]


@pytest.mark.parametrize("shape", R.LOSS_SHAPES)
@pytest.mark.parametrize("dtype16", DT16)
def test_composed_cases_keep_their_yardsticks_floor_and_margins(shape, dtype16):
    B, T, E = shape
    s, t = _rows(B, T, E)
    assert not R.undecided(s).any() and not R.undecided(t).any()
    for mask in (True, False):
        if B == 1 and mask:
            continue                                               # the exact-zero case: nothing to bound
        r, allow_loss, allow_ds, y = R.loss_bounds(s, t, T, dtype16, mask=mask)
        print(f"{shape} {R.DT_NAME[dtype16]} mask {mask}: loss {float(r['loss']):.4f} e32 z {y['e32_z']:.2e} du {y['e32_du']:.2e} "
              f"n {y['e32_n']:.2e} flippable {y['flips']} allow loss {allow_loss:.2e} "
              f"ds {(allow_ds.max() / r['ds'].abs().max()).item():.2e} of max|ds| top1 margin {y['top1_margin']:.2e}")
        assert max(y["e32_z"], y["e32_du"], y["e32_n"]) <= E32_MAX
        assert float(r["loss"]) >= R.LOSS_FLOOR
        assert allow_loss <= 1e-3 * float(r["loss"])                                   # a relative bound that means something
        assert (allow_ds.max() / r["ds"].abs().max()).item() <= 2e-2
        assert y["top1_margin"] > 2 * y["e_z"]
        # the cap the flip term must stay under: every entry of a row off by the spacing at 2
        cap = R.ulp16(torch.tensor([2.0], dtype=F64), dtype16).item() * r["v16"].abs().max(1).values.sum().item() / (2 * B * T * R.TAU)
        flips = torch.where(R.tie_distance(r["dz"], dtype16) <= 1.0, R.ulp16(r["dz"], dtype16), torch.zeros_like(r["dz"]))
        assert ((flips @ r["v16"].abs()) / (2 * B * T * R.TAU)).max().item() <= cap


def test_the_small_case_is_below_the_floor():
    s, t = _rows(2, 1, 64)
    assert float(R.loss_exact(s, t, 1)["loss"]) < R.LOSS_FLOOR


@pytest.mark.parametrize("M,E", [(M, E) for M in R.PREP_M for E in R.PREP_E])
def test_prep_inputs_are_decided_and_within_the_yardstick(M, E):
    s, t = R.prep_inputs(M, E)
    assert not R.undecided(s).any() and not R.undecided(t).any()
    r64, r32 = R.prep_ref(s, t), R.prep_ref(s, t, F32)
    free = ~R.clamp_rows(s)
    for k in ("u", "v"):
        assert R.e32_of(r32[k], r64[k]) <= E32_MAX
    if free.any():
        assert R.e32_of(r32["inv_s"][free], r64["inv_s"][free]) <= E32_MAX
    if M >= 63:
        assert list((~free).nonzero().flatten()) == [1, 2] and not r64["u"][2].any() and not r64["v"][3].any()
        assert abs(r64["u"][1].norm().item() - 1e-7 / R.EPS) < 1e-6


@pytest.mark.parametrize("M,T,kind", R.SOFTMAX_CASES)
def test_softmax_cases_keep_their_yardstick(M, T, kind):
    z = R.softmax_inputs(M, kind)
    r64, r32 = R.softmax_ref(z, T), R.softmax_ref(z, T, F32)
    for k in ("lse_row", "lse_col"):
        assert R.e32_of(r32[k], r64[k]) <= E32_MAX
    assert torch.isfinite(r64["dz"]).all() and r64["dz"].abs().max().item() <= 2.0
    assert abs(float(r64["dz"].sum())) <= 1e-9 * M                     # rows of p_row and columns of p_col sum to 1 each
    if kind == "80":
        assert 0 < r64["dz"].diagonal()[::3].abs().max().item() < 1e-5                 # p_row_ii and p_col_ii next to 1
        assert (z.max() - z.min()).item() == 160.0


@pytest.mark.parametrize("M,E", R.NORM_BWD_CASES)
def test_norm_bwd_reference_is_the_gradient_of_the_normalisation(M, E):
    s, du = R.norm_bwd_inputs(M, E)
    sr = s.to(F64).clone().requires_grad_(True)
    u = sr / sr.norm(dim=-1, keepdim=True).clamp(min=R.EPS)
    u.backward(du.to(F64))
    r64 = R.norm_bwd_ref(du, s)
    assert (r64 - sr.grad).abs().max().item() <= 1e-10 * r64.abs().max().item()
    free = ~R.clamp_rows(s)
    assert R.e32_of(R.norm_bwd_ref(du, s, F32)[free], r64[free]) <= E32_MAX


# ---------------------------------------------------------------------------------------------- the public function's argument errors
def test_unknown_mode_keeps_its_message():
    from vimo_clip_amd.losses import distillation_loss
    x = torch.zeros(2, 3, 64)
    with pytest.raises(ValueError, match=r"^Unsupported mode 'bogus'\. Choose 'mse' or 'cosine'\.$"):
        distillation_loss(x, x, mode="bogus")
    with pytest.raises(ValueError, match=r"^Unsupported mode 'bogus'\. Choose 'mse' or 'cosine'\.$"):
        distillation_loss(x, x, mode="bogus", temperature=0.1, compute_dtype=torch.float16, mask_same_clip=False, return_top1=True)


def test_contrastive_rejects_a_temperature_that_is_not_positive():
    """Fails on a tree without the mode: there "contrastive" is an unknown mode (or the keyword an unknown argument)."""
    from vimo_clip_amd.losses import distillation_loss
    x = torch.zeros(2, 3, 64)
    for bad in (0, 0.0, -0.07, float("nan")):
        with pytest.raises(ValueError, match="temperature must be positive"):
            distillation_loss(x, x, mode="contrastive", temperature=bad)


def test_contrastive_argument_errors_fire_before_any_launch():
    """Host tensors: a launch (or even a pointer lookup) would raise RuntimeError, never ValueError."""
    from vimo_clip_amd.losses import CONTRASTIVE_MAX_ROWS, distillation_loss
    x = torch.zeros(2, 3, 64)
    for bad in (torch.float32, torch.float64, torch.int16, None):
        with pytest.raises(ValueError, match="compute_dtype must be"):
            distillation_loss(x, x, mode="contrastive", compute_dtype=bad)
    with pytest.raises(ValueError, match="multiple of 64"):
        distillation_loss(torch.zeros(2, 3, 96), torch.zeros(2, 3, 96), mode="contrastive")
    with pytest.raises(ValueError, match="multiple of 64"):
        distillation_loss(torch.zeros(4, 32), torch.zeros(4, 32), mode="contrastive")
    with pytest.raises(ValueError, match="rows"):
        distillation_loss(torch.zeros(0, 3, 64), torch.zeros(0, 3, 64), mode="contrastive")
    big = torch.zeros(1, 64).expand(CONTRASTIVE_MAX_ROWS + 1, 64)
    with pytest.raises(ValueError, match="rows"):
        distillation_loss(big, big, mode="contrastive")
    with pytest.raises(ValueError, match=r"\[B, T, E\] or \[M, E\]"):
        distillation_loss(torch.zeros(2, 2, 3, 64), torch.zeros(2, 2, 3, 64), mode="contrastive")
