"""CPU checks of tests/student_step_refs.py: the float64 step against float64 autograd through oracle/vit.py and oracle/student.py
and its attention against attention_refs' closed forms, the conditions that make the measure mean something (for every case, dtype
and level), the measure on a float32 evaluation of the model, and ten mutants of that evaluation that it must catch."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_refs as AR                      # noqa: E402
import student_step_refs as R                    # noqa: E402
from oracle import student as ostudent           # noqa: E402
from oracle import vit as ovit                   # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16      # noqa: E402

F64 = torch.float64
DTYPES = (BF16, F16)
CONFIGS = [(c["name"], dt) for c in R.CASES for dt in DTYPES]
CFG_ID = lambda v: v if isinstance(v, str) else DT_NAME[v]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _oracle_sd(inp, prefix=""):
    """The oracle's state dict in float64 on the values the kernels see (16-bit weight copies widened, fp32 everything else)."""
    sd = {}
    for n in R.param_shapes(inp["case"]):
        src = inp["w16"][n] if n in inp["w16"] else inp["p32"][n]
        sd[(prefix if n not in R.HEAD_PARAMS else "") + n] = src.to(F64).clone().requires_grad_(True)
    return sd


@pytest.mark.parametrize("name", ["a", "b", "d", "g"])
def test_tower_ref64_is_float64_autograd_through_the_oracle(name):
    """Embeddings and the gradient of every VisionTransformer parameter to 1e-12 relative (cls_only or not: the same function)."""
    inp, r = R.make_inputs(name, BF16), R.step_ref64(name, BF16)
    sd = _oracle_sd(inp)
    pix = ovit.normalize_u8(ovit.to_pil_wrap_u8(inp["frames"]), F64)
    emb = ovit.vit_forward(sd, pix, R.HEADS, dtype=F64)
    emb.backward(inp["up"]["E"].to(F64))
    assert _rel(r["E"], emb.detach()) <= 1e-12
    checked = 0
    for n in R.param_shapes(inp["case"]):
        assert sd[n].grad is not None and _rel(r["g." + n], sd[n].grad) <= 1e-12, n
        checked += 1
    assert checked == 5 + 12 * R.LAYERS + 3 == len([k for k in R.tensor_names(r) if k.startswith("g.")])


@pytest.mark.parametrize("name", ["s1", "s2"])
def test_student_ref64_is_float64_autograd_through_the_oracle(name):
    """The three outputs and every gradient, the heads' included; the three upstream gradients meet at the embeddings."""
    inp, r = R.make_inputs(name, BF16), R.step_ref64(name, BF16)
    c = inp["case"]
    sd = _oracle_sd(inp, "visual_encoder.")
    vids = inp["frames"].reshape(c["B"], c["T"], 3, c["R"], c["R"])
    outs = ostudent.student_forward(sd, vids, R.HEADS, alpha=R.ALPHA, wrap_quirk=True, dtype=F64)
    names = ("emb", "emb_distill", "logits")
    torch.autograd.backward(list(outs), [inp["up"][n].to(F64).reshape(o.shape) for n, o in zip(names, outs)])
    for n, o in zip(names, outs):
        assert _rel(r[n], o.detach().reshape(r[n].shape)) <= 1e-12, n
    for n in R.param_shapes(c):
        g = sd[(("visual_encoder." if n not in R.HEAD_PARAMS else "") + n)].grad
        assert g is not None and _rel(r["g." + n], g) <= 1e-12, n
    assert len([k for k in R.tensor_names(r) if k.startswith("g.")]) == 5 + 12 * R.LAYERS + 3 + 8


@pytest.mark.parametrize("F,N", [(3, 17), (2, 65)])
def test_attention_piece_is_attention_refs_closed_form(F, N):
    """The reference's attention under float64 autograd equals attn_ref64's out, dq, dk, dv on a packed qkv."""
    D = R.WIDTH
    qkv16 = AR.vit_random(F, N, R.HEADS, BF16, 5)
    dout = torch.randn(F * N, D, generator=torch.Generator().manual_seed(6)).to(BF16)
    qkv = qkv16.to(F64).requires_grad_(True)
    out = R.attn_plain(qkv, F, N)
    out.backward(dout.to(F64))
    q, k, v = AR.vit_split(qkv16, R.HEADS)
    ref = AR.attn_ref64(q, k, v, None, dout, shape=(F, R.HEADS, N, N, 64))
    assert _rel(out.detach(), ref["out"]) <= 1e-12
    for i, n in enumerate(("dq", "dk", "dv")):
        assert _rel(qkv.grad[:, i * D:(i + 1) * D], ref[n]) <= 1e-12, n


def test_cases_reach_the_kernels_they_are_listed_for():
    """attn_route.h through attention_refs' port: the forward configuration and the backward kernel of every token count."""
    want = {"a": (17, 7, AR.BM), "b": (50, 6, AR.BM), "c": (65, 9, AR.BM), "d": (197, 5, AR.BM), "e": (257, 0, AR.BM), "f": (577, 577, AR.LB)}
    for name, (N, inst, bwd) in want.items():
        c = R.BY_NAME[name]
        assert c["N"] == N
        kern, got_inst, _ = AR.route_vit(N, N, c["F"], R.HEADS)
        assert (kern, got_inst) == (("ATTN_VIT", inst) if N <= 288 else ("ATTN_VIT_LONG", 577))
        assert AR.route_bwd(N, N, 64)[0] == bwd
        assert AR.bwd_family_of({"bwd": bwd}) is AR.FAM_LDS
    assert [c["name"] for c in R.CASES if c["parks_stream"]] == ["i"] and [c["name"] for c in R.CASES if c["parks_conv1"]] == ["s2"]
    assert not R.BY_NAME["h"]["arena"]
    assert [R.BY_NAME[n]["K"] % 64 for n in "abcdef"] == [0, 0, 0, 48, 48, 48] and R.BY_NAME["d"]["E"] % 64 and R.BY_NAME["f"]["E"] % 64


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_inputs_make_the_measure_mean_something(name, dtype):
    """From the two references alone: 2 rms(E) <= 0.1 rms(r64) for every tensor; 4 max|E| <= 0.25 rms(r64) for every f16 tensor and
    for at least three quarters of the bf16 tensors; attention not trivially uniform; the head's ReLU populated on both sides and off
    its edge; f16 gradients inside f16's range."""
    inp, r, m = R.make_inputs(name, dtype), R.step_ref64(name, dtype), R.step_model16(name, dtype)
    c = inp["case"]
    bad_rms, bad_max = R.vacuity(r, m)
    n = len(R.tensor_names(r))
    print(f"{name} {DT_NAME[dtype]}: {n} tensors, stress {inp['stress']}, max condition missed by {bad_max}")
    assert n == (1 if c["level"] == "tower" else 3) + 5 + 12 * R.LAYERS + 3 + (8 if c["level"] == "student" else 0)
    assert not bad_rms, bad_rms
    if dtype == F16:
        assert not bad_max, bad_max
    else:
        assert 4 * len(bad_max) <= n, bad_max
    assert len(r["attn_peak"]) == R.LAYERS and min(r["attn_peak"]) >= 4.0 / c["N"], r["attn_peak"]
    if c["level"] == "student":
        for o in (r, m):
            assert 0.02 <= o["relu_negative_share"] <= 0.98 and o["relu_min_abs"] >= 0.02, (o["relu_negative_share"], o["relu_min_abs"])
        assert inp["relu_margin"] >= 0.02
    assert R.UP_SCALE[BF16] == 1.0 and math.log2(R.UP_SCALE[F16]) == round(math.log2(R.UP_SCALE[F16]))      # a power of two
    assert max(float(u.abs().max()) for u in inp["up"].values()) <= 8 * R.UP_SCALE[dtype]                   # N(0, 1) times it
    if dtype == F16:
        assert m["stored"]
        for tag, (mx, sub) in m["stored"].items():
            assert mx <= 2.0 ** 14 and sub < 0.01, (tag, mx, sub)
    for k in R.tensor_names(r):
        assert torch.isfinite(r[k]).all() and torch.isfinite(m[k]).all() and float(r[k].abs().max()) > 0, k


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_measure_passes_a_float32_evaluation_of_the_model(name, dtype):
    r, m = R.step_ref64(name, dtype), R.step_model16(name, dtype)
    ms, bad = R.check(R.step_eval32(name, dtype), r, m)
    assert len(ms) == len(R.tensor_names(r))
    print(f"{name} {DT_NAME[dtype]}: float32 self-evaluation, worst rms ratio {max(x['ratio_rms'] for x in ms):.3f}, "
          f"worst max ratio {max(x['ratio_max'] for x in ms):.3f}")
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_measure_catches_the_mutants(mutant, dtype):
    """Each wrong step fails the case named for it, in both dtypes."""
    name = R.MUTANT_CASE[mutant]
    r, m = R.step_ref64(name, dtype), R.step_model16(name, dtype)
    _, bad = R.check(R.step_eval32(name, dtype, bug=mutant), r, m)
    print(f"{mutant} on case {name} {DT_NAME[dtype]}: {len(bad)} tensors fail, e.g. {bad[:2]}")
    assert bad, f"{mutant} passes case {name} in {DT_NAME[dtype]}"
