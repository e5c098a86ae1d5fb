"""CPU checks of tests/tfam_chain_refs.py: the float64 step against float64 autograd through oracle/tfam.py and against
attention_refs' closed forms, the CPU dropout masks, the conditions that make the measure mean something (for every case, dtype and
dropout setting), the measure on a float32 evaluation of the model, and eight mutants of that evaluation that it must catch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_refs as AR                      # noqa: E402
import tfam_chain_refs as R                      # noqa: E402
from oracle import tfam as otfam                 # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16, drop_share_tolerance      # noqa: E402

F64 = torch.float64
DTYPES = (BF16, F16)
CONFIGS = [(c["name"], dt, drop) for c in R.CASES for dt in DTYPES for drop in R.DROPS]
CFG_ID = lambda v: v if isinstance(v, str) else (DT_NAME[v] if isinstance(v, torch.dtype) else f"p{v[0]}")


def _oracle_sd(inp):
    """The oracle's state dict in float64 on the values the kernels see (16-bit weight copies widened, fp32 everything else)."""
    val = lambda n: (inp["w16"][n] if n in inp["w16"] else inp["p32"][n]).to(F64).clone().requires_grad_(True)
    return {theirs: val(mine) for mine, theirs in _pairs(inp["case"])}


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", ["a", "c", "e", "f", "g1", "g2"])
def test_ref64_is_float64_autograd_through_the_oracle(name):
    """Dropout 0, every mode the oracle has: logits, every parameter gradient and the token gradients to 1e-12 relative."""
    drop = R.DROPS[0]
    inp, r = R.make_inputs(name, BF16, drop), R.chain_ref64(name, BF16, drop)
    c = inp["case"]
    B, T, Tk, D = c["B"], c["T"], c["Tk"], c["D"]
    sd = _oracle_sd(inp)
    leaf = lambda t: t.to(F64).clone().requires_grad_(True)
    if c["mode"] == "feature":
        xc = inp["xcat"].reshape(B, T, 2 * D)
        rgb = leaf(torch.cat([xc[..., :D], torch.zeros(B, 1, D)], 1))
        mot = leaf(xc[..., D:])
        kw = dict(mask_rgb=torch.ones(B, T + 1, dtype=torch.bool), mask_flow=inp["mask"], use_cross_attention=False, concat_dim=-1)
    else:
        rgb = leaf(inp["x"].reshape(B, T, D))
        mot = leaf(inp["motion"].reshape(B, Tk, D)) if Tk else torch.zeros(B, 1, D, dtype=F64)
        kw = dict(mask_rgb=inp["mask"], mask_flow=inp["mask_kv"], use_cross_attention=c["mode"] == "cross", use_only_rgb=c["mode"] == "self")
    logits = otfam.amo_clip_forward(sd, rgb, mot, nhead=c["H"], **kw)
    logits.backward(inp["dlogits"].to(F64))
    assert _rel(r["logits"], logits.detach()) <= 1e-12
    if c["mode"] == "feature":
        want = torch.cat([rgb.grad[:, :T], mot.grad], -1).reshape(B * T, 2 * D)
        assert _rel(r["dXcat"], want) <= 1e-12
    else:
        assert _rel(r["dX"], rgb.grad.reshape(B * T, D)) <= 1e-12
        if Tk:
            assert _rel(r["dMotion"], mot.grad.reshape(B * Tk, D)) <= 1e-12
    names = {"g." + mine: theirs for mine, theirs in _pairs(c)}
    checked = 0
    for k in R.tensor_names(r):
        if k.startswith("g."):
            g = sd[names[k]].grad
            assert g is not None and _rel(r[k], g) <= 1e-12, k
            checked += 1
    assert checked == len([k for k in r if k.startswith("g.")]) and checked >= 17


def _pairs(c):
    out = []
    for l in range(c["L"]):
        for mine, theirs in (("w_self_in", "self_attn.in_proj_weight"), ("b_self_in", "self_attn.in_proj_bias"),
                             ("w_self_out", "self_attn.out_proj.weight"), ("b_self_out", "self_attn.out_proj.bias"),
                             ("w_cross_in", "cross_attn.in_proj_weight"), ("b_cross_in", "cross_attn.in_proj_bias"),
                             ("w_cross_out", "cross_attn.out_proj.weight"), ("b_cross_out", "cross_attn.out_proj.bias"),
                             ("w_ffn0", "ffn.0.weight"), ("b_ffn0", "ffn.0.bias"), ("w_ffn3", "ffn.3.weight"), ("b_ffn3", "ffn.3.bias"),
                             ("ln_self_g", "norm_self.weight"), ("ln_self_b", "norm_self.bias"), ("ln_cross_g", "norm_cross.weight"),
                             ("ln_cross_b", "norm_cross.bias"), ("ln_ffn_g", "norm_ffn.weight"), ("ln_ffn_b", "norm_ffn.bias")):
            out.append((f"L{l}.{mine}", f"layers.{l}.{theirs}"))
    out += [("head.cls_ln_g", "classifier.0.weight"), ("head.cls_ln_b", "classifier.0.bias"), ("head.w_cls1", "classifier.1.weight"),
            ("head.b_cls1", "classifier.1.bias"), ("head.w_cls4", "classifier.4.weight"), ("head.b_cls4", "classifier.4.bias"),
            ("proj.w_proj", "projection_layer.weight"), ("proj.b_proj", "projection_layer.bias")]
    return out


@pytest.mark.parametrize("shape,p", [((2, 8, 16, 15, 64), 0.0), ((2, 8, 20, 50, 96), 0.1), ((3, 8, 16, 16, 64), 0.1)])
def test_attention_piece_is_attention_refs_closed_form(shape, p):
    """The reference's attention under float64 autograd equals attn_ref64's out, dq, dk, dv (key mask, dropout on the probabilities)."""
    B, H, Tq, Tk, dh = shape
    mask = R.key_mask(B, Tk, 5)
    t = AR.random_inputs(shape, BF16, 31, mask=mask)
    fac = AR.dropout_fac(p, 1234567, B, H, Tq, Tk) if p > 0 else None
    q, k, v = (t[n].to(F64).requires_grad_(True) for n in ("q", "k", "v"))
    out = R._attn_plain(q, k, v, mask, fac, shape)
    out.backward(t["dout"].to(F64))
    ref = AR.attn_ref64(t["q"], t["k"], t["v"], mask, t["dout"], fac, shape=shape)
    for got, n in ((out.detach(), "out"), (q.grad, "dq"), (k.grad, "dk"), (v.grad, "dv")):
        assert _rel(got, ref[n]) <= 1e-12, n


@pytest.mark.parametrize("p", [R.P_DROP, R.P_MLP])
def test_cpu_masks_are_deterministic_and_drop_the_stated_share(p):
    M, N = 48, 512
    a, b = R.fac2d(p, 991, M, N), R.fac2d(p, 991, M, N)
    assert torch.equal(a, b) and not torch.equal(a, R.fac2d(p, 992, M, N))
    assert set(a.unique().tolist()) == {0.0, R.inv_keep(p)}
    assert abs(float((a == 0).double().mean()) - p) <= drop_share_tolerance(p, M * N)
    f = AR.dropout_fac(p, 991, 3, 8, 16, 15)
    assert abs(float((f == 0).double().mean()) - p) <= drop_share_tolerance(p, f.numel())
    assert R.fac2d(0.0, 991, M, N) is None


@pytest.mark.parametrize("name,dtype,drop", CONFIGS, ids=CFG_ID)
def test_inputs_make_the_measure_mean_something(name, dtype, drop):
    """From the two references alone: 2 rms(E) <= 0.1 rms(r64) for every tensor; 4 max|E| <= 0.25 rms(r64) for every f16 tensor and
    for at least three quarters of the bf16 tensors; ReLU populated on both sides and off its edge; f16 gradients inside f16's range."""
    r, m = R.chain_ref64(name, dtype, drop), R.chain_model16(name, dtype, drop)
    bad_rms, bad_max = R.vacuity(r, m)
    n = len(R.tensor_names(r))
    print(f"{name} {DT_NAME[dtype]} p{drop[0]}: {n} tensors, max condition missed by {bad_max}")
    assert not bad_rms, bad_rms
    if dtype == F16:
        assert not bad_max, bad_max
    else:
        assert 4 * len(bad_max) <= n, bad_max
    assert all(0.02 <= s <= 0.98 for s in r["relu_negative_share"]), r["relu_negative_share"]
    assert all(0.02 <= s <= 0.98 for s in m["relu_negative_share"])
    assert min(R.make_inputs(name, dtype, drop)["relu_margin"].values()) >= 0.02      # 2.5 bf16 ulps of a pre-activation of size one
    if dtype == F16:
        for tag, (mx, sub) in m["stored"].items():
            assert mx <= 2.0 ** 14 and sub < 0.01, (tag, mx, sub)
    for k in R.tensor_names(r):
        assert torch.isfinite(r[k]).all() and torch.isfinite(m[k]).all() and float(r[k].abs().max()) > 0, k


@pytest.mark.parametrize("name,dtype,drop", CONFIGS, ids=CFG_ID)
def test_measure_passes_a_float32_evaluation_of_the_model(name, dtype, drop):
    r, m = R.chain_ref64(name, dtype, drop), R.chain_model16(name, dtype, drop)
    ms = R.measure_all(R.chain_eval32(name, dtype, drop), r, m)
    assert len(ms) == len(R.tensor_names(r))
    assert not R.failures(ms), R.failures(ms)


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_measure_catches_the_mutants(mutant, dtype):
    """Each wrong step fails the case named for it, in both dtypes, with dropout on (ln_last_row and bias_last_tile also without)."""
    name, drop = R.MUTANT_CASE[mutant], R.DROPS[1]
    r, m = R.chain_ref64(name, dtype, drop), R.chain_model16(name, dtype, drop)
    bad = R.failures(R.measure_all(R.chain_eval32(name, dtype, drop, mutant=mutant), r, m))
    print(f"{mutant} on case {name} {DT_NAME[dtype]}: {len(bad)} tensors fail, e.g. {bad[:2]}")
    assert bad, f"{mutant} passes case {name} in {DT_NAME[dtype]}"
