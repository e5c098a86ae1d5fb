"""CPU checks of tests/drop_path_refs.py and of the host side of drop path: the kernel restatements and the float64 step against plain
float64 autograd, the measure on a float32 evaluation of the model and on six mutants of it, the conditions that make the measure mean
something, the K_l / p_l / s_l rule, argument validation before anything touches a device, the --drop_path flags, the byte model."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import drop_path_refs as R                       # noqa: E402
import student_step_refs as S                    # noqa: E402
from oracle import student as ostudent           # noqa: E402
from oracle import vit as ovit                   # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16, F32      # noqa: E402

F64 = torch.float64
DTYPES = (BF16, F16)
CONFIGS = [(c["name"], dt) for c in R.CASES for dt in DTYPES]
CFG_ID = lambda v: v if isinstance(v, str) else DT_NAME[v]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------- the kernel restatements
def test_sampler_reference_is_the_block_row_of_the_patch_sampler():
    from attention_refs import hash32
    seed, block, F, K = 0x1234567, 5, 17, 9
    keep, slot = R.sample(seed, block, F, K)
    key = hash32(seed, np.uint64(block * F) + np.arange(F, dtype=np.uint64)).astype(np.int64)
    rank = key * F + np.arange(F)                                  # (key, f) as one integer
    kept = np.zeros(F, dtype=bool)
    kept[keep] = True
    assert keep.dtype == np.int32 and (np.diff(keep) > 0).all() and rank[kept].max() < rank[~kept].min()
    assert (slot[keep] == np.arange(K)).all() and (slot[~kept] == -1).all()
    assert (R.sample(seed, 0, F, F)[0] == np.arange(F)).all()
    assert not np.array_equal(R.sample(seed, 4, F, K)[0], keep) and not np.array_equal(R.sample(seed + 1, block, F, K)[0], keep)


@pytest.mark.parametrize("F,keep", [(3, (0, 2)), (5, (1, 2, 4)), (4, (0, 1, 2, 3)), (2, (1,))])
def test_data_kernel_references_are_float64_autograd(F, keep):
    """x_pass + mask s (scatter(y) - x_pass) and its gradients; the gather's backward sums its two gradients."""
    K, row = len(keep), 6
    g = torch.Generator().manual_seed(F * 10 + K)
    slot = R.slots(keep, F)
    s = F / K
    c = 1.0 - s
    x = torch.randn(F, row, generator=g, dtype=F64).requires_grad_(True)
    y = torch.randn(K, row, generator=g, dtype=F64).requires_grad_(True)
    dout = torch.randn(F, row, generator=g, dtype=F64)
    idx = torch.tensor(keep)
    mask = torch.zeros(F, 1, dtype=F64).index_fill(0, idx, 1.0)
    out = x + mask * s * (torch.zeros(F, row, dtype=F64).index_copy(0, idx, y) - x)
    out.backward(dout)
    ref, mag, kept = R.merge(x.detach(), y.detach(), slot, c, s)
    assert _rel(ref, out.detach()) <= 1e-14 and kept.tolist() == [f in keep for f in range(F)]
    assert torch.equal(ref[~kept], x.detach()[~kept]) and (mag[~kept] == 0).all() and (mag[kept] >= ref[kept].abs() - 1e-12).all()
    dx, _, _, dy, _ = R.merge_bwd(dout, keep, slot, c, s)
    assert _rel(dx, x.grad) <= 1e-14 and _rel(dy, y.grad) <= 1e-14 and torch.equal(dx[~kept], dout[~kept])
    xs = torch.randn(F, row, generator=g, dtype=F64).requires_grad_(True)
    d_sub, d_pass = torch.randn(K, row, generator=g, dtype=F64), torch.randn(F, row, generator=g, dtype=F64)
    sub = R.gather(xs, keep)
    assert torch.equal(sub.detach(), xs.detach()[idx])
    ((sub * d_sub).sum() + (xs * d_pass).sum()).backward()
    got, _, _ = R.scatter_add(d_pass, d_sub, slot)
    assert _rel(got, xs.grad) <= 1e-14


def test_bound_constants():
    """The kept-row bound is a handful of fp32 ulps of the two terms plus half an ulp of the store; exact rows have no bound at all."""
    assert 1.0 < R.KAPPA < 1.001 and R.FP32_TINY < 1e-37
    one = torch.ones(1, dtype=F64)
    assert float(R.kept_bound(one, 2 * one, F32)) == pytest.approx(2.0 ** -22, rel=1e-3)
    assert float(R.kept_bound(one, 2 * one, BF16)) == pytest.approx(2.0 ** -8, rel=1e-3)
    assert float(R.kept_bound(one, 2 * one, F16)) == pytest.approx(2.0 ** -11, rel=1e-3)
    assert R.scales(3, 2) == (-0.5, 1.5) and R.scales(64, 48) == (float(np.float32(1 - 64 / 48)), float(np.float32(64 / 48)))


# ---------------------------------------------------------------------------------------------- the float64 step
def _dense_tower(sd, pix, heads, drop, F, cls_only):
    """oracle.vit.vit_forward's graph in masked-dense form: every block runs on every frame and mask s (Block(x) - x) is added."""
    g = lambda k: sd[k]
    D = g("conv1.weight").shape[0]
    x = Fn.conv2d(pix, g("conv1.weight"), stride=g("conv1.weight").shape[-1]).reshape(F, D, -1).permute(0, 2, 1)
    x = torch.cat([g("class_embedding").view(1, 1, D).expand(F, 1, D), x], 1) + g("positional_embedding")
    x = ovit.layer_norm(x, g("ln_pre.weight"), g("ln_pre.bias"))
    N, dh = x.shape[1], D // heads
    for i, kept in enumerate(drop):
        pre = f"transformer.resblocks.{i}."
        h = ovit.layer_norm(x, g(pre + "ln_1.weight"), g(pre + "ln_1.bias"))
        q, k, v = ((h @ g(pre + "attn.in_proj_weight").t() + g(pre + "attn.in_proj_bias")).split(D, -1)[j].view(F, N, heads, dh).transpose(1, 2)
                   for j in range(3))
        o = (torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1) @ v).transpose(1, 2).reshape(F, N, D)
        y = x + o @ g(pre + "attn.out_proj.weight").t() + g(pre + "attn.out_proj.bias")
        y = y + ovit.quick_gelu(ovit.layer_norm(y, g(pre + "ln_2.weight"), g(pre + "ln_2.bias")) @ g(pre + "mlp.c_fc.weight").t()
                                + g(pre + "mlp.c_fc.bias")) @ g(pre + "mlp.c_proj.weight").t() + g(pre + "mlp.c_proj.bias")
        if kept is None:
            x = y
            continue
        mask = torch.zeros(F, 1, 1, dtype=F64).index_fill(0, torch.tensor(kept), 1.0)
        if cls_only and i + 1 == len(drop):              # only the class rows go on: the merge is taken on them
            x, y = x[:, :1], y[:, :1]
        x = x + mask * (F / len(kept)) * (y - x)
    return ovit.layer_norm(x[:, 0], g("ln_post.weight"), g("ln_post.bias")) @ g("proj")


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["name"] != "dp_i"])
def test_ref64_is_float64_autograd_in_masked_dense_form(name):
    """The subset form of the reference equals block-then-mask under float64 autograd: outputs and every gradient to 1e-12."""
    dc = R.DBY_NAME[name]
    inp, r = R.make_inputs(dc["base"], BF16), R.step_ref64(name, BF16)
    c = inp["case"]
    sd = {}
    for n in R.param_shapes(c):
        sd[n] = (inp["w16"][n] if n in inp["w16"] else inp["p32"][n]).to(F64).clone().requires_grad_(True)
    pix = ovit.normalize_u8(ovit.to_pil_wrap_u8(inp["frames"]), F64)
    emb = _dense_tower(sd, pix, R.HEADS, dc["drop"], c["F"], c["cls_only"])
    if c["level"] == "tower":
        outs = {"E": emb}
    else:
        e3 = emb.view(c["B"], c["T"], -1)
        h = torch.relu(e3.mean(1) @ sd["classification_head.0.weight"].t() + sd["classification_head.0.bias"])
        outs = {"emb": emb, "emb_distill": ostudent.residual_mlp(sd, emb, R.ALPHA),
                "logits": h @ sd["classification_head.2.weight"].t() + sd["classification_head.2.bias"]}
    torch.autograd.backward(list(outs.values()), [inp["up"][n].to(F64).reshape(o.shape) for n, o in outs.items()])
    for n, o in outs.items():
        assert _rel(r[n], o.detach().reshape(r[n].shape)) <= 1e-12, n
    for n in R.param_shapes(c):
        assert sd[n].grad is not None and _rel(r["g." + n], sd[n].grad) <= 1e-12, n


def test_cases_are_what_they_are_listed_for():
    a, g, i, s1 = (R.DBY_NAME[n] for n in ("dp_a", "dp_g", "dp_i", "dp_s1"))
    assert a["drop"] == g["drop"] == ((0, 2), (1, 2)) and a["cls_only"] and not g["cls_only"] and a["F"] == 3
    assert i["drop"][0] is None and len(i["drop"][1]) == 48 and i["F"] == 64
    assert S.BY_NAME["i"]["parks_stream"] and (48 * i["N"]) % 128 != 0 and 48 * i["N"] == 2400        # grouped in block 0, per linear in block 1
    assert s1["level"] == "student" and s1["drop"] == ((0, 1, 3), (2, 3))
    assert R.LAYERS == 2 and set(R.MUTANT_CASE) == set(R.MUTANTS) and set(R.MUTANT_CASE.values()) <= set(R.DBY_NAME)
    assert R.DBY_NAME[R.MUTANT_CASE["merge_token_rows"]]["cls_only"]


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_inputs_make_the_measure_mean_something(name, dtype):
    """The conditions test_student_step_refs_host.py asserts for its cases, on the references with drop path."""
    dc = R.DBY_NAME[name]
    inp, r, m = R.make_inputs(dc["base"], dtype), R.step_ref64(name, dtype), R.step_model16(name, dtype)
    c = inp["case"]
    bad_rms, bad_max = R.vacuity(r, m)
    n = len(R.tensor_names(r))
    print(f"{name} {DT_NAME[dtype]}: {n} tensors, max condition missed by {bad_max}")
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
    assert max(float(u.abs().max()) for u in inp["up"].values()) <= 8 * S.UP_SCALE[dtype]
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
    name = R.MUTANT_CASE[mutant]
    _, bad = R.check(R.step_eval32(name, dtype, bug=mutant), R.step_ref64(name, dtype), R.step_model16(name, dtype))
    print(f"{mutant} on case {name} {DT_NAME[dtype]}: {len(bad)} tensors fail, e.g. {bad[:2]}")
    assert bad, f"{mutant} passes case {name} in {DT_NAME[dtype]}"


# ---------------------------------------------------------------------------------------------- host logic
def test_rate_count_and_scale_table():
    from vimo_clip_amd import ops
    # (p, l, L, F) -> (p_l, K_l)
    table = [((0.5, 0, 2, 4), (0.0, 4)), ((0.5, 1, 2, 4), (0.5, 2)), ((0.1, 11, 12, 512), (0.1, 460)), ((0.1, 1, 12, 512), (0.1 / 11, 507)),
             ((0.2, 6, 12, 544), (1.2 / 11, 484)), ((0.4, 23, 24, 256), (0.4, 153)), ((0.9, 1, 2, 3), (0.9, 1)), ((0.3, 0, 1, 8), (0.0, 8)),
             ((0.99, 1, 2, 16), (0.99, 1)), ((0.0, 5, 12, 64), (0.0, 64))]
    for (p, l, L, F), (p_l, K) in table:
        assert ops.drop_path_rate(p, l, L) == pytest.approx(p_l, abs=1e-15)
        assert ops.drop_path_keep_count(F, ops.drop_path_rate(p, l, L)) == K == R.keep_count(F, p, l, L), (p, l, L, F)
    assert ops.drop_path_keep_count(544, 0.25) == ops.patch_keep_count(544, 0.25)                      # one rounding rule
    assert ops.DROP_PATH_MAX_F == 8192


def _student(**kw):
    from vimo_clip_amd.models.student_model import FlowStudentModel
    torch.manual_seed(0)
    return FlowStudentModel("ViT-tiny/14", device="cpu", num_classes=12, **kw)


def test_flags_and_their_defaults():
    from vimo_clip_amd.clip_vit import VisionTransformer
    v = VisionTransformer.from_name("ViT-tiny/32")
    assert v.drop_path == 0.0 and v.drop_path_seed == 0 and v.drop_path_seed_address is None
    assert _student().visual_encoder.drop_path == 0.0
    m = _student(drop_path=0.2, drop_path_seed=11)
    assert m.visual_encoder.drop_path == 0.2 and m.visual_encoder.drop_path_seed == 11
    assert set(m.state_dict()) == set(_student().state_dict())                       # a flag, not a parameter
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="drop_path"):
            _student(drop_path=bad)


def test_nothing_is_drawn_without_training_or_gradients():
    """drop_keep_for returns all None -- before any device call: these towers live on the CPU -- unless p > 0, train() and grad."""
    from vimo_clip_amd.autograd_vit import drop_keep_for
    from vimo_clip_amd.clip_vit import VisionTransformer
    v = VisionTransformer.from_name("ViT-tiny/32").train()
    L = len(v.transformer.resblocks)
    assert drop_keep_for(v, 4, "cpu") == [None] * L                                   # p = 0
    v.drop_path = 0.5
    with torch.no_grad():
        assert drop_keep_for(v, 4, "cpu") == [None] * L
    assert drop_keep_for(v.eval(), 4, "cpu") == [None] * L
    assert getattr(v, "_drop_path_calls", 0) == 0                                     # none of them consumed a draw
    v.train().drop_path = 1.0
    with pytest.raises(ValueError, match="drop_path"):
        drop_keep_for(v, 4, "cpu")
    v.drop_path = 0.5
    with pytest.raises(ValueError, match="8192"):                                     # the sampler's limit, named before any launch
        drop_keep_for(v, 8193, "cpu")


def test_argument_validation_precedes_the_device():
    from vimo_clip_amd import ops
    from vimo_clip_amd.autograd_vit import vit_tokens_train
    x = torch.zeros((4, 64), dtype=torch.bfloat16)
    keep, slot = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0, -1, 1, -1], dtype=torch.int32)
    with pytest.raises(ValueError, match="int32"):
        ops.frame_gather(x, keep.long())
    with pytest.raises(ValueError, match="contiguous"):
        ops.frame_gather(x.t(), keep)
    with pytest.raises(ValueError, match="of 4"):
        ops.drop_path_merge(x, x[:2].contiguous(), slot[:3].contiguous(), 2.0)
    with pytest.raises(ValueError, match="dtype"):
        ops.drop_path_merge(x, x[:2].float(), slot, 2.0)
    with pytest.raises(ValueError, match="dtype"):
        ops.frame_scatter_add(x, x[:2].float(), slot)
    with pytest.raises(ValueError, match="8192"):
        ops.drop_path_sample(1, 0, 8193, 4, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):                             # valid arguments: there is no fallback
        ops.frame_gather(x, keep)
    m = _student()
    vids = torch.zeros((1, 2, 3, 56, 56), dtype=torch.uint8)
    with pytest.raises(ValueError, match="drop_path_keep"):
        with torch.no_grad():
            m(vids, drop_path_keep=[None, None, keep])
    v = m.visual_encoder.train()
    assert len(v.transformer.resblocks) == 3
    for bad, msg in (([None], "one per residual block"), ([None, None, keep.long()], "int32"),
                     ([None, None, torch.zeros(3, dtype=torch.int32)], "1..2")):
        with pytest.raises(ValueError, match=msg):
            vit_tokens_train(v, vids[0], drop_keep=bad)
    with pytest.raises(ValueError, match="training forward"):
        vit_tokens_train(v.eval(), vids[0], drop_keep=[None, None, keep])


def test_drop_path_flag_parsing():
    from vimo_clip_amd import train, train_frame_diff_mn
    a = train.build_parser().parse_args([])
    assert not hasattr(a, "drop_path") and train.drop_path_kwargs(a) == {}            # a run without it: the namespace it always had
    a = train.build_parser().parse_args(["--drop_path", "0.1"])
    assert a.drop_path == 0.1
    assert train.drop_path_kwargs(a) == {"drop_path": 0.1, "drop_path_seed": train.DROP_PATH_SEED}
    assert train.drop_path_kwargs(a, rank=3)["drop_path_seed"] == train.DROP_PATH_SEED + 3      # a stream per rank
    assert train.drop_path_kwargs(train.build_parser().parse_args(["--drop_path", "0"])) == {}
    assert train.DROP_PATH_SEED != train.PATCH_DROPOUT_SEED
    for bad in ("1", "1.0", "-0.25", "half"):
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(["--drop_path", bad])
    with pytest.raises(Exception, match="drop_path"):
        train._drop_path_arg("1.5")
    need = ["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c"]
    q = train_frame_diff_mn.build_parser()
    assert q.parse_args(need).drop_path == 0.0 and train.drop_path_kwargs(q.parse_args(need)) == {}
    assert q.parse_args(need + ["--drop_path", "0.2"]).drop_path == 0.2
    m = _student(**train.drop_path_kwargs(a, rank=1))
    assert m.visual_encoder.drop_path == 0.1 and m.visual_encoder.drop_path_seed == train.DROP_PATH_SEED + 1


def test_saved_activation_bytes_per_block():
    from vimo_clip_amd.autograd_vit import saved_activation_bytes as sab
    name, (Rr, p, D, L, H, _E) = "ViT-B/32", (224, 32, 768, 12, 12, 512)
    N, F = 50, 512
    for kw in ({}, {"cls_only": False}, {"recompute": "block"}, {"tokens": 25}, {"bytes16": 2, "residual_bytes": 2}):
        assert sab(name, F, drop_path=0.0, **kw) == sab(name, F, **kw)                # off: today's value
    row_attn, row_mlp = 14 * D + 4 * H + 8, 22 * D + 8
    for dp in (0.1, 0.2, 0.4):
        K = [max(1, int(F * (1.0 - dp * l / (L - 1)))) for l in range(L)]
        assert K[0] == F and K[-1] == int(F * (1 - dp)) and K == sorted(K, reverse=True)
        assert sab(name, F, cls_only=False, drop_path=dp) == sum(k * N * (row_attn + row_mlp) for k in K)
        assert sab(name, F, drop_path=dp) == sum(k * N * (row_attn + row_mlp) for k in K[:-1]) + K[-1] * (N * row_attn + 2 * D + row_mlp)
        assert sab(name, F, "block", drop_path=dp) == sum(k * N * 4 * D for k in K)
        assert sab(name, F, drop_path=dp) < sab(name, F)
        assert math.isclose(sab(name, F, cls_only=False, drop_path=dp) / sab(name, F, cls_only=False), sum(K) / (L * F), rel_tol=1e-12)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="drop_path"):
            sab(name, F, drop_path=bad)
