"""CPU: everything tests/lora_refs.py gives the GPU tests is checked here first -- the model against plain float64 autograd, the
conditions that make the kernel cases and the step cases mean something (from the references alone), the measures on a faithful
float32 evaluation and on every mutant -- and the host layer of vimo_clip_amd/lora.py: parameter names, what trains, the arena,
``merge_lora`` and the adapter-only state dict (no device)."""
import math

import pytest
import torch

import lora_refs as LR
from lora_refs import BF16, DT16, DT_NAME, F16, F32, F64

DT_ID = lambda v: DT_NAME[v] if v in DT_NAME else str(v)


# ---------------------------------------------------------------------------------------------- 1. the model with rounding off
@pytest.mark.parametrize("dt", DT16, ids=DT_ID)
@pytest.mark.parametrize("shape", [c["name"] for c in LR.LINEAR_SHAPES])
def test_model_without_rounding_is_plain_autograd(shape, dt):
    """x (W + s B A)^T + b in float64 autograd against LoraLinearRef under Policy() (concat form, hand-written backward)."""
    inp = LR.linear_inputs(shape, dt)
    got, want = LR.linear_ref64(shape, dt), LR.linear_plain64(inp)
    for k, w in want.items():
        assert float((got[k] - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), k
        assert float(w.abs().max()) > 0, k


# ---------------------------------------------------------------------------------------------- 2. the kernel cases mean something
@pytest.mark.parametrize("dt", DT16, ids=DT_ID)
@pytest.mark.parametrize("c", LR.DOWN_CASES, ids=[c["name"] for c in LR.DOWN_CASES])
def test_down_cases_pin_most_elements(c, dt):
    P = LR.down_prepared(c["name"], dt)
    print(f"down {LR.case_id(c, dt)}: e32 {P['e32']:.2e} pinned {P['pinned']:.3f}")
    assert P["e32"] <= LR.E32_MAX and P["pinned"] >= LR.SHARE_MIN[dt]
    assert c["K"] % 64 == 0 and c["r"] % 8 == 0 and 8 <= c["r"] <= 64 and float(P["r64"].abs().max()) < 6e4


@pytest.mark.parametrize("dt", DT16, ids=DT_ID)
@pytest.mark.parametrize("c", LR.WGRAD_CASES, ids=[c["name"] for c in LR.WGRAD_CASES])
def test_wgrad_cases_have_a_yardstick(c, dt):
    P = LR.wgrad_prepared(c["name"], dt)
    assert P["e32"] <= LR.E32_MAX and float(P["r64"].abs().max()) > 0
    assert LR.measure32(P["r32"], P["r64"], P["e32"])["ok"]
    # the measure sees a dropped token slice and an untransposed store
    short = P["t"][:-64].to(F32).t() @ P["x"][:-64].to(F32)
    assert not LR.measure32(short, P["r64"], P["e32"])["ok"]
    if c["r"] != c["C"]:
        assert not LR.measure32(P["r32"].t().contiguous().view(c["r"], c["C"]), P["r64"], P["e32"])["ok"]


# ---------------------------------------------------------------------------------------------- 3. the measures reject the mutants
@pytest.mark.parametrize("dt", DT16, ids=DT_ID)
@pytest.mark.parametrize("c", LR.DOWN_CASES, ids=[c["name"] for c in LR.DOWN_CASES])
def test_down_check_accepts_the_faithful_kernel_and_rejects_the_mutants(c, dt):
    m, bad = LR.check_down(c, dt, LR.down_concat_model(c, dt))
    assert not bad and m["bad"] == 0, bad
    for mut, word in (("s_twice", "ts:"), ("tail_not_zeroed", "tail"), ("trunc16", "ts:")):
        if mut == "tail_not_zeroed" and c["r"] == LR.TAIL:      # the widest rank has no tail
            continue
        _, bad = LR.check_down(c, dt, LR.down_concat_model(c, dt, mut))
        assert len(bad) == 1 and word in bad[0], (mut, bad)
    flipped = LR.down_concat_model(c, dt)
    flipped[c["M"] // 2, 3] = -flipped[c["M"] // 2, 3] - 1.0
    assert "copied" in LR.check_down(c, dt, flipped)[1][0]


@pytest.mark.parametrize("dt", DT16, ids=DT_ID)
@pytest.mark.parametrize("shape", [c["name"] for c in LR.LINEAR_SHAPES])
def test_linear_measure_on_itself_and_on_the_mutants(shape, dt):
    """A float32 evaluation of the model passes; s applied twice, s missing from dA and dB written untransposed fail, each in the
    tensors it touches and in no other; a ``us`` built from the unrounded dy fails the interval rule on ``us`` (lora_refs.us_check)."""
    r, m = LR.linear_ref64(shape, dt), LR.linear_model16(shape, dt)
    names = ("y", "dx", "dA", "dB", "db")

    def failing(mut):
        got = LR.linear_eval32(shape, dt, mut)
        return {k for k in names if not LR.measure(k, got[k], r, m)["ok"]}
    assert failing(None) == set()
    assert failing("s_twice") == {"y", "dB"}
    assert failing("s_missing_dA") == {"dA"}
    assert failing("dB_untransposed") == {"dB"}
    ok, mut = LR.us_check(shape, dt), LR.us_check(shape, dt, "us_unrounded_dy")
    assert ok["ok"] and ok["pinned"] >= LR.SHARE_MIN[dt] and ok["e32"] <= LR.E32_MAX
    assert not mut["ok"] and mut["bad"] > 0
    assert set(LR.LINEAR_MUTANTS) == {"s_twice", "s_missing_dA", "dB_untransposed", "us_unrounded_dy"}


STEP_CONFIGS = [(c["name"], dt) for c in LR.STEP_CASES for dt in DT16]


@pytest.mark.parametrize("name,dt", STEP_CONFIGS, ids=DT_ID)
def test_step_inputs_make_the_measure_mean_something(name, dt):
    """The conditions of tests/test_student_step_refs_host.py on the adapted step, from the two references alone."""
    inp, r, m = LR.step_inputs(name, dt), LR.step_ref64(name, dt), LR.step_model16(name, dt)
    c = inp["case"]
    names = LR.ST.tensor_names(r)
    n_sites = 2 * len(c["targets"]) * c["L"]
    assert len(names) == 3 + 2 * n_sites + 8 and len(LR.adapter_names(c)) == n_sites
    bad_rms, bad_max = LR.vacuity(r, m)
    print(f"{name} {DT_NAME[dt]}: {len(names)} tensors, stress {inp['stress']}, max condition missed by {bad_max}")
    assert not bad_rms, bad_rms
    assert (not bad_max) if dt == F16 else 4 * len(bad_max) <= len(names), bad_max
    assert len(r["attn_peak"]) == c["L"] and min(r["attn_peak"]) >= 4.0 / c["N"]
    for o in (r, m):
        assert 0.02 <= o["relu_negative_share"] <= 0.98 and o["relu_min_abs"] >= 0.02
    assert inp["relu_margin"] >= 0.02
    assert LR.UP_SCALE[BF16] == 1.0 and math.log2(LR.UP_SCALE[F16]) == round(math.log2(LR.UP_SCALE[F16]))
    if dt == F16:
        assert m["stored"]
        for tag, (mx, sub) in m["stored"].items():
            assert mx <= 2.0 ** 14 and sub < 0.01, (tag, mx, sub)
    for k in names:
        assert torch.isfinite(r[k]).all() and torch.isfinite(m[k]).all() and float(r[k].abs().max()) > 0, k
    # the adapter term is neither negligible nor dominant: the embeddings move by 5 % .. 100 % of their size when it is dropped
    base = LR.step_ref64(name, dt, False, False)
    rel = float((r["emb"] - base["emb"]).abs().max() / r["emb"].abs().max())
    assert 0.05 <= rel <= 1.0, rel


@pytest.mark.parametrize("dt", DT16, ids=DT_ID)
@pytest.mark.parametrize("mut", sorted(LR.STEP_MUTANT_CASE))
def test_step_measure_on_itself_and_on_the_mutants(mut, dt):
    name = LR.STEP_MUTANT_CASE[mut]
    r, m = LR.step_ref64(name, dt), LR.step_model16(name, dt)
    ok = LR.ST.measure_all(LR.step_eval32(name, dt), r, m)
    assert len(ok) == len(LR.ST.tensor_names(r)) and not LR.ST.failures(ok), LR.ST.failures(ok)
    assert LR.ST.failures(LR.ST.measure_all(LR.step_eval32(name, dt, mut), r, m)), mut


def test_fresh_adapters_are_the_base_model():
    """B = 0: the float64 step equals the base model's, every dA is exactly zero and every dB is not."""
    name = LR.STEP_CASES[0]["name"]
    r, base = LR.step_ref64(name, BF16, True), LR.step_ref64(name, BF16, True, False)
    for k in ("emb", "emb_distill", "logits"):
        assert torch.equal(r[k], base[k]), k
    for _w, an, bn in LR.adapter_names(LR.STEP_BY_NAME[name]):
        assert float(r["g." + an].abs().max()) == 0.0 and float(r["g." + bn].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- 4. add_lora / merge_lora / state_dict
def _student(**kw):
    from vimo_clip_amd.models.student_model import FlowStudentModel
    torch.manual_seed(0)
    return FlowStudentModel("ViT-tiny/14", device="cpu", num_classes=12, **kw)


def test_add_lora_names_what_trains_and_the_arena():
    from vimo_clip_amd.optim import GradArena
    plain = _student()
    keys0 = list(plain.state_dict())
    assert list(_student(lora_rank=0).state_dict()) == keys0              # rank 0: the model it always was
    m = _student(lora_rank=8, lora_targets=("attn", "mlp"))
    L = m.visual_encoder.layers
    want = [f"visual_encoder.transformer.resblocks.{i}.{n}" for i in range(L)
            for n in ("attn.in_proj_lora_A", "attn.in_proj_lora_B", "attn.out_proj.lora_A", "attn.out_proj.lora_B", "mlp.c_fc.lora_A",
                      "mlp.c_fc.lora_B", "mlp.c_proj.lora_A", "mlp.c_proj.lora_B")]
    assert set(m.state_dict()) == set(keys0) | set(want)
    attn_only = _student(lora_rank=16)
    assert {k for k in attn_only.state_dict() if "lora_" in k} == {k for k in want if ".attn." in k}
    D = m.visual_encoder.width
    sd = m.state_dict()
    assert sd[want[0]].shape == (8, D) and sd[want[1]].shape == (3 * D, 8) and sd[want[6]].shape == (8, 4 * D) and sd[want[7]].shape == (D, 8)
    for k in want:
        v = sd[k]
        assert v.dtype == F32
        if k.endswith("_B"):
            assert float(v.abs().max()) == 0.0
        else:       # kaiming_uniform_(a = sqrt 5): U(-1 / sqrt K, 1 / sqrt K)
            bound = v.shape[1] ** -0.5
            assert 0.5 * bound < float(v.abs().max()) <= bound
    st = m.visual_encoder.lora
    assert st.rank == 8 and st.alpha == 16.0 and st.scale == 2.0 and st.targets == ("attn", "mlp") and len(st.sites()) == 4 * L
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    heads = {n for n in keys0 if n.startswith(("residual_mlp.", "classification_head."))}
    assert trainable == set(want) | heads and len(heads) == 8
    arena = GradArena(m.parameters())
    assert len(arena.params) == len(trainable)
    # adapters + heads, every slot rounded up to the arena's 64-element granularity (optim._ALIGN)
    assert arena.numel == sum((p.numel() + 63) // 64 * 64 for n, p in m.named_parameters() if n in trainable)
    assert all(getattr(p, "_vmc_grad", None) is None for n, p in m.named_parameters() if n not in trainable)
    assert arena.numel < 0.2 * sum(p.numel() for p in plain.parameters())


def test_add_lora_refuses_what_it_cannot_do():
    from vimo_clip_amd.lora import add_lora
    for kw in (dict(rank=4), dict(rank=12), dict(rank=72), dict(rank=8, targets=("qkv",)), dict(rank=8, targets=())):
        with pytest.raises(ValueError):
            add_lora(_student().visual_encoder, **kw)
    m = _student(lora_rank=8)
    with pytest.raises(ValueError, match="already"):
        add_lora(m.visual_encoder, 8)
    with pytest.raises(ValueError, match="recompute"):
        _student(lora_rank=8, recompute="block")
    blocked = _student()
    blocked.visual_encoder.recompute = "block"
    with pytest.raises(ValueError, match="recompute"):
        add_lora(blocked.visual_encoder, 8)
    with pytest.raises(RuntimeError, match="merge_lora"):             # the inference path never silently ignores live adapters
        m.visual_encoder._encode_patches(torch.zeros((16, 640), dtype=torch.bfloat16), 1)


def test_merge_lora_folds_the_adapters_and_restores_the_model():
    from vimo_clip_amd import lora
    plain = _student()
    keys0, req0 = list(plain.state_dict()), {n: p.requires_grad for n, p in plain.named_parameters()}
    m = _student(lora_rank=8, lora_alpha=4.0, lora_targets=("attn", "mlp"))
    vit = m.visual_encoder
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for s in vit.lora.sites():
            s.B.copy_(torch.randn(s.B.shape, generator=g) * 0.1)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    want = {}
    for n, p in vit.named_parameters():
        if n.endswith("lora_A"):
            w = n.replace("in_proj_lora_A", "in_proj_weight").replace(".lora_A", ".weight")
            b = n[:-1] + "B"
            want["visual_encoder." + w] = (before["visual_encoder." + w].double()
                                           + 0.5 * before["visual_encoder." + b].double() @ before["visual_encoder." + n].double())
    assert len(want) == 4 * vit.layers
    snap = lora.merged_state_dict(m)                                   # the checkpoint form, adapters left alive
    assert list(snap) == keys0 and getattr(vit, "lora", None) is not None
    only = lora.lora_state_dict(vit)
    assert {k for k in only if not k.startswith("lora.")} == {n for n, _ in vit.named_parameters() if "lora_" in n}
    assert only["lora.rank"] == 8 and only["lora.alpha"] == 4.0 and only["lora.targets"] == ["attn", "mlp"]
    lora.merge_lora(vit)
    assert getattr(vit, "lora", None) is None and list(m.state_dict()) == keys0
    assert {n: p.requires_grad for n, p in m.named_parameters()} == req0
    plain.load_state_dict(m.state_dict(), strict=True)                 # exactly the keys of a model that never had adapters
    for n, p in m.named_parameters():
        assert torch.equal(snap[n], p.detach()), n
        if n not in want:
            assert torch.equal(p.detach(), before[n]), n
            continue
        ref = want[n]
        e32 = float((ref.float().double() - ref).abs().max() / ref.abs().max())      # one fp32 rounding of the merged weight
        assert LR.measure32(p.detach(), ref, e32)["ok"] and float((ref - before[n].double()).abs().max()) > 1e-3, n
    with pytest.raises(ValueError):
        lora.merge_lora(vit)
    # the adapters alone travel: into a fresh model with the same adapters, and not into one with others
    m2 = _student(lora_rank=8, lora_targets=("attn", "mlp"))
    lora.load_lora_state_dict(m2.visual_encoder, only)
    assert m2.visual_encoder.lora.scale == 0.5
    for k, v in only.items():
        if not k.startswith("lora."):
            assert torch.equal(dict(m2.visual_encoder.named_parameters())[k].detach(), v)
    with pytest.raises(ValueError):
        lora.load_lora_state_dict(_student(lora_rank=16, lora_targets=("attn", "mlp")).visual_encoder, only)
    with pytest.raises(ValueError):
        lora.load_lora_state_dict(_student(lora_rank=8).visual_encoder, only)


def test_command_line_reaches_the_model():
    from vimo_clip_amd import train, train_frame_diff_mn
    a = train.build_parser().parse_args([])
    assert not hasattr(a, "lora_rank") and train.lora_kwargs(a) == {}          # a run without adapters: the namespace it always had
    a = train.build_parser().parse_args(["--lora_rank", "16", "--lora_targets", "attn+mlp", "--lora_alpha", "8"])
    assert train.lora_kwargs(a) == {"lora_rank": 16, "lora_alpha": 8.0, "lora_targets": ("attn", "mlp")}
    b = train_frame_diff_mn.build_parser().parse_args(["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c",
                                                       "--lora-rank", "8"])
    assert train.lora_kwargs(b) == {"lora_rank": 8, "lora_alpha": None, "lora_targets": ("attn",)}
    m = _student(**train.lora_kwargs(a))
    assert m.visual_encoder.lora.rank == 16 and m.visual_encoder.lora.scale == 0.5
