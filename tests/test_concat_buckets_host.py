"""CPU: length buckets for the two concatenation modes (vimo_clip_amd/graphs.py concat_mode / pad_concat_to_bucket,
GraphedTrainStep(concat=), TFAM/train_and_eval.py GraphedEvalForward(concat_bucket=), Config.graph_bucket_concat).

Both streams of a concatenation batch are zero-padded to their own bucket and the concatenation is rebuilt with the real rows as a
prefix (tests/concat_ref.py restates the kernel's contract, include/vmc.h K19), so one pool length serves the concatenated
sequence.  Here: the plumbing, and the identity itself in float64 against the oracle at the batch's own lengths;
tests/test_gpu_concat_buckets.py checks the kernel and the model on the GPU.
"""
import pytest
import torch
import torch.nn.functional as F

from concat_ref import clamp_lens, concat_ref
from oracle import make_golden as mg
from oracle import tfam as otfam
from vimo_clip_amd import graphs, synth


class _Arena:
    pass


class _Opt:           # the attribute surface GraphedTrainStep uses of optim.FusedAdam in device-state mode
    def __init__(self, n=8):
        self.arena = _Arena()
        self.arena.flat_param, self.arena.flat_grad = torch.zeros(n), torch.zeros(n)
        self.m, self.v = torch.zeros(n), torch.zeros(n)
        self.dev_state, self.dev_hyper = torch.zeros(4, dtype=torch.int64), torch.zeros(4)
        self.step_count = 0


def _recording_factory(log):
    class _Stub:          # stands in for GraphedCallable: records what a capture and every replay are handed
        def __init__(self, fn, *example_inputs, warmup=1):
            self.fn = fn
            log.append(("capture", example_inputs))

        def __call__(self, *inputs):
            log.append(("replay", inputs))
            return self.fn(*inputs)
    return _Stub


def _batch(T_rgb, B=3, D=8, masks=True):
    T_mot = T_rgb - 1
    rgb, mot = torch.randn(B, T_rgb, D), torch.randn(B, T_mot, D)
    mr, mf = (torch.ones(B, T_rgb, dtype=torch.bool), torch.ones(B, T_mot, dtype=torch.bool)) if masks else (None, None)
    if masks:
        mr[0, T_rgb - 3:] = False                      # a clip shorter than the batch's own T_max
        mf[0, T_mot - 3:] = False
    return rgb, mot, mr, mf, torch.zeros(B, 4)


def _tiny(**kw):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    return AMO_CLIP(d_model=64, nhead=1, num_layers=1, dim_feedforward=64, num_classes=4, device="cpu", **kw)


def test_concat_mode_names_the_two_concatenations():
    assert graphs.concat_mode(_tiny()) is None
    assert graphs.concat_mode(_tiny(use_only_rgb=True)) is None
    assert graphs.concat_mode(_tiny(use_only_flow=True)) is None
    assert graphs.concat_mode(_tiny(use_only_rgb=True, use_cross_attention=False)) is None
    assert graphs.concat_mode(_tiny(use_cross_attention=False, concat_dim=1)) == "time"
    assert graphs.concat_mode(_tiny(use_cross_attention=False, concat_dim=-1)) == "feature"
    for m in (_tiny(), _tiny(use_cross_attention=False, concat_dim=1), _tiny(use_cross_attention=False, concat_dim=-1)):
        assert (graphs.concat_mode(m) is None) == (graphs.pooled_stream(m) is not None)      # every model has exactly one of the two


def test_pad_concat_to_bucket_shapes_masks_and_T_out():
    rgb, mot, mr, mf, _ = _batch(21)
    prgb, pmot, pmr, pmf, nr, nm, T_out = graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 16, "time")
    assert (nr, nm, T_out) == (21, 20, 48)                      # roundup(21 - 1 + 20, 16), not 32 + 32
    assert prgb.shape == (3, 32, 8) and pmot.shape == (3, 32, 8) and pmr.shape == (3, 32) and pmf.shape == (3, 32)
    assert torch.equal(prgb[:, :21], rgb) and torch.equal(pmot[:, :20], mot)
    assert prgb[:, 21:].abs().max() == 0 and pmot[:, 20:].abs().max() == 0
    assert pmr.dtype == mr.dtype and torch.equal(pmr[:, :21], mr) and not pmr[:, 21:].any()
    assert torch.equal(pmf[:, :20], mf) and not pmf[:, 20:].any()
    out = graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 16, "feature")
    assert out[4:] == (21, 20, 32) and out[0].shape == (3, 32, 8)            # T_out = the padded motion length
    # 33 / 32 tokens: the streams land in different buckets, the motion stream is left alone
    rgb, mot, mr, mf, _ = _batch(33)
    out = graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 16, "time")
    assert out[0].shape[1] == 48 and out[1] is mot and out[3] is mf and out[4:] == (33, 32, 64)
    assert graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 16, "feature")[4:] == (33, 32, 32)
    # short clips stay within the fused chains' 64 tokens: 32 + 31 - 1 = 62 -> 64, where two rounded lengths would give 32 + 32
    rgb, mot, mr, mf, _ = _batch(32)
    assert graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 32, "time")[6] == 64
    rgb, mot, mr, mf, _ = _batch(9)
    assert graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 32, "time")[4:] == (9, 8, 32)


def test_pad_concat_to_bucket_synthesises_masks_over_the_original_length():
    rgb, mot, _, _, _ = _batch(21, masks=False)
    for mode in ("time", "feature"):
        _, _, pmr, pmf, nr, nm, _ = graphs.pad_concat_to_bucket(rgb, mot, None, None, 16, mode)
        assert (nr, nm) == (21, 20) and pmr.shape == (3, 32) and pmf.shape == (3, 32)
        assert pmr[:, :21].all() and not pmr[:, 21:].any()        # otherwise the new rows would be attended to
        assert pmf[:, :20].all() and not pmf[:, 20:].any()


@pytest.mark.parametrize("bucket,mode", [(1, "time"), (0, "feature"), (16, None)])
def test_pad_concat_to_bucket_identity(bucket, mode):
    rgb, mot, mr, mf, _ = _batch(21)
    out = graphs.pad_concat_to_bucket(rgb, mot, mr, mf, bucket, mode)
    assert out[0] is rgb and out[1] is mot and out[2] is mr and out[3] is mf and out[4:] == (None, None, None)


def test_two_lengths_of_one_bucket_share_one_train_graph_and_hand_over_their_own_lengths():
    log, seen = [], []

    def step_fn(rgb, mot, mr, mf, labels, n_rgb, n_mot, T_out):
        seen.append((tuple(rgb.shape), tuple(mot.shape), tuple(mr.shape), tuple(mf.shape), tuple(labels.shape), int(n_rgb), int(n_mot), T_out))
        return rgb.sum()

    step = graphs.GraphedTrainStep(step_fn, _Opt(), bucket=16, pooled=None, concat="time", graph_factory=_recording_factory(log))
    for T in (21, 19):
        step(*_batch(T))
    captures = [a for kind, a in log if kind == "capture"]
    assert len(captures) == 1 and step.n_graphs == 1
    replays = [a for kind, a in log if kind == "replay"]
    assert len(replays) == 2
    for T, a in zip((21, 19), replays):
        rgb, mot, mr, mf, labels, n_rgb, n_mot, T_out = a
        assert rgb.shape == (3, 32, 8) and mot.shape == (3, 32, 8) and mr.shape == (3, 32) and mf.shape == (3, 32) and labels.shape == (3, 4)
        for n, want in ((n_rgb, T), (n_mot, T - 1)):
            assert n.dtype == torch.int32 and n.numel() == 1 and int(n) == want
        assert isinstance(T_out, int) and T_out == 48
    assert [s[5:] for s in seen] == [(21, 20, 48), (19, 18, 48)]
    # T_out is part of the key by value: 27 + 26 - 1 = 52 -> 64 at the same padded stream lengths is another graph
    step(*_batch(27))
    assert step.n_graphs == 2 and seen[-1][:2] == ((3, 32, 8), (3, 32, 8)) and seen[-1][5:] == (27, 26, 64)
    # the feature mode keys on the padded stream lengths alone
    log2 = []
    step = graphs.GraphedTrainStep(lambda *a: a[0].sum(), _Opt(), bucket=16, pooled=None, concat="feature", graph_factory=_recording_factory(log2))
    for T in (21, 19, 27):
        step(*_batch(T))
    assert step.n_graphs == 1 and [(int(a[5]), int(a[6]), a[7]) for k, a in log2 if k == "replay"] == [(21, 20, 32), (19, 18, 32), (27, 26, 32)]


def test_defaults_are_unchanged_for_a_concatenation_model():
    from vimo_clip_amd.TFAM.train_and_eval import Config, GraphedEvalForward
    for concat_dim in (1, -1):
        m = _tiny(use_cross_attention=False, concat_dim=concat_dim)
        cfg = Config(batch_size=3, d_model=64, device="cpu")
        gf = GraphedEvalForward(m, cfg, bucket=16, streams=1)
        assert gf.bucket == 1 and gf.pooled is None and gf.concat is None
        on = GraphedEvalForward(m, cfg, bucket=16, streams=1, concat_bucket=True)
        assert on.bucket == 16 and on.pooled is None and on.concat == ("time" if concat_dim == 1 else "feature")
        log = []
        step = graphs.GraphedTrainStep(lambda *a: a[0].sum(), _Opt(), bucket=16, pooled=graphs.pooled_stream(m),
                                       graph_factory=_recording_factory(log))
        for T in (21, 19):
            step(*_batch(T))
        assert step.n_graphs == 2 and all(len(a) == 5 for _, a in log)          # exact shapes, nothing appended
        rgb, mot, mr, mf, _ = _batch(21, D=64)
        with pytest.raises(ValueError, match="pool_len"):
            m(rgb, mot, mask_rgb=mr, mask_flow=mf, pool_len=21)
    cross = GraphedEvalForward(_tiny(), Config(batch_size=3, d_model=64, device="cpu"), bucket=16, streams=1, concat_bucket=True)
    assert cross.bucket == 16 and cross.pooled == "rgb" and cross.concat is None       # the switch does not touch the pooled modes


def test_token_lens_refusals():
    rgb, mot, mr, mf, _ = _batch(21, D=64)
    with pytest.raises(ValueError, match="concatenation"):
        _tiny()(rgb, mot, mask_rgb=mr, mask_flow=mf, token_lens=(21, 20))
    with pytest.raises(ValueError, match="concatenation"):
        _tiny(use_only_flow=True, use_cross_attention=False)(rgb, mot, mask_rgb=mr, mask_flow=mf, token_lens=(21, 20))
    time_m, feat_m = _tiny(use_cross_attention=False, concat_dim=1), _tiny(use_cross_attention=False, concat_dim=-1)
    for m in (time_m, feat_m):
        with pytest.raises(ValueError, match="pool_len"):
            m(rgb, mot, mask_rgb=mr, mask_flow=mf, token_lens=(21, 20), pool_len=21)
        with pytest.raises(ValueError, match="require grad"):
            m(rgb.clone().requires_grad_(True), mot, mask_rgb=mr, mask_flow=mf, token_lens=(21, 20))
        with pytest.raises(ValueError, match="require grad"):
            m(rgb, mot.clone().requires_grad_(True), mask_rgb=mr, mask_flow=mf, token_lens=(21, 20))
    with pytest.raises(ValueError, match="mask_flow"):
        feat_m(rgb, mot, mask_rgb=mr, token_lens=(21, 20))
    with pytest.raises(ValueError, match="T_rgb >= T_motion"):
        feat_m(mot, rgb, mask_rgb=mf, mask_flow=mr, token_lens=(20, 21))
    with pytest.raises(ValueError, match="concat_len"):
        time_m(rgb, mot, mask_rgb=mr, mask_flow=mf, concat_len=48)


def test_config_graph_bucket_concat_default_and_yaml(tmp_path):
    from vimo_clip_amd.TFAM.train_and_eval import Config
    assert Config().graph_bucket_concat is False
    assert Config(graph_bucket_concat=True).graph_bucket_concat is True
    yaml = pytest.importorskip("yaml")
    cfg = dict(training=dict(mode="train", seed=1, lr=1e-4, epochs=1, batch_size=8, num_workers=0, device="cuda"),
               logging=dict(log_dir="l", checkpoint_dir="c"),
               data=dict(num_classes=4, class_names_dir=None, train_dataset_path=None, val_dataset_path=None, flow_dataset_path=None),
               model=dict(d_model=64, nhead=1, num_layers=1, dim_feedforward=64, use_cross_attention=False, concat_dim=1, dropout=0.1,
                          mlp_dropout=0.1, use_pe=False, use_only_rgb=False, use_only_flow=False))
    p = tmp_path / "a.yaml"
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).graph_bucket_concat is False
    cfg["training"]["graph_bucket_concat"] = True
    cfg["training"]["graph_bucket"] = 32
    p.write_text(yaml.safe_dump(cfg))
    c = Config.from_yaml(str(p))
    assert c.graph_bucket_concat is True and c.graph_bucket == 32


# ---- the contract's restatement ----------------------------------------------------------------------------------------------------

def test_concat_ref_clamps_and_layout():
    B, Tr, Tm, D = 3, 9, 8, 6
    rgb, mot = torch.randn(B, Tr, D), torch.randn(B, Tm, D)
    mr, mf = torch.rand(B, Tr) < 0.7, torch.rand(B, Tm) < 0.7
    x, m, n = concat_ref(rgb, mot, mr, mf, 16)
    assert n == 16 and torch.equal(x, torch.cat([rgb[:, :-1], mot], 1)) and torch.equal(m.bool(), torch.cat([mr[:, :-1], mf], 1))
    assert clamp_lens(None, None, Tr, Tm, 24) == (8, 8, 16)
    assert clamp_lens(5, 3, Tr, Tm, 16) == (4, 3, 7)
    assert clamp_lens(1, 1, Tr, Tm, 16) == (0, 1, 1)
    assert clamp_lens(0, 0, Tr, Tm, 16) == (0, 1, 1)                # clamped up to 1
    assert clamp_lens(-7, 2, Tr, Tm, 16) == (0, 2, 2)
    assert clamp_lens(100, 100, Tr, Tm, 16) == (8, 8, 16)           # clamped down to the tensors
    assert clamp_lens(100, 100, Tr, Tm, 12) == (8, 4, 12)           # ... and cut at T_out
    assert clamp_lens(9, 8, Tr, Tm, 5) == (5, 0, 5)
    x, m, n = concat_ref(rgb, mot, None, None, 24, 5, 3)
    assert n == 7 and torch.equal(x[:, :4], rgb[:, :4]) and torch.equal(x[:, 4:7], mot[:, :3]) and x[:, 7:].abs().max() == 0
    assert m[:, :7].all() and not m[:, 7:].any()


# ---- the identity, float64 ---------------------------------------------------------------------------------------------------------

def _tail(sd, pooled):
    h = F.layer_norm(pooled, (pooled.shape[-1],), sd["classifier.0.weight"], sd["classifier.0.bias"], 1e-5)
    h = F.gelu(h @ sd["classifier.1.weight"].t() + sd["classifier.1.bias"])
    return h @ sd["classifier.4.weight"].t() + sd["classifier.4.bias"]


@pytest.mark.parametrize("pe", [False, True], ids=["nope", "pe"])
@pytest.mark.parametrize("mode", ["concat1", "concat-1"])
def test_padded_prefix_concatenation_is_the_reference_forward(mode, pe):
    """B = 4, 21 / 20 tokens with shorter clips, padded to bucket 16 (32 / 32 tokens, 48 concatenated): the layers and the classifier
    tail of the oracle on concat_ref's rows, pooled over n, against oracle.tfam.amo_clip_forward on the unpadded batch, in float64.
    Bound 1e-12 (the operations on rows 0..n-1 are the same ones; only the reduction shapes of the matrix products differ)."""
    D, H, L, FF, C = 64, 4, 2, 128, 10
    c = dict(B=4, Tr=21, Tf=20, D=D, ragged=True, seed=911)
    sd = {k: v.double() for k, v in synth.tfam_state_dict(D, H, L, FF, C, 912).items()}
    rgb, mot, mr, mf = mg.tfam_inputs(c)
    rgb, mot = rgb.double(), mot.double()
    assert int(mr.sum(1).min()) < 21
    ref = otfam.amo_clip_forward(sd, rgb, mot, mr, mf, nhead=H, use_pe=pe, **mg.tfam_mode_kwargs(mode))
    cmode = "time" if mode == "concat1" else "feature"
    prgb, pmot, pmr, pmf, nr, nm, T_out = graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 16, cmode)
    assert (prgb.shape[1], pmot.shape[1], nr, nm) == (32, 32, 21, 20)
    if pe:                                                       # per stream, over the PADDED length: row t gets the same phase
        prgb = prgb + otfam.positional_encoding(32, D).unsqueeze(0)
        pmot = pmot + otfam.positional_encoding(32, D).unsqueeze(0)
    if cmode == "time":
        assert T_out == 48
        x, m, n = concat_ref(prgb, pmot, pmr, pmf, T_out, nr, nm)
        assert n == 40
    else:
        x = torch.cat([prgb[:, :pmot.shape[1]], pmot], -1) @ sd["projection_layer.weight"].t() + sd["projection_layer.bias"]
        m, n = pmf, nm
    kpm = ~m.bool()
    for i in range(L):
        x = otfam.attention_layer(sd, f"layers.{i}.", x, H, src_kpm=kpm)
    got = _tail(sd, x[:, :n].mean(dim=1))
    err = (got - ref).abs().max().item()
    print(f"concat identity {mode} pe={pe}: max |d logits| {err:.3e} (|ref|max {ref.abs().max().item():.3f})")
    assert err <= 1e-12
    # the control: pooling the padded rows as well is NOT the reference
    assert (_tail(sd, x.mean(dim=1)) - ref).abs().max().item() > 1e-6
