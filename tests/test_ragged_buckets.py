"""CPU: the length-bucket rule of the graph managers (vimo_clip_amd/graphs.py) for ragged clip batches.

A batch zero-padded to the next multiple of ``bucket`` shares one captured graph with every batch of that bucket; its own length
travels as ``pool_len``, one more static input (the mean-pool kernels read it from device memory; tests/test_gpu_tfam_ragged.py
checks the arithmetic on the GPU).  Here: which graphs are captured, what they are handed, and what the padding helper writes.
"""
import pytest
import torch

from vimo_clip_amd import graphs


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


LENGTHS = [17, 20, 31, 32, 33, 40, 48]


def test_bucketed_train_step_captures_one_graph_per_padded_shape():
    log, seen = [], []

    def step_fn(rgb, mot, mr, mf, labels, pool_len=None):
        seen.append((tuple(rgb.shape), tuple(mot.shape), tuple(mr.shape), tuple(mf.shape), tuple(labels.shape),
                     None if pool_len is None else int(pool_len)))
        return rgb.sum()

    step = graphs.GraphedTrainStep(step_fn, _Opt(), bucket=16, graph_factory=_recording_factory(log))
    for T in LENGTHS:
        step(*_batch(T))
    captures = [a for kind, a in log if kind == "capture"]
    assert [(a[0].shape[1], a[1].shape[1]) for a in captures] == [(32, 16), (32, 32), (48, 32), (48, 48)]
    assert len(step._graphs) == 4
    replays = [a for kind, a in log if kind == "replay"]
    assert len(replays) == len(LENGTHS)
    for T, a in zip(LENGTHS, replays):
        rgb, mot, mr, mf, labels, pool_len = a
        Tr, Tf = -(-T // 16) * 16, -(-(T - 1) // 16) * 16
        assert rgb.shape == (3, Tr, 8) and mot.shape == (3, Tf, 8) and mr.shape == (3, Tr) and mf.shape == (3, Tf)
        assert labels.shape == (3, 4)
        assert pool_len.dtype == torch.int32 and pool_len.numel() == 1 and int(pool_len) == T      # the ORIGINAL RGB length
    assert [s[5] for s in seen] == LENGTHS             # step_fn saw it as its last argument
    assert step.opt.step_count == len(LENGTHS)


def test_bucket_1_keys_on_exact_shapes_and_passes_no_pool_len():
    log = []

    def step_fn(*inputs):
        assert len(inputs) == 5                        # exactly what the caller passed: today's behaviour
        return inputs[0].sum()

    step = graphs.GraphedTrainStep(step_fn, _Opt(), graph_factory=_recording_factory(log))
    for T in LENGTHS:
        step(*_batch(T))
    captures = [a for kind, a in log if kind == "capture"]
    assert len(captures) == len(step._graphs) == 7
    assert [a[0].shape[1] for a in captures] == LENGTHS


def test_motion_pooled_models_carry_the_motion_length():
    log = []
    step = graphs.GraphedTrainStep(lambda *a: a[0].sum(), _Opt(), bucket=16, pooled="motion", graph_factory=_recording_factory(log))
    step(*_batch(20))
    assert int(log[-1][1][-1]) == 19


def test_pad_to_bucket_zero_fills_tokens_and_masks():
    rgb, mot, mr, mf, _ = _batch(21)
    prgb, pmot, pmr, pmf, n = graphs.pad_to_bucket(rgb, mot, mr, mf, 16)
    assert n == 21 and prgb.shape == (3, 32, 8) and pmot.shape == (3, 32, 8)
    assert torch.equal(prgb[:, :21], rgb) and torch.equal(pmot[:, :20], mot)
    assert prgb[:, 21:].abs().max() == 0 and pmot[:, 20:].abs().max() == 0
    assert pmr.dtype == mr.dtype and torch.equal(pmr[:, :21], mr) and not pmr[:, 21:].any()
    assert torch.equal(pmf[:, :20], mf) and not pmf[:, 20:].any()
    # a length that already is a multiple of the bucket is left alone (same tensors), and still reports its length
    rgb, mot, mr, mf, _ = _batch(33)
    out = graphs.pad_to_bucket(rgb, mot, mr, mf, 16)
    assert out[0].shape[1] == 48 and out[1] is mot and out[3] is mf and out[4] == 33


def test_pad_to_bucket_synthesises_masks_over_the_original_length():
    rgb, mot, _, _, _ = _batch(21, masks=False)
    _, _, pmr, pmf, n = graphs.pad_to_bucket(rgb, mot, None, None, 16)
    assert n == 21 and pmr.shape == (3, 32) and pmf.shape == (3, 32)
    assert pmr[:, :21].all() and not pmr[:, 21:].any()        # otherwise the new rows would be attended to
    assert pmf[:, :20].all() and not pmf[:, 20:].any()
    # also when the length needs no padding: the model then sees the same mask an unmasked call implies
    rgb, mot = torch.randn(2, 32, 8), torch.randn(2, 31, 8)
    _, _, pmr, pmf, n = graphs.pad_to_bucket(rgb, mot, None, None, 16)
    assert n == 32 and pmr.all() and pmr.shape == (2, 32) and pmf[:, :31].all() and not pmf[:, 31:].any()


def test_concat_modes_are_left_at_exact_shapes():
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    kw = dict(d_model=64, nhead=1, num_layers=1, dim_feedforward=64, num_classes=4, device="cpu")
    assert graphs.pooled_stream(AMO_CLIP(**kw)) == "rgb"
    assert graphs.pooled_stream(AMO_CLIP(use_only_rgb=True, **kw)) == "rgb"
    assert graphs.pooled_stream(AMO_CLIP(use_only_flow=True, **kw)) == "motion"
    for concat_dim in (1, -1):
        m = AMO_CLIP(use_cross_attention=False, concat_dim=concat_dim, **kw)
        assert graphs.pooled_stream(m) is None
        rgb, mot, mr, mf, labels = _batch(21)
        out = graphs.pad_to_bucket(rgb, mot, mr, mf, 16, graphs.pooled_stream(m))
        assert out[0] is rgb and out[1] is mot and out[2] is mr and out[3] is mf and out[4] is None
        log = []
        step = graphs.GraphedTrainStep(lambda *a: a[0].sum(), _Opt(), bucket=16, pooled=graphs.pooled_stream(m),
                                       graph_factory=_recording_factory(log))
        for T in (17, 20):
            step(*_batch(T))
        assert len(step._graphs) == 2 and all(len(a) == 5 for _, a in log)
        with pytest.raises(ValueError, match="pool_len"):
            m(rgb, mot, mask_rgb=mr, mask_flow=mf, pool_len=21)


def test_config_graph_bucket_default_and_yaml(tmp_path):
    from vimo_clip_amd.TFAM.train_and_eval import Config
    assert Config().graph_bucket == 1 and Config().use_graphs is False
    assert Config(graph_bucket=16).graph_bucket == 16
    yaml = pytest.importorskip("yaml")
    cfg = dict(training=dict(mode="train", seed=1, lr=1e-4, epochs=1, batch_size=8, num_workers=0, device="cuda"),
               logging=dict(log_dir="l", checkpoint_dir="c"),
               data=dict(num_classes=4, class_names_dir=None, train_dataset_path=None, val_dataset_path=None, flow_dataset_path=None),
               model=dict(d_model=64, nhead=1, num_layers=1, dim_feedforward=64, use_cross_attention=True, concat_dim=1, dropout=0.1,
                          mlp_dropout=0.1, use_pe=False, use_only_rgb=False, use_only_flow=False))
    p = tmp_path / "a.yaml"
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).graph_bucket == 1
    cfg["training"]["graph_bucket"] = 32
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).graph_bucket == 32
