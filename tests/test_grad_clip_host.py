"""CPU: the host side of device-side gradient clipping (vmc_grad_clip_dev; the arithmetic is checked on the GPU in
tests/test_gpu_grad_clip.py).  The trainer's option, which device slot the optimiser's host writes go to, what the graph manager
saves around a capture, and the combinations that must keep raising.
"""
import pytest
import torch

from vimo_clip_amd import graphs
from vimo_clip_amd.optim import FusedAdam, GradArena


def _yaml_cfg():
    return dict(training=dict(mode="train", seed=1, lr=1e-4, epochs=1, batch_size=8, num_workers=0, device="cuda"),
                logging=dict(log_dir="l", checkpoint_dir="c"),
                data=dict(num_classes=4, class_names_dir=None, train_dataset_path=None, val_dataset_path=None, flow_dataset_path=None),
                model=dict(d_model=64, nhead=1, num_layers=1, dim_feedforward=64, use_cross_attention=True, concat_dim=1, dropout=0.1,
                           mlp_dropout=0.1, use_pe=False, use_only_rgb=False, use_only_flow=False))


def test_config_grad_clip_norm_default_and_yaml(tmp_path):
    from vimo_clip_amd.TFAM.train_and_eval import Config
    assert Config().grad_clip_norm is None
    assert Config(grad_clip_norm=0.5).grad_clip_norm == 0.5
    yaml = pytest.importorskip("yaml")
    cfg = _yaml_cfg()
    p = tmp_path / "a.yaml"
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).grad_clip_norm is None
    cfg["training"]["grad_clip_norm"] = 1
    p.write_text(yaml.safe_dump(cfg))
    got = Config.from_yaml(str(p)).grad_clip_norm
    assert got == 1.0 and isinstance(got, float)
    assert Config.from_yaml(str(p), grad_clip_norm=None).grad_clip_norm is None      # overrides win, as for every key


class _Arena:
    pass


class _Opt:           # the attribute surface GraphedTrainStep uses of optim.FusedAdam in device-state mode
    def __init__(self, n=8, clip=False):
        self.arena = _Arena()
        self.arena.flat_param, self.arena.flat_grad = torch.zeros(n), torch.zeros(n)
        self.m, self.v = torch.zeros(n), torch.zeros(n)
        self.dev_state, self.dev_hyper = torch.zeros(4, dtype=torch.int64), torch.zeros(4)
        self.step_count = 0
        if clip:
            self.dev_clip = torch.tensor([0.5, 0.7, 0.0, 0.0])


def _warming_factory(log):
    class _Stub:          # stands in for GraphedCallable: the capture runs fn once (the warm-up), a replay only records
        def __init__(self, fn, *example_inputs, warmup=1):
            log.append("capture")
            fn(*example_inputs)

        def __call__(self, *inputs):
            log.append("replay")
    return _Stub


def test_capture_restores_the_clip_state_of_the_warm_up():
    opt = _Opt(clip=True)

    def step_fn(x):                                     # what a warm-up step leaves behind: norm, coefficient, final scale
        opt.dev_clip[2:] = torch.tensor([3.0, 0.25])
        opt.dev_hyper[3] = 0.125
        opt.arena.flat_param += 1

    log = []
    step = graphs.GraphedTrainStep(step_fn, opt, graph_factory=_warming_factory(log))
    step(torch.zeros(2, 3))
    assert log == ["capture", "replay"]
    assert opt.dev_clip.tolist() == [0.5, pytest.approx(0.7), 0.0, 0.0]
    assert opt.dev_hyper[3] == 0 and opt.arena.flat_param.abs().max() == 0 and opt.step_count == 1


def test_optimisers_without_clip_state_still_capture():
    opt = _Opt()
    assert not hasattr(opt, "dev_clip")
    log = []
    step = graphs.GraphedTrainStep(lambda x: opt.arena.flat_param.add_(1), opt, graph_factory=_warming_factory(log))
    assert len(step._live()) == 6
    step(torch.zeros(2, 3))
    step(torch.zeros(2, 3))
    assert log == ["capture", "replay", "replay"] and opt.arena.flat_param.abs().max() == 0 and opt.step_count == 2
    opt.dev_clip = None                                 # FusedAdam before the first clipped step
    assert len(step._live()) == 6


def _cpu_optimizer():
    ps = [torch.nn.Parameter(torch.randn(16, 8)), torch.nn.Parameter(torch.randn(8))]
    return FusedAdam(GradArena(ps), lr=1e-3).enable_device_state()


def test_host_writes_go_to_the_clip_slots_while_clipping_is_on():
    opt = _cpu_optimizer()
    assert opt.dev_clip is None
    with pytest.raises(RuntimeError, match="clipping"):
        opt.last_clip_coef
    opt.sync_hyper(grad_scale=0.5)
    assert opt.dev_hyper[3] == 0.5
    opt._set_clip(0.7)                                  # what step(max_grad_norm=0.7) does first
    assert opt.dev_clip.shape == (4,) and opt.dev_clip.dtype == torch.float32
    assert opt.dev_clip[0] == 0.5 and opt.dev_clip[1] == torch.tensor(0.7)      # base_scale carried over, threshold
    opt.dev_hyper[3] = -1.0                             # now the device's slot: the host must leave it alone
    opt.sync_hyper(grad_scale=0.25)
    assert opt.dev_clip[0] == 0.25 and opt.dev_hyper[3] == -1.0
    opt.dev_clip[0] = 9.0                               # unchanged (lr, grad_scale, max_norm): no write
    opt.sync_hyper(grad_scale=0.25)
    assert opt.dev_clip[0] == 9.0
    clip = opt.dev_clip
    opt._set_clip(1.5)                                  # a new threshold re-writes both host slots of the SAME buffer
    assert opt.dev_clip is clip and clip[0] == 0.25 and clip[1] == 1.5
    assert opt.last_grad_norm.data_ptr() == clip[2:3].data_ptr() and opt.last_clip_coef.data_ptr() == clip[3:4].data_ptr()
    assert opt.last_grad_norm.shape == opt.last_clip_coef.shape == (1,)
    opt._set_clip(None)                                 # clipping off: hyper[3] is the host's again
    assert opt.dev_hyper[3] == 0.25
    opt.sync_hyper(grad_scale=1.0)
    assert opt.dev_hyper[3] == 1.0 and clip[0] == 0.25


def test_clipping_with_backward_overlap_still_raises(monkeypatch):
    class _Stream:
        def __init__(self, *a, **k):
            pass
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    for device_state in (False, True):
        ps = [torch.nn.Parameter(torch.randn(16, 8)), torch.nn.Parameter(torch.randn(8))]
        opt = FusedAdam(GradArena(ps), lr=1e-3)
        if device_state:
            opt.enable_device_state()
        opt.enable_backward_overlap([[ps[0]]])
        opt._ov["used"] = opt._ov["done"][0] = True     # as after group_ready(0) during a backward
        with pytest.raises(ValueError, match="overlap"):
            opt.step(max_grad_norm=1.0)
        assert getattr(opt, "dev_clip", None) is None
