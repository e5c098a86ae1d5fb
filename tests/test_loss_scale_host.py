"""CPU: dynamic loss scaling (DESIGN.md "Dynamic loss scaling") -- the reference state machine of tests/loss_scale_ref.py against
torch._amp_update_scale_ bit for bit, the scaler record's ctypes mirror against include/vmc.h, the Python error paths and the
trainers' --loss_scale / --compute_dtype arguments.  The kernels themselves: tests/test_gpu_loss_scale.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loss_scale_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_run(scale, found_seq, growth, backoff, interval):
    s = torch.tensor([scale], dtype=torch.float32)
    tracker = torch.zeros(1, dtype=torch.int32)
    out = []
    for f in found_seq:
        torch._amp_update_scale_(s, tracker, torch.tensor([1.0 if f else 0.0]), growth, backoff, interval)
        out.append((np.float32(s.item()), int(tracker.item())))
    return out


def _same(ref, tor):
    assert len(ref) == len(tor)
    for i, ((s, t, _), (ts, tt)) in enumerate(zip(ref, tor)):
        assert np.float32(s).tobytes() == np.float32(ts).tobytes() and t == tt, (i, s, t, ts, tt)


def test_the_two_sequences_of_the_design_note():
    seq = [0, 0, 1, 0, 0, 0]
    ref = R.run(65536.0, seq, 2.0, 0.5, 2)
    assert [float(s) for s, _, _ in ref] == [65536.0, 131072.0, 65536.0, 65536.0, 131072.0, 131072.0]
    assert [k for _, _, k in ref] == [0, 0, 1, 1, 1, 1]
    _same(ref, _torch_run(65536.0, seq, 2.0, 0.5, 2))
    big = R.run(3e38, [0, 0], 2.0, 0.5, 1)                 # 6e38 is not finite in fp32: S stays, the tracker is reset all the same
    assert [float(s) for s, _, _ in big] == [float(np.float32(3e38))] * 2 and [t for _, t, _ in big] == [0, 0]
    _same(big, _torch_run(3e38, [0, 0], 2.0, 0.5, 1))


@pytest.mark.parametrize("interval", [1, 3, 2000])
@pytest.mark.parametrize("growth,backoff", [(2.0, 0.5), (1.0, 1.0), (2.0, 2.0 ** -8)])
def test_random_sequences_equal_torch_bit_for_bit(growth, backoff, interval):
    for seed in range(4):
        rng = np.random.default_rng(100 * seed + interval)
        seq = (rng.random(64) < (0.5, 0.2, 0.05, 0.8)[seed]).astype(int).tolist()
        for s0 in (65536.0, 1.0, 2.0 ** 100, 3.0e38, 2.0 ** -120):
            ref = R.run(s0, seq, growth, backoff, interval)
            _same(ref, _torch_run(s0, seq, growth, backoff, interval))
            assert ref[-1][2] == sum(seq)                  # skipped = the overflowing steps


def test_loss_scale_struct_mirrors_the_header():
    """vmc_loss_scale_state (include/vmc.h) is written from Python through the ctypes mirror LossScaleStruct: the same field names in
    the same order, four floats then four ints, 32 bytes, found_inf (the Adam entries' skip flag) at byte 24."""
    from vimo_clip_amd.optim import LossScaleStruct
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vmc.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vmc_loss_scale_state\s*\{(.*?)\}\s*vmc_loss_scale_state\s*;", src, flags=re.S).group(1)
    names, kinds = [], []
    for d in (d.strip() for d in body.split(";") if d.strip()):
        m = re.match(r"^(float|int)\s+(\w+)$", d)
        assert m, d
        names.append(m.group(2))
        kinds.append(ctypes.c_float if m.group(1) == "float" else ctypes.c_int)
    assert names == [f[0] for f in LossScaleStruct._fields_] and kinds == [f[1] for f in LossScaleStruct._fields_]
    assert names == ["scale", "growth_factor", "backoff_factor", "base_scale", "growth_interval", "growth_tracker", "found_inf", "skipped"]
    assert ctypes.sizeof(LossScaleStruct) == 32 and LossScaleStruct.found_inf.offset == 24 and LossScaleStruct.base_scale.offset == 12


def _cpu_optimizer():
    from vimo_clip_amd.optim import FusedAdam, GradArena
    ps = [torch.nn.Parameter(torch.zeros(8, 8)), torch.nn.Parameter(torch.zeros(5))]
    return ps, FusedAdam(GradArena(ps), lr=1e-3)


def test_enable_loss_scaling_needs_device_state():
    _, opt = _cpu_optimizer()
    with pytest.raises(RuntimeError, match="enable_device_state"):
        opt.enable_loss_scaling()
    with pytest.raises(RuntimeError, match="loss scaling is off"):
        opt.loss_scale
    loss = torch.ones(())
    assert opt.scale_loss(loss) is loss and opt.scale_grad(loss) is loss          # off: nothing is wrapped


def test_loss_scaling_excludes_backward_overlap_both_ways(monkeypatch):
    ps, opt = _cpu_optimizer()
    opt.enable_device_state().enable_loss_scaling(init_scale=1024.0, growth_interval=7)
    with pytest.raises(RuntimeError, match="loss scaling"):
        opt.enable_backward_overlap([ps])                   # raises before it creates its side stream
    rec = opt.dev_ls
    assert rec.dtype == torch.int32 and rec.numel() == 8
    assert rec.view(torch.float32)[:4].tolist() == [1024.0, 2.0, 0.5, 1.0] and rec[4:].tolist() == [7, 0, 0, 0]
    assert opt.loss_scale.item() == 1024.0 and opt.last_found_inf.item() == 0 and opt.skipped_steps.item() == 0
    opt.sync_hyper(grad_scale=0.25)                         # the reducer's 1 / world goes to the record, not to hyper[3]
    assert opt.dev_ls.view(torch.float32)[3].item() == 0.25 and opt.dev_hyper[3].item() == 1.0
    sd = opt.state_dict()
    assert sd["loss_scale"].tolist() == opt.dev_ls.tolist() and sd["step"] == 0
    opt.disable_loss_scaling()
    assert opt.dev_ls is None and opt.dev_hyper[3].item() == 0.25                 # the host owns hyper[3] again
    ps2, opt2 = _cpu_optimizer()
    opt2.enable_device_state()
    opt2._ov = {"ranges": [], "used": False}                # what enable_backward_overlap leaves (its stream needs a device)
    with pytest.raises(RuntimeError, match="enable_backward_overlap"):
        opt2.enable_loss_scaling()
    for bad in (dict(init_scale=0.0), dict(init_scale=float("inf")), dict(growth_factor=0.5), dict(backoff_factor=0.0),
                dict(backoff_factor=2.0), dict(growth_interval=0)):
        opt2._ov = None
        with pytest.raises(ValueError):
            opt2.enable_loss_scaling(**bad)


def test_state_dict_round_trip_carries_the_record():
    _, a = _cpu_optimizer()
    a.enable_device_state().enable_loss_scaling(init_scale=4096.0, growth_factor=2.0, backoff_factor=0.25, growth_interval=11)
    a.dev_ls[5:] = torch.tensor([3, 1, 9], dtype=torch.int32)
    a.dev_state[0] = 17                                     # the true step count; the host mirror counts attempts
    a.step_count = 26
    sd = a.state_dict()
    assert sd["step"] == 17
    _, b = _cpu_optimizer()
    b.enable_device_state().enable_loss_scaling()
    b.load_state_dict(sd)
    assert b.dev_ls.tolist() == a.dev_ls.tolist() and int(b.dev_state[0]) == 17 and b.step_count == 17
    _, c = _cpu_optimizer()                                  # a checkpoint written without scaling loads as before
    c.enable_device_state()
    plain = c.state_dict()
    assert "loss_scale" not in plain and set(plain) == {"step", "m", "v", "lr"}
    b.load_state_dict(plain)
    assert b.dev_ls.tolist()[:3] == a.dev_ls.tolist()[:3]   # the record is left alone


TODAY_STUDENT = dict(synthetic=256, clip_model_name="ViT-B/32", num_classes=140, batch_size=8, sequence_length=17, epochs=1,
                     learning_rate=1e-3, distillation_loss_mode="cosine", class_positive_weight=9, residual_alpha=0.1,
                     grad_clip_norm=None, checkpoint_dir=None, recompute="none", accum_steps=1, single_label=False,
                     clip_embeddings_dir=None, flow_videos_dir=None, val_clip_embeddings_dir=None, val_flow_videos_dir=None)


def test_loss_scale_argument_parsing_and_untouched_defaults():
    from vimo_clip_amd import train, train_frame_diff_mn
    from vimo_clip_amd.TFAM.train_and_eval import Config
    assert train.parse_loss_scale("off") is None and train.parse_loss_scale("dynamic") == {}
    assert train.parse_loss_scale("1024") == {"init_scale": 1024.0, "growth_factor": 1.0, "backoff_factor": 1.0}
    assert train.parse_loss_scale(" 2.5e3 ")["init_scale"] == 2500.0
    for bad in ("on", "", "-4", "0", "inf", "nan"):
        with pytest.raises(ValueError, match="loss_scale"):
            train.parse_loss_scale(bad)
    ns = vars(train.build_parser().parse_args([]))
    assert ns.pop("compute_dtype") == "bf16" and ns.pop("loss_scale") == "off"
    assert ns == TODAY_STUDENT                               # everything else: the namespace as it was
    ns = train.build_parser().parse_args(["--compute_dtype", "f16", "--loss_scale", "Dynamic"])
    assert ns.compute_dtype == "f16" and ns.loss_scale == "dynamic"
    assert train.build_parser().parse_args(["--loss_scale", "512"]).loss_scale == "512"
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--loss_scale", "sometimes"])
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--compute_dtype", "f32"])
    need = ["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c"]
    mn = train_frame_diff_mn.build_parser().parse_args(need)
    assert mn.compute_dtype == "bf16" and mn.loss_scale == "off"
    assert train_frame_diff_mn.build_parser().parse_args(need + ["--loss-scale", "dynamic", "--compute-dtype", "f16"]).loss_scale == "dynamic"
    assert Config().loss_scale == "off" and Config(loss_scale="dynamic").loss_scale == "dynamic"


def test_tfam_yaml_loss_scale(tmp_path):
    import yaml
    from vimo_clip_amd.TFAM.train_and_eval import Config
    base = dict(training=dict(mode="both", seed=1, lr=1e-4, epochs=1, batch_size=2, num_workers=0, device="cuda"),
                logging=dict(log_dir="l", checkpoint_dir="c"),
                data=dict(num_classes=4, class_names_dir="n", train_dataset_path="t", val_dataset_path="v", flow_dataset_path="f"),
                model=dict(d_model=64, nhead=2, num_layers=1, dim_feedforward=64, use_cross_attention=True, concat_dim=1, dropout=0.0,
                           mlp_dropout=0.0, use_pe=False, use_only_rgb=False, use_only_flow=False))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(base))
    assert Config.from_yaml(str(p)).loss_scale == "off"
    for value, want in (("dynamic", "dynamic"), (1024, "1024"), (False, "off")):
        base["training"]["loss_scale"] = value
        p.write_text(yaml.safe_dump(base))
        assert Config.from_yaml(str(p)).loss_scale == want
    assert Config.from_yaml(str(p), loss_scale="dynamic").loss_scale == "dynamic"
