"""CPU: the references of the weight-average kernels (tests/ema_refs.py) against torch's own EMA helper and the closed form, the
warm-up weight, the e32 yardstick, mutants of the arithmetic that the element bound must reject, the kept resource-usage remarks of
ema.hip, the ctypes table, the command lines / YAML key, and the optimiser's host-side state machine with the launches replaced by the
reference."""
import os
import re

import numpy as np
import pytest
import torch

import ema_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SIZES = [1, 3, 4, 1023, 4101]


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1e-4, 1e-2, 0.5, 0.75])
def test_float64_reference_equals_torch_swa_utils(w):
    from torch.optim.swa_utils import get_ema_multi_avg_fn
    w32 = np.float32(w)
    decay = 1.0 - float(w32)                                             # exact in float64: w32 has 24 significant bits
    assert 1.0 - decay == float(w32)
    e, p = R.inputs(4101, seed=1)
    avg = [torch.from_numpy(e.astype(np.float64))]
    get_ema_multi_avg_fn(decay)(avg, [torch.from_numpy(p.astype(np.float64))], 1)
    r64 = R.ema_ref(e, p, w32)
    assert r64.dtype == np.float64
    assert np.abs(avg[0].numpy() - r64).max() <= 1e-15 * np.abs(r64).max()


def test_closed_form_for_constant_parameters():
    e0, p = R.inputs(257, seed=2)
    for w in (np.float32(1e-2), np.float32(0.5), np.float32(1e-4)):
        e = e0.astype(np.float64)
        for k in range(1, 41):
            e = R.ema_ref(e, p, w)                                       # float64 all the way: no per-step fp32 rounding
            want = p.astype(np.float64) + (1.0 - float(w)) ** k * (e0.astype(np.float64) - p.astype(np.float64))
            assert np.abs(e - want).max() <= 1e-12 * np.abs(want).max(), (w, k)


def test_warmup_weight_is_one_minus_the_usual_decay_schedule():
    for decay in (0.9999, 0.999, 0.99):
        omd = R.one_minus_decay(decay)
        assert omd.dtype == np.float32 and abs(float(omd) - (1.0 - decay)) <= 2.0 ** -24 * (1.0 - decay)
        worst = 0.0
        for t in range(1, 10 ** 5 + 1):
            w = R.weight_of(omd, True, t)
            want = 1.0 - min(decay, (1.0 + t) / (10.0 + t))
            worst = max(worst, abs(float(w) - want) / want)
        assert worst <= 2.0 ** -23, (decay, worst)
        assert R.weight_of(omd, False, 1) == omd and R.weight_of(omd, True, 10 ** 7) == omd
    assert R.weight_of(np.float32(1e-4), True, 1) == np.float32(9.0) / np.float32(11.0)
    assert np.float32(1.0) - np.float32(0.9999) != R.one_minus_decay(0.9999)      # why the host passes 1 - decay, not decay
    assert abs(float(np.float32(1.0) - np.float32(0.9999)) - 1e-4) / 1e-4 > 1e-4


CASES = [(n, w) for n in HOST_SIZES for w in R.WEIGHTS + (float(np.float32(9.0) / np.float32(11.0)),)]


@pytest.mark.parametrize("n,w", CASES)
def test_e32_yardstick_and_the_fp32_model_inside_the_bound(n, w):
    e, p = R.inputs(n, seed=3)
    assert R.e32_of(e, p, w) <= R.E32_MAX
    assert R.excess(R.ema_model32(e, p, w), e, p, w) <= 1.0              # the kernel's arithmetic, modelled in fp32
    assert R.excess(R.ema_ref(e, p, w).astype(np.float32), e, p, w) <= 1.0


def test_fp32_model_stays_inside_the_bound_without_the_quotient_slack():
    """2^20 normal samples per weight: |model32 - r64| <= 2^-24 (w |p - e| + |r64|) + 2^-149, the bound without the 2 units granted
    to a device quotient one ulp away."""
    e, p = R.inputs(1 << 20, seed=4)
    for w in R.WEIGHTS + (float(np.float32(9.0) / np.float32(11.0)),):
        r64 = R.ema_ref(e, p, w)
        tight = R.EPS24 * (float(np.float32(w)) * np.abs(p.astype(np.float64) - e.astype(np.float64)) + np.abs(r64)) + R.TINY
        assert (np.abs(R.ema_model32(e, p, w).astype(np.float64) - r64) <= tight).all(), w


# ---- mutants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1e-2, 1e-4])
def test_mutant_decay_where_one_minus_decay_belongs(w):
    e, p = R.inputs(4101, seed=5)
    assert R.excess(R.ema_model32(e, p, np.float32(1.0) - np.float32(w)), e, p, w) > 1.0


@pytest.mark.parametrize("t", [1, 2, 89, 90])
def test_mutant_warmup_count_off_by_one(t):
    e, p = R.inputs(4101, seed=6)
    omd = R.one_minus_decay(0.9999)
    w = R.weight_of(omd, True, t)
    for other in (t - 1, t + 1):
        assert R.excess(R.ema_model32(e, p, R.weight_of(omd, True, other)), e, p, w) > 1.0, (t, other)


@pytest.mark.parametrize("w", [1e-2, 1e-4, 0.5])
def test_mutant_reversed_difference(w):
    e, p = R.inputs(4101, seed=7)
    d = (e - p).astype(np.float32)                                       # e - p where p - e belongs
    got = (np.float64(np.float32(w)) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)
    assert R.excess(got, e, p, w) > 1.0


def test_mutant_skip_ignored_and_tick_not_taken_back():
    n, omd = 1023, R.one_minus_decay(0.9999)
    e0, _ = R.inputs(n, seed=8)
    ps = [R.inputs(n, seed=9 + i)[1] for i in range(4)]
    ref, ws, t = R.run(e0, ps, omd, True, skips={1})
    assert t == 3 and ws[1] is None and np.array_equal(ref[1], ref[0])   # the skipped step keeps the bytes and the count
    assert ws[2] == R.weight_of(omd, True, 2)                             # the next step uses the count that was taken back
    ignored, _, _ = R.run(e0, ps, omd, True, skips=())
    assert R.excess(ignored[1], ref[0], ps[1], 0.0) > 1.0                 # against "nothing happened": e stays
    assert R.excess(ignored[2], ref[1], ps[2], ws[2]) > 1.0
    # the tick not taken back: step 2 would use the weight of t = 3
    late = R.ema_model32(ref[1], ps[2], R.weight_of(omd, True, 3))
    assert R.excess(late, ref[1], ps[2], ws[2]) > 1.0


def test_mutant_two_roundings_is_told_apart_by_bits_not_by_the_bound():
    """fl(fl(w d) + e) at w = 1e-4 PASSES the element bound on random inputs (its extra rounding is 2^-24 w |d|, inside the three
    units granted), so it is told apart on planted inputs where every element's bits differ; tests/test_gpu_ema_kernels.py asks the
    kernel for the fma's bits there."""
    e, p = R.inputs(4101, seed=10)
    assert R.excess(R.ema_two_rounding32(e, p, 1e-4), e, p, 1e-4) <= 1.0
    e, p, w = R.planted_two_rounding_input()
    assert len(e) == 64 and ((p - e).astype(np.float32).astype(np.float64) == p.astype(np.float64) - e.astype(np.float64)).all()
    assert (R.ema_model32(e, p, w) != R.ema_two_rounding32(e, p, w)).all()
    assert R.excess(R.ema_model32(e, p, w), e, p, w) <= 1.0


# ---- the build -----------------------------------------------------------------------------------------------------------------------
def test_kernel_resource_usage_reports_no_scratch_no_spill_no_lds():
    path = os.path.join(ROOT, "vimo_clip_amd", "csrc", "build", "ema.usage.txt")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    blocks = re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]
    kernels = [b for b in blocks if "ema_update_kernel" in b.split()[0] or "ema_swap_kernel" in b.split()[0]]
    assert len(kernels) == 2
    for b in kernels:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0
        assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 0


def test_ctypes_signatures_match_the_header():
    from vimo_clip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vmc.h")).read(), flags=re.S)
    for name, n in (("vmc_ema_update", 9), ("vmc_ema_swap", 4)):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == n == len(_lib.SIGNATURES[name][1])
        assert _lib.SIGNATURES[name][0] is _lib.I and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES["vmc_ema_update"][1][5] is __import__("ctypes").c_longlong


# ---- command lines and the YAML key --------------------------------------------------------------------------------------------------
def test_ema_decay_on_the_command_lines():
    from vimo_clip_amd import train, train_frame_diff_mn
    p = train.build_parser()
    off = p.parse_args([])
    assert not hasattr(off, "ema_decay") and train.ema_kwargs(off) is None         # off: the namespace it always was
    on = p.parse_args(["--ema_decay", "0.999"])
    assert train.ema_kwargs(on) == {"decay": 0.999, "warmup": True}
    assert train.ema_kwargs(p.parse_args(["--ema_decay", "0.9999", "--ema_no_warmup"])) == {"decay": 0.9999, "warmup": False}
    for bad in ("0", "1", "1.5", "-0.1", "nan", "most"):
        with pytest.raises(SystemExit):
            p.parse_args(["--ema_decay", bad])
    need = ["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c"]
    q = train_frame_diff_mn.build_parser()
    assert q.parse_args(need).ema_decay is None and train.ema_kwargs(q.parse_args(need)) is None
    got = q.parse_args(need + ["--ema-decay", "0.99", "--ema_no_warmup"])
    assert train.ema_kwargs(got) == {"decay": 0.99, "warmup": False}
    with pytest.raises(ValueError, match="ema_decay"):                             # refused before any file is opened
        train_frame_diff_mn.train(q.parse_args(need + ["--ema_decay", "1.0"]))


def test_ema_decay_in_the_tfam_config(tmp_path):
    yaml = pytest.importorskip("yaml")
    from vimo_clip_amd.TFAM.train_and_eval import Config
    assert Config().ema_decay is None and Config(ema_decay=0.999).ema_decay == 0.999
    cfg = {"training": dict(mode="both", seed=1, lr=1e-4, epochs=1, batch_size=2, num_workers=0, device="cuda"),
           "logging": dict(log_dir="l", checkpoint_dir="c"),
           "data": dict(num_classes=140, class_names_dir="n", train_dataset_path="t", val_dataset_path="v", flow_dataset_path="f"),
           "model": dict(d_model=256, nhead=8, num_layers=2, dim_feedforward=512, use_cross_attention=True, concat_dim=1, dropout=0.0,
                         mlp_dropout=0.0, use_pe=False, use_only_rgb=False, use_only_flow=False)}
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(path)).ema_decay is None
    cfg["training"]["ema_decay"] = 0.9995
    path.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(path)).ema_decay == 0.9995
    assert Config.from_yaml(str(path), ema_decay=0.99).ema_decay == 0.99           # the command line's --ema-decay overrides


# ---- the optimiser's state machine, launches replaced by the reference ---------------------------------------------------------------
@pytest.fixture
def cpu_opt(monkeypatch):
    from vimo_clip_amd.optim import FusedAdam, GradArena
    calls = []

    def update(self):
        calls.append(("update", self.step_count))
        w = R.weight_of(self._ema_w, self._ema_warmup, self.step_count)
        self.ema.copy_(torch.from_numpy(R.ema_ref(self.ema.numpy(), self.arena.flat_param.numpy(), w).astype(np.float32)))

    def swap(self):
        calls.append(("swap",))
        a, b = self.arena.flat_param, self.ema
        tmp = a.clone()
        a.copy_(b)
        b.copy_(tmp)

    def adam(self, lo, hi, grad_scale=1.0, background=False):
        self.arena.flat_param[lo:hi] -= 0.5 * self.arena.flat_grad[lo:hi]

    monkeypatch.setattr(FusedAdam, "_ema_update", update)
    monkeypatch.setattr(FusedAdam, "_ema_swap", swap)
    monkeypatch.setattr(FusedAdam, "_update_range", adam)
    monkeypatch.setattr("vimo_clip_amd.optim.invalidate_weight_copies", lambda opt=None: None)
    params = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i))) for i, s in enumerate([(5, 7), (130,), (3,)])]
    return FusedAdam(GradArena(params), lr=1e-3), calls


def test_enable_ema_arguments_and_allocation(cpu_opt):
    opt, calls = cpu_opt
    assert opt.ema is None and "ema" not in opt.state_dict()
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            opt.enable_ema(bad)
    assert opt.ema is None
    with pytest.raises(RuntimeError, match="enable_ema"):
        with opt.ema_weights():
            pass
    assert opt.enable_ema(0.9999) is opt
    assert opt.ema.dtype == torch.float32 and opt.ema.numel() == opt.arena.numel and torch.equal(opt.ema, opt.arena.flat_param)
    assert opt.ema.data_ptr() != opt.arena.flat_param.data_ptr()
    assert np.float32(opt._ema_w) == R.one_minus_decay(0.9999) and opt._ema_warmup is True
    sd = opt.state_dict()
    assert sd["ema"] is opt.ema and sd["ema_one_minus_decay"] == opt._ema_w and sd["ema_warmup"] is True
    opt.disable_ema()
    assert opt.ema is None and set(opt.state_dict()) == {"step", "m", "v", "lr"} and calls == []


def test_step_updates_the_average_once_and_the_context_rules(cpu_opt):
    opt, calls = cpu_opt
    a = opt.arena
    a.flat_grad.fill_(1.0)
    opt.step()
    assert calls == []                                                   # off: no launch
    opt.enable_ema(0.99, warmup=True)
    e0 = opt.ema.clone()
    opt.step()
    assert calls == [("update", 2)]                                      # host-state mode passes step_count, after its increment
    want = R.ema_ref(e0.numpy(), a.flat_param.numpy(), R.weight_of(R.one_minus_decay(0.99), True, 2)).astype(np.float32)
    assert np.array_equal(opt.ema.numpy(), want)
    del calls[:]
    live, avg = a.flat_param.clone(), opt.ema.clone()
    with opt.ema_weights() as o:
        assert o is opt and torch.equal(a.flat_param, avg) and torch.equal(opt.ema, live)
        with pytest.raises(RuntimeError, match="nest"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.disable_ema()
        assert torch.equal(a.flat_param, avg)                            # the refused calls changed nothing
    assert calls == [("swap",), ("swap",)] and torch.equal(a.flat_param, live) and torch.equal(opt.ema, avg)
    with pytest.raises(KeyError):                                        # an exception inside still swaps back
        with opt.ema_weights():
            raise KeyError("x")
    assert torch.equal(a.flat_param, live) and not opt._ema_active
    a._pending = 1
    with pytest.raises(RuntimeError, match="pending"):
        with opt.ema_weights():
            pass
    a._pending = 0
    opt._step_open = True
    with pytest.raises(RuntimeError, match="overlapped"):
        with opt.ema_weights():
            pass
    opt._step_open = False
    assert torch.equal(a.flat_param, live) and calls[2:] == [("swap",), ("swap",)]


def test_state_dict_round_trip_carries_the_average(cpu_opt):
    from vimo_clip_amd.optim import FusedAdam, GradArena
    opt, _ = cpu_opt
    opt.enable_ema(0.999, warmup=False)
    opt.arena.flat_grad.fill_(0.25)
    opt.step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    other = FusedAdam(GradArena([torch.nn.Parameter(p.detach().clone()) for p in opt.arena.params]), lr=1e-3)
    assert other.ema is None
    other.load_state_dict(sd)                                            # allocates the average when it was not on yet
    assert torch.equal(other.ema, opt.ema) and other._ema_w == opt._ema_w and other._ema_warmup is False and other.step_count == 1
    plain = FusedAdam(GradArena([torch.nn.Parameter(torch.zeros(4))]), lr=1e-3)
    plain.load_state_dict({k: v for k, v in plain.state_dict().items()})
    assert plain.ema is None
