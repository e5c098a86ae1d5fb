"""GPU: the weight average inside training steps (optim.FusedAdam.enable_ema).  The average after every step is held to
the element bound of tests/ema_refs.py against ema_ref(previous average, parameters after the step, weight_of(...)); parameters and
moments keep the bits of a run without the average; skipped, captured, overlapped, LoRA and resumed steps; ema_weights(); the trainers;
and the off path against digests recorded before the feature existed."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import ema_refs as R
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
PATHS = ("host", "device", "device_fused")              # host-state vmc_adam_step | device-state two-kernel | vmc_adam_cast_multi_skip
TINY_TFAM = dict(D=256, H=8, L=2, ff=512, C=140, B=8, Tr=16, Tf=15, seed=77)
CHAIN_TFAM = dict(TINY_TFAM, D=512, ff=1024, B=4)        # the smallest geometry the fused training chains take: their backward reports groups


# ---- models and steps -----------------------------------------------------------------------------------------------------------------
def _student(dtype=torch.bfloat16, name="ViT-tiny/32", seed=71, **kw):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.models import FlowStudentModel
    ag.weights.clear()
    m = FlowStudentModel(name, device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype, **kw)
    m.load_state_dict(synth.student_state_dict(name, seed), strict=not kw)
    return m.train()


def _student_batch(step, B=4, T=5, name="ViT-tiny/32"):
    R_, E = synth.VIT_GEOMETRY[name][0], synth.VIT_GEOMETRY[name][5]
    return (synth.randint_u8(71 + step, "vids", (B, T, 3, R_, R_)).cuda(), synth.normal(71 + step, "teacher", (B, T + 1, E)).cuda(),
            synth.multi_hot_labels(71 + step, "labels", B, 140).cuda())


def _student_loss(m, vids, teacher, labels):
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    _, emb_d, logits = m(vids)
    return distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)


def _student_opt(m, path, lr=1e-3):
    from vimo_clip_amd.optim import FusedAdam, GradArena
    opt = FusedAdam(GradArena(m.parameters()), lr=lr)
    if path != "host":
        opt.enable_device_state(base_seed=11)
    if path == "device":
        opt.FUSED_CAST = False                          # the two-kernel path: vmc_adam_step_dev_skip + the refresh launch
    return opt


def _student_step(m, opt, step):
    if getattr(opt, "dev_state", None) is not None:
        opt.tick()
    opt.scale_loss(_student_loss(m, *_student_batch(step))).backward()


def _tfam(c=TINY_TFAM, dtype=torch.bfloat16):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    ag.weights.clear()
    m = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=c["C"], dropout=0.0, mlp_dropout=0.0,
                 device="cuda", compute_dtype=dtype).cuda()
    m.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]), strict=True)
    return m.train()


def _tfam_batch(step, c=TINY_TFAM):
    return (synth.normal(500 + step, "rgb", (c["B"], c["Tr"], c["D"])).cuda(), synth.normal(500 + step, "mot", (c["B"], c["Tr"] - 1, c["D"])).cuda(),
            synth.multi_hot_labels(500 + step, "y", c["B"], c["C"]).cuda())


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(t):
    return t.detach().view(torch.int32).cpu()


def _check_update(opt, prev, t, what):
    """The average against the reference fed the PREVIOUS average and the parameters as the step left them."""
    w = R.weight_of(opt._ema_w, opt._ema_warmup, t)
    got = _np(opt.ema)
    x = R.excess(got, prev, _np(opt.arena.flat_param), w)
    print(f"{what}: t {t} w {float(w):.6g} excess {x:.3f}")
    assert x <= 1.0, (what, t, x)
    assert not np.array_equal(got, prev), (what, t)
    return got


# ---- three steps on every optimiser path ---------------------------------------------------------------------------------------------
def _three_student_steps(path, decay=None, warmup=True):
    m = _student()
    opt = _student_opt(m, path)
    if decay is not None:
        opt.enable_ema(decay, warmup=warmup)
        prev = _np(opt.ema)
        assert np.array_equal(prev, _np(opt.arena.flat_param))
    for step in range(3):
        _student_step(m, opt, step)
        opt.step()
        if decay is not None:
            prev = _check_update(opt, prev, step + 1, path)
    torch.cuda.synchronize()
    assert (getattr(opt, "_fused_plan", None) is not None) == (path == "device_fused"), path
    return opt


@pytest.mark.parametrize("path", PATHS)
def test_average_follows_the_reference_and_leaves_the_step_its_bits(path):
    plain = _three_student_steps(path)
    kept = [t.clone() for t in (plain.arena.flat_param, plain.m, plain.v)]
    assert plain.ema is None
    for decay, warmup in ((0.9999, True), (0.99, False)):
        opt = _three_student_steps(path, decay, warmup)
        for a, b in zip(kept, (opt.arena.flat_param, opt.m, opt.v)):
            assert torch.equal(_bits(a), _bits(b)), (path, decay)
        assert opt.ema.numel() == opt.arena.numel and opt.ema.dtype == torch.float32


# ---- the off path ----------------------------------------------------------------------------------------------------------------------
# sha256 of flat_param after the three steps of _three_student_steps(path), recorded on an MI355X on the commit before the weight average
# existed, with this sequence of calls (the three paths are the same arithmetic, element for element, and repeat their bits run to run)
OFF_PATH_DIGESTS = {
    "host": "55576e35477401966f88cd60c89a25950a6de0ee6c76a7992086a1dc35fd82d6",
    "device": "55576e35477401966f88cd60c89a25950a6de0ee6c76a7992086a1dc35fd82d6",
    "device_fused": "55576e35477401966f88cd60c89a25950a6de0ee6c76a7992086a1dc35fd82d6",
}


@pytest.mark.parametrize("path", PATHS)
def test_steps_without_the_average_keep_the_bits_they_had(path):
    opt = _three_student_steps(path)
    assert hashlib.sha256(opt.arena.flat_param.detach().cpu().numpy().tobytes()).hexdigest() == OFF_PATH_DIGESTS[path]
    assert opt.ema is None and "ema" not in opt.state_dict() and set(opt.state_dict()) == {"step", "m", "v", "lr"}
    with pytest.raises(RuntimeError, match="enable_ema"):
        with opt.ema_weights():
            pass
    # nothing arena-sized beyond parameters, gradients and the two moments was allocated by the optimiser
    tensors = [v for v in vars(opt).values() if torch.is_tensor(v) and v.numel() >= opt.arena.numel]
    assert len(tensors) == 2


# ---- a step the loss scale skips -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["device", "device_fused"])
def test_a_skipped_step_leaves_the_average_and_its_warmup_count(path):
    m = _student()
    opt = _student_opt(m, path).enable_loss_scaling(init_scale=1024.0, growth_factor=1.0, backoff_factor=1.0).enable_ema(0.9999)
    prev = _np(opt.ema)
    t = 0
    for step in range(3):
        _student_step(m, opt, step)
        if step == 1:
            opt.arena.flat_grad[opt.arena.numel // 2] = float("inf")
        before_p = _bits(opt.arena.flat_param)
        opt.step()
        if step == 1:
            assert opt.last_found_inf.item() == 1 and int(opt.dev_state[0].item()) == t
            assert np.array_equal(_np(opt.ema).view(np.int32), prev.view(np.int32))      # the average's bits, not just its values
            assert torch.equal(_bits(opt.arena.flat_param), before_p)
        else:
            t += 1
            assert opt.last_found_inf.item() == 0 and int(opt.dev_state[0].item()) == t
            prev = _check_update(opt, prev, t, f"{path} with a skipped step")          # step 2 uses the weight of t = 2: 9 / 12
    assert t == 2 and opt.skipped_steps.item() == 1 and opt.step_count == 3           # the host mirror counts attempts; the kernel does not read it


# ---- ema_weights() ---------------------------------------------------------------------------------------------------------------------
def _run_with_context(path, enter):
    from vimo_clip_amd.models import FlowStudentModel
    m = _student()
    opt = _student_opt(m, path).enable_ema(0.99)
    out = {}
    for step in range(3):
        if step == 2 and enter:
            live = _bits(opt.arena.flat_param)
            avg = _bits(opt.ema)
            out["sd"] = opt.ema_state_dict(m)
            assert torch.equal(_bits(opt.arena.flat_param), live) and torch.equal(_bits(opt.ema), avg)
            vids = _student_batch(9)[0]
            m.eval()
            with opt.ema_weights(), torch.no_grad():
                assert torch.equal(_bits(opt.arena.flat_param), avg) and torch.equal(_bits(opt.ema), live)
                out["inside"] = [t.clone() for t in m(vids)]
                with pytest.raises(RuntimeError, match="nest"):
                    with opt.ema_weights():
                        pass
                with pytest.raises(RuntimeError, match="ema_weights"):
                    opt.step()
            with torch.no_grad():
                out["live"] = [t.clone() for t in m(vids)]
            m.train()
            assert torch.equal(_bits(opt.arena.flat_param), live) and torch.equal(_bits(opt.ema), avg)
            fresh =FlowStudentModel("ViT-tiny/32", device="cuda", num_classes=140, alpha=0.1, compute_dtype=torch.bfloat16).eval()
            fresh.load_state_dict(out["sd"], strict=True)
            with torch.no_grad():
                out["fresh"] = [t.clone() for t in fresh(vids)]
        _student_step(m, opt, step)
        opt.step()
    torch.cuda.synchronize()
    out["end"] = [_bits(t) for t in (opt.arena.flat_param, opt.m, opt.v, opt.ema)]
    return out, opt


@pytest.mark.parametrize("path", ["host", "device_fused"])
def test_ema_weights_swaps_in_the_average_and_gives_the_live_weights_back(path):
    entered, opt = _run_with_context(path, True)
    never, _ = _run_with_context(path, False)
    assert all(k in entered["sd"] for k in synth.student_state_dict("ViT-tiny/32", 71)) and all(not v.is_cuda for v in entered["sd"].values())
    for a, b in zip(entered["inside"], entered["fresh"]):             # the forward inside the context = a fresh model with the averaged weights
        assert torch.isfinite(a).all().item() and torch.equal(a, b)
    assert not torch.equal(entered["inside"][2], entered["live"][2])  # and not the live model's
    for a, b in zip(entered["end"], never["end"]):                     # the step after the context: as if it had never been entered
        assert torch.equal(a, b)


def test_ema_weights_raises_while_capturing_pending_or_mid_overlap():
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    m = _tfam(CHAIN_TFAM)
    arena = GradArena(m.used_parameters())
    opt = FusedAdam(arena, lr=1e-3, weight_decay=0.1, decoupled=True).enable_ema(0.99)
    rgb, mot, y = _tfam_batch(0, CHAIN_TFAM)
    # a pending accumulation
    bce_with_logits_loss(m(rgb, mot), y).backward()
    arena.accumulate(0.5)
    with pytest.raises(RuntimeError, match="pending"):
        with opt.ema_weights():
            pass
    arena.zero_grad()
    # an overlapped step that is open: the backward has updated groups, step() has not joined yet
    opt.enable_backward_overlap(m.parameter_groups_by_layer())
    m.grad_group_callback = opt.group_ready
    bce_with_logits_loss(m(rgb, mot), y).backward()
    assert opt._ov["used"]
    with pytest.raises(RuntimeError, match="overlapped"):
        with opt.ema_weights():
            pass
    opt.step()
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="backward inside ema_weights"):      # an overlapped update of the averaged weights is refused
            opt.group_ready(0)
    assert not opt._ov["used"] and not getattr(opt, "_step_open", False)
    m.grad_group_callback = None
    opt.disable_backward_overlap()
    # inside a capture: ema_weights and enable_ema both refuse
    live = _bits(arena.flat_param)
    avg = _bits(opt.ema)
    for call in (lambda: opt.ema_weights().__enter__(), lambda: opt.enable_ema(0.5)):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="captured"):                # as tests/test_gpu_grad_accum.py raises out of a capture
            with torch.cuda.graph(graph):
                arena.flat_grad.mul_(2.0)
                call()
        torch.cuda.synchronize()
    assert torch.equal(_bits(arena.flat_param), live) and torch.equal(_bits(opt.ema), avg) and not opt._ema_active
    assert abs(opt._ema_w - 0.01) < 1e-8                                   # the refused enable_ema changed nothing


# ---- captured steps --------------------------------------------------------------------------------------------------------------------
def test_captured_steps_follow_the_recurrence_and_the_warmup_run_leaks_nothing():
    """GraphedTrainStep over a small TFAM at B = 8, four replays.  The capture's warm-up run is undone -- the average with the
    parameters -- and the kernel reads the step count from device memory: replay i uses the weight of t = i, so the first average is
    9 / 11 of the way to the first parameters.  A leaked update or tick would fail the first comparison."""
    from vimo_clip_amd.graphs import GraphedTrainStep
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    m = _tfam()
    opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-3, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=11).enable_ema(0.9999)
    m.use_device_seeds(opt)

    def step(rgb, mot, y):
        opt.tick()
        loss = bce_with_logits_loss(m(rgb, mot), y)
        loss.backward()
        opt.step()
        return loss.detach()

    run = GraphedTrainStep(step, opt)
    assert any(t is opt.ema for t in run._live())
    prev = _np(opt.ema)
    for i in range(4):
        run(*_tfam_batch(i))
        torch.cuda.synchronize()
        assert int(opt.dev_state[0].item()) == i + 1
        prev = _check_update(opt, prev, i + 1, "captured")
    assert run.n_graphs == 1


# ---- backward overlap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_state", [False, True], ids=["host-scalars", "device-state"])
def test_overlapped_steps_update_the_average_after_the_join(device_state):
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    ends = []
    for overlap in (True, False):
        m = _tfam(CHAIN_TFAM)
        opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-3, weight_decay=0.1, decoupled=True)
        if device_state:
            opt.enable_device_state(base_seed=11)
            m.use_device_seeds(opt)
        opt.enable_ema(0.999)
        hits = []
        if overlap:
            opt.enable_backward_overlap(m.parameter_groups_by_layer())
            m.grad_group_callback = lambda i: (hits.append(i), opt.group_ready(i))
        prev = _np(opt.ema)
        for step in range(2):
            rgb, mot, y = _tfam_batch(step, CHAIN_TFAM)
            if device_state:
                opt.tick()
            bce_with_logits_loss(m(rgb, mot), y).backward()
            assert not overlap or opt._ov["used"]
            opt.step()
            prev = _check_update(opt, prev, step + 1, "overlap" if overlap else "plain")
        assert bool(hits) == overlap
        ends.append((_bits(opt.arena.flat_param), _bits(opt.ema)))
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1])      # same kernels over the same values


# ---- LoRA ------------------------------------------------------------------------------------------------------------------------------
def test_lora_averages_the_adapters_and_heads_and_save_best_merges_from_them(tmp_path):
    from vimo_clip_amd import train as T
    from vimo_clip_amd.checkpoint import load_file, strip_prefix
    from vimo_clip_amd.lora import merged_state_dict
    m = _student(lora_rank=8)
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    opt = _student_opt(m, "device_fused").enable_ema(0.99)
    assert frozen and opt.ema.numel() == opt.arena.numel < sum(p.numel() for p in m.parameters())
    prev = _np(opt.ema)
    for step in range(3):
        _student_step(m, opt, step)
        opt.step()
        prev = _check_update(opt, prev, step + 1, "lora")
    live = {k: v.cpu() for k, v in merged_state_dict(m).items()}
    path = str(tmp_path / "run - best" / "student_best.pth")
    with opt.ema_weights():
        T.save_best(m, path)
        want = {k: v.cpu() for k, v in merged_state_dict(m).items()}
    got = strip_prefix(load_file(path))
    assert set(got) == set(want) == set(synth.student_state_dict("ViT-tiny/32", 71))
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert any(not torch.equal(got[k], live[k]) for k in want)        # the average, not the last iterate
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p.detach(), frozen[n]), n


# ---- resuming --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "device_fused"])
def test_state_dict_round_trip_continues_bit_for_bit(path):
    m = _student()
    opt = _student_opt(m, path).enable_ema(0.999)
    for step in range(2):
        _student_step(m, opt, step)
        opt.step()
    sd = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    params = opt.arena.flat_param.detach().clone()
    assert set(sd) == {"step", "m", "v", "lr", "ema", "ema_one_minus_decay", "ema_warmup"} and sd["step"] == 2
    _student_step(m, opt, 2)
    opt.step()
    want = [_bits(opt.arena.flat_param), _bits(opt.ema)]
    m2 = _student(seed=5)                                              # other weights: everything must come from the checkpoint
    opt2 = _student_opt(m2, path)
    opt2.arena.flat_param.copy_(params)
    opt2.load_state_dict(sd)
    assert opt2.ema is not None and opt2._ema_w == opt._ema_w and opt2._ema_warmup
    _student_step(m2, opt2, 2)
    opt2.step()
    assert torch.equal(_bits(opt2.arena.flat_param), want[0]) and torch.equal(_bits(opt2.ema), want[1])


# ---- the trainers ----------------------------------------------------------------------------------------------------------------------
def test_student_trainer_evaluates_and_writes_the_average(capsys, tmp_path, monkeypatch):
    from vimo_clip_amd import autograd_ops, train as T
    from vimo_clip_amd.checkpoint import load_file, strip_prefix
    from vimo_clip_amd.dataset import SyntheticSegmentDataset
    from vimo_clip_amd.lora import merged_state_dict
    from vimo_clip_amd.optim import FusedAdam
    sets = (SyntheticSegmentDataset(16, 6, 64, 140, resolution=64, seed=3), SyntheticSegmentDataset(8, 6, 64, 140, resolution=64, seed=4))
    seen = {}
    enable, evaluate, save_best = FusedAdam.enable_ema, T.evaluate, T.save_best
    monkeypatch.setattr(FusedAdam, "enable_ema", lambda self, *a, **k: (seen.setdefault("opt", self), enable(self, *a, **k))[1])
    monkeypatch.setattr(T, "evaluate", lambda model, *a, **k: (seen.setdefault("eval_active", seen["opt"]._ema_active), evaluate(model, *a, **k))[1])
    monkeypatch.setattr(T, "save_best", lambda model, path: (seen.update(model=model, save_active=seen["opt"]._ema_active), save_best(model, path))[1])
    autograd_ops.weights.clear()
    ckpt = str(tmp_path / "run")
    args = T.build_parser().parse_args(["--clip_model_name", "ViT-tiny/32", "--batch_size", "4", "--sequence_length", "6", "--lora_rank", "8",
                                        "--ema_decay", "0.9", "--checkpoint_dir", ckpt])
    best = T.train(args, datasets=sets)
    line = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert np.isfinite(best) and line["ema"] is True
    opt, model = seen["opt"], seen["model"]
    assert seen["eval_active"] is True and seen["save_active"] is True and not opt._ema_active
    assert abs(opt._ema_w - 0.1) < 1e-7 and opt._ema_warmup and opt.step_count == 4
    got = strip_prefix(load_file(f"{ckpt} - best/student_best.pth"))
    with opt.ema_weights():
        want = {k: v.cpu() for k, v in merged_state_dict(model).items()}
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    epoch_file = strip_prefix(load_file(f"{ckpt}/student_epoch_1.pth"))              # the live weights, adapters as they are
    assert any("lora_" in k for k in epoch_file)
    assert all(torch.equal(v, model.state_dict()[k].cpu()) for k, v in epoch_file.items())
    # off: no key in the line, no average
    autograd_ops.weights.clear()
    T.train(T.build_parser().parse_args(["--clip_model_name", "ViT-tiny/32", "--batch_size", "4", "--sequence_length", "6"]), datasets=sets)
    line = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert "ema" not in line


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_tfam_trainer_validates_and_checkpoints_the_average(graphs, tmp_path):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTester, ModelTrainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z = np.load(os.path.join(root, "tests", "golden", "ak_labels.npz"))
    lab = lambda split, n: torch.from_numpy(np.unpackbits(z[f"{split}/labels"], axis=1)[:n, :140].astype(np.float32))      # noqa: E731
    c = TINY_TFAM
    tr = SyntheticEmbeddingDataset(lab("train", 48), c["D"], tmin=12, tmax=16, seed=5, signal=0.6)
    va = SyntheticEmbeddingDataset(lab("val", 16), c["D"], tmin=12, tmax=16, seed=6, signal=0.6)
    ag.weights.clear()
    cfg = Config(epochs=1, batch_size=8, d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], dropout=0.0, mlp_dropout=0.0,
                 device="cuda", checkpoint_dir=str(tmp_path), use_graphs=graphs, ema_decay=0.9)

    def model():
        m = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=140, dropout=0.0, mlp_dropout=0.0,
                     device="cuda").cuda()
        m.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], 140, c["seed"]), strict=True)
        return m
    t = ModelTrainer(model(), tr, va, cfg)
    opt = t.optimizer
    assert opt.ema is not None and abs(opt._ema_w - 0.1) < 1e-7
    t.train_epoch(0)
    live, avg = _bits(opt.arena.flat_param), _bits(opt.ema)
    assert not torch.equal(live, avg)
    vl, vm = t.validate(0)
    assert torch.equal(_bits(opt.arena.flat_param), live) and torch.equal(_bits(opt.ema), avg) and not opt._ema_active
    state = t.save_checkpoint(vl, vm, 0)
    with opt.ema_weights():
        averaged = {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()}
    sd, live_sd = state["state_dict"], state["live_state_dict"]
    assert all(torch.equal(sd["module." + k], v) for k, v in averaged.items())
    assert all(torch.equal(live_sd["module." + k], v.detach().cpu()) for k, v in t.model.state_dict().items())
    assert torch.equal(state["optimizer"]["ema"].view(torch.int32), avg) and not state["optimizer"]["ema"].is_cuda
    # what was validated is what the tester reads back from best_model.pth: the same loss on the same set
    cfg_plain = Config(**{**vars(cfg), "ema_decay": None, "checkpoint_dir": None})
    tester = ModelTester(model(), va, cfg_plain).load_best_model(str(tmp_path))
    assert all(torch.equal(p.detach().cpu(), averaged[k]) for k, p in tester.model.state_dict().items())
    check = ModelTrainer(tester.model, tr, va, cfg_plain)
    assert check.optimizer.ema is None
    vl2, vm2 = check.validate(0)
    print(f"graphs {graphs}: averaged val loss {vl:.6f} mAP {vm:.6f}; reloaded {vl2:.6f} {vm2:.6f}")
    assert vl2 == vl and vm2 == vm
