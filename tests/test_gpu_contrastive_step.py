"""GPU: the contrastive distillation mode inside the student trainer (vimo_clip_amd/train.py) -- one optimiser step of a ViT-tiny/32
student on 2 clips x 4 frames: a finite loss, every trainable parameter moved, the gradient arriving at the model's distillation
embeddings equal to what the public function gives on the same tensors, ``val_top1`` in the epoch line; and the default cosine step
left as it was: the same bits with the new keywords spelled out."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ARGS = ["--clip_model_name", "ViT-tiny/32", "--batch_size", "2", "--sequence_length", "5", "--learning_rate", "1e-3"]


def _sets():
    from vimo_clip_amd.dataset import SyntheticSegmentDataset
    return (SyntheticSegmentDataset(2, 5, 64, 140, resolution=64, seed=3), SyntheticSegmentDataset(2, 5, 64, 140, resolution=64, seed=4))


def _train(monkeypatch, extra_args, loss_wrapper=None):
    """One epoch = one step of train.train; returns (epoch line, parameters before, parameters after, what the loss wrapper saw)."""
    from vimo_clip_amd import autograd_ops, synth, train as T
    seen = {"calls": []}
    build, loss = T.FlowStudentModel, T.distillation_loss

    def model(*a, **k):
        m = build(*a, **k)
        # the reference initialises residual_mlp.fc2 with zeros, so fc1 has a gradient of exactly zero in the first step whatever the
        # loss: the step starts from weights with a live fc2, and then every parameter has to move
        m.load_state_dict(synth.student_state_dict("ViT-tiny/32", 71), strict=True)
        seen["model"] = m
        return m

    def distill(student, teacher, **k):
        if seen.get("before") is None:                              # the first call is the training step's
            seen["before"] = {n: p.detach().clone() for n, p in seen["model"].named_parameters()}
        return loss(student, teacher, **k) if loss_wrapper is None else loss_wrapper(loss, seen, student, teacher, **k)
    monkeypatch.setattr(T, "FlowStudentModel", model)
    monkeypatch.setattr(T, "distillation_loss", distill)
    autograd_ops.weights.clear()
    torch.manual_seed(0)
    best = T.train(T.build_parser().parse_args(ARGS + extra_args), datasets=_sets())
    torch.cuda.synchronize()
    after = {n: p.detach().clone() for n, p in seen["model"].named_parameters()}
    return best, seen["before"], after, seen


def test_one_contrastive_step_trains_every_parameter_and_reports_top1(monkeypatch, capsys):
    from vimo_clip_amd.losses import distillation_loss

    def spy(loss, seen, student, teacher, **k):
        out = loss(student, teacher, **k)
        rec = {"student": student.detach().clone(), "teacher": teacher.detach().clone(), "kwargs": dict(k), "loss": out, "grad": None}
        if student.requires_grad:
            student.register_hook(lambda g, rec=rec: rec.__setitem__("grad", g.detach().clone()))
        seen["calls"].append(rec)
        return out
    best, before, after, seen = _train(monkeypatch, ["--distillation_loss_mode", "contrastive", "--distill_temperature", "0.1"], spy)
    line = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    step, val = seen["calls"][0], seen["calls"][1]
    assert len(seen["calls"]) == 2 and np.isfinite(best)
    assert step["student"].shape == (2, 4, 64) and step["kwargs"] == {"mode": "contrastive", "temperature": 0.1, "compute_dtype": torch.bfloat16}
    assert val["kwargs"] == dict(step["kwargs"], return_top1=True)
    assert torch.isfinite(step["loss"]).item() and float(step["loss"].detach()) > 0.0
    # every trainable parameter moved, nothing became non-finite
    params = dict(seen["model"].named_parameters())
    assert all(torch.isfinite(after[n]).all().item() for n in params)
    stuck = [n for n, p in params.items() if p.requires_grad and torch.equal(before[n], after[n])]
    assert not stuck, f"did not move: {stuck}"
    # the gradient that reached the model is the public function's on the same tensors (upstream gradient 1)
    s = step["student"].requires_grad_(True)
    loss = distillation_loss(s, step["teacher"], **step["kwargs"])
    loss.backward()
    assert torch.equal(loss.detach().view(torch.int32), step["loss"].detach().view(torch.int32))
    assert step["grad"] is not None and torch.equal(s.grad.view(torch.int32), step["grad"].view(torch.int32)) and s.grad.any().item()
    # the epoch line: the validation top-1 share of the one validation batch, in this mode only
    v_loss, v_frac = val["loss"]
    assert line["val_top1"] == pytest.approx(float(v_frac), abs=1e-7) and 0.0 <= line["val_top1"] <= 1.0
    assert line["val_distill"] == pytest.approx(float(v_loss), rel=1e-6)
    assert float(v_frac) * 8 == round(float(v_frac) * 8)            # a count of the 8 frames


def test_cosine_step_keeps_its_bits_with_the_new_keywords_spelled_out(monkeypatch, capsys):
    def explicit(loss, seen, student, teacher, **k):
        seen["calls"].append(dict(k))
        return loss(student, teacher, temperature=0.07, compute_dtype=torch.bfloat16, mask_same_clip=True, return_top1=False, **k)
    _, before_a, after_a, seen_a = _train(monkeypatch, [], lambda loss, seen, s, t, **k: (seen["calls"].append(dict(k)), loss(s, t, **k))[1])
    line_a = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    monkeypatch.undo()
    _, before_b, after_b, seen_b = _train(monkeypatch, [], explicit)
    line_b = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert seen_a["calls"] == seen_b["calls"] == [{"mode": "cosine"}] * 2          # the trainer passes nothing new in this mode
    assert "val_top1" not in line_a and {k: v for k, v in line_a.items() if "frames_per_s" not in k} == \
        {k: v for k, v in line_b.items() if "frames_per_s" not in k}
    assert all(torch.equal(before_a[n], before_b[n]) for n in before_a)
    assert all(torch.equal(after_a[n].view(torch.int32), after_b[n].view(torch.int32)) for n in after_a)
    assert any(not torch.equal(before_a[n], after_a[n]) for n in after_a)
