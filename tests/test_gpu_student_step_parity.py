"""GPU: one training step of the student -- autograd_vit.vit_forward_train (tower) or FlowStudentModel.forward (student level) and
torch.autograd.backward with given upstream gradients -- against tests/student_step_refs.py: a float64 step and a float64 model of
it that rounds where the path rounds.  Every output and every parameter gradient, from the gradient arena's slots
where the case has an arena (pre-filled with NaN: an element the backward does not write fails `finite`), from ``.grad`` otherwise.

VMC_STUDENT_PARITY_JSON=<path>: one line per checked tensor (case, dtype, tensor, both ratios, the distance to the model)."""
import functools
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import student_step_refs as R                    # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16      # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (BF16, F16)
CONFIGS = [(c["name"], dt) for c in R.CASES for dt in DTYPES]
CFG_ID = lambda v: v if isinstance(v, str) else DT_NAME[v]


def _tower(c, dtype):
    from vimo_clip_amd.clip_vit import VisionTransformer
    m = VisionTransformer(c["R"], c["p"], R.WIDTH, R.LAYERS, R.HEADS, c["E"], compute_dtype=dtype)
    m.cls_only_last_block = c["cls_only"]
    return m


def step_on_gpu(name, dtype):
    """Build the case's model, load its weights, run forward and backward; returns {tensor name: CPU tensor} under the names of
    student_step_refs."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.autograd_vit import vit_forward_train
    from vimo_clip_amd.optim import GradArena
    inp = R.make_inputs(name, dtype)
    c = inp["case"]
    student = c["level"] == "student"
    if student:
        from vimo_clip_amd.models.student_model import FlowStudentModel
        m = FlowStudentModel("ViT-tiny/32", device="cuda", num_classes=c["C"], alpha=0.1, compute_dtype=dtype)
        assert m.visual_encoder.output_dim == c["E"] and m.visual_encoder.width == R.WIDTH
        m.visual_encoder = _tower(c, dtype)          # the case's geometry; the heads depend on E alone
        prefix = "visual_encoder."
    else:
        m, prefix = _tower(c, dtype), ""
    m = m.cuda().train()
    sd = {(prefix if n not in R.HEAD_PARAMS else "") + n: v for n, v in inp["p32"].items()}
    m.load_state_dict(sd, strict=True)
    params = dict(m.named_parameters())
    assert set(params) == set(sd)
    arena = GradArena(m.parameters()) if c["arena"] else None
    if arena is not None:
        arena.flat_grad.fill_(float("nan"))
    frames = inp["frames"].cuda()
    if student:
        outs = m(frames.reshape(c["B"], c["T"], 3, c["R"], c["R"]))
        names = ("emb", "emb_distill", "logits")
    else:
        outs, names = (vit_forward_train(m, frames, wrap_quirk=True),), ("E",)
    ups = [inp["up"][n].reshape(o.shape).cuda() for n, o in zip(names, outs)]
    parked, push = [], ag.wgrad_queue.push
    ag.wgrad_queue.push = lambda *a: (parked.append(a[2].shape), push(*a))[1]
    try:
        torch.autograd.backward(list(outs), ups)
    finally:
        del ag.wgrad_queue.push                  # the instance attribute: the class's method is back
    ag.wgrad_queue.flush()
    torch.cuda.synchronize()
    # the parked grouped launch is taken where the case says so and nowhere else: by conv1, and by the linears on all F N token
    # rows (four per ordinary block and the last block's in_proj, whose three other linears see the F class rows when cls_only)
    conv1 = [s for s in parked if tuple(s) == (R.WIDTH, c["K"])]
    assert len(conv1) == int(c["parks_conv1"]), parked
    assert len(parked) - len(conv1) == (4 * (R.LAYERS - 1) + (1 if c["cls_only"] else 4) if c["parks_stream"] else 0), parked
    got = {n: o.detach().float().cpu().reshape(inp["up"][n].shape) for n, o in zip(names, outs)}
    for n in inp["p32"]:
        p = params[(prefix if n not in R.HEAD_PARAMS else "") + n]
        g = p._vmc_grad if arena is not None else p.grad
        assert g is not None, f"{n}: no gradient"
        assert (arena is None) == (getattr(p, "_vmc_grad", None) is None)
        got["g." + n] = g.detach().float().cpu().reshape(inp["p32"][n].shape)
    return got


@functools.lru_cache(maxsize=None)
def _measured(name, dtype):
    r, m16 = R.step_ref64(name, dtype), R.step_model16(name, dtype)
    got = step_on_gpu(name, dtype)
    assert set(got) == set(R.tensor_names(r)), set(got) ^ set(R.tensor_names(r))
    ms, bad = R.check(got, r, m16)
    path = os.environ.get("VMC_STUDENT_PARITY_JSON")
    if path:
        with open(path, "a") as f:
            for m in ms:
                f.write(json.dumps(dict(case=name, dtype=DT_NAME[dtype], tensor=m["name"], ratio_rms=round(m["ratio_rms"], 4),
                                        ratio_max=round(m["ratio_max"], 4), model_dist=round(m["model_dist"], 4),
                                        max_exempt=m["max_exempt"], ok=m["ok"])) + "\n")
    return ms, bad


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_step_matches_the_float64_model(name, dtype):
    ms, bad = _measured(name, dtype)
    assert len(ms) == len(R.tensor_names(R.step_ref64(name, dtype)))
    worst = max(ms, key=lambda m: m["ratio_rms"])
    print(f"{name} {DT_NAME[dtype]}: {len(ms)} tensors, worst rms ratio {worst['ratio_rms']:.3f} ({worst['name']}), "
          f"worst max ratio {max(m['ratio_max'] for m in ms if not m['max_exempt']):.3f}")
    assert not bad, "\n".join(bad)


def test_report_ratios():
    """rms(got - r64) / rms(E) and max|got - r64| / max|E| per tensor (the figures of profiles/student_step_parity.md), from the
    measurements of the tests above: nothing runs twice."""
    for name, dtype in CONFIGS:
        ms, _ = _measured(name, dtype)
        for m in ms:
            print(f"ratio {name} {DT_NAME[dtype]} {m['name']} rms {m['ratio_rms']:.3f} max {m['ratio_max']:.3f}"
                  f"{' (max-exempt)' if m['max_exempt'] else ''}")
