"""GPU: one training step of FlowStudentModel with LoRA adapters (vimo_clip_amd/lora.py) -- forward, torch.autograd.backward with given
upstream gradients -- against tests/lora_refs.py: a float64 step and the float64 model of it that rounds where the path rounds
(method of §5.4).  The three outputs, every adapter gradient and the head gradients are read from the gradient
arena's slots (pre-filled with NaN: an element the backward does not write fails `finite`).  The conditions on the cases are asserted
on the CPU by tests/test_lora_refs_host.py.  Then: fresh adapters (B = 0), what stays frozen, two optimiser steps, merge_lora and the
recompute guard."""
import functools

import pytest
import torch

import lora_refs as LR
from lora_refs import BF16, DT16, DT_NAME, F32

pytestmark = pytest.mark.gpu

CONFIGS = [(c["name"], dt) for c in LR.STEP_CASES for dt in DT16]
CFG_ID = lambda v: v if isinstance(v, str) else DT_NAME[v]
PREFIX = "visual_encoder."


def build(name, dtype, fresh=False):
    """The case's student on the device with its weights and adapters loaded, and the arena (built after add_lora)."""
    from vimo_clip_amd.models.student_model import FlowStudentModel
    from vimo_clip_amd.optim import GradArena
    inp = LR.step_inputs(name, dtype, fresh)
    c = inp["case"]
    m = FlowStudentModel(c["geometry"], device="cuda", num_classes=c["C"], alpha=0.1, compute_dtype=dtype, lora_rank=c["rank"],
                         lora_alpha=c["alpha"], lora_targets=c["targets"]).train()
    vit = m.visual_encoder
    assert (vit.input_resolution, vit.patch_size, vit.layers, vit.output_dim, vit.width) == (c["R"], c["p"], c["L"], c["E"], LR.ST.WIDTH)
    sd = {(PREFIX if n not in LR.ST.HEAD_PARAMS else "") + n: v for n, v in inp["p32"].items()}
    sd.update({PREFIX + n: v for n, v in inp["ad32"].items()})
    m.load_state_dict(sd, strict=True)
    arena = GradArena(m.parameters())
    arena.flat_grad.fill_(float("nan"))
    return m, arena, inp


def run(m, inp):
    c = inp["case"]
    outs = m(inp["frames"].cuda().reshape(c["B"], c["T"], 3, c["R"], c["R"]))
    return dict(zip(("emb", "emb_distill", "logits"), outs))


def step_on_gpu(name, dtype, fresh=False):
    from vimo_clip_amd import autograd_ops as ag
    m, arena, inp = build(name, dtype, fresh)
    outs = run(m, inp)
    torch.autograd.backward(list(outs.values()), [inp["up"][n].reshape(o.shape).cuda() for n, o in outs.items()])
    ag.wgrad_queue.flush()
    torch.cuda.synchronize()
    got = {n: o.detach().float().cpu().reshape(inp["up"][n].shape) for n, o in outs.items()}
    params = dict(m.named_parameters())
    trained = list(inp["ad32"]) + list(LR.ST.HEAD_PARAMS)
    for n in trained:
        p = params[(PREFIX if n not in LR.ST.HEAD_PARAMS else "") + n]
        assert p.requires_grad and getattr(p, "_vmc_grad", None) is not None, f"{n}: no arena slot"
        got["g." + n] = p._vmc_grad.detach().float().cpu().clone()
    # no frozen parameter gets a gradient or an arena slot
    frozen = [n for n in params if n not in {(PREFIX if t not in LR.ST.HEAD_PARAMS else "") + t for t in trained}]
    assert len(frozen) == len(inp["p32"]) - 8
    for n in frozen:
        p = params[n]
        assert not p.requires_grad and p.grad is None and getattr(p, "_vmc_grad", None) is None, n
    assert len(arena.params) == len(trained)
    return got


@functools.lru_cache(maxsize=None)
def _measured(name, dtype):
    r, m16 = LR.step_ref64(name, dtype), LR.step_model16(name, dtype)
    got = step_on_gpu(name, dtype)
    assert set(got) == set(LR.ST.tensor_names(r)), set(got) ^ set(LR.ST.tensor_names(r))
    return LR.ST.check(got, r, m16)


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_step_matches_the_float64_model(name, dtype):
    ms, bad = _measured(name, dtype)
    worst = max(ms, key=lambda m: m["ratio_rms"])
    print(f"{name} {DT_NAME[dtype]}: {len(ms)} tensors, worst rms ratio {worst['ratio_rms']:.3f} ({worst['name']}), "
          f"worst max ratio {max(m['ratio_max'] for m in ms if not m['max_exempt']):.3f}")
    assert len(ms) == len(LR.ST.tensor_names(LR.step_ref64(name, dtype))) and not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DT16, ids=CFG_ID)
@pytest.mark.parametrize("name", ["t32-r8-attn", "t14-r8-attn+mlp"])
def test_fresh_adapters_start_as_the_base_model(name, dtype):
    """B = 0: every dA is exactly zero (us = round16(s dz 0)), every dB is not, and the outputs are the base model's: held to the same
    measure against the reference WITHOUT adapters."""
    got = step_on_gpu(name, dtype, fresh=True)
    inp = LR.step_inputs(name, dtype, True)
    for _w, an, bn in LR.adapter_names(inp["case"]):
        assert float(got["g." + an].abs().max()) == 0.0, an
        assert float(got["g." + bn].abs().max()) > 0.0 and bool(torch.isfinite(got["g." + bn]).all()), bn
    r, m16 = LR.step_ref64(name, dtype, True, False), LR.step_model16(name, dtype, True, False)
    ms, bad = LR.ST.check({k: got[k] for k in ("emb", "emb_distill", "logits")}, r, m16)
    assert len(ms) == 3 and not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DT16, ids=CFG_ID)
def test_two_optimiser_steps_move_the_adapters_and_nothing_else(dtype):
    """FusedAdam on the arena: the base masters are bit-identical before and after, and the second forward differs from the first --
    the re-cast tails of Wcat / WcatT and A16 / B16^T are what the kernels read.  The no-grad forward sees the adapters too."""
    from vimo_clip_amd.optim import FusedAdam
    m, arena, inp = build("t32-r16-attn+mlp", dtype)
    trained = {id(p) for p in arena.params}
    base = {n: p.detach().clone() for n, p in m.named_parameters() if id(p) not in trained}
    arena.zero_grad()                       # the slots' alignment gaps too: the optimiser walks the whole arena
    opt = FusedAdam(arena, lr=1e-2)
    embs = []
    for _ in range(2):
        outs = run(m, inp)
        embs.append(outs["emb"].detach().float().cpu())
        torch.autograd.backward(list(outs.values()), [inp["up"][n].reshape(o.shape).cuda() / LR.UP_SCALE[dtype] for n, o in outs.items()])
        opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if n in base:
            assert torch.equal(p.detach(), base[n]), f"{n}: a frozen master moved"
    assert not torch.equal(embs[0], embs[1]) and bool(torch.isfinite(embs[1]).all())
    with torch.no_grad():
        e_eval = run(m, inp)["emb"].float().cpu()
    e_train = run(m, inp)["emb"].detach().float().cpu()
    # same launches up to c_fc's side output (vmc_linear against vmc_linear_preact): the same values to within the compute type's
    # spacing at the largest embedding (2^-7 bf16, 2^-10 f16; two of them), far from the step the optimiser made
    gap, moved = float((e_eval - e_train).abs().max()), float((e_eval - embs[1]).abs().max())
    print(f"no-grad vs training forward {DT_NAME[dtype]}: max gap {gap:.3e}, moved by the second step {moved:.3e}")
    assert gap <= 2.0 ** (-6 if dtype is BF16 else -9) * float(e_train.abs().max()) and moved > 4 * gap and moved > 0


@pytest.mark.parametrize("dtype", DT16, ids=CFG_ID)
def test_merge_lora_returns_to_the_inference_path(dtype):
    from vimo_clip_amd import lora
    name = "t14-r16-attn"
    m, _arena, inp = build(name, dtype)
    c = inp["case"]
    vit = m.visual_encoder
    with torch.no_grad():
        live = run(m, inp)["emb"].float().cpu()
    keys_live = set(m.state_dict())
    lora.merge_lora(vit)
    torch.cuda.synchronize()
    assert getattr(vit, "lora", None) is None and all(p.requires_grad for p in m.parameters())
    assert set(m.state_dict()) == {k for k in keys_live if "lora_" not in k}
    params = dict(vit.named_parameters())
    for wn, an, bn in LR.adapter_names(c):
        W, A, B = inp["p32"][wn].double(), inp["ad32"][an].double(), inp["ad32"][bn].double()
        r64 = W + inp["s"] * (B @ A)
        r32 = (inp["p32"][wn] + inp["s"] * (inp["ad32"][bn] @ inp["ad32"][an])).double()
        res = LR.measure32(params[wn].detach().cpu(), r64, LR.e32_of(r32, r64))
        assert res["ok"], (wn, res)
    with torch.no_grad():
        frames = inp["frames"].cuda()
        merged = vit.encode_frames_u8(frames, wrap_quirk=True).float().cpu()          # the unchanged inference path
        again = m(frames.reshape(c["B"], c["T"], 3, c["R"], c["R"]))[0].float().cpu().reshape(merged.shape)
    assert bool(torch.isfinite(merged).all()) and torch.equal(again, merged)
    gap = float((merged - live.reshape(merged.shape)).abs().max() / live.abs().max())
    print(f"merged vs live-adapter embeddings, {name} {DT_NAME[dtype]}: max gap {gap:.3e} of max|emb| (the two round W differently)")


def test_recompute_guard():
    from vimo_clip_amd.autograd_vit import vit_forward_train
    from vimo_clip_amd.models.student_model import FlowStudentModel
    with pytest.raises(ValueError, match="recompute"):
        FlowStudentModel("ViT-tiny/32", device="cuda", num_classes=12, recompute="block", lora_rank=8)
    m = FlowStudentModel("ViT-tiny/32", device="cuda", num_classes=12, lora_rank=8)
    m.visual_encoder.recompute = "block"
    with pytest.raises(ValueError, match="recompute"):
        vit_forward_train(m.visual_encoder, torch.zeros((2, 3, 64, 64), dtype=torch.uint8, device="cuda"))
