"""GPU: drop path in the student's training step (autograd_vit.vit_forward_train(drop_keep=), FlowStudentModel(drop_path=)).

Every case of tests/drop_path_refs.py is run in bf16 and f16 with explicit keep sets and given upstream gradients; every output and
every parameter gradient, read from the slots of a NaN-filled gradient arena, is held to the float64 model with student_step_refs'
measure and thresholds (no new tolerance).  Then the properties a subset form has and a masked form need not: a dropped frame's
stream cannot depend on the block it skipped (exact bits), nothing new is launched unless the feature is on in a training forward,
the draw stream, the compositions, and a captured step that draws anew on every replay."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import drop_path_refs as R                       # noqa: E402
import student_step_refs as S                    # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16      # noqa: E402
from vimo_clip_amd import synth                  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (BF16, F16)
CONFIGS = [(c["name"], dt) for c in R.CASES for dt in DTYPES]
CFG_ID = lambda v: v if isinstance(v, str) else DT_NAME[v]
NEW_OPS = ("drop_path_sample", "frame_gather", "frame_scatter_add", "drop_path_merge", "drop_path_merge_bwd")


def _keeps(drop):
    return [None if d is None else torch.tensor(d, dtype=torch.int32, device="cuda") for d in drop]


# ---------------------------------------------------------------------------------------------- parity with the float64 model
def step_on_gpu(name, dtype):
    """test_gpu_student_step_parity.step_on_gpu with the case's keep sets: {tensor name: CPU tensor} under student_step_refs' names."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.autograd_vit import vit_forward_train
    from vimo_clip_amd.clip_vit import VisionTransformer
    from vimo_clip_amd.optim import GradArena
    dc = R.DBY_NAME[name]
    inp = R.make_inputs(dc["base"], dtype)
    c = inp["case"]
    student = c["level"] == "student"
    tower = VisionTransformer(c["R"], c["p"], S.WIDTH, S.LAYERS, S.HEADS, c["E"], compute_dtype=dtype)
    tower.cls_only_last_block = c["cls_only"]
    if student:
        from vimo_clip_amd.models.student_model import FlowStudentModel
        m = FlowStudentModel("ViT-tiny/32", device="cuda", num_classes=c["C"], alpha=0.1, compute_dtype=dtype)
        m.visual_encoder, prefix = tower, "visual_encoder."
    else:
        m, prefix = tower, ""
    m = m.cuda().train()
    sd = {(prefix if n not in S.HEAD_PARAMS else "") + n: v for n, v in inp["p32"].items()}
    m.load_state_dict(sd, strict=True)
    params = dict(m.named_parameters())
    arena = GradArena(m.parameters())
    arena.flat_grad.fill_(float("nan"))
    frames = inp["frames"].cuda()
    keeps = _keeps(dc["drop"])
    if student:
        outs = m(frames.reshape(c["B"], c["T"], 3, c["R"], c["R"]), drop_path_keep=keeps)
        names = ("emb", "emb_distill", "logits")
    else:
        outs, names = (vit_forward_train(m, frames, wrap_quirk=True, drop_keep=keeps),), ("E",)
    ups = [inp["up"][n].reshape(o.shape).cuda() for n, o in zip(names, outs)]
    parked, push = [], ag.wgrad_queue.push
    ag.wgrad_queue.push = lambda *a: (parked.append(a[2].shape), push(*a))[1]
    try:
        torch.autograd.backward(list(outs), ups)
    finally:
        del ag.wgrad_queue.push
    ag.wgrad_queue.flush()
    torch.cuda.synchronize()
    # dp_i: block 0 is not wrapped and its four linears on 3200 rows leave as grouped launches; block 1's 2400 rows do not
    assert len(parked) == (4 if name == "dp_i" else 0), parked
    got = {n: o.detach().float().cpu().reshape(inp["up"][n].shape) for n, o in zip(names, outs)}
    for n in inp["p32"]:
        g = params[(prefix if n not in S.HEAD_PARAMS else "") + n]._vmc_grad
        assert g is not None, f"{n}: no gradient slot"
        got["g." + n] = g.detach().float().cpu().reshape(inp["p32"][n].shape)
    return got


@functools.lru_cache(maxsize=None)
def _measured(name, dtype):
    r, m16 = R.step_ref64(name, dtype), R.step_model16(name, dtype)
    got = step_on_gpu(name, dtype)
    assert set(got) == set(R.tensor_names(r)), set(got) ^ set(R.tensor_names(r))
    return R.check(got, r, m16)


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_step_matches_the_float64_model(name, dtype):
    ms, bad = _measured(name, dtype)
    assert len(ms) == len(R.tensor_names(R.step_ref64(name, dtype)))
    worst = max(ms, key=lambda m: m["ratio_rms"])
    print(f"{name} {DT_NAME[dtype]}: {len(ms)} tensors, worst rms ratio {worst['ratio_rms']:.3f} ({worst['name']}), "
          f"worst max ratio {max(m['ratio_max'] for m in ms if not m['max_exempt']):.3f}")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- small student steps
B, T = 2, 2
FRAMES = B * T
NAME = "ViT-tiny/32"               # 64 x 64 frames, 5 tokens, 2 blocks


def _student(seed=61, dtype=BF16, cls_only=True, **kw):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.models import FlowStudentModel
    ag.weights.clear()
    m = FlowStudentModel(NAME, device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype, **kw)
    missing, unexpected = m.load_state_dict(synth.student_state_dict(NAME, seed), strict=False)
    assert not unexpected and all("lora" in k for k in missing), (missing, unexpected)
    m.visual_encoder.cls_only_last_block = cls_only
    return m.train()


def _inputs(seed=61, b=B, t=T):
    R_, E = synth.VIT_GEOMETRY[NAME][0], synth.VIT_GEOMETRY[NAME][5]
    return (synth.randint_u8(seed, "vids", (b, t, 3, R_, R_)).cuda(), synth.normal(seed, "teacher", (b, t + 1, E)).cuda(),
            synth.multi_hot_labels(seed, "labels", b, 140).cuda())


def _loss(m, vids, teacher, labels, **fwd):
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    emb, emb_d, logits = m(vids, **fwd)
    return (emb, emb_d, logits), distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)


def _step(m, vids, teacher, labels, **fwd):
    """One student step on a NaN-filled arena: (outputs, gradients of the trained parameters by name)."""
    from vimo_clip_amd.optim import GradArena
    arena = GradArena(m.parameters())
    arena.flat_grad.fill_(float("nan"))
    outs, loss = _loss(m, vids, teacher, labels, **fwd)
    loss.backward()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


class _Spy:
    """Counts the calls of the five new ops wrappers and keeps what the sampler returned."""

    def __init__(self, monkeypatch):
        from vimo_clip_amd import ops
        self.calls = dict.fromkeys(NEW_OPS, 0)
        self.draws = []
        for name in NEW_OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def inner(*a, **kw):
            self.calls[name] += 1
            out = fn(*a, **kw)
            if name == "drop_path_sample":
                self.draws.append((a[1], out[0].clone(), out[1].clone()))          # (block, keep, slot)
            return out
        return inner

    @property
    def total(self):
        return sum(self.calls.values())


def _assert_same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what


def test_a_dropped_frame_does_not_depend_on_the_block_it_skipped():
    """Drop only in block 1, not cls_only: the stream rows of the dropped frames behind the tower are the same bits whatever block
    1's weights are; the kept frames' rows are not."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.autograd_vit import vit_tokens_train
    vids = _inputs(67)[0]
    frames = vids.view(FRAMES, 3, 64, 64)
    keep = [None, torch.tensor([1, 2], dtype=torch.int32, device="cuda")]
    streams = []
    for garbage in (False, True):
        v = _student(67, cls_only=False).visual_encoder
        if garbage:
            gen = torch.Generator(device="cuda").manual_seed(3)
            with torch.no_grad():
                for p in v.transformer.resblocks[1].parameters():
                    p.copy_(torch.randn(p.shape, generator=gen, device="cuda") * 0.5)          # finite garbage
            ag.weights.clear()
        xs, Fr, N, rows_are_cls = vit_tokens_train(v, frames, True, cls_only=False, drop_keep=keep)
        assert (Fr, N, rows_are_cls) == (FRAMES, 5, False) and torch.isfinite(xs).all().item()
        streams.append(xs.detach().view(FRAMES, N, -1).clone())
    a, b = streams
    for f in (0, 3):
        _assert_same(a[f], b[f], f"dropped frame {f}")
    for f in (1, 2):
        assert not torch.equal(a[f], b[f]), f"kept frame {f} ignores its block"


def test_default_launches_nothing_new(monkeypatch):
    vids, teacher, labels = _inputs(71)
    spy = _Spy(monkeypatch)
    plain = _student(71)
    assert plain.visual_encoder.drop_path == 0.0
    plain_out, plain_grads = _step(plain, vids, teacher, labels)
    assert spy.total == 0, spy.calls
    on = _student(71, drop_path=0.3)
    for x, y in zip([o.detach() for o in on.eval()(vids)], [o.detach() for o in plain.eval()(vids)]):
        _assert_same(x, y, "eval()")
    on.train(), plain.train()
    with torch.no_grad():
        for x, y in zip(on(vids), plain(vids)):
            _assert_same(x, y, "no_grad()")
    assert spy.total == 0, spy.calls
    # on, in a training forward: the 2-block model wraps block 1 alone -- one draw, one gather, one merge, and their backwards
    got_out, got_grads = _step(_student(71, drop_path=0.5), vids, teacher, labels)
    assert spy.calls == dict.fromkeys(NEW_OPS, 1), spy.calls
    block, keep, slot = spy.draws[0]
    assert block == 1 and keep.numel() == 2 and slot.numel() == FRAMES
    assert not torch.equal(got_out[0], plain_out[0])
    for k, g in got_grads.items():
        assert torch.isfinite(g).all().item(), k
    # a model that was built with the feature and has it switched off again is the model without it, bit for bit
    off = _student(71, drop_path=0.5)
    off.visual_encoder.drop_path = 0.0
    off_out, off_grads = _step(off, vids, teacher, labels)
    for x, y in zip(off_out, plain_out):
        _assert_same(x, y, "drop_path = 0")
    for k, g in plain_grads.items():
        _assert_same(off_grads[k], g, k)


def test_draw_stream(monkeypatch):
    vids = _inputs(73, b=4, t=4)[0]              # 16 frames: K_1 = 8
    F = 16
    spy = _Spy(monkeypatch)
    fwd = lambda m: [o.detach().clone() for o in m(vids)]
    a = _student(73, drop_path=0.5, drop_path_seed=7)
    a1, a2 = fwd(a), fwd(a)
    assert spy.calls["drop_path_sample"] == 2
    k1 = spy.draws[0][1].cpu().numpy()
    assert k1.shape == (8,) and (np.diff(k1) > 0).all() and k1.min() >= 0 and k1.max() < F
    assert not torch.equal(spy.draws[0][1], spy.draws[1][1]) and not torch.equal(a1[0], a2[0])          # the next call differs
    b1 = fwd(_student(73, drop_path=0.5, drop_path_seed=7))
    assert torch.equal(spy.draws[2][1], spy.draws[0][1]) and torch.equal(spy.draws[2][2], spy.draws[0][2])      # same seed, same call index
    for x, y in zip(a1, b1):
        _assert_same(x, y, "same seed and call index")
    c = _student(73, drop_path=0.5, drop_path_seed=8)
    fwd(c)
    assert not torch.equal(spy.draws[3][1], spy.draws[0][1])                                          # another seed, another draw
    # a seed in device-address form is used as it is: the draw is the reference's for the stored value
    cell = torch.tensor([1234567], dtype=torch.int64, device="cuda")
    c.visual_encoder.drop_path_seed_address = (1 << 63) | cell.data_ptr()
    fwd(c)
    keep, slot = R.sample(1234567, 1, F, 8)
    assert np.array_equal(spy.draws[4][1].cpu().numpy(), keep) and np.array_equal(spy.draws[4][2].cpu().numpy(), slot)
    # an explicit keep set overrides the draw
    before = spy.calls["drop_path_sample"]
    d = [o.detach().clone() for o in c(vids, drop_path_keep=[None, torch.from_numpy(keep).cuda()])]
    assert spy.calls["drop_path_sample"] == before
    for x, y in zip(d, fwd(c)):                                                                      # the cell still holds 1234567
        _assert_same(x, y, "explicit keep set = the draw it restates")


# ---------------------------------------------------------------------------------------------- compositions
KEEPS = [(0, 1, 3), (2, 3)]


@pytest.mark.parametrize("cls_only", [True, False])
def test_block_recompute_is_bit_identical_under_the_same_keep_sets(cls_only):
    vids, teacher, labels = _inputs(79)
    got = {mode: _step(_student(79, cls_only=cls_only, recompute=mode), vids, teacher, labels, drop_path_keep=_keeps(KEEPS))
           for mode in ("none", "block")}
    for a, b in zip(got["none"][0], got["block"][0]):
        _assert_same(a, b, "outputs")
    assert set(got["none"][1]) == set(got["block"][1])
    for k, g in got["none"][1].items():
        assert torch.isfinite(g).all().item(), k
        _assert_same(g, got["block"][1][k], k)


def test_with_patch_dropout():
    """N' = 3 token rows per frame (the class token and 2 of 4 patches) under both keep sets."""
    vids, teacher, labels = _inputs(83)
    patch_keep = torch.tensor([(0, 3), (1, 2), (0, 1), (2, 3)], dtype=torch.int32, device="cuda")
    outs, grads = _step(_student(83), vids, teacher, labels, patch_keep=patch_keep, drop_path_keep=_keeps(KEEPS))
    plain, _ = _step(_student(83), vids, teacher, labels, patch_keep=patch_keep)
    assert all(torch.isfinite(o).all().item() for o in outs) and not torch.equal(outs[0], plain[0])
    for k, g in grads.items():
        assert torch.isfinite(g).all().item(), k
    m = _student(83, patch_dropout=0.5, drop_path=0.5)                          # and both drawn
    outs, grads = _step(m, vids, teacher, labels)
    assert all(torch.isfinite(o).all().item() for o in outs) and all(torch.isfinite(g).all().item() for g in grads.values())


def test_with_lora_adapters():
    vids, teacher, labels = _inputs(89)
    m = _student(89, lora_rank=8)
    torch.manual_seed(89)
    for k, p in m.named_parameters():
        if k.endswith("lora_B"):                               # zero-initialised: give the adapters something to do
            p.data.normal_(std=0.02)
    outs, grads = _step(m, vids, teacher, labels, drop_path_keep=_keeps(KEEPS))
    trained = {k for k, p in m.named_parameters() if p.requires_grad}
    assert trained and any("lora" in k for k in trained) and set(grads) == trained
    for k in trained:
        assert torch.isfinite(grads[k]).all().item(), k
        if "lora_A" in k or "lora_B" in k:
            assert float(grads[k].abs().max()) > 0, k          # every block's adapters saw kept frames
    assert all(torch.isfinite(o).all().item() for o in outs)


# ---------------------------------------------------------------------------------------------- a captured step
def test_captured_step_draws_anew_on_every_replay():
    """graphs.GraphedTrainStep with the seed address of FusedAdam's device state: the captured sampler launch re-reads the seed that
    vmc_train_tick rewrites, so two replays on the same batch keep different frames (lr = 0: nothing else changes between them), and
    each replay is the eager forward with the reference's keep set for the seed it read.  This process keeps the default number of
    hardware queues."""
    from vimo_clip_amd.graphs import GraphedTrainStep
    from vimo_clip_amd.optim import FusedAdam, GradArena
    vids, teacher, labels = _inputs(97, b=4, t=4)
    F, K = 16, 8
    m = _student(97, drop_path=0.5)
    opt = FusedAdam(GradArena(m.parameters()), lr=0.0).enable_device_state(base_seed=11)
    m.visual_encoder.drop_path_seed_address = opt.seed_address(0)

    def step(v, t, y):
        opt.tick()
        outs, loss = _loss(m, v, t, y)
        loss.backward()
        opt.step()
        return outs[0].detach()

    run = GraphedTrainStep(step, opt)
    embs, seeds = [], []
    for _ in range(2):
        embs.append(run(vids, teacher, labels).clone())
        torch.cuda.synchronize()
        seeds.append(int(opt.dev_state[2].item()) & 0xFFFFFFFFFFFFFFFF)
    assert run.n_graphs == 1 and seeds[0] != seeds[1]
    assert not torch.equal(embs[0], embs[1])
    keeps = [R.sample(s, 1, F, K)[0] for s in seeds]
    assert not np.array_equal(keeps[0], keeps[1])
    for emb, keep in zip(embs, keeps):
        eager = m(vids, drop_path_keep=[None, torch.from_numpy(keep).cuda()])[0].detach()
        _assert_same(emb.view(eager.shape), eager, "replay = eager forward with the reference's keep set")
