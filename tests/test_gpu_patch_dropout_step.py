"""GPU: patch dropout in the student's training step (autograd_vit.vit_tokens_train(keep=), FlowStudentModel(patch_dropout=)).

The yardstick is the existing, separately pinned path.  Three facts carry the file:
  * keeping every patch is the plain step;
  * when every frame keeps the SAME Kp patches, the step is the existing model at the smaller resolution R' = sqrt(Kp) p whose
    positional embedding holds the gathered rows, fed frames re-tiled from the kept patches: every GEMM, LayerNorm and attention
    launch then has the same shape and operands, so outputs and parameter gradients are the same bits;
  * no operator couples frames, so with per-frame keep sets row f of the output is row f of the shared-keep run that uses keep_f.
Only the positional / class gradients may differ from the smaller model's (it sums over frames with vmc_colsum, the keep path in
frame order): they are held to the fp32 reassociation bound F 2^-23 sum_f |addend|, the addends being the dx rows handed to the
backward kernel.  Geometry: ViT-tiny/32 at R = 128 and ViT-tiny/14 at R = 56 (K-padded patch rows), g = 4, F = 4 frames; the
gradient arena is pre-filled with NaN."""
import numpy as np
import pytest
import torch

import patch_dropout_ref as PR
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
B, T = 2, 2
FRAMES = B * T
G_SIDE = 4
POS_KEY, CLS_KEY = "visual_encoder.positional_embedding", "visual_encoder.class_embedding"
NEW_OPS = ("patch_keep_sample", "gather_rows16", "assemble_tokens_keep", "assemble_tokens_keep_bwd")

# shared keep sets on the 4 x 4 grid (ascending ids)
KEEP4 = (1, 6, 8, 15)
KEEP9 = (0, 2, 3, 5, 6, 9, 11, 12, 14)


def _base(patch):
    return {32: "ViT-tiny/32", 14: "ViT-tiny/14"}[patch]


def _weights(patch, seed):
    """Student weights of the base geometry with a 17-row positional embedding (g = 4)."""
    name = _base(patch)
    sd = synth.student_state_dict(name, seed)
    D = synth.vit_geometry(name)[2]
    sd[POS_KEY] = synth.normal(seed, "pos17", (G_SIDE * G_SIDE + 1, D), std=D ** -0.5)
    return sd


def _student(patch, side, sd, dtype=BF16, cls_only=True, recompute="none", **kw):
    """FlowStudentModel of the base geometry at resolution side x patch, weights `sd` (whose positional embedding has side^2 + 1 rows)."""
    from vimo_clip_amd.models import FlowStudentModel
    m = FlowStudentModel(_base(patch), device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype, recompute=recompute, **kw)
    v = m.visual_encoder
    v.input_resolution = side * patch
    v.positional_embedding = torch.nn.Parameter(torch.empty((side * side + 1, v.width), device="cuda"),
                                                requires_grad=v.positional_embedding.requires_grad)       # frozen under LoRA
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("lora" in k for k in missing), (missing, unexpected)      # only adapters keep their initial values
    v.cls_only_last_block = cls_only
    return m.train()


def _inputs(patch, seed):
    E = synth.vit_geometry(_base(patch))[5]
    R = G_SIDE * patch
    return (synth.randint_u8(seed, "vids", (B, T, 3, R, R)).cuda(), synth.normal(seed, "teacher", (B, T + 1, E)).cuda(),
            synth.multi_hot_labels(seed, "labels", B, 140).cuda())


def _keep_tensor(rows):
    return torch.tensor(rows, dtype=torch.int32, device="cuda")


def _retile(vids, keep_rows, patch):
    """Frames of side sqrt(Kp) x patch made of the kept patches of every frame, in keep order (row-major on the smaller grid)."""
    Fr = vids.shape[0] * vids.shape[1]
    g, p = G_SIDE, patch
    Kp = len(keep_rows[0])
    s = int(round(Kp ** 0.5))
    assert s * s == Kp
    tiles = vids.reshape(Fr, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(Fr, g * g, 3, p, p)
    idx = torch.tensor(keep_rows, dtype=torch.long, device=vids.device)
    sel = torch.gather(tiles, 1, idx.view(Fr, Kp, 1, 1, 1).expand(Fr, Kp, 3, p, p))
    small = sel.view(Fr, s, s, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(Fr, 3, s * p, s * p)
    return small.reshape(vids.shape[0], vids.shape[1], 3, s * p, s * p).contiguous()


def _step(m, vids, teacher, labels, **fwd):
    """One student step on a NaN-filled arena: (outputs, loss, gradients by name)."""
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    from vimo_clip_amd.optim import GradArena
    arena = GradArena(m.parameters())
    arena.flat_grad.fill_(float("nan"))
    emb, emb_d, logits = m(vids, **fwd)
    loss = distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)
    loss.backward()
    torch.cuda.synchronize()
    return ([o.detach().clone() for o in (emb, emb_d, logits)], loss.detach().clone(),
            {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})


class _Spy:
    """Counts the calls of the new ops wrappers and keeps what the backward kernel was handed."""

    def __init__(self, monkeypatch):
        from vimo_clip_amd import ops
        self.calls = dict.fromkeys(NEW_OPS, 0)
        self.dx, self.keeps = [], []
        for name in NEW_OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def inner(*a, **kw):
            self.calls[name] += 1
            if name == "assemble_tokens_keep_bwd":
                self.dx.append(a[0].detach().clone())
            out = fn(*a, **kw)
            if name == "patch_keep_sample":
                self.keeps.append(out.clone())
            return out
        return inner

    @property
    def total(self):
        return sum(self.calls.values())


def _sum_bound(dx, Kp):
    """[Kp + 1, D] float64: F 2^-23 sum_f |dx[f, t]|, the reassociation bound of a sum over the frames per token slot."""
    d = dx.double().cpu().view(FRAMES, Kp + 1, -1)
    return PR.reassociation_bound(FRAMES, d.abs().sum(0).numpy())


def _assert_same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what


# ---------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_keeping_every_patch_is_the_plain_step(monkeypatch, dtype):
    sd = _weights(32, 61)
    vids, teacher, labels = _inputs(32, 61)
    plain = _step(_student(32, G_SIDE, sd, dtype), vids, teacher, labels)
    spy = _Spy(monkeypatch)
    ident = _keep_tensor([list(range(16))] * FRAMES)
    kept = _step(_student(32, G_SIDE, sd, dtype), vids, teacher, labels, patch_keep=ident)
    assert spy.calls == {"patch_keep_sample": 0, "gather_rows16": 1, "assemble_tokens_keep": 1, "assemble_tokens_keep_bwd": 1}
    for a, b in zip(plain[0], kept[0]):
        _assert_same(a, b, "outputs")
    _assert_same(plain[1], kept[1], "loss")
    bound = _sum_bound(spy.dx[0], 16)
    for k, g in plain[2].items():
        assert torch.isfinite(kept[2][k]).all().item(), k
        if k == POS_KEY:
            err = (g.double() - kept[2][k].double()).abs().cpu().numpy()
            print(f"identity keep, dpos: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
            assert (err <= bound).all()
        elif k == CLS_KEY:
            assert ((g.double() - kept[2][k].double()).abs().cpu().numpy() <= bound[0]).all()
        else:
            _assert_same(g, kept[2][k], k)


# ---------------------------------------------------------------------------------------------- shared keep = smaller geometry
def _small_weights(sd, keep_row):
    small = dict(sd)
    small[POS_KEY] = sd[POS_KEY][[0] + [n + 1 for n in keep_row]].clone()
    return small


def _check_against_smaller_model(big, small, keep_row, dx):
    Kp = len(keep_row)
    bound = _sum_bound(dx, Kp)
    rows = [0] + [n + 1 for n in keep_row]
    dropped = [r for r in range(17) if r not in rows]
    for a, b in zip(big[0], small[0]):
        _assert_same(a, b, "outputs")
    _assert_same(big[1], small[1], "loss")
    for k, g in small[2].items():
        assert torch.isfinite(big[2][k]).all().item(), k
        if k == POS_KEY:
            err = (big[2][k][rows].double() - g.double()).abs().cpu().numpy()
            print(f"Kp={Kp}, dpos at the kept rows: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
            assert (err <= bound).all()
            assert (big[2][k][dropped].view(torch.int32) == 0).all().item()          # dropped positions: exact zeros
            assert (big[2][k][rows].abs().sum(1) > 0).all().item()
        elif k == CLS_KEY:
            assert ((big[2][k].double() - g.double()).abs().cpu().numpy() <= bound[0]).all()
        else:
            _assert_same(big[2][k], g, k)


@pytest.mark.parametrize("patch,keep_row,dtype,cls_only", [
    (32, KEEP4, BF16, True), (32, KEEP9, BF16, True), (32, KEEP4, F16, True), (32, KEEP9, BF16, False), (32, KEEP4, BF16, False),
    (14, KEEP4, BF16, True),                                   # p = 14: 588 patch columns padded to 640 (R' = 28; the patch kernels need R % 4 == 0)
], ids=lambda v: str(v).replace("torch.", ""))
def test_shared_keep_set_is_the_smaller_model_student_level(monkeypatch, patch, keep_row, dtype, cls_only):
    sd = _weights(patch, 67)
    vids, teacher, labels = _inputs(patch, 67)
    side = int(round(len(keep_row) ** 0.5))
    small = _step(_student(patch, side, _small_weights(sd, keep_row), dtype, cls_only), _retile(vids, [keep_row] * FRAMES, patch), teacher,
                  labels)
    spy = _Spy(monkeypatch)
    big = _step(_student(patch, G_SIDE, sd, dtype, cls_only), vids, teacher, labels, patch_keep=_keep_tensor([keep_row] * FRAMES))
    assert spy.calls["assemble_tokens_keep_bwd"] == 1 and spy.calls["patch_keep_sample"] == 0
    _check_against_smaller_model(big, small, keep_row, spy.dx[0])


def _tower(patch, side, sd, dtype=BF16, cls_only=True, recompute="none"):
    return _student(patch, side, sd, dtype, cls_only, recompute).visual_encoder


def _tower_step(v, frames, cot, keep=None):
    from vimo_clip_amd.autograd_vit import vit_forward_train
    from vimo_clip_amd.optim import GradArena
    arena = GradArena(v.parameters())
    arena.flat_grad.fill_(float("nan"))
    out = vit_forward_train(v, frames, wrap_quirk=True, keep=keep)
    out.backward(cot)
    torch.cuda.synchronize()
    return [out.detach().clone()], out.detach().sum(), {"visual_encoder." + k: p.grad.detach().clone() for k, p in v.named_parameters()}


@pytest.mark.parametrize("keep_row,cls_only", [(KEEP4, True), (KEEP9, True), (KEEP9, False)], ids=lambda v: str(v))
def test_shared_keep_set_is_the_smaller_model_tower_level(monkeypatch, keep_row, cls_only):
    from vimo_clip_amd.autograd_vit import vit_tokens_train
    sd = _weights(32, 71)
    vids = _inputs(32, 71)[0]
    frames = vids.view(FRAMES, 3, 128, 128)
    cot = synth.normal(71, "cot", (FRAMES, 64)).cuda()
    side = int(round(len(keep_row) ** 0.5))
    small_frames = _retile(vids, [keep_row] * FRAMES, 32).view(FRAMES, 3, side * 32, side * 32)
    small = _tower_step(_tower(32, side, _small_weights(sd, keep_row), cls_only=cls_only), small_frames, cot)
    spy = _Spy(monkeypatch)
    v = _tower(32, G_SIDE, sd, cls_only=cls_only)
    keep = _keep_tensor([keep_row] * FRAMES)
    big = _tower_step(v, frames, cot, keep)
    _check_against_smaller_model(big, small, keep_row, spy.dx[0])
    xs, Fr, N, rows_are_cls = vit_tokens_train(v, frames, True, cls_only=cls_only, keep=keep)       # the N it reports is N'
    assert (Fr, N, rows_are_cls) == (FRAMES, len(keep_row) + 1, cls_only)
    assert xs.shape[0] == (FRAMES if cls_only else FRAMES * N)


# ---------------------------------------------------------------------------------------------- per-frame keep sets
PER_FRAME = [(0, 5, 10, 15), (1, 6, 8, 15), (2, 3, 12, 13), (4, 7, 9, 14)]        # nobody keeps patch 11


def test_per_frame_keep_sets_forward_rows_and_backward(monkeypatch):
    from vimo_clip_amd.autograd_vit import vit_forward_train
    sd = _weights(32, 73)
    vids = _inputs(32, 73)[0]
    frames = vids.view(FRAMES, 3, 128, 128)
    v = _tower(32, G_SIDE, sd)
    cot = synth.normal(73, "cot", (FRAMES, 64)).cuda()
    outs, _, grads = _tower_step(v, frames, cot, _keep_tensor(PER_FRAME))
    for f, row in enumerate(PER_FRAME):
        with torch.enable_grad():
            shared = vit_forward_train(v, frames, wrap_quirk=True, keep=_keep_tensor([row] * FRAMES)).detach()
        _assert_same(outs[0][f], shared[f], f"frame {f}")
        assert not torch.equal(outs[0][(f + 1) % FRAMES], shared[(f + 1) % FRAMES])         # ... and the keep set matters
    kept = sorted({0} | {n + 1 for row in PER_FRAME for n in row})
    dropped = [r for r in range(17) if r not in kept]
    assert dropped == [12]
    for k, g in grads.items():
        assert torch.isfinite(g).all().item(), k
    dpos = grads[POS_KEY]
    assert (dpos[dropped].view(torch.int32) == 0).all().item() and (dpos[kept].abs().sum(1) > 0).all().item()


# ---------------------------------------------------------------------------------------------- recompute, LoRA
@pytest.mark.parametrize("cls_only", [True, False])
def test_block_recompute_with_a_keep_set_is_bit_identical(cls_only):
    sd = _weights(32, 79)
    vids, teacher, labels = _inputs(32, 79)
    keep = _keep_tensor(PER_FRAME)
    got = {mode: _step(_student(32, G_SIDE, sd, BF16, cls_only, recompute=mode), vids, teacher, labels, patch_keep=keep) for mode in ("none", "block")}
    for a, b in zip(got["none"][0], got["block"][0]):
        _assert_same(a, b, "outputs")
    for k, g in got["none"][2].items():
        assert torch.isfinite(g).all().item(), k
        _assert_same(g, got["block"][2][k], k)


def test_lora_adapters_train_under_a_keep_set():
    """A frozen tower with adapters: the keep path's class / positional gradients have no slot to go to and every trained gradient is
    finite; the no-grad forward of the live adapters sees every token."""
    sd = _weights(32, 83)
    vids, teacher, labels = _inputs(32, 83)
    m = _student(32, G_SIDE, sd, lora_rank=8, patch_dropout=0.5)
    torch.manual_seed(83)
    for k, p in m.named_parameters():
        if k.endswith("lora_B"):                               # zero-initialised: give the adapters something to do
            p.data.normal_(std=0.02)
    outs, loss, grads = _step(m, vids, teacher, labels, patch_keep=_keep_tensor(PER_FRAME))
    assert torch.isfinite(loss).item()
    trained = {k for k, p in m.named_parameters() if p.requires_grad}
    assert trained and POS_KEY not in trained
    for k in trained:
        assert torch.isfinite(grads[k]).all().item(), k
    ref = _student(32, G_SIDE, sd, lora_rank=8)
    ref.load_state_dict(m.state_dict())
    with torch.no_grad():
        for a, b in zip(m(vids), ref(vids)):
            _assert_same(a, b, "no-grad forward with live adapters")


# ---------------------------------------------------------------------------------------------- sampling at model level
def _forward(m, vids):
    return [o.detach().clone() for o in m(vids)]


def test_model_level_sampling(monkeypatch):
    sd = _weights(32, 89)
    vids = _inputs(32, 89)[0]
    spy = _Spy(monkeypatch)
    a = _student(32, G_SIDE, sd, patch_dropout=0.5, patch_dropout_seed=7)
    a1, a2 = _forward(a, vids), _forward(a, vids)
    assert spy.calls["patch_keep_sample"] == 2 and all(tuple(k.shape) == (FRAMES, 8) for k in spy.keeps)       # Kp = 8 of 16
    k1 = spy.keeps[0].cpu().numpy()
    assert (np.diff(k1, axis=1) > 0).all() and k1.min() >= 0 and k1.max() < 16
    assert not torch.equal(spy.keeps[0], spy.keeps[1]) and not torch.equal(a1[0], a2[0])                       # the next call differs
    b = _student(32, G_SIDE, sd, patch_dropout=0.5, patch_dropout_seed=7)
    b1 = _forward(b, vids)
    assert torch.equal(spy.keeps[2], spy.keeps[0])                                   # same seed, same call index: the same draw
    for x, y in zip(a1, b1):
        _assert_same(x, y, "same seed and call index")
    c = _student(32, G_SIDE, sd, patch_dropout=0.5, patch_dropout_seed=8)
    _forward(c, vids)
    assert not torch.equal(spy.keeps[3], spy.keeps[0])                               # another seed, another draw
    # a seed in device-address form is used as it is: the draw is the reference's for the stored value
    cell = torch.tensor([1234567], dtype=torch.int64, device="cuda")
    c.visual_encoder.patch_dropout_seed_address = (1 << 63) | cell.data_ptr()
    _forward(c, vids)
    assert np.array_equal(spy.keeps[4].cpu().numpy(), PR.keep_sample(1234567, FRAMES, 16, 8))
    # evaluation and no-grad see every token: the bits of a model that has no patch dropout, and nothing new is launched
    plain = _student(32, G_SIDE, sd)
    before = spy.total
    for x, y in zip(_forward(a.eval(), vids), _forward(plain.eval(), vids)):
        _assert_same(x, y, "eval()")
    a.train(), plain.train()
    with torch.no_grad():
        for x, y in zip(_forward(a, vids), _forward(plain, vids)):
            _assert_same(x, y, "no_grad()")
    assert spy.total == before


def test_default_launches_nothing_new(monkeypatch):
    sd = _weights(32, 97)
    vids, teacher, labels = _inputs(32, 97)
    spy = _Spy(monkeypatch)
    m = _student(32, G_SIDE, sd)
    assert m.visual_encoder.patch_dropout == 0.0
    _step(m, vids, teacher, labels)
    assert spy.total == 0, spy.calls
    _step(_student(32, G_SIDE, sd, patch_dropout=0.5), vids, teacher, labels)          # the spy does see the feature when it is on
    assert spy.calls == {"patch_keep_sample": 1, "gather_rows16": 1, "assemble_tokens_keep": 1, "assemble_tokens_keep_bwd": 1}
