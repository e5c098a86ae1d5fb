"""GPU: bilinear resize of u8 frames (vmc_resize_bilinear_u8), to_pil_image's quantisation (vmc_unit_f32_to_u8) and what is built on
them: the student's floating-point input route, ``forward(..., unit_u8=True)`` and dataset_frame_diff_mn.collate_fn_device.

Every operation of the recipes is a single correctly rounded float32 operation, so every comparison is exact: f32 outputs are
compared as uint32, bytes with ``torch.equal``.  The reference is tests/bilinear_ref.py (pinned against aten's CPU kernel and the
stored outputs of the reference's ``_resize_frames`` by tests/test_bilinear_host.py); torch's CPU kernel is never called here."""
import os

import numpy as np
import pytest
import torch

import bilinear_ref as ref
from vimo_clip_amd import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPES = ("aten", "separable", "weights4")

# name -> (source shape [F,C,H,W], output size, key in tests/golden/bilinear_mn.npz or None)
CASES = {
    "37x53-32x48": ((2, 3, 37, 53), (32, 48), "a"),
    "1x1-16x16": ((1, 3, 1, 1), (16, 16), "b"),
    "45x80-28x31": ((2, 3, 45, 80), (28, 31), None),           # odd width: ragged row ends, unaligned rows
    "20x30-64x64": ((1, 3, 20, 30), (64, 64), "c"),            # upscale; OH + OW == 128, the last size of aten's small-output recipe
    "c1-64x64-32x32": ((1, 1, 64, 64), (32, 32), None),        # C = 1, scale exactly 2
    "identity-32x32": ((1, 3, 32, 32), (32, 32), None),
    "37x53-70x59": ((1, 3, 37, 53), (70, 59), None),           # OH + OW == 129: the first size of aten's separable recipe; odd width
    "5x40-10x517": ((1, 1, 5, 40), (10, 517), None),           # three column tiles, the last one ragged; two row tiles
}


@pytest.fixture(scope="module")
def golden_mn():
    return np.load(os.path.join(ROOT, "tests", "golden", "bilinear_mn.npz"))


@pytest.fixture(scope="module")
def refs(golden_mn):
    """name -> (u8 input, {recipe: f32 reference}), computed once and never written to."""
    out = {}
    for name, (shape, size, key) in CASES.items():
        if key:
            x = golden_mn[key + "_in"]
        else:
            x = np.random.default_rng(sum(shape) * 100 + size[1]).integers(0, 256, shape, dtype=np.uint8)
            x.reshape(-1)[:2] = (0, 255)
        want = {r: ref.resize_f32(x, size, r) for r in RECIPES}
        for w in want.values():
            w.setflags(write=False)
        out[name] = (x, want)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_f32_output_is_bit_equal_to_the_restatement_and_the_fixture(name, refs, golden_mn):
    shape, size, key = CASES[name]
    x, want = refs[name]
    xd = torch.from_numpy(x).cuda()
    for recipe in RECIPES:
        got = ops.resize_bilinear_u8(xd, size, recipe=recipe)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape[:2] + size and got.is_contiguous()
        diff = int((_bits(got.cpu().numpy()) != _bits(want[recipe])).sum())
        print(f"{name} {recipe}: {diff} of {got.numel()} f32 outputs differ")
        assert diff == 0, (name, recipe)
    if key:                                                    # what the reference's _resize_frames computed
        got = ops.resize_bilinear_u8(xd, size).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(golden_mn[key + "_f32"]))
    if name.startswith("identity"):
        assert np.array_equal(want["aten"], ref.unit(x))


@pytest.mark.parametrize("name", sorted(CASES))
def test_u8_output_equals_the_restatement_and_the_quantised_f32_output(name, refs, golden_mn):
    shape, size, key = CASES[name]
    x, want = refs[name]
    xd = torch.from_numpy(x).cuda()
    for recipe in RECIPES:
        got = ops.resize_bilinear_u8(xd, size, as_u8=True, recipe=recipe)
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape[:2] + size
        assert np.array_equal(got.cpu().numpy(), ref.to_u8(want[recipe])), (name, recipe)
        assert torch.equal(got, ops.unit_f32_to_u8(ops.resize_bilinear_u8(xd, size, recipe=recipe))), (name, recipe)
    if key:
        assert np.array_equal(ops.resize_bilinear_u8(xd, size, as_u8=True).cpu().numpy(), golden_mn[key + "_u8"])
    if name.startswith("identity"):
        assert torch.equal(ops.resize_bilinear_u8(xd, size, as_u8=True), xd)


def test_channels_last_source_is_read_in_place(refs):
    """A decoded [T,H,W,3] stack, permuted to [T,3,H,W] and row-cropped (nothing contiguous), gives what its NCHW copy gives; ``out``
    slices at odd byte offsets (scalar stores) hold the same values."""
    x, want = refs["45x80-28x31"]
    thwc = torch.from_numpy(np.ascontiguousarray(np.pad(x, ((0, 0), (0, 0), (1, 2), (0, 0))).transpose(0, 2, 3, 1))).cuda()
    view = thwc.permute(0, 3, 1, 2)[:, :, 1:-2]
    assert not view.is_contiguous() and view.stride(1) == 1 and view.stride(3) == 3 and torch.equal(view, torch.from_numpy(x).cuda())
    for as_u8 in (False, True):
        a = ops.resize_bilinear_u8(view, (28, 31), as_u8=as_u8)
        assert torch.equal(a, ops.resize_bilinear_u8(view.contiguous(), (28, 31), as_u8=as_u8))
        buf = torch.zeros(1 + a.numel() + 3, dtype=a.dtype, device="cuda")
        out = buf[1:1 + a.numel()].view(a.shape)               # one element past the allocation's alignment
        assert ops.resize_bilinear_u8(view, (28, 31), out=out, as_u8=as_u8) is out
        assert torch.equal(out, a) and not buf[0].item() and not buf[-3:].any().item()
    assert np.array_equal(_bits(ops.resize_bilinear_u8(view, (28, 31)).cpu().numpy()), _bits(want["aten"]))


def test_unit_f32_to_u8():
    v = torch.arange(256, device="cuda")
    assert torch.equal(ops.unit_f32_to_u8(v.float() / 255.0), v.to(torch.uint8))                  # same-size frames pass through
    assert torch.equal(ops.unit_f32_to_u8(v.float()), ((256 - v) % 256).to(torch.uint8))          # the wrap of integer-valued floats
    x = np.random.default_rng(3).random(1003, dtype=np.float32)                                   # 250 vectors and a tail of 3
    x[:2] = (0.0, 1.0)
    xd = torch.from_numpy(x).cuda()
    assert np.array_equal(ops.unit_f32_to_u8(xd).cpu().numpy(), ref.to_u8(x))
    assert np.array_equal(ops.unit_f32_to_u8(xd[1:]).cpu().numpy(), ref.to_u8(x[1:]))             # 4-byte aligned only: the scalar kernel
    assert tuple(ops.unit_f32_to_u8(xd[:1002].view(2, 3, 167)).shape) == (2, 3, 167)


# ---- the student -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def student():
    from vimo_clip_amd.models.student_model import FlowStudentModel
    torch.manual_seed(12)
    m = FlowStudentModel("ViT-B/32", device="cuda", num_classes=12)
    with torch.no_grad():                      # fc2 starts at zero, which would hide the frames from emb_distill's residual branch
        m.residual_mlp.fc2.weight.normal_(0, 0.02)
    return m


def _unit_frames(seed, hw):
    x = np.random.default_rng(seed).random((1, 2, 3) + hw, dtype=np.float32)
    x.reshape(-1)[:2] = (0.0, 1.0)
    return torch.from_numpy(x), torch.from_numpy(ref.to_u8(x))


@pytest.mark.parametrize("hw", [(224, 224), (64, 80)], ids=["224x224", "64x80-bicubic"])
def test_float_frames_are_quantised_like_to_pil_image(student, hw):
    """[0,1] float frames (what dataset_frame_diff_mn hands over) == their PIL pixels with unit_u8 == the heads on the encoder's
    output for those pixels without the wrap.  (64, 80) goes through the Pillow-exact bicubic resize + crop first."""
    m = student.eval()
    x, q = _unit_frames(hw[0], hw)
    with torch.no_grad():
        a = m(x)
        b = m(q, unit_u8=True)
        emb = m.visual_encoder.encode_frames_u8(q.view((2, 3) + hw).cuda(), wrap_quirk=False)
        c = m._heads(emb, False, 1, 2)
        wrapped = m(q)
    for ya, yb, yc in zip(a, b, c):
        assert torch.isfinite(ya).all() and torch.equal(ya, yb) and torch.equal(ya, yc)
    assert not torch.equal(a[0], wrapped[0])                   # plain u8 input keeps the wrap quirk


def test_integer_valued_float_frames_equal_their_u8_cast(student):
    m = student.eval()
    u8 = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (1, 2, 3, 224, 224), dtype=np.uint8))
    with torch.no_grad():
        for ya, yb in zip(m(u8), m(u8.float())):
            assert torch.equal(ya, yb)
        for ya, yb in zip(m(u8), m(u8.double().cuda())):
            assert torch.equal(ya, yb)


def test_train_mode_float_and_unit_u8_routes_agree(student):
    from vimo_clip_amd.losses import cross_entropy_loss, distillation_loss
    m = student.train()
    x, q = _unit_frames(9, (224, 224))
    teacher = torch.from_numpy(np.random.default_rng(10).standard_normal((1, 3, 512)).astype(np.float32)).cuda()
    target = torch.tensor([7], device="cuda")

    def step(frames, **kw):
        for p in m.parameters():
            p.grad = None
        _, emb_d, logits = m(frames, **kw)
        loss = distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + cross_entropy_loss(logits, target)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    la, ga = step(x)
    lb, gb = step(q, unit_u8=True)
    assert torch.isfinite(la) and torch.equal(la, lb)
    assert ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert all(torch.isfinite(g).all() for g in ga.values()) and float(ga["visual_encoder.conv1.weight"].abs().max()) > 0
    m.eval()


# ---- the device-side collate -------------------------------------------------------------------------------------------------
def test_collate_fn_device_equals_the_per_sample_restatement():
    """Two raw_u8 samples with different source sizes (one a permuted [T,H,W,3] view, as the dataset yields) into one u8 batch whose
    second slice starts at an odd byte offset."""
    from vimo_clip_amd.dataset_frame_diff_mn import collate_fn_device
    rng = np.random.default_rng(21)
    size, n = (15, 13), 3
    a = rng.integers(0, 256, (n, 20, 30, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (n, 3, 9, 7), dtype=np.uint8)
    samples = [{"video_id": "a", "rgb_emb": torch.zeros(n + 1, 4), "frame_diff": torch.from_numpy(a).permute(0, 3, 1, 2), "labels": torch.eye(3)[0]},
               {"video_id": "b", "rgb_emb": torch.ones(n + 1, 4), "frame_diff": torch.from_numpy(b), "labels": torch.eye(3)[2]}]
    batch = collate_fn_device(samples, size, "cuda")
    assert list(batch) == ["video_id", "rgb_emb", "frame_diff", "labels"] and batch["video_id"] == ["a", "b"]
    fd = batch["frame_diff"]
    assert fd.is_cuda and fd.dtype == torch.uint8 and tuple(fd.shape) == (2, n, 3) + size
    assert np.array_equal(fd[0].cpu().numpy(), ref.resize_u8(a.transpose(0, 3, 1, 2), size))
    assert np.array_equal(fd[1].cpu().numpy(), ref.resize_u8(b, size))
    assert tuple(batch["rgb_emb"].shape) == (2, n + 1, 4) and batch["labels"].argmax(1).tolist() == [0, 2]
    w4 = collate_fn_device(samples, (70, 59), "cuda", recipe="weights4")["frame_diff"]
    assert np.array_equal(w4[1].cpu().numpy(), ref.resize_u8(b, (70, 59), "weights4"))
