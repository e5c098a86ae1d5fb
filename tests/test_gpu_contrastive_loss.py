"""GPU: vimo_clip_amd.losses.distillation_loss(mode="contrastive") against the composed float64 reference of tests/contrastive_refs.py
(both 16-bit roundings included) under the bounds derived there: loss and gradient, the strided teacher, the upstream scale, a student
without gradient, the mask switch, the single-clip zero, run-to-run bits, a captured graph, and the top-1 figure."""
import functools

import pytest
import torch

import contrastive_refs as R
from contrastive_refs import BF16, DT16, DT_NAME, F16, F32, F64

pytestmark = pytest.mark.gpu
CASES = [(shape, d) for shape in R.LOSS_SHAPES for d in DT16]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{DT_NAME[d]}" for s, d in CASES]


@functools.lru_cache(maxsize=None)
def _bounds(shape, dtype16, mask=True):
    B, T, E = shape
    s, buf = R.loss_inputs(B, T, E)
    return R.loss_bounds(s.view(B * T, E), buf[:, :T].reshape(B * T, E), T, dtype16, mask=mask)


def _run(shape, dtype16, mask=True, grad=True, scale=None, dense=False, top1=False):
    """(loss, ds or None, top1 fraction or None) of the public function on the case's inputs, on the CPU."""
    from vimo_clip_amd.losses import distillation_loss
    B, T, E = shape
    s, buf = R.loss_inputs(B, T, E)
    sd = s.cuda().requires_grad_(grad)
    bd = buf.cuda()
    teacher = bd[:, :T].contiguous() if dense else bd[:, :-1]
    assert dense or not teacher.is_contiguous() or B == 1
    out = distillation_loss(sd, teacher, mode="contrastive", temperature=R.TAU, compute_dtype=dtype16, mask_same_clip=mask, return_top1=top1)
    loss, frac = out if top1 else (out, None)
    if grad:
        (loss if scale is None else scale * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), sd.grad.cpu() if grad else None, None if frac is None else frac.cpu()


def _check(shape, dtype16, loss, ds, mask=True, scale=1.0, tag=""):
    B, T, E = shape
    r, allow_loss, allow_ds, y = _bounds(shape, dtype16, mask)
    d = abs(float(loss) - float(r["loss"]))
    x = ((ds.view(B * T, E).double() / scale - r["ds"]).abs() / allow_ds).max().item()
    rel = ((ds.view(B * T, E).double() / scale - r["ds"]).abs().max() / r["ds"].abs().max()).item()
    print(f"{shape} {DT_NAME[dtype16]} mask {mask} {tag}: loss {float(loss):.6f} off by {d:.2e} of {allow_loss:.2e} ({d / allow_loss:.3f}); "
          f"ds excess {x:.3f} of its element bound, {rel:.2e} of max|ds|; flippable dz16 entries {y['flips']}")
    assert d <= allow_loss, (shape, tag, "loss", d, allow_loss)
    assert x <= 1.0, (shape, tag, "ds", x)


# one clip with the mask on is the exact-zero case further down; its unmasked form is in the mask test
@pytest.mark.parametrize("shape,dtype16", [c for c in CASES if c[0][0] > 1], ids=[i for i, c in zip(IDS, CASES) if c[0][0] > 1])
def test_loss_and_gradient_meet_the_derived_bounds_with_the_strided_teacher(shape, dtype16):
    loss, ds, _ = _run(shape, dtype16)
    _check(shape, dtype16, loss, ds, tag="slice")
    loss_d, ds_d, _ = _run(shape, dtype16, dense=True)            # the dense copy of the same rows: the same bits
    assert torch.equal(loss_d.view(torch.int32), loss.view(torch.int32)) and torch.equal(ds_d.view(torch.int32), ds.view(torch.int32))


@pytest.mark.parametrize("shape,dtype16", CASES, ids=IDS)
def test_mask_off_uses_every_pair(shape, dtype16):
    loss, ds, _ = _run(shape, dtype16, mask=False)
    _check(shape, dtype16, loss, ds, mask=False, tag="no mask")
    if shape[0] > 1:
        assert float(loss) > float(_bounds(shape, dtype16)[0]["loss"])          # more negatives: a larger loss than with the mask


@pytest.mark.parametrize("dtype16", DT16, ids=[DT_NAME[d] for d in DT16])
def test_upstream_scale_scales_the_gradient(dtype16):
    shape = R.LOSS_SHAPES[0]
    loss, ds, _ = _run(shape, dtype16)
    loss3, ds3, _ = _run(shape, dtype16, scale=3.0)
    assert torch.equal(loss3.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(ds3, 3.0 * ds)                              # one fp32 product per element
    _check(shape, dtype16, loss3, ds3, scale=3.0, tag="3 x loss")


def test_student_without_gradient_skips_the_gradient_half(monkeypatch):
    from vimo_clip_amd import losses
    shape = R.LOSS_SHAPES[1]
    want, _, _ = _run(shape, BF16)
    calls = {"linear": 0, "dz": [], "norm_bwd": 0}
    linear, softmax, norm_bwd = losses.ops.linear, losses.lib.vmc_contrastive_softmax, losses.lib.vmc_contrastive_norm_bwd

    def count_linear(*a, **k):
        calls["linear"] += 1
        return linear(*a, **k)

    def see_softmax(*a):
        calls["dz"].append(a[8])
        return softmax(*a)

    def count_norm_bwd(*a):
        calls["norm_bwd"] += 1
        return norm_bwd(*a)
    monkeypatch.setattr(losses.ops, "linear", count_linear)
    monkeypatch.setattr(losses.lib, "vmc_contrastive_softmax", see_softmax)
    monkeypatch.setattr(losses.lib, "vmc_contrastive_norm_bwd", count_norm_bwd)
    loss, _, _ = _run(shape, BF16, grad=False)
    assert calls == {"linear": 1, "dz": [None], "norm_bwd": 0}
    assert torch.equal(loss.view(torch.int32), want.view(torch.int32)) and not loss.requires_grad
    with torch.no_grad():                                          # and under no_grad with a student that would want one
        from vimo_clip_amd.losses import distillation_loss
        s, buf = R.loss_inputs(*shape)
        out = distillation_loss(s.cuda().requires_grad_(True), buf.cuda()[:, :-1], mode="contrastive", temperature=R.TAU)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))
    loss, ds, _ = _run(shape, BF16)                                # with a gradient: both GEMMs, a dz16 buffer, the backward
    assert calls["linear"] == 4 and calls["dz"][-1] is not None and calls["norm_bwd"] == 1 and ds is not None


@pytest.mark.parametrize("dtype16", DT16, ids=[DT_NAME[d] for d in DT16])
def test_one_clip_gives_exactly_zero(dtype16):
    loss, ds, frac = _run((1, 65, 64), dtype16, top1=True)
    assert float(loss) == 0.0 and not ds.any().item() and float(frac) == 1.0
    s2 = R.loss_inputs(3, 5, 64)[0].view(15, 64)                   # a 2-D input: every row its own clip, nothing is masked
    from vimo_clip_amd.losses import distillation_loss
    t2 = R.loss_inputs(3, 5, 64)[1][:, :5].reshape(15, 64)
    l2 = distillation_loss(s2.cuda(), t2.cuda(), mode="contrastive", temperature=R.TAU, compute_dtype=dtype16)
    l3, _, _ = _run((3, 5, 64), dtype16, mask=False, grad=False)
    assert torch.equal(l2.cpu().view(torch.int32), l3.view(torch.int32))


@pytest.mark.parametrize("shape,dtype16", [CASES[2], CASES[5]], ids=[IDS[2], IDS[5]])
def test_two_runs_give_the_same_bits(shape, dtype16):
    a, b = _run(shape, dtype16, top1=True), _run(shape, dtype16, top1=True)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype16", DT16, ids=[DT_NAME[d] for d in DT16])
def test_captured_graph_replays_on_new_inputs_bit_for_bit(dtype16):
    from vimo_clip_amd.losses import distillation_loss
    B, T, E = R.LOSS_SHAPES[0]
    s, buf = R.loss_inputs(B, T, E)
    s_in, t_in = s.cuda().requires_grad_(True), buf.cuda()

    def step():
        loss, frac = distillation_loss(s_in, t_in[:, :-1], mode="contrastive", temperature=R.TAU, compute_dtype=dtype16, return_top1=True)
        (g,) = torch.autograd.grad(loss, s_in)
        return loss, frac, g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up off the capture, as torch asks
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    with torch.no_grad():                                          # other values in the captured buffers: rows in another order, scaled
        s_in.copy_(s.flip(0).cuda() * 1.25)
        t_in.copy_(torch.nan_to_num(buf, nan=3.0).flip(1).cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = [x.detach().clone() for x in out]
    want = step()
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32), y.detach().view(torch.int32)) for x, y in zip(got, want))
    assert torch.isfinite(got[0]).item() and float(got[0]) > 0.0 and got[2].any().item()


@pytest.mark.parametrize("shape,dtype16", CASES, ids=IDS)
def test_top1_fraction_agrees_with_the_reference(shape, dtype16):
    B, T, E = shape
    for mask in (True, False):
        r, _, _, y = _bounds(shape, dtype16, mask)
        assert y["top1_margin"] > 2 * y["e_z"]                     # the count is decided on these inputs
        _, _, frac = _run(shape, dtype16, mask=mask, grad=False, top1=True)
        assert frac.shape == (1,) and frac.dtype == torch.float32
        assert float(frac) == pytest.approx(r["top1"] / (B * T), abs=1e-7), (shape, mask)
