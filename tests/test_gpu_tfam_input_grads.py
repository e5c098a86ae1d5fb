"""GPU: gradients wrt the input tokens out of the fused TFAM training chains (AMO_CLIP.fused_input_grads; the vmc_tfam_*_inputs
entries and vmc_concat_tokens_len_bwd, include/vmc.h).

References: torch autograd through the CPU oracle (oracle.tfam.amo_clip_forward) in float64 at dropout 0, and the per-op path with
dropout 0.1 on the same seeds (same masks).  All runs use bf16, C = 8, dim_feedforward = 512.  Bounds, restated unchanged from
tests/test_gpu_tfam_train.py: loss 5e-3 relative; logits 8e-3 * max(1, |ref|max); d rgb / d motion relative L2 <= 4e-2 against the
oracle (the bound of the chain's parameter gradients, measured there 0.5-1.5e-2) and <= 5e-2 against the per-op path with dropout.

The shapes are the smallest that reach each path (every case has B * T <= 256):
  a  cross, B 3, T 16 / 15, D 512, L 2   two clips per row block with an odd clip count; dMotion accumulated over two layers
  b  cross, B 2, T 24 / 23, D 512, L 2   one clip per block, two key tiles
  c  cross, B 2, T 40 / 39, D 512, L 1   query parts, four key tiles; one layer (dMotion written once, no residual operand)
  d  cross, B 2, T 16 / 15, D 768, L 2   head dim 96, the K = 1536 ring (dMotion) and the KC = 384 ring (dX)
  e  rgb-only, flow-only                 dX lands on the right stream, the other gets None
  f  concat 1, B 2, T 9 + 8              exact shape, and token_lens with bucket 16
  g  concat -1, D 512 and 768            dXcat (K = D, N = 2 D) with fused_feature_training
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from concat_bwd_ref import concat_bwd_ref      # noqa: E402
from oracle import make_golden as mg           # noqa: E402
from oracle import tfam as otfam               # noqa: E402
from vimo_clip_amd import synth                # noqa: E402

pytestmark = pytest.mark.gpu


def _case(name, mode, B, Tr, Tf, D, L, seed, H=8, ragged=True):
    return dict(name=name, mode=mode, B=B, Tr=Tr, Tf=Tf, D=D, H=H, L=L, ff=512, C=8, pe=False, ragged=ragged, seed=seed)


CASES = [
    _case("a_cross_b3", "cross", 3, 16, 15, 512, 2, 1101),
    _case("b_cross_t24", "cross", 2, 24, 23, 512, 2, 1102),
    _case("c_cross_t40", "cross", 2, 40, 39, 512, 1, 1103),
    _case("d_cross_d768", "cross", 2, 16, 15, 768, 2, 1104),
    _case("e_rgb", "rgb", 2, 16, 15, 512, 2, 1105),
    _case("e_flow", "flow", 2, 16, 15, 512, 2, 1106),
    _case("f_concat1", "concat1", 2, 9, 8, 512, 2, 1107),
    _case("g_concat-1_d512", "concat-1", 2, 16, 15, 512, 2, 1108),
    _case("g_concat-1_d768", "concat-1", 2, 16, 15, 768, 2, 1109),
]
BY_NAME = {c["name"]: c for c in CASES}
PARAM = pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])


def _pick(*names):
    return pytest.mark.parametrize("c", [BY_NAME[n] for n in names], ids=lambda c: c["name"])


def _model(c, dropout=0.0):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    m = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=c["C"], use_pe=c["pe"],
                 dropout=dropout, mlp_dropout=dropout, device="cuda", compute_dtype=torch.bfloat16, **mg.tfam_mode_kwargs(c["mode"])).cuda()
    m.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]), strict=True)
    m.fused_feature_training = True      # case g trains on the chains that start at the projection
    return m.train()


def _param_grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _step(m, c, switch, grad_inputs=True, fused=True, inputs=None, seed=None, **fwd_kw):
    """One step; returns (loss, logits, d rgb, d motion, parameter gradients, logits.grad_fn's name), everything on the device."""
    from vimo_clip_amd.losses import bce_with_logits_loss
    m.fused_training, m.fused_input_grads = fused, switch
    m.zero_grad(set_to_none=True)
    if seed is not None:
        m.set_dropout_seed(seed)
    rgb, mot, mr, mf = inputs if inputs is not None else (t.cuda() for t in mg.tfam_inputs(c))
    rgb = rgb.detach().clone().requires_grad_(grad_inputs)
    mot = mot.detach().clone().requires_grad_(grad_inputs)
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).cuda()
    logits = m(rgb, mot, mask_rgb=mr, mask_flow=mf, **fwd_kw)
    node = type(logits.grad_fn).__name__
    loss = bce_with_logits_loss(logits, y)
    loss.backward()
    return loss.item(), logits.detach(), rgb.grad, mot.grad, _param_grads(m), node


_ORACLE = {}


def _oracle(c):
    """(loss, logits, d rgb, d motion) of float64 autograd through the oracle; computed once per case and left unchanged."""
    if c["name"] not in _ORACLE:
        sd = {k: v.double() for k, v in synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]).items()}
        rgb, mot, mr, mf = mg.tfam_inputs(c)
        rgb, mot = rgb.double().requires_grad_(), mot.double().requires_grad_()
        y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).double()
        logits = otfam.amo_clip_forward(sd, rgb, mot, mr, mf, nhead=c["H"], use_pe=c["pe"], **mg.tfam_mode_kwargs(c["mode"]))
        loss = otfam.bce_with_logits_mean(logits, y)
        loss.backward()
        _ORACLE[c["name"]] = (loss.item(), logits.detach(), rgb.grad, mot.grad)
    return _ORACLE[c["name"]]


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@PARAM
def test_input_gradients_vs_oracle_autograd(c):
    """The chain is taken (logits come out of the TfamTrainFn node) and returns the oracle's d rgb / d motion."""
    m = _model(c)
    loss, logits, drgb, dmot, _, node = _step(m, c, True)
    assert node == "TfamTrainFnBackward", f"the fused training chain was not taken: {node}"
    ref_loss, ref_logits, ref_rgb, ref_mot = _oracle(c)
    err = (logits.double().cpu() - ref_logits).abs().max().item()
    print(f"{c['name']}: loss {loss:.6f} vs {ref_loss:.6f}, logits max abs err {err:.3e} (|ref|max {ref_logits.abs().max():.2f})")
    for tag, got, ref in (("d rgb", drgb, ref_rgb), ("d motion", dmot, ref_mot)):
        if ref is None:      # the stream the mode does not use
            assert got is None, f"{tag}: a gradient on the unused stream"
            print(f"{c['name']}: {tag} None on both")
            continue
        assert got is not None and got.shape == ref.shape and got.dtype == torch.float32
        print(f"{c['name']}: {tag} rel L2 {_rel_l2(got, ref):.3e} (|ref| {ref.norm():.3e})")
    assert abs(loss - ref_loss) <= 5e-3 * abs(ref_loss)
    assert err <= 8e-3 * max(1.0, ref_logits.abs().max().item())
    for tag, got, ref in (("d rgb", drgb, ref_rgb), ("d motion", dmot, ref_mot)):
        if ref is not None:
            assert _rel_l2(got, ref) <= 4e-2, (tag, _rel_l2(got, ref))
    if c["mode"] in ("concat1", "concat-1"):      # the RGB row the concatenation drops
        assert not drgb[:, -1].any()


@_pick("a_cross_b3", "d_cross_d768", "f_concat1", "g_concat-1_d768")
def test_input_gradients_equal_the_per_op_path_with_dropout(c):
    """dropout 0.1, same seeds: both paths draw the same masks, so the gradients agree up to 16-bit rounding points."""
    m = _model(c, dropout=0.1)
    l0, y0, r0, m0, _, n0 = _step(m, c, True, fused=False, seed=1234)
    l1, y1, r1, m1, _, n1 = _step(m, c, True, fused=True, seed=1234)
    assert n1 == "TfamTrainFnBackward" and n0 != n1
    print(f"{c['name']}: per-op loss {l0:.6f}, fused {l1:.6f}; d rgb rel L2 {_rel_l2(r1, r0):.3e}, d motion rel L2 {_rel_l2(m1, m0):.3e}")
    assert abs(l0 - l1) <= 5e-3 * abs(l0)
    assert _rel_l2(r1, r0) <= 5e-2 and _rel_l2(m1, m0) <= 5e-2


@_pick("a_cross_b3", "e_rgb", "f_concat1", "g_concat-1_d512")
def test_nothing_changes_when_nobody_asks(c):
    """Detached inputs: switch on == switch off, bit for bit.  Grad-requiring inputs with the switch on: the parameter gradients are
    those of the detached run, bit for bit.  Switch off with grad-requiring inputs: the per-op path, as always."""
    m = _model(c, dropout=0.1)
    _, y_off, _, _, g_off, n_off = _step(m, c, False, grad_inputs=False, seed=77)
    _, y_on, r, mo, g_on, n_on = _step(m, c, True, grad_inputs=False, seed=77)
    assert n_off == n_on == "TfamTrainFnBackward" and r is None and mo is None
    assert torch.equal(y_off, y_on) and set(g_off) == set(g_on)
    for k in g_off:
        assert torch.equal(g_off[k], g_on[k]), k
    _, y_in, _, _, g_in, n_in = _step(m, c, True, grad_inputs=True, seed=77)
    assert n_in == "TfamTrainFnBackward" and torch.equal(y_in, y_on) and set(g_in) == set(g_on)
    for k in g_on:
        assert torch.equal(g_in[k], g_on[k]), k
    assert _step(m, c, False, grad_inputs=True, seed=77)[5] != "TfamTrainFnBackward"


def test_pool_len_padding_rows_get_exact_zeros():
    """Cross mode under pool_len: rows >= pool_len of d rgb are exactly 0, the rows before them are the unpadded batch's."""
    c = _case("pad_cross", "cross", 3, 12, 11, 512, 2, 1110, ragged=False)
    m = _model(c)
    rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
    _, y0, r0, m0, _, _ = _step(m, c, True, inputs=(rgb, mot, mr, mf))
    pad = lambda t, T: torch.nn.functional.pad(t, (0, 0) * (t.dim() - 2) + (0, T - t.shape[1]))
    _, y1, r1, m1, _, node = _step(m, c, True, inputs=(pad(rgb, 16), pad(mot, 16), pad(mr, 16), pad(mf, 16)), pool_len=12)
    assert node == "TfamTrainFnBackward"
    print(f"pool_len: logits diff {(y0 - y1).abs().max().item():.3e}, d rgb rel L2 {_rel_l2(r1[:, :12], r0):.3e}, "
          f"d motion rel L2 {_rel_l2(m1[:, :11], m0):.3e}")
    assert not r1[:, 12:].any() and not m1[:, 11:].any()
    assert _rel_l2(r1[:, :12], r0) <= 4e-2 and _rel_l2(m1[:, :11], m0) <= 4e-2


def test_token_lens_gives_gradients_instead_of_raising():
    """concat 1 with token_lens (bucket 16): the concatenation is an autograd node; the rows behind each stream's own length and the
    dropped RGB row get exact zeros, the others the gradients of the exact-shape batch."""
    c = BY_NAME["f_concat1"]
    n_rgb, n_mot = 7, 6
    m = _model(c)
    rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(dict(c, ragged=False)))
    small = dict(c, Tr=n_rgb, Tf=n_mot)
    _, y0, r0, m0, _, _ = _step(m, small, True, inputs=(rgb[:, :n_rgb].contiguous(), mot[:, :n_mot].contiguous(), mr[:, :n_rgb], mf[:, :n_mot]))
    rgb_p, mot_p, mr_p, mf_p = rgb.clone(), mot.clone(), mr.clone(), mf.clone()
    rgb_p[:, n_rgb:], mot_p[:, n_mot:], mr_p[:, n_rgb:], mf_p[:, n_mot:] = 0, 0, False, False
    _, y1, r1, m1, _, node = _step(m, c, True, inputs=(rgb_p, mot_p, mr_p, mf_p), token_lens=(n_rgb, n_mot), concat_len=16)
    assert node == "TfamTrainFnBackward"
    print(f"token_lens: logits diff {(y0 - y1).abs().max().item():.3e}, d rgb rel L2 {_rel_l2(r1[:, :n_rgb - 1], r0[:, :n_rgb - 1]):.3e}, "
          f"d motion rel L2 {_rel_l2(m1[:, :n_mot], m0):.3e}")
    assert not r1[:, n_rgb - 1:].any() and not m1[:, n_mot:].any() and not r0[:, n_rgb - 1].any()
    assert _rel_l2(r1[:, :n_rgb - 1], r0[:, :n_rgb - 1]) <= 4e-2 and _rel_l2(m1[:, :n_mot], m0) <= 4e-2
    m.fused_input_grads = False
    with pytest.raises(ValueError, match="must not require grad"):
        m(rgb_p.requires_grad_(), mot_p, mask_rgb=mr_p, mask_flow=mf_p, token_lens=(n_rgb, n_mot), concat_len=16)


# (T_rgb, T_motion, T_out, n_rgb, n_motion, D): the lengths of tests/test_host_tfam_input_route.py; D = 6 takes the 4-byte path
@pytest.mark.parametrize("T_rgb,T_motion,T_out,n_rgb,n_motion,D", [
    (6, 5, 10, 1, 3, 512), (6, 5, 10, 4, 0, 512), (6, 5, 10, 6, 5, 512), (6, 5, 16, 3, 2, 768), (6, 5, 16, None, None, 512), (6, 5, 4, 5, 5, 512),
    (9, 8, 16, 7, 6, 6), (9, 8, 16, 99, -3, 512)])
def test_concat_backward_kernel_is_the_reference(T_rgb, T_motion, T_out, n_rgb, n_motion, D):
    from vimo_clip_amd import ops
    B = 3
    dx = synth.normal(5, f"dx{T_out}{D}", (B, T_out, D)).cuda()
    lr = None if n_rgb is None else torch.tensor([n_rgb], dtype=torch.int32, device="cuda")
    lm = None if n_motion is None else torch.tensor([n_motion], dtype=torch.int32, device="cuda")
    got_r, got_m = ops.concat_tokens_bwd(dx, T_rgb, T_motion, lr, lm)
    want_r, want_m = concat_bwd_ref(dx.double(), T_rgb, T_motion, n_rgb, n_motion)
    assert torch.equal(got_r.double(), want_r) and torch.equal(got_m.double(), want_m)


@_pick("a_cross_b3", "d_cross_d768", "g_concat-1_d512")
def test_input_gradients_repeat_bit_for_bit(c):
    m = _model(c, dropout=0.1)
    a = _step(m, c, True, seed=5)
    b = _step(m, c, True, seed=5)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


@_pick("a_cross_b3", "f_concat1", "g_concat-1_d768")
def test_per_layer_backward_gives_the_same_input_gradients(c):
    """The layer-by-layer backward (what a gradient-ready callback or the data-parallel reducer switches on:
    vmc_tfam_layer_bwd_inputs / vmc_tfam_layer0_bwd_proj_inputs) returns the one-call backward's input and parameter gradients, bit for bit."""
    m = _model(c, dropout=0.1)
    one = _step(m, c, True, seed=9)
    groups = []
    m.grad_group_callback = groups.append
    per = _step(m, c, True, seed=9)
    del m.grad_group_callback
    assert groups == list(range(c["L"], -1, -1)) and per[5] == "TfamTrainFnBackward"
    assert torch.equal(one[2], per[2]) and torch.equal(one[3], per[3])
    assert set(one[4]) == set(per[4])
    for k in one[4]:
        assert torch.equal(one[4][k], per[4][k]), k


@_pick("a_cross_b3", "g_concat-1_d512")
def test_captured_step_replays_the_eager_input_gradients(c):
    """One step under torch.cuda.graph, captured the way the trainers capture theirs (parameter gradients into a GradArena, the loss
    kernel's own dlogits, a warm-up on a side stream, which allocates): the replay's input gradients are the eager step's.  The
    token leaves are made inside the step and nothing of autograd refers to a parameter's gradient edge, so no stream but the
    capturing one takes part."""
    from vimo_clip_amd.graphs import GraphedCallable
    from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad
    from vimo_clip_amd.optim import GradArena
    m = _model(c)
    m.fused_input_grads = True
    arena = GradArena(m.used_parameters())
    rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).cuda()
    nodes = []

    def step(rgb, mot):
        rgb, mot = rgb.detach().requires_grad_(), mot.detach().requires_grad_()
        logits = m(rgb, mot, mask_rgb=mr, mask_flow=mf)
        nodes.append(type(logits.grad_fn).__name__)
        _, dlogits = loss_and_grad(bce_with_logits_loss, logits, y)
        logits.backward(dlogits)
        return logits.detach(), rgb.grad, mot.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step(rgb, mot)]
        eager_params = arena.flat_grad.clone()
    torch.cuda.current_stream().wait_stream(side)
    graphed = GraphedCallable(step, rgb, mot, warmup=1)
    arena.flat_grad.zero_()
    out = graphed(rgb, mot)
    torch.cuda.synchronize()
    assert set(nodes) == {"TfamTrainFnBackward"}
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    assert torch.equal(eager_params, arena.flat_grad)
    out = graphed(rgb * 0.5, mot)      # and it is a replay of the computation, not of the values
    torch.cuda.synchronize()
    assert not torch.equal(eager[1], out[1])


def test_adapter_in_front_of_tfam_trains_through_the_fused_node():
    """A ResidualMLP on the motion embeddings in cross mode: its parameters get their gradients through the fused node, and they are
    the per-op path's."""
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.models.student_model import ResidualMLP
    c = BY_NAME["a_cross_b3"]
    m = _model(c)
    adapter = ResidualMLP(c["D"]).cuda().train()
    with torch.no_grad():      # fc2 starts at zero, which would leave fc1 without a gradient
        adapter.fc2.weight.copy_(synth.normal(c["seed"], "fc2", tuple(adapter.fc2.weight.shape)).cuda() * 0.05)
    rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).cuda()
    res = []
    for fused in (False, True):
        m.fused_training, m.fused_input_grads = fused, True
        m.zero_grad(set_to_none=True)
        adapter.zero_grad(set_to_none=True)
        logits = m(rgb, adapter(mot), mask_rgb=mr, mask_flow=mf)
        res.append(type(logits.grad_fn).__name__)
        bce_with_logits_loss(logits, y).backward()
        res.append({n: p.grad.detach().clone() for n, p in adapter.named_parameters()})
    assert res[2] == "TfamTrainFnBackward" and res[0] != res[2]
    for n, ref in res[1].items():
        rel = _rel_l2(res[3][n], ref)
        print(f"adapter {n}: rel L2 {rel:.3e} (|ref| {ref.norm().item():.3e})")
        assert ref.norm().item() > 0 and rel <= 5e-2, (n, rel)
