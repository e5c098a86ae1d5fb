"""GPU: the feature-concatenation mode (use_cross_attention=False, concat_dim=-1) training on the fused chains with projection_layer
inside them (AMO_CLIP.fused_feature_training; vmc_tfam_train_fwd_proj / _bwd_proj / vmc_tfam_layer0_bwd_proj, include/vmc.h).

References: torch autograd through the fp32 CPU oracle (oracle.tfam.amo_clip_forward) for every parameter, the reference's own
train-mode step (tests/golden/tfam.npz, case concat_embed), and the per-op path with dropout on (same seeds -> same masks).  All
runs use bf16.  Bounds, restated unchanged from tests/test_gpu_tfam_train.py: loss 5e-3 relative; logits 8e-3 * max(1, |ref|max);
gradients relative L2 <= 4e-2 per parameter, 1e-1 for ``.ffn.0.`` (behind the ReLU); per-op against fused with dropout: loss 5e-3,
logits 1.6e-2 * max(1, |y|max), gradients 5e-2.

T is the motion stream's length (the RGB stream loses its last position).  The geometries are the smallest that reach: two clips per
row block with a ragged last block (M = 60), K = 2 * 768 with head dim 96 and one clip per block, query parts with four key tiles,
one partial row block with a ragged class tile (M = 6, 20 classes), and the full 256 rows.
"""
import pytest
import torch

from oracle import make_golden as mg
from oracle import tfam as otfam
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = next(c for c in mg.TFAM_CASES if c["name"] == "concat_embed")
CASES = [
    GOLDEN,
    dict(name="d768_t20", D=768, H=8, L=2, ff=1024, C=140, B=3, Tr=21, Tf=20, mode="concat-1", pe=False, ragged=True, seed=901),
    dict(name="d512_t40", D=512, H=8, L=1, ff=1024, C=140, B=3, Tr=41, Tf=40, mode="concat-1", pe=False, ragged=True, seed=902),
    dict(name="b1_t6", D=512, H=8, L=1, ff=512, C=20, B=1, Tr=7, Tf=6, mode="concat-1", pe=False, ragged=False, seed=903),
    dict(name="m256", D=768, H=12, L=1, ff=512, C=140, B=16, Tr=17, Tf=16, mode="concat-1", pe=False, ragged=True, seed=904),
]
BY_NAME = {c["name"]: c for c in CASES}
PARAM = pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])


def _model(c, dropout=0.0, mlp_dropout=0.0, switch=True):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    m = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=c["C"], use_pe=c["pe"],
                 dropout=dropout, mlp_dropout=mlp_dropout, device="cuda", compute_dtype=torch.bfloat16, **mg.tfam_mode_kwargs(c["mode"])).cuda()
    m.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]), strict=True)
    m.fused_feature_training = switch
    return m.train()


def _count_fused(monkeypatch):
    from vimo_clip_amd import tfam_train
    calls = []
    orig = tfam_train.forward_train

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(tfam_train, "forward_train", spy)
    return calls


def _grads(m):
    used = {id(q) for q in m.used_parameters()}
    grads = {}
    for n, p in m.named_parameters():
        g = getattr(p, "_vmc_grad", None) if id(p) in used else None          # arena slot (written in place), else autograd's .grad
        g = p.grad if g is None else g
        if g is not None:
            grads[n] = g.detach().float().cpu().clone()
    return grads


def _step(m, c, switch, inputs=None, **fwd_kw):
    """One step on the case's batch (or on ``inputs``): fused_training stays on; ``switch`` is fused_feature_training."""
    from vimo_clip_amd.losses import bce_with_logits_loss
    m.fused_training, m.fused_feature_training = True, switch
    if not any(getattr(p, "_vmc_grad", None) is not None for p in m.parameters()):
        m.zero_grad(set_to_none=True)
    rgb, mot, mr, mf = inputs if inputs is not None else (t.cuda() for t in mg.tfam_inputs(c))
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).cuda()
    logits = m(rgb, mot, mask_rgb=mr, mask_flow=mf, **fwd_kw)
    loss = bce_with_logits_loss(logits, y)
    loss.backward()
    return loss.item(), logits.detach().float().cpu(), _grads(m)


_ORACLE = {}


def _oracle_grads(c):
    """(loss, logits, gradients) of torch autograd through the fp32 oracle; computed once per case and left unchanged."""
    if c["name"] not in _ORACLE:
        sd = {k: v.clone().requires_grad_(True) for k, v in synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]).items()}
        rgb, mot, mr, mf = mg.tfam_inputs(c)
        y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"])
        logits = otfam.amo_clip_forward(sd, rgb, mot, mr, mf, nhead=c["H"], use_pe=c["pe"], **mg.tfam_mode_kwargs(c["mode"]))
        loss = otfam.bce_with_logits_mean(logits, y)
        loss.backward()
        _ORACLE[c["name"]] = (loss.item(), logits.detach(), {k: v.grad for k, v in sd.items() if v.grad is not None})
    return _ORACLE[c["name"]]


def _rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def _check_vs_oracle(tag, got, ref, other=None):
    """The bounds of the module docstring; ``other``: the per-op path's result, printed beside every fused figure."""
    (loss, logits, grads), (ref_loss, ref_logits, ref_g) = got, ref
    err = (logits - ref_logits).abs().max().item()
    line = f"{tag}: loss {loss:.6f} vs {ref_loss:.6f}, logits max abs err {err:.3e} (|ref|max {ref_logits.abs().max():.2f})"
    if other is not None:
        line += f"; per-op loss {other[0]:.6f}, logits err {(other[1] - ref_logits).abs().max().item():.3e}"
    print(line)
    worst = ("", 0.0)
    for k, r in ref_g.items():
        if k in grads:
            rel = _rel_l2(grads[k], r)
            worst = max(worst, (k, rel), key=lambda t: t[1])
            po = f" (per-op {_rel_l2(other[2][k], r):.3e})" if other is not None and k in other[2] else ""
            print(f"    grad {k}: rel L2 {rel:.3e}{po}")
    print(f"{tag}: worst gradient rel L2 {worst[1]:.3e} ({worst[0]})")
    assert abs(loss - ref_loss) <= 5e-3 * abs(ref_loss)
    assert err <= 8e-3 * max(1.0, ref_logits.abs().max().item())
    assert set(grads) == set(ref_g), set(grads) ^ set(ref_g)
    assert "projection_layer.weight" in grads and "projection_layer.bias" in grads
    for k, r in ref_g.items():
        rel = _rel_l2(grads[k], r)
        assert rel <= (1e-1 if ".ffn.0." in k else 4e-2), (k, rel)


@PARAM
def test_the_chain_is_taken_only_with_the_switch(c, monkeypatch):
    """fused_feature_training on: forward_train runs the chain.  Off (the default): the feature mode never reaches it."""
    import numpy as np
    calls = _count_fused(monkeypatch)
    m = _model(c)
    loss, _, grads = _step(m, c, True)
    assert calls == [True], "the fused training chain was not taken"
    assert np.isfinite(loss) and "projection_layer.weight" in grads
    del calls[:]
    loss, _, grads = _step(m, c, False)
    assert calls == [] and np.isfinite(loss) and "projection_layer.weight" in grads
    m.fused_training = False                     # and the switch alone does nothing
    m.fused_feature_training = True
    rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
    m(rgb, mot, mask_rgb=mr, mask_flow=mf)
    assert calls == []


@PARAM
def test_every_gradient_vs_oracle_autograd(c):
    """Loss, logits and EVERY parameter gradient (the projection's included) of one step (dropout 0) against torch autograd through
    the fp32 CPU oracle; the per-op path's figures for the same case are printed beside the fused ones."""
    m = _model(c)
    perop = _step(m, c, False)
    fused = _step(m, c, True)
    _check_vs_oracle(c["name"], fused, _oracle_grads(c), other=perop)


def test_golden_concat_embed(golden, monkeypatch):
    """Loss and the five recorded gradients of the reference's own train-mode step (dropout 0)."""
    calls = _count_fused(monkeypatch)
    c, name = GOLDEN, "concat_embed"
    m = _model(c)
    loss, _, grads = _step(m, c, True)
    assert calls == [True]
    g = golden["tfam"]
    ref_loss = float(g[f"{name}/train_loss"])
    assert abs(loss - ref_loss) <= 5e-3 * abs(ref_loss), (loss, ref_loss)
    for k in ("classifier.4.weight", "classifier.1.bias", "layers.0.ffn.0.bias", "layers.0.self_attn.in_proj_bias", "layers.0.norm_self.weight"):
        ref = torch.from_numpy(g[f"{name}/grad/{k}"])
        got = grads[k]
        rel = (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
        rel_l2 = _rel_l2(got, ref)
        print(f"{name} grad {k}: rel-to-max {rel:.3e}, rel L2 {rel_l2:.3e}")
        assert rel_l2 <= 4e-2, (k, rel_l2)
        assert rel <= (2e-1 if "ffn.0" in k else 6e-2), (k, rel)
    used = {n for n, p in m.named_parameters() if id(p) in {id(q) for q in m.used_parameters()}}
    assert set(grads) == used


@pytest.mark.parametrize("name", ["concat_embed", "d768_t20"])
def test_fused_equals_per_op_path_with_dropout(name):
    """dropout 0.1 / mlp_dropout 0.3 from the same seed: the projection draws none, so the chain draws the rgb-only order and both
    paths apply identical masks."""
    c = BY_NAME[name]
    m = _model(c, dropout=0.1, mlp_dropout=0.3)
    out = []
    for switch in (False, True):
        m.set_dropout_seed(1234)
        out.append(_step(m, c, switch))
    (l0, y0, g0), (l1, y1, g1) = out
    err = (y0 - y1).abs().max().item()
    print(f"{name}: per-op loss {l0:.6f}, fused {l1:.6f}, logits diff {err:.3e}")
    assert abs(l0 - l1) <= 5e-3 * abs(l0)
    assert err <= 1.6e-2 * max(1.0, y0.abs().max().item())
    assert set(g0) == set(g1) and "projection_layer.weight" in g1
    for k in g0:
        rel = _rel_l2(g1[k], g0[k])
        print(f"    grad {k}: rel L2 {rel:.3e}")
    for k in g0:
        assert _rel_l2(g1[k], g0[k]) <= 5e-2, k
    m.set_dropout_seed(99)                       # dropout is really on: another seed changes the result
    l2, _, _ = _step(m, c, True)
    assert l2 != l1


def test_deterministic_and_writes_into_the_arena():
    """Two fused steps from the same state are bit-identical, and with a GradArena every used element is written in place, the
    projection's slots included."""
    from vimo_clip_amd.optim import GradArena
    c = BY_NAME["d768_t20"]
    m = _model(c, dropout=0.1, mlp_dropout=0.1)
    m.set_dropout_seed(5)
    l0, y0, g0 = _step(m, c, True)
    arena = GradArena(m.used_parameters())
    arena.flat_grad.fill_(float("nan"))
    m.set_dropout_seed(5)
    l1, y1, g1 = _step(m, c, True)
    assert l0 == l1 and torch.equal(y0, y1)
    assert set(g0) == set(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    pl = m.projection_layer
    assert torch.equal(pl.weight._vmc_grad.float().cpu(), g1["projection_layer.weight"]) and bool(g1["projection_layer.weight"].abs().sum() > 0)
    used = torch.zeros(arena.numel, dtype=torch.bool)
    for p, o in zip(arena.params, arena.offsets):
        used[o:o + p.numel()] = True
    assert any(p is pl.weight for p in arena.params) and any(p is pl.bias for p in arena.params)
    assert torch.isfinite(arena.flat_grad.cpu()[used]).all()


def test_padded_batch_matches_the_unpadded_oracle(monkeypatch):
    """21 / 20 tokens padded to 32 / 32 with token_lens: the oracle's results on the unpadded batch, dx0 exactly zero on the rows
    behind n_motion, and the same bits whether the lengths are ints or device tensors."""
    from vimo_clip_amd import graphs
    from vimo_clip_amd import tfam_train as tt
    from vimo_clip_amd._lib import lib
    c = BY_NAME["d768_t20"]
    calls = _count_fused(monkeypatch)
    seen = {}
    orig_bwd = tt.TfamTrainFn.backward

    def spy_bwd(ctx, dl):
        seen["ws"], seen["dims"] = ctx.ws, ctx.dims      # the workspace outlives the backward through this reference
        return orig_bwd(ctx, dl)
    monkeypatch.setattr(tt.TfamTrainFn, "backward", staticmethod(spy_bwd))

    def padded():
        rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
        prgb, pmot, pmr, pmf, nr, nm, T_out = graphs.pad_concat_to_bucket(rgb, mot, mr, mf, 16, "feature")
        assert (nr, nm) == (21, 20) and prgb.shape[1] == pmot.shape[1] == 32
        return (prgb, pmot, pmr, pmf), (nr, nm), T_out

    m = _model(c)
    inputs, lens, T_out = padded()
    dev = tuple(torch.tensor([n], dtype=torch.int32, device="cuda") for n in lens)
    got_dev = _step(m, c, True, inputs, token_lens=dev, concat_len=T_out)
    B, T, D = c["B"], 32, c["D"]
    assert seen["dims"][:2] == (B, T)
    off = lib.vmc_tfam_train_proj_dx0_offset(B, T, D, c["H"], c["ff"], c["L"], c["C"])
    assert off > 0 and off + B * T * D * 4 <= seen["ws"].numel()
    dx0 = seen["ws"][off:off + B * T * D * 4].view(torch.float32).view(B, T, D).cpu()
    assert bool((dx0[:, lens[1]:] == 0).all()), "dx0 is not zero behind n_motion"
    assert bool((dx0[:, :lens[1]] != 0).any(dim=-1).all()), "a pooled row without a gradient"
    inputs, lens, T_out = padded()
    got_int = _step(m, c, True, inputs, token_lens=lens, concat_len=T_out)
    assert calls == [True, True]
    assert torch.equal(got_int[1], got_dev[1])
    for k in got_dev[2]:
        assert torch.equal(got_int[2][k], got_dev[2][k]), k
    inputs, lens, T_out = padded()
    perop = _step(m, c, False, inputs, token_lens=lens, concat_len=T_out)
    _check_vs_oracle("d768_t20 padded to 32", got_dev, _oracle_grads(c), other=perop)


def test_per_layer_backward_reports_the_projection_with_layer_0():
    """grad_group_callback: the per-layer backward gives the bits of the one-call backward, reports projection_layer.weight / .bias
    behind layer 0's own parameters and before done(0), and closes L + 1 groups."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.optim import GradArena
    c = BY_NAME["concat_embed"]
    L = c["L"]
    m = _model(c, dropout=0.1, mlp_dropout=0.1)
    arena = GradArena(m.used_parameters())
    names = {id(p): n for n, p in m.named_parameters()}
    m.set_dropout_seed(7)
    l0, y0, g0 = _step(m, c, True)
    events = []
    hook = lambda p: events.append(("grad", names[id(p)]))
    arena.flat_grad.fill_(float("nan"))
    m.grad_group_callback = lambda i: events.append(("done", i))
    ag.grad_ready_hooks.append(hook)
    try:
        m.set_dropout_seed(7)
        l1, y1, g1 = _step(m, c, True)
    finally:
        ag.grad_ready_hooks.remove(hook)
        m.grad_group_callback = None
    assert l0 == l1 and torch.equal(y0, y1)
    assert set(g0) == set(g1) == {names[id(p)] for p in m.used_parameters()}
    for k in g0:                                 # the arena slots (the gaps between them keep their NaN fill)
        assert torch.equal(g0[k], g1[k]) and bool(torch.isfinite(g1[k]).all()), f"{k}: per-layer backward differs from the one-call backward"
    done = [e[1] for e in events if e[0] == "done"]
    assert done == list(range(L, -1, -1)) and len(done) == L + 1
    at = {n: events.index(("grad", n)) for n in ("projection_layer.weight", "projection_layer.bias", "layers.0.self_attn.in_proj_bias")}
    d0, d1 = events.index(("done", 0)), events.index(("done", 1))
    assert d1 < at["layers.0.self_attn.in_proj_bias"] < at["projection_layer.weight"] < at["projection_layer.bias"] < d0
    assert sum(1 for e in events if e == ("grad", "projection_layer.weight")) == 1
    reported = {e[1] for e in events if e[0] == "grad"}
    assert reported == {names[id(p)] for p in m.used_parameters()}


def test_one_captured_step_replays_bit_for_bit():
    """GraphedTrainStep(bucket=16, concat="feature") with the switch on, fed 21, 19, 21 RGB tokens (one padded shape, 32 / 32) with
    dropout 0.1: one graph, whose replays give the losses, logits and parameters of eager steps on the same padded tensors."""
    import numpy as np
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd import graphs, tfam_train as tt
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    base = dict(name="graph", D=512, H=8, L=2, ff=1024, C=140, B=4, Tr=21, Tf=20, mode="concat-1", pe=False, ragged=True, seed=910)
    runs = []
    for captured in (False, True):
        ag.weights.clear()
        m = _model(base, dropout=0.1, mlp_dropout=0.1)
        opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-3, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=11)
        m.use_device_seeds(opt)
        taken = []
        orig = tt.forward_train

        def step(a, b, cm, d, yy, nr, nm, T_out):
            opt.tick()
            out = m(a, b, mask_rgb=cm, mask_flow=d, token_lens=(nr, nm), concat_len=T_out)
            loss = bce_with_logits_loss(out, yy)
            loss.backward()
            opt.step()
            return loss.detach(), out.detach()

        def spy(*a, **k):
            out = orig(*a, **k)
            taken.append(out is not None and k.get("proj", False))
            return out
        tt.forward_train = spy
        try:
            run = graphs.GraphedTrainStep(step, opt, bucket=16, pooled=None, concat="feature", max_graphs=16 if captured else 0)
            outs = []
            for Tr in (21, 19, 21):
                c = dict(base, Tr=Tr, Tf=Tr - 1)
                rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
                y = synth.multi_hot_labels(c["seed"] + Tr, "labels", c["B"], c["C"]).cuda()
                loss, logits = run(rgb, mot, mr, mf, y)
                outs.append((float(loss.clone()), logits.clone()))
        finally:
            tt.forward_train = orig
        assert taken and all(taken), "the chain with the projection was not taken"
        assert run.n_graphs == (1 if captured else 0)
        runs.append((outs, {k: p.detach().clone() for k, p in m.named_parameters()}, int(opt.dev_state[0].item())))
    (oe, pe, de), (oc, pc, dc) = runs
    print(f"one captured feature step: eager {[o[0] for o in oe]} captured {[o[0] for o in oc]}")
    assert de == dc == 3
    assert all(np.isfinite(o[0]) for o in oe) and oe[0][0] != oe[1][0]
    for (le, ye), (lc, yc) in zip(oe, oc):
        assert le == lc and torch.equal(ye, yc)
    for k in pe:
        assert torch.equal(pe[k], pc[k]), k
