"""GPU: length buckets for the two concatenation modes.  Both streams of a batch are zero-padded to their own bucket and the
concatenation is rebuilt with the real rows as a prefix -- by vmc_concat_tokens_len (include/vmc.h K19) for the token
concatenation, whose split position is a device value, and by the motion mask + pool length for the feature concatenation -- so
one captured graph serves a whole bucket (AMO_CLIP.forward(token_lens=, concat_len=), graphs.pad_concat_to_bucket,
GraphedTrainStep(concat=), GraphedEvalForward(concat_bucket=), Config.graph_bucket_concat).

References: tests/concat_ref.py (the kernel's contract in plain torch; bit for bit) and oracle.tfam.amo_clip_forward (with torch
autograd through it) on the CPU at the batch's OWN lengths, no bucket.

Bounds, restated unchanged from tests/test_gpu_tfam_ragged.py:
  logits  |d| <= TOL[dtype] * max(1, |ref|max), TOL = {float16: 1e-3, bfloat16: 8e-3}
  loss 5e-3 relative; gradients relative L2 <= 4e-2 per parameter, 1e-1 for ``.ffn.0.``
A padded and an unpadded batch may take different kernels, so padded-vs-exact agreement is within these tolerances; bit-identity
is asked between a graph replay and an eager run on the same padded tensors, between ints and device tensors as lengths, and
between the store and the loader path at the same buckets.
"""
import os

import numpy as np
import pytest
import torch

from concat_ref import clamp_lens, concat_ref
from oracle import make_golden as mg
from oracle import tfam as otfam
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
MODES = pytest.mark.parametrize("mode", ["concat1", "concat-1"])
CMODE = {"concat1": "time", "concat-1": "feature"}
D, H, L, FF, C = 512, 8, 2, 1024, 140


# ---- the kernel through the C ABI ----------------------------------------------------------------------------------------------------

GUARD = 64      # elements in front of and behind every output, which the kernel must leave alone


def _guarded(numel, dtype, fill, skew):
    """A [numel] view, 16-byte aligned plus ``skew`` elements, inside a buffer pre-filled with ``fill`` -> (buffer, view)."""
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD + skew:GUARD + skew + numel]


LENS = [(None, None), (9, 8), (5, 3), (1, 1), (2, 8), (0, 0), (100, 100)]


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("T_out", [12, 16, 24])
@pytest.mark.parametrize("Dk,skew", [(512, 0), (6, 0), (512, 1)], ids=["d512", "d6", "d512_skewed"])
def test_concat_tokens_len_is_the_contract_bit_for_bit(Dk, skew, T_out, masks):
    """B = 3, 9 RGB and 8 motion tokens.  d512: the 16-byte path; d6 (D % 4 != 0) and d512_skewed (every token pointer 4 bytes past
    16-byte alignment): the 4-byte path.  Outputs pre-filled with NaN / 0xFF stand for torch.empty; guard elements around them must
    keep their fill.  (100, 100) is clamped to the tensors and, at T_out = 12, cut at T_out; (0, 0) is clamped up to (1, 1)."""
    from vimo_clip_amd._lib import lib, stream
    B, Tr, Tm = 3, 9, 8
    _, rgb = _guarded(B * Tr * Dk, torch.float32, 0.0, skew)
    _, mot = _guarded(B * Tm * Dk, torch.float32, 0.0, skew)
    rgb, mot = rgb.view(B, Tr, Dk), mot.view(B, Tm, Dk)
    rgb.copy_(synth.normal(3, "ct_rgb", (B, Tr, Dk)))
    mot.copy_(synth.normal(3, "ct_mot", (B, Tm, Dk)))
    assert rgb.data_ptr() % 16 == mot.data_ptr() % 16 == 4 * skew
    mr = (synth.randint(3, "ct_mr", (B, Tr), 0, 4) > 0).to(torch.uint8).cuda() if masks else None
    mf = (synth.randint(3, "ct_mf", (B, Tm), 0, 4) > 0).to(torch.uint8).cuda() if masks else None
    if masks:
        assert 0 < int(mr.sum()) < mr.numel() and 0 < int(mf.sum()) < mf.numel()
    ptr = lambda t: None if t is None else t.data_ptr()
    for lr, lm in LENS:
        xb, x = _guarded(B * T_out * Dk, torch.float32, float("nan"), skew)
        mb, m = _guarded(B * T_out, torch.uint8, 0xFF, 0)
        nb, n = _guarded(1, torch.int32, -77, 0)
        lens = [None if v is None else torch.tensor([v], dtype=torch.int32, device="cuda") for v in (lr, lm)]
        rc = lib.vmc_concat_tokens_len(ptr(rgb), ptr(mot), ptr(mr), ptr(mf), ptr(x), ptr(m), ptr(n), B, Tr, Tm, T_out, Dk,
                                       ptr(lens[0]), ptr(lens[1]), stream())
        assert rc == 0
        torch.cuda.synchronize()
        rx, rm, rn = concat_ref(rgb, mot, mr, mf, T_out, lr, lm)
        assert rn == clamp_lens(lr, lm, Tr, Tm, T_out)[2] and 1 <= rn <= T_out
        assert int(n) == rn, (lr, lm)
        assert torch.equal(x.view(B, T_out, Dk).view(torch.int32), rx.view(torch.int32)), (lr, lm)      # as bits: -0.0, no NaN left
        assert torch.equal(m.view(B, T_out), rm), (lr, lm)
        for buf, fill in ((xb, None), (mb, 0xFF), (nb, -77)):
            for g in (buf[:GUARD], buf[-GUARD + (skew if fill is None else 0):]):
                assert bool(torch.isnan(g).all()) if fill is None else bool((g == fill).all()), "the kernel wrote outside its output"
        if (lr, lm) == (None, None) and T_out == 16:                # the reference's own concatenation
            assert torch.equal(x.view(B, T_out, Dk), torch.cat([rgb[:, :-1], mot], 1))
            want = torch.cat([mr[:, :-1], mf], 1) if masks else torch.ones(B, 16, dtype=torch.uint8, device="cuda")
            assert torch.equal(m.view(B, T_out), want)
    if T_out == 12:
        assert clamp_lens(100, 100, Tr, Tm, T_out) == (8, 4, 12)    # cut at T_out


def test_concat_tokens_len_argument_errors_and_the_wrapper():
    from vimo_clip_amd import ops
    from vimo_clip_amd._lib import lib, stream
    B, Tr, Tm, Dk, T_out = 2, 5, 4, 8, 8
    rgb, mot = synth.normal(4, "w_rgb", (B, Tr, Dk)).cuda(), synth.normal(4, "w_mot", (B, Tm, Dk)).cuda()
    x = torch.empty(B, T_out, Dk, device="cuda")
    m = torch.empty(B, T_out, dtype=torch.uint8, device="cuda")
    n = torch.empty(1, dtype=torch.int32, device="cuda")

    def call(rgb_=rgb.data_ptr(), mot_=mot.data_ptr(), x_=x.data_ptr(), m_=m.data_ptr(), n_=n.data_ptr(), dims=(B, Tr, Tm, T_out, Dk)):
        return lib.vmc_concat_tokens_len(rgb_, mot_, None, None, x_, m_, n_, *dims, None, None, stream())
    E_ARG, E_SHAPE = -1, -3
    assert call() == 0
    assert call(rgb_=None) == call(mot_=None) == call(x_=None) == call(m_=None) == call(n_=None) == E_ARG
    for k in range(5):
        for bad in (0, -3):
            dims = [B, Tr, Tm, T_out, Dk]
            dims[k] = bad
            assert call(dims=tuple(dims)) == E_SHAPE, (k, bad)
    # the wrapper: fresh outputs, bool masks taken as bytes, lengths as device tensors, caller-owned outputs
    mr, mf = torch.ones(B, Tr, dtype=torch.bool, device="cuda"), torch.ones(B, Tm, dtype=torch.bool, device="cuda")
    mr[1, 3:] = False
    lens = [torch.tensor([v], dtype=torch.int32, device="cuda") for v in (4, 2)]
    gx, gm, gn = ops.concat_tokens(rgb, mot, mr, mf, T_out, *lens)
    rx, rm, rn = concat_ref(rgb, mot, mr, mf, T_out, 4, 2)
    assert gm.dtype == torch.uint8 and gn.dtype == torch.int32 and int(gn) == rn == 5
    assert torch.equal(gx, rx) and torch.equal(gm, rm)
    out = ops.concat_tokens(rgb, mot, None, None, T_out, out=(x, m, n))
    assert out[0] is x and out[1] is m and out[2] is n and int(n) == 8 and torch.equal(x, torch.cat([rgb[:, :-1], mot], 1)) and bool(m.all())
    with pytest.raises(TypeError):
        ops.concat_tokens(rgb, mot, None, None, T_out, 4, 2)                   # ints: ops.pool_len_tensor makes the tensors
    with pytest.raises(ValueError):
        ops.concat_tokens(rgb, mot[:, :, :4], None, None, T_out)
    with pytest.raises(ValueError):
        ops.concat_tokens(rgb, mot, None, None, T_out, out=(x[:, :4], m, n))


# ---- the model: padded + token_lens vs the oracle at the batch's own lengths ---------------------------------------------------------

def _case(mode, Tr, pe=False, B=4, seed=800):
    return dict(name=f"{mode}_t{Tr}", D=D, H=H, L=L, ff=FF, C=C, B=B, Tr=Tr, Tf=Tr - 1, mode=mode, pe=pe, ragged=True,
                seed=seed + Tr + 3 * ["concat1", "concat-1"].index(mode))


def _model(c, dtype, train=False, p_drop=0.0):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, use_pe=c["pe"], dropout=p_drop, mlp_dropout=p_drop,
                 device="cuda", compute_dtype=dtype, **mg.tfam_mode_kwargs(c["mode"])).cuda()
    m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, c["seed"]), strict=True)
    return m.train() if train else m.eval()


def _padded(c, bucket=16):
    """(unpadded CPU inputs, padded device inputs, (n_rgb, n_mot), T_out).  Fresh tensors on every call: with use_pe the model adds
    the positional encoding in place."""
    from vimo_clip_amd import graphs
    rgb, mot, mr, mf = mg.tfam_inputs(c)
    assert c["Tr"] % bucket != 0 and c["Tf"] % bucket != 0, "bucket padding present in both streams"
    assert int(mr.sum(1).max()) == c["Tr"] and int(mr.sum(1).min()) < c["Tr"], "one clip shorter than T_max (loader padding present)"
    prgb, pmot, pmr, pmf, nr, nm, T_out = graphs.pad_concat_to_bucket(rgb.cuda(), mot.cuda(), mr.cuda(), mf.cuda(), bucket, CMODE[c["mode"]])
    assert (nr, nm) == (c["Tr"], c["Tf"]) and prgb.shape[1] % bucket == 0 and pmot.shape[1] % bucket == 0 and T_out % bucket == 0
    return (rgb, mot, mr, mf), (prgb, pmot, pmr, pmf), (nr, nm), T_out


def _oracle(c, inputs, sd=None):
    sd = sd or synth.tfam_state_dict(D, H, L, FF, C, c["seed"])
    return otfam.amo_clip_forward(sd, *inputs, nhead=H, use_pe=c["pe"], **mg.tfam_mode_kwargs(c["mode"]))


def _dev_lens(lens):
    return tuple(torch.tensor([n], dtype=torch.int32, device="cuda") for n in lens)


def _eval_check(c, dtype, fused, monkeypatch, switch=None):
    """``fused``: whether the fused eval chain must have run; ``switch``: fused_inference, when it is not the same thing."""
    from vimo_clip_amd import tfam_fused as tf
    m = _model(c, dtype)
    m.fused_inference = fused if switch is None else switch
    calls = []
    orig = tf.TfamPack.forward
    monkeypatch.setattr(tf.TfamPack, "forward", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    exact, _, lens, T_out = _padded(c)
    ref = _oracle(c, exact)
    bound = TOL[dtype] * max(1.0, ref.abs().max().item())
    with torch.no_grad():
        prgb, pmot, pmr, pmf = _padded(c)[1]
        y_int = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, token_lens=lens, concat_len=T_out).float().cpu()
        prgb, pmot, pmr, pmf = _padded(c)[1]
        y_dev = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, token_lens=_dev_lens(lens), concat_len=T_out).float().cpu()
        prgb, pmot, pmr, pmf = _padded(c)[1]
        full = (prgb.shape[1], pmot.shape[1])          # the control: the padded lengths as if they were the batch's own
        y_all = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, token_lens=full, concat_len=T_out).float().cpu()
    assert bool(calls) == fused, "fused chain taken" if calls else "the fused chain was not taken"
    err, err_all = (y_int - ref).abs().max().item(), (y_all - ref).abs().max().item()
    print(f"concat eval {c['name']} pe={c['pe']} {dtype} fused={fused}: ({c['Tr']}, {c['Tf']}) -> {tuple(prgb.shape[1:2])}{tuple(pmot.shape[1:2])} "
          f"T_out {T_out}: err {err:.3e} (bound {bound:.3e}, |ref|max {ref.abs().max():.2f}); with the padded lengths as token_lens {err_all:.3e}")
    assert torch.equal(y_int, y_dev)                       # an int is the same length as a device tensor
    assert err <= bound
    assert err_all > bound, "the padded lengths as token_lens must change the logits beyond the tolerance"


@DTYPES
@MODES
@pytest.mark.parametrize("pe", [False, True], ids=["nope", "pe"])
@pytest.mark.parametrize("fused", [False, True], ids=["perop", "fused"])
def test_eval_logits_short_clips(dtype, mode, pe, fused, monkeypatch):
    """21 / 20 tokens -> 32 / 32; concatenated 40 -> 48 (192 token rows: the fused eval chain) or 32 features rows per clip."""
    _eval_check(_case(mode, 21, pe=pe), dtype, fused, monkeypatch)


@DTYPES
def test_eval_logits_past_64_tokens(dtype, monkeypatch):
    """40 / 39 tokens -> 48 / 48; concatenated 78 -> 80: past the fused chains' 64 tokens, the per-op path with fused_inference on."""
    _eval_check(_case("concat1", 40), dtype, False, monkeypatch, switch=True)


def _oracle_grads(c, exact, y):
    sd = {k: v.clone().requires_grad_(True) for k, v in synth.tfam_state_dict(D, H, L, FF, C, c["seed"]).items()}
    logits = _oracle(c, exact, sd)
    loss = otfam.bce_with_logits_mean(logits, y)
    loss.backward()
    return loss.item(), logits.detach(), {k: v.grad for k, v in sd.items() if v.grad is not None}


def _train_check(c, dtype, fused, expect_chain, monkeypatch):
    from vimo_clip_amd import tfam_train as tt
    from vimo_clip_amd.losses import bce_with_logits_loss
    m = _model(c, dtype, train=True)
    m.fused_training = fused
    taken = []
    orig_ft = tt.forward_train

    def spy_ft(*a, **k):
        out = orig_ft(*a, **k)
        taken.append(out is not None)
        return out
    monkeypatch.setattr(tt, "forward_train", spy_ft)
    exact, (prgb, pmot, pmr, pmf), lens, T_out = _padded(c)
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"])
    logits = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, token_lens=lens, concat_len=T_out)
    assert any(taken) == expect_chain, "fused training chain taken / not taken as expected"
    loss = bce_with_logits_loss(logits, y.cuda())
    loss.backward()
    used = {id(q) for q in m.used_parameters()}
    grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if id(p) in used and p.grad is not None}
    ref_loss, ref_logits, ref = _oracle_grads(c, exact, y)
    err = (logits.detach().float().cpu() - ref_logits).abs().max().item()
    print(f"concat train {c['name']} {dtype} fused={fused}: loss {loss.item():.6f} vs {ref_loss:.6f}, logits err {err:.3e}")
    assert abs(loss.item() - ref_loss) <= 5e-3 * abs(ref_loss)
    assert err <= TOL[dtype] * max(1.0, ref_logits.abs().max().item())
    assert set(grads) == set(ref), set(grads) ^ set(ref)
    assert ("projection_layer.weight" in ref) == (c["mode"] == "concat-1")
    worst = ("", 0.0)
    for k, r in ref.items():
        rel_l2 = ((grads[k] - r).norm() / (r.norm() + 1e-20)).item()
        worst = max(worst, (k, rel_l2), key=lambda t: t[1])
        print(f"    grad {k}: rel L2 {rel_l2:.3e}")
    print(f"concat train {c['name']} {dtype} fused={fused}: worst gradient rel L2 {worst[1]:.3e} ({worst[0]})")
    for k, r in ref.items():
        rel_l2 = ((grads[k] - r).norm() / (r.norm() + 1e-20)).item()
        assert rel_l2 <= (1e-1 if ".ffn.0." in k else 4e-2), (k, rel_l2)


@DTYPES
@MODES
@pytest.mark.parametrize("fused", [False, True], ids=["perop", "fused"])
def test_training_step_matches_oracle_autograd(dtype, mode, fused, monkeypatch):
    """One train-mode step (dropout 0) on the padded batch with token_lens: loss, logits and EVERY parameter gradient (the
    projection layer's in the feature mode) against torch autograd through the fp32 oracle on the unpadded batch.  The feature
    mode trains on the per-op path whatever the switch says."""
    _train_check(_case(mode, 21), dtype, fused, fused and mode == "concat1", monkeypatch)


@DTYPES
def test_training_step_past_64_tokens(dtype, monkeypatch):
    _train_check(_case("concat1", 40), dtype, True, False, monkeypatch)


# ---- one graph, two lengths -----------------------------------------------------------------------------------------------------------

@DTYPES
@MODES
def test_one_eval_graph_serves_both_lengths(dtype, mode):
    """GraphedEvalForward(bucket=16, concat_bucket=True) fed 21 then 19 RGB tokens: ONE graph, every replay bit-identical to an eager
    forward on the same padded tensors and within the tolerance of the oracle at the exact lengths."""
    from vimo_clip_amd import graphs
    from vimo_clip_amd.TFAM.train_and_eval import Config, GraphedEvalForward
    base = dict(_case(mode, 21), seed=860)
    m = _model(base, dtype)
    gf = GraphedEvalForward(m, Config(batch_size=base["B"], d_model=D, device="cuda"), bucket=16, streams=1, concat_bucket=True)
    assert gf.bucket == 16 and gf.concat == CMODE[mode]
    for Tr in (21, 19):
        c = dict(base, Tr=Tr, Tf=Tr - 1)
        rgb, mot, mr, mf = mg.tfam_inputs(c)
        assert int(mr.sum(1).min()) < Tr
        batch = {"embeddings": rgb.cuda(), "flow_embeddings": mot.cuda(), "mask_rgb": mr.cuda(), "mask_flow": mf.cuda()}
        with torch.no_grad():
            got = gf(batch)
            prgb, pmot, pmr, pmf, nr, nm, T_out = graphs.pad_concat_to_bucket(rgb.cuda(), mot.cuda(), mr.cuda(), mf.cuda(), 16, CMODE[mode])
            eager = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, token_lens=_dev_lens((nr, nm)), concat_len=T_out)
        assert torch.equal(got, eager), Tr
        ref = _oracle(c, (rgb, mot, mr, mf))
        err = (got.float().cpu() - ref).abs().max().item()
        print(f"one eval graph {mode} {dtype}: T_rgb {Tr} -> T_out {T_out}: err vs oracle {err:.3e}")
        assert err <= TOL[dtype] * max(1.0, ref.abs().max().item())
    assert len(gf._graphs) == 1, list(gf._graphs)
    assert list(gf._graphs) == [(0, base["B"], 32, 32, D, 48 if mode == "concat1" else 32)]


@DTYPES
@MODES
def test_one_train_graph_serves_both_lengths(dtype, mode):
    """GraphedTrainStep(bucket=16, concat=...) fed 21, 19, 21 RGB tokens with dropout 0.1: ONE graph, and the same losses and
    parameters, bit for bit, as eager device-state steps on the same padded tensors (max_graphs = 0)."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd import graphs
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    base = dict(_case(mode, 21, B=8), seed=870)
    runs = []
    for captured in (False, True):
        ag.weights.clear()
        m = _model(base, dtype, train=True, p_drop=0.1)
        opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-3, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=11)
        m.use_device_seeds(opt)

        def step(a, b, cm, d, yy, nr, nm, T_out):
            opt.tick()
            out = m(a, b, mask_rgb=cm, mask_flow=d, token_lens=(nr, nm), concat_len=T_out)
            loss = bce_with_logits_loss(out, yy)
            loss.backward()
            opt.step()
            return loss.detach(), out.detach()

        run = graphs.GraphedTrainStep(step, opt, bucket=16, pooled=None, concat=CMODE[mode], max_graphs=16 if captured else 0)
        losses = []
        for Tr in (21, 19, 21):
            c = dict(base, Tr=Tr, Tf=Tr - 1)
            rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
            y = synth.multi_hot_labels(c["seed"] + Tr, "labels", c["B"], c["C"]).cuda()
            losses.append(float(run(rgb, mot, mr, mf, y)[0].clone()))
        assert run.n_graphs == (1 if captured else 0)
        runs.append((losses, {k: p.detach().clone() for k, p in m.named_parameters()}, opt.step_count, int(opt.dev_state[0].item())))
    (le, pe, ce, de), (lc, pc, cc, dc) = runs
    print(f"one train graph {mode} {dtype}: eager {le} captured {lc}")
    assert ce == de == cc == dc == 3
    assert all(np.isfinite(le)) and le == lc and le[0] != le[1]
    for k in pe:
        assert torch.equal(pe[k], pc[k]), k


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------

def _labels(split, n):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ak_labels.npz"))
    return torch.from_numpy(np.unpackbits(z[f"{split}/labels"], axis=1)[:n, :140].astype(np.float32))


def _padded_shapes(batch_list, bucket, cmode):
    from vimo_clip_amd import graphs
    shapes = set()
    for b in batch_list:
        out = graphs.pad_concat_to_bucket(b["embeddings"], b["flow_embeddings"], b["mask_rgb"], b["mask_flow"], bucket, cmode)
        shapes.add((out[0].shape[1], out[1].shape[1], out[6]))
    return shapes


def _trainer(mode, dtype, tr, va, BS, **cfg_kw):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer
    ag.weights.clear()
    cfg = Config(epochs=1, batch_size=BS, d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, dropout=0.1, mlp_dropout=0.1, device="cuda",
                 checkpoint_dir=None, use_graphs=True, graph_bucket=16, graph_bucket_concat=True, **mg.tfam_mode_kwargs(mode), **cfg_kw)
    model = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, dropout=0.1, mlp_dropout=0.1, device="cuda",
                     compute_dtype=dtype, **mg.tfam_mode_kwargs(mode)).cuda()
    model.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 83), strict=True)
    model.set_dropout_seed(cfg.seed * 1000)
    return ModelTrainer(model, tr, va, cfg), model


@MODES
def test_bucketed_trainer_captured_equals_bucketed_eager(mode):
    """ModelTrainer(use_graphs, graph_bucket=16, graph_bucket_concat) over one epoch of 12 ragged batches with dropout 0.1: at most one
    training graph per distinct padded shape (fewer than the exact shapes), and the epoch's statistics and the parameters equal,
    bit for bit, those of the same trainer whose bucketed steps run eagerly (max_graphs = 0).  The validation pass (captured eval
    forwards, two slots) gives both trainers the same numbers."""
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    from vimo_clip_amd.TFAM.train_and_eval import batches
    BS = 4
    tr = SyntheticEmbeddingDataset(_labels("train", 12 * BS), D, tmin=17, tmax=64, seed=5, signal=0.6)
    va = SyntheticEmbeddingDataset(_labels("val", 2 * BS), D, tmin=17, tmax=64, seed=6, signal=0.6)
    order = torch.randperm(len(tr), generator=torch.Generator().manual_seed(49)).tolist()        # train_epoch(0)'s order (Config.seed + 0)
    bs = list(batches(tr, BS, order=order))
    shapes = _padded_shapes(bs, 16, CMODE[mode])
    assert len(shapes) < len({b["embeddings"].shape[1] for b in bs})
    runs = []
    for captured in (False, True):
        t, model = _trainer(mode, torch.bfloat16, tr, va, BS)
        assert t.config.seed == 49 and t._graphed_train.bucket == 16 and t._graphed_train.concat == CMODE[mode]
        assert t._graphed_eval.bucket == 16 and t._graphed_eval.concat == CMODE[mode]
        if not captured:
            t._graphed_train.max_graphs = 0
        stats = t.train_epoch(0)
        runs.append((stats, {k: v.detach().clone() for k, v in model.state_dict().items()}, t, t.validate(0)))
    (se, we, te, ve), (sg, wg, tg, vg) = runs
    print(f"bucketed concat trainer {mode}: eager {se} captured {sg}; {tg._graphed_train.n_graphs} graphs for {len(shapes)} padded shapes; "
          f"validation {ve} {vg}")
    assert te._graphed_train.n_graphs == 0 and 1 <= tg._graphed_train.n_graphs <= len(shapes)
    assert int(tg.optimizer.dev_state[0].item()) == int(te.optimizer.dev_state[0].item()) == 12
    assert np.isfinite(se[0]) and se == sg
    for k in we:
        assert torch.equal(we[k], wg[k]), k
    assert np.isfinite(ve[0]) and ve == vg


def test_store_path_equals_loader_path_at_the_same_buckets():
    """Token concatenation, ModelTrainer(use_graphs, graph_bucket=16, graph_bucket_concat) over one epoch of 8 steps with dropout
    0.1, with and without device_store: the store gathers at the bucketed stream lengths, hands its max_len tensors over as
    token_lens and keys the step on T_out by value -- the assembled batches, the epoch's statistics and every parameter are
    bit-identical to the loader path's, the graph count is at most the number of padded shapes, the status word stays 0."""
    from vimo_clip_amd import graphs
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    from vimo_clip_amd.TFAM.train_and_eval import batches, index_batches
    BS = 4
    tr = SyntheticEmbeddingDataset(_labels("train", 8 * BS), D, tmin=17, tmax=64, seed=5, signal=0.6)
    va = SyntheticEmbeddingDataset(_labels("val", BS), D, tmin=17, tmax=64, seed=6, signal=0.6)
    order = torch.randperm(len(tr), generator=torch.Generator().manual_seed(49)).tolist()
    bs = list(batches(tr, BS, order=order))
    shapes = _padded_shapes(bs, 16, "time")
    runs = []
    for device_store in (False, True):
        t, model = _trainer("concat1", torch.bfloat16, tr, va, BS, device_store=device_store)
        assert (t._train_store is not None) == device_store and t._store_concat == ("time" if device_store else None)
        if device_store:                                   # the batches, before any step
            store = t._train_store
            for (pos, ids), b in zip(index_batches(len(store), BS, order=order), bs):
                want = graphs.pad_concat_to_bucket(b["embeddings"].cuda(), b["flow_embeddings"].cuda(), b["mask_rgb"].cuda(), b["mask_flow"].cuda(),
                                                   16, "time")
                T_rgb, T_mot = t._store_lengths(store, ids)
                g = store.gather(torch.tensor(ids, dtype=torch.int32, device="cuda"), T_rgb, T_mot)
                assert torch.equal(g["embeddings"], want[0]) and torch.equal(g["flow_embeddings"], want[1])
                assert torch.equal(g["mask_rgb"], want[2]) and torch.equal(g["mask_flow"], want[3]) and torch.equal(g["labels"], b["labels"].cuda())
                assert (int(g["max_len_rgb"]), int(g["max_len_flow"]), t._store_concat_len(store, ids, T_mot)) == want[4:]
        stats = t.train_epoch(0)
        runs.append((stats, {k: v.detach().clone() for k, v in model.state_dict().items()}, t))
    (sl, wl, tl), (ss, ws, ts) = runs
    print(f"concat trainer, loader {sl} store {ss}; graphs: loader {tl._graphed_train.n_graphs} store {ts._graphed_train.n_graphs} "
          f"for padded shapes {sorted(shapes)}")
    assert np.isfinite(sl[0]) and sl == ss
    for k in wl:
        assert torch.equal(wl[k], ws[k]), k
    assert 1 <= ts._graphed_train.n_graphs <= len(shapes) and 1 <= tl._graphed_train.n_graphs <= len(shapes)
    assert int(ts.optimizer.dev_state[0].item()) == int(tl.optimizer.dev_state[0].item()) == 8
    assert ts._train_store.read_status() == 0 and ts._val_store.read_status() == 0
