"""GPU: ragged clip batches padded to a length bucket give the unpadded batch's logits and gradients when the mean-pool is told
the batch's own length (``pool_len``: one int32 in device memory, read by the pool kernels at replay time; include/vmc.h "POOL
LENGTH") -- so one captured graph serves a whole bucket (vimo_clip_amd/graphs.py pad_to_bucket / GraphedTrainStep(bucket=),
TFAM/train_and_eval.py GraphedEvalForward(bucket=), Config.graph_bucket).

Reference: oracle.tfam.amo_clip_forward (and torch autograd through it) on the CPU at the batch's OWN T_max, no bucket; that
restatement is pinned to the imported reference module by tests/test_oracle_golden.py.

Bounds, restated unchanged from the tests of the same paths:
  logits  |d| <= TOL[dtype] * max(1, |ref|max), TOL = {float16: 1e-3, bfloat16: 8e-3}            (tests/test_gpu_tfam_fused.py)
  loss 5e-3 relative; gradients relative L2 <= 4e-2 per parameter, 1e-1 for ``.ffn.0.``          (tests/test_gpu_tfam_train.py)
A padded and an unpadded batch may take different kernels (attention switches at 64 keys, the GEMMs on the row count), so
padded-vs-exact agreement is within these tolerances; bit-identity is asked only between a graph replay and an eager run on
the same padded tensors.

Every batch here has a T_max that is not a multiple of the bucket AND a clip shorter than T_max (``_padded`` asserts it), so
both kinds of padding -- the loader's and the bucket's -- are present.
"""
import os

import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from oracle import tfam as otfam
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
WIDTHS = pytest.mark.parametrize("D", [512, 768], ids=["d512", "d768"])
MODES = pytest.mark.parametrize("mode", ["cross", "rgb", "flow"])


def _case(mode, D, Tr, pe=False, B=4, L=2, ff=1024, seed=700):
    return dict(name=f"{mode}_d{D}_t{Tr}", D=D, H=8, L=L, ff=ff, C=140, B=B, Tr=Tr, Tf=Tr - 1, mode=mode, pe=pe, ragged=True,
                seed=seed + Tr + D // 256 + 3 * ["cross", "rgb", "flow"].index(mode))


def _model(c, dtype, train=False):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    m = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=c["C"], use_pe=c["pe"],
                 dropout=0.0, mlp_dropout=0.0, device="cuda", compute_dtype=dtype, **mg.tfam_mode_kwargs(c["mode"])).cuda()
    m.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]), strict=True)
    return m.train() if train else m.eval()


def _padded(c, bucket):
    """(unpadded CPU inputs, padded device inputs, T_max of the pooled stream).  Fresh tensors on every call: with use_pe the model
    adds the positional encoding in place."""
    from vimo_clip_amd import graphs
    rgb, mot, mr, mf = mg.tfam_inputs(c)
    pooled = "motion" if c["mode"] == "flow" else "rgb"
    pm, T_max = (mf, c["Tf"]) if pooled == "motion" else (mr, c["Tr"])
    lens = pm.sum(1)
    assert T_max % bucket != 0, "T_max must not be a multiple of the bucket (bucket padding present)"
    assert int(lens.max()) == T_max and int(lens.min()) < T_max, "one clip must be shorter than T_max (loader padding present)"
    prgb, pmot, pmr, pmf, n = graphs.pad_to_bucket(rgb.cuda(), mot.cuda(), mr.cuda(), mf.cuda(), bucket, pooled)
    assert n == T_max and (prgb.shape[1] if pooled == "rgb" else pmot.shape[1]) == -(-T_max // bucket) * bucket
    return (rgb, mot, mr, mf), (prgb, pmot, pmr, pmf), T_max


def _oracle(c, inputs):
    sd = synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"])
    return otfam.amo_clip_forward(sd, *inputs, nhead=c["H"], use_pe=c["pe"], **mg.tfam_mode_kwargs(c["mode"]))


# ---- the pool kernels through the C ABI --------------------------------------------------------------------------------------

@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_mean_pool_len_and_its_backward(xdtype):
    from vimo_clip_amd._lib import check, dt, lib, ptr, stream
    B, T, D = 3, 13, 768
    d16 = torch.float16 if xdtype == torch.float16 else torch.bfloat16
    x = synth.normal(5, "pool_x", (B, T, D)).to(xdtype).cuda().contiguous()
    dout = synth.normal(5, "pool_dout", (B, D)).cuda().contiguous()

    def fwd(n_dev, plain=False):
        o16 = torch.empty((B, D), dtype=d16, device="cuda")
        o32 = torch.empty((B, D), dtype=torch.float32, device="cuda")
        if plain:
            check(lib.vmc_mean_pool(ptr(x), ptr(o16), ptr(o32), B, T, D, dt(x), dt(d16), stream()), "mean_pool")
        else:
            check(lib.vmc_mean_pool_len(ptr(x), ptr(o16), ptr(o32), B, T, D, ptr(n_dev), dt(x), dt(d16), stream()), "mean_pool_len")
        return o16, o32

    def bwd(n_dev, dx_dtype, plain=False):
        dx = torch.full((B, T, D), float("nan"), dtype=dx_dtype, device="cuda")         # stands for torch.empty: every row must be written
        if plain:
            check(lib.vmc_mean_pool_bwd(ptr(dout), ptr(dx), B, T, D, dt(dout), dt(dx), dt(d16), stream()), "mean_pool_bwd")
        else:
            check(lib.vmc_mean_pool_bwd_len(ptr(dout), ptr(dx), B, T, D, ptr(n_dev), dt(dout), dt(dx), dt(d16), stream()), "mean_pool_bwd_len")
        return dx

    # one rounding to 16 bits: relative 2^-8 (bf16) / 2^-11 (f16, 10 mantissa bits, round to nearest); f16 values below 2^-14 are
    # subnormal with spacing 2^-24, so there the error is absolute
    ulp16, abs16 = (2.0 ** -8, 1e-30) if d16 == torch.bfloat16 else (2.0 ** -11, 2.0 ** -24)
    for n_arg, n in ((1, 1), (7, 7), (T, T), (0, 1), (T + 5, T)):              # the last two: clamped into [1, T] by the kernels
        n_dev = torch.tensor([n_arg], dtype=torch.int32, device="cuda")
        o16, o32 = fwd(n_dev)
        ref = x[:, :n].double().mean(1)
        # fp32 accumulation of at most 13 values of |x| < 6: 13 roundings of 2^-24 relative to partial sums < 78
        assert (o32.double() - ref).abs().max().item() <= 13 * 78 * 2.0 ** -24, (xdtype, n_arg)
        assert ((o16.double() - o32.double()).abs() <= ulp16 * o32.double().abs() + abs16).all()
        for dx_dtype in (torch.float32, d16):
            dx = bwd(n_dev, dx_dtype)
            want = (dout / n).unsqueeze(1).expand(B, n, D)
            tol, atol = (2.0 ** -22, 1e-30) if dx_dtype == torch.float32 else (ulp16, abs16)
            assert ((dx[:, :n].double() - want.double()).abs() <= tol * want.double().abs() + atol).all(), (xdtype, n_arg, dx_dtype)
            assert dx[:, n:].numel() == B * (T - n) * D and bool((dx[:, n:] == 0).all()), "rows >= n of dx must be exactly 0"
    # NULL = the entry without the suffix, bit for bit; and so is n = T
    full = torch.tensor([T], dtype=torch.int32, device="cuda")
    for a, b, c3 in zip(fwd(None), fwd(None, plain=True), fwd(full)):
        assert torch.equal(a, b) and torch.equal(a, c3)
    for dx_dtype in (torch.float32, d16):
        a, b, c3 = bwd(None, dx_dtype), bwd(None, dx_dtype, plain=True), bwd(full, dx_dtype)
        assert torch.equal(a, b) and torch.equal(a, c3) and bool(torch.isfinite(a.float()).all())


# ---- eval logits: padded to the bucket + pool_len vs the oracle at the batch's own T_max -----------------------------------------

def _eval_check(c, dtype, bucket, fused, monkeypatch):
    from vimo_clip_amd import tfam_fused as tf
    m = _model(c, dtype)
    m.fused_inference = fused
    calls = []
    orig = tf.TfamPack.forward
    monkeypatch.setattr(tf.TfamPack, "forward", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    exact, _, T_max = _padded(c, bucket)
    ref = _oracle(c, exact)
    bound = TOL[dtype] * max(1.0, ref.abs().max().item())
    with torch.no_grad():
        prgb, pmot, pmr, pmf = _padded(c, bucket)[1]
        y_int = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, pool_len=T_max).float().cpu()
        prgb, pmot, pmr, pmf = _padded(c, bucket)[1]
        y_dev = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, pool_len=torch.tensor([T_max], dtype=torch.int32, device="cuda")).float().cpu()
        prgb, pmot, pmr, pmf = _padded(c, bucket)[1]
        y_all = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf).float().cpu()           # what bucket > 1 computed before: mean over all padded rows
    assert bool(calls) == fused, "fused chain taken" if calls else "the fused chain was not taken"
    err, err_all = (y_int - ref).abs().max().item(), (y_all - ref).abs().max().item()
    print(f"ragged eval {c['name']} pe={c['pe']} {dtype} fused={fused}: T_max {T_max} -> bucket {bucket}: err {err:.3e} "
          f"(bound {bound:.3e}, |ref|max {ref.abs().max():.2f}); without pool_len {err_all:.3e}")
    assert torch.equal(y_int, y_dev)                       # an int is the same length as a device tensor
    assert err <= bound
    assert T_max <= 0.75 * (-(-T_max // bucket) * bucket)
    assert err_all > bound, "padding to the bucket without pool_len must change the logits beyond the tolerance"


@DTYPES
@WIDTHS
@MODES
@pytest.mark.parametrize("pe", [False, True], ids=["nope", "pe"])
@pytest.mark.parametrize("fused", [False, True], ids=["perop", "fused"])
def test_eval_logits_short_clips(dtype, D, mode, pe, fused, monkeypatch):
    """T_max 21 (20 motion tokens) -> 32: (a) the per-op path, (b) the fused eval chain (B * T_padded = 128 rows)."""
    _eval_check(_case(mode, D, 21, pe=pe), dtype, 16, fused, monkeypatch)


@DTYPES
@WIDTHS
@MODES
@pytest.mark.parametrize("pe", [False, True], ids=["nope", "pe"])
def test_eval_logits_whole_videos(dtype, D, mode, pe, monkeypatch):
    """(c) T_max 141 (140 motion tokens) -> 192: past 64 tokens, the per-op path with the tiled attention kernels."""
    _eval_check(_case(mode, D, 141, pe=pe, B=3), dtype, 64, False, monkeypatch)


# ---- training: loss and every parameter gradient vs oracle autograd at T_max ------------------------------------------------------

def _oracle_grads(c, exact, y):
    sd = {k: v.clone().requires_grad_(True) for k, v in synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]).items()}
    logits = otfam.amo_clip_forward(sd, *exact, nhead=c["H"], use_pe=c["pe"], **mg.tfam_mode_kwargs(c["mode"]))
    loss = otfam.bce_with_logits_mean(logits, y)
    loss.backward()
    return loss.item(), logits.detach(), {k: v.grad for k, v in sd.items() if v.grad is not None}


@DTYPES
@WIDTHS
@MODES
@pytest.mark.parametrize("fused", [False, True], ids=["perop", "fused"])
def test_training_step_matches_oracle_autograd(dtype, D, mode, fused, monkeypatch):
    """One train-mode step (dropout 0) on the batch padded 21 -> 32 with pool_len = 21: loss, logits and EVERY parameter gradient
    against torch autograd through the fp32 oracle on the unpadded batch; the gradient the pool hands back is exactly 0 on the
    bucket's rows."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd import tfam_train as tt
    from vimo_clip_amd._lib import lib
    from vimo_clip_amd.losses import bce_with_logits_loss
    c = _case(mode, D, 21)
    m = _model(c, dtype, train=True)
    m.fused_training = fused
    taken = []
    orig_ft = tt.forward_train

    def spy_ft(*a, **k):
        out = orig_ft(*a, **k)
        taken.append(out is not None)
        return out
    monkeypatch.setattr(tt, "forward_train", spy_ft)
    pool_dx = []
    orig_apply = ag.MeanPoolFn.apply

    def spy_pool(x, *a):
        x.register_hook(lambda g: pool_dx.append(g.detach().clone()))           # the pool is the only consumer of x: g is its dx
        return orig_apply(x, *a)
    monkeypatch.setattr(ag.MeanPoolFn, "apply", staticmethod(spy_pool))
    exact, (prgb, pmot, pmr, pmf), T_max = _padded(c, 16)
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"])
    logits = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, pool_len=T_max)
    assert taken == ([True] if fused else []), "fused training chain taken / not taken as asked"
    ws = logits.grad_fn.ws if fused else None                # the chain's workspace: the head's backward leaves the pool's dx there
    loss = bce_with_logits_loss(logits, y.cuda())
    loss.backward()
    B, T = (pmot if mode == "flow" else prgb).shape[:2]
    if fused:
        cross = mode == "cross"
        off = lib.vmc_tfam_train_pool_grad_offset(B, T, pmot.shape[1] if cross else 0, D, c["H"], c["ff"], c["L"], c["C"], int(cross))
        assert off >= 0
        dx = ws[off:off + B * T * D * 4].view(torch.float32).view(B, T, D)
    else:
        assert len(pool_dx) == 1
        dx = pool_dx[0].view(B, T, D).float()
    assert T > T_max and bool((dx[:, T_max:] == 0).all()), "the pool's dx must be exactly 0 on rows >= T_max"
    assert bool((dx[:, :T_max] != 0).any())
    used = {id(q) for q in m.used_parameters()}
    grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if id(p) in used and p.grad is not None}
    ref_loss, ref_logits, ref = _oracle_grads(c, exact, y)
    err = (logits.detach().float().cpu() - ref_logits).abs().max().item()
    print(f"ragged train {c['name']} {dtype} fused={fused}: loss {loss.item():.6f} vs {ref_loss:.6f}, logits err {err:.3e}")
    assert abs(loss.item() - ref_loss) <= 5e-3 * abs(ref_loss)
    assert err <= TOL[dtype] * max(1.0, ref_logits.abs().max().item())
    assert set(grads) == set(ref), set(grads) ^ set(ref)
    worst = ("", 0.0)
    for k, r in ref.items():
        rel_l2 = ((grads[k] - r).norm() / (r.norm() + 1e-20)).item()
        worst = max(worst, (k, rel_l2), key=lambda t: t[1])
        print(f"    grad {k}: rel L2 {rel_l2:.3e}")
    print(f"ragged train {c['name']} {dtype} fused={fused}: worst gradient rel L2 {worst[1]:.3e} ({worst[0]})")
    for k, r in ref.items():
        rel_l2 = ((grads[k] - r).norm() / (r.norm() + 1e-20)).item()
        assert rel_l2 <= (1e-1 if ".ffn.0." in k else 4e-2), (k, rel_l2)


def test_backward_twice_raises_a_clear_error():
    from vimo_clip_amd.losses import bce_with_logits_loss
    c = _case("cross", 512, 21)
    m = _model(c, torch.bfloat16, train=True)
    _, (prgb, pmot, pmr, pmf), T_max = _padded(c, 16)
    logits = m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, pool_len=T_max)
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).cuda()
    dl = torch.autograd.grad(bce_with_logits_loss(logits, y), logits)[0]
    logits.backward(dl, retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        logits.backward(dl)


def test_freezing_a_parameter_rebuilds_the_pointer_tables():
    """The fused chain caches its pointer tables; the key carries requires_grad, so a parameter frozen after the first step no
    longer has its arena slot written."""
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import GradArena
    c = _case("cross", 512, 21)
    m = _model(c, torch.bfloat16, train=True)
    arena = GradArena(m.used_parameters())
    y = synth.multi_hot_labels(c["seed"], "labels", c["B"], c["C"]).cuda()
    w, b = m.classifier[4].weight, m.classifier[4].bias

    def step():
        _, (prgb, pmot, pmr, pmf), T_max = _padded(c, 16)
        arena.flat_grad.fill_(float("nan"))
        bce_with_logits_loss(m(prgb, pmot, mask_rgb=pmr, mask_flow=pmf, pool_len=T_max), y).backward()
        torch.cuda.synchronize()
    step()
    assert bool(torch.isfinite(w._vmc_grad).all()) and bool(torch.isfinite(b._vmc_grad).all())
    w.requires_grad_(False)
    b.requires_grad_(False)
    step()
    assert bool(torch.isnan(w._vmc_grad).all()) and bool(torch.isnan(b._vmc_grad).all()), "a frozen parameter's gradient slot was written"
    assert bool(torch.isfinite(m.classifier[1].weight._vmc_grad).all())


# ---- one graph, several lengths ---------------------------------------------------------------------------------------------------

@DTYPES
@WIDTHS
def test_one_eval_graph_serves_every_length_of_its_bucket(dtype, D):
    """The eval forward captured ONCE at padded length 32 and replayed with pool_len 17, 25 and 32 (inputs re-padded): each replay is
    bit-identical to an eager forward on the same padded tensors, and within the tolerance of the oracle at the exact length."""
    from vimo_clip_amd import graphs
    m = None
    g = None
    for Tr in (17, 25, 32):
        c = dict(_case("cross", D, Tr), seed=640 + D // 256)              # one set of weights for the three lengths
        if m is None:
            m = _model(c, dtype)

            def fwd(a, b, cm, d, n):
                with torch.no_grad():
                    return m(a, b, mask_rgb=cm, mask_flow=d, pool_len=n)
        rgb, mot, mr, mf = mg.tfam_inputs(c)
        assert int(mr.sum(1).min()) < Tr
        args = graphs.pad_to_bucket(rgb.cuda(), mot.cuda(), mr.cuda(), mf.cuda(), 32)
        args = args[:4] + (torch.tensor([args[4]], dtype=torch.int32, device="cuda"),)
        assert args[0].shape[1] == args[1].shape[1] == 32 and int(args[4]) == Tr
        if g is None:
            g = graphs.GraphedCallable(fwd, *args)
        got = g(*args).clone()
        eager = fwd(*args)
        assert torch.equal(got, eager), Tr
        ref = _oracle(c, (rgb, mot, mr, mf))
        err = (got.float().cpu() - ref).abs().max().item()
        print(f"one graph, T_max {Tr} of 32, {dtype} d{D}: err vs oracle {err:.3e}")
        assert err <= TOL[dtype] * max(1.0, ref.abs().max().item())


@DTYPES
@WIDTHS
@pytest.mark.parametrize("p_drop", [0.0, 0.1], ids=["nodrop", "drop"])
def test_one_train_graph_serves_every_length_of_its_bucket(dtype, D, p_drop):
    """The training step (tick + forward + loss + backward + AdamW) captured once at padded length 32 and replayed with T_max 17,
    25, 32, 17: the same parameters, bit for bit, as eager device-state steps on the same padded tensors -- also with dropout,
    whose masks are indexed by the padded shape on both sides."""
    from vimo_clip_amd import graphs
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    base = dict(_case("cross", D, 17, B=8), seed=660 + D // 256)
    runs = []
    for captured in (False, True):
        m = AMO_CLIP(d_model=D, nhead=base["H"], num_layers=base["L"], dim_feedforward=base["ff"], num_classes=base["C"], dropout=p_drop,
                     mlp_dropout=p_drop, device="cuda", compute_dtype=dtype).cuda().train()
        m.load_state_dict(synth.tfam_state_dict(D, base["H"], base["L"], base["ff"], base["C"], base["seed"]), strict=True)
        opt = FusedAdam(GradArena(m.used_parameters()), lr=1e-3, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=11)
        m.use_device_seeds(opt)

        def step(a, b, cm, d, yy, n=None):
            opt.tick()
            out = m(a, b, mask_rgb=cm, mask_flow=d, pool_len=n)
            loss = bce_with_logits_loss(out, yy)
            loss.backward()
            opt.step()
            return loss.detach(), out.detach()

        run = graphs.GraphedTrainStep(step, opt, bucket=32, max_graphs=16 if captured else 0)      # max_graphs = 0: same padding, eager steps
        losses = []
        for Tr in (17, 25, 32, 17):
            c = dict(base, Tr=Tr, Tf=Tr - 1)
            rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
            y = synth.multi_hot_labels(c["seed"] + Tr, "labels", c["B"], c["C"]).cuda()
            losses.append(float(run(rgb, mot, mr, mf, y)[0].clone()))
        assert len(run._graphs) == (1 if captured else 0)
        runs.append((losses, {k: p.detach().clone() for k, p in m.named_parameters()}, opt.step_count, int(opt.dev_state[0].item())))
    (le, pe, ce, de), (lc, pc, cc, dc) = runs
    print(f"one train graph {dtype} d{D} dropout {p_drop}: eager {le} captured {lc}")
    assert ce == de == cc == dc == 4
    assert le == lc
    for k in pe:
        assert torch.equal(pe[k], pc[k]), k


# ---- the managers over a ragged list ----------------------------------------------------------------------------------------------------

def _labels(split, n):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ak_labels.npz"))
    return torch.from_numpy(np.unpackbits(z[f"{split}/labels"], axis=1)[:n, :140].astype(np.float32))


def _padded_pairs(batch_list, bucket):
    pairs = set()
    for b in batch_list:
        Tr, Tf = b["embeddings"].shape[1], b["flow_embeddings"].shape[1]
        assert b["mask_rgb"].sum(1).max() == Tr
        pairs.add((-(-Tr // bucket) * bucket, -(-Tf // bucket) * bucket))
    return pairs


@DTYPES
@pytest.mark.parametrize("fused", [False, True], ids=["perop", "fused"])
def test_graphed_eval_forward_over_a_ragged_list(dtype, fused):
    """GraphedEvalForward(bucket=16) over 24 ragged batches (T_rgb ~ U{17..64}; 3 clips each, so that the batch maxima spread over
    the buckets): at most one graph per distinct padded (T_rgb, T_motion) pair and slot; every batch's logits within the tolerance
    of the oracle at that batch's exact shape, through the captured per-op path and the captured fused chain."""
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, GraphedEvalForward, batches
    D, H, L, FF, C, BS = 512, 8, 2, 1024, 140, 3
    ds = SyntheticEmbeddingDataset(_labels("val", 24 * BS), D, tmin=17, tmax=64, seed=9, signal=0.6)
    cfg = Config(batch_size=BS, d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, device="cuda")
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, device="cuda", compute_dtype=dtype).cuda().eval()
    sd = synth.tfam_state_dict(D, H, L, FF, C, 81)
    m.load_state_dict(sd, strict=True)
    m.fused_inference = fused
    bs = list(batches(ds, BS))
    assert len(bs) == 24
    pairs = _padded_pairs(bs, 16)
    assert len(pairs) <= 6 and len({b["embeddings"].shape[1] for b in bs}) > len(pairs)      # fewer graphs than exact shapes
    assert any(b["embeddings"].shape[1] % 16 for b in bs)
    gf = GraphedEvalForward(m, cfg, bucket=16)
    with torch.no_grad():
        got = list(gf.pipelined(iter(bs)))
    per_slot = {}
    for key in gf._graphs:
        per_slot[key[0]] = per_slot.get(key[0], 0) + 1
    assert per_slot and max(per_slot.values()) <= len(pairs), (per_slot, pairs)
    worst = 0.0
    for b, out in got:
        ref = otfam.amo_clip_forward(sd, b["embeddings"], b["flow_embeddings"], b["mask_rgb"], b["mask_flow"], nhead=H)
        err = (out.float().cpu() - ref).abs().max().item()
        worst = max(worst, err / max(1.0, ref.abs().max().item()))
        assert err <= TOL[dtype] * max(1.0, ref.abs().max().item()), (b["embeddings"].shape, err)
    print(f"GraphedEvalForward(bucket=16) {dtype} fused={fused}: {len(gf._graphs)} graphs in {len(per_slot)} slots for {len(pairs)} padded shapes, "
          f"worst err / max(1, |ref|) {worst:.3e}")


@DTYPES
def test_bucketed_trainer_captured_equals_bucketed_eager(dtype):
    """ModelTrainer(use_graphs, graph_bucket=16) over one epoch of 24 ragged batches, dropout 0: at most one training graph per
    distinct padded shape, and the parameters after the 24 captured steps equal, bit for bit, those of the same trainer whose
    bucketed steps run eagerly (GraphedTrainStep.max_graphs = 0: same padding, same pool_len, no capture)."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer, batches
    D, H, L, FF, C, BS = 512, 8, 2, 1024, 140, 8
    tr = SyntheticEmbeddingDataset(_labels("train", 24 * BS), D, tmin=17, tmax=64, seed=5, signal=0.6)
    va = SyntheticEmbeddingDataset(_labels("val", BS), D, tmin=17, tmax=64, seed=6, signal=0.6)
    order = torch.randperm(len(tr), generator=torch.Generator().manual_seed(49)).tolist()        # train_epoch(0)'s order (Config.seed + 0)
    pairs = _padded_pairs(list(batches(tr, BS, order=order)), 16)
    assert len(pairs) <= 6
    runs = []
    for captured in (False, True):
        ag.weights.clear()
        cfg = Config(epochs=1, batch_size=BS, d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, dropout=0.0, mlp_dropout=0.0,
                     device="cuda", checkpoint_dir=None, use_graphs=True, graph_bucket=16)
        assert cfg.seed == 49
        model = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, dropout=0.0, mlp_dropout=0.0, device="cuda",
                         compute_dtype=dtype).cuda()
        model.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 83), strict=True)
        t = ModelTrainer(model, tr, va, cfg)
        assert t._graphed_train.bucket == 16 and t._graphed_eval.bucket == 16
        if not captured:
            t._graphed_train.max_graphs = 0
        stats = t.train_epoch(0)
        runs.append((stats, {k: v.detach().clone() for k, v in model.state_dict().items()}, t))
    (se, we, te), (sg, wg, tg) = runs
    print(f"bucketed trainer {dtype}: eager {se} captured {sg}; {len(tg._graphed_train._graphs)} graphs for {len(pairs)} padded shapes")
    assert len(te._graphed_train._graphs) == 0 and 1 <= len(tg._graphed_train._graphs) <= len(pairs)
    assert int(tg.optimizer.dev_state[0].item()) == int(te.optimizer.dev_state[0].item()) == 24
    assert np.isfinite(se[0]) and se == sg
    for k in we:
        assert torch.equal(we[k], wg[k]), k


# ---- the concatenation modes keep exact shapes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["concat1", "concat-1"])
def test_concat_modes_refuse_pool_len_and_run_at_exact_shapes(mode):
    from vimo_clip_amd.TFAM.train_and_eval import Config, GraphedEvalForward
    c = dict(_case("cross", 512, 21), mode=mode)
    m = _model(c, torch.bfloat16)
    rgb, mot, mr, mf = (t.cuda() for t in mg.tfam_inputs(c))
    with pytest.raises(ValueError, match="pool_len"):
        m(rgb, mot, mask_rgb=mr, mask_flow=mf, pool_len=21)
    cfg = Config(batch_size=c["B"], d_model=512, device="cuda")
    gf = GraphedEvalForward(m, cfg, bucket=16, streams=1)
    assert gf.bucket == 1 and gf.pooled is None
    batch = {"embeddings": rgb, "flow_embeddings": mot, "mask_rgb": mr, "mask_flow": mf}
    with torch.no_grad():
        got = gf(batch)
        eager = m(rgb, mot, mask_rgb=mr, mask_flow=mf)
    assert list(gf._graphs) == [(0, c["B"], 21, 20, 512)]                  # exact lengths in the key
    assert torch.equal(got, eager)
    ref = _oracle(c, mg.tfam_inputs(c))
    assert (got.float().cpu() - ref).abs().max().item() <= TOL[torch.bfloat16] * max(1.0, ref.abs().max().item())
