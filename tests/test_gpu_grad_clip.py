"""GPU: gradient clipping computed on the device (vmc_grad_clip_dev, include/vmc.h) -- what lets ``clip_grad_norm_`` (train.py:105-106)
into device-state optimiser steps, captured steps, the two-graph data-parallel step and the bucketed replay.

Accuracy bound of the norm (items 2, 3, 5): the relative error of the existing host path (``GradArena.grad_norm()``: fp32 partials,
float atomics) measured on the same gradient, with a floor of 2 fp32 ulps (2^-22) so that an accidentally exact yardstick does not
set an impossible bar.  The reference is ``flat_grad.double().norm()``.
"""
import os

import numpy as np
import pytest
import torch

from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -22


def _labels(split, n):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ak_labels.npz"))
    return torch.from_numpy(np.unpackbits(z[f"{split}/labels"], axis=1)[:n, :140].astype(np.float32))


def _clip_call(grad, base, max_norm):
    """One vmc_grad_clip_dev call through the C ABI on fresh buffers: (clip[4], hyper[4]) on the host."""
    from vimo_clip_amd._lib import check, lib, ptr, stream
    clip = torch.tensor([base, max_norm, -1.0, -1.0], dtype=torch.float32, device=grad.device)
    hyper = torch.full((4,), -1.0, dtype=torch.float32, device=grad.device)
    ws = torch.empty(int(lib.vmc_grad_clip_workspace_bytes(grad.numel())), dtype=torch.uint8, device=grad.device)
    check(lib.vmc_grad_clip_dev(ptr(grad), grad.numel(), ptr(hyper), ptr(clip), ptr(ws), ws.numel(), stream()), "grad_clip_dev")
    torch.cuda.synchronize()
    return clip.cpu(), hyper.cpu()


# ---- 1. against torch ------------------------------------------------------------------------------------------------------------

def _three_params():
    return [torch.nn.Parameter(synth.normal(8, f"p{i}", sh).cuda()) for i, sh in enumerate([(64, 32), (32,), (8, 8)])]


def _device_state_steps(max_grad_norm, steps=3):
    """The parameters, seeded gradients x 3 and lr of test_fused_adam_grad_clip_matches_torch, stepped in device-state mode."""
    from vimo_clip_amd.optim import FusedAdam, GradArena
    ps = _three_params()
    opt = FusedAdam(GradArena(ps), lr=1e-2).enable_device_state()
    norms, coefs = [], []
    for step in range(steps):
        for i, p in enumerate(ps):
            p._vmc_grad.copy_(synth.normal(9 + step, f"g{i}", tuple(p.shape)).cuda() * 3.0)
        opt.tick()
        opt.step(max_grad_norm=max_grad_norm)
        if max_grad_norm is not None:
            norms.append(opt.last_grad_norm.item())
            coefs.append(opt.last_clip_coef.item())
    return [p.detach().clone() for p in ps], norms, coefs, opt


def _torch_steps(max_grad_norm, steps=3):
    ref = [torch.nn.Parameter(p.detach().clone()) for p in _three_params()]
    topt = torch.optim.Adam(ref, lr=1e-2)
    for step in range(steps):
        for i, r in enumerate(ref):
            r.grad = synth.normal(9 + step, f"g{i}", tuple(r.shape)).cuda() * 3.0
        torch.nn.utils.clip_grad_norm_(ref, max_grad_norm)
        topt.step()
    return [r.detach() for r in ref]


def test_device_state_grad_clip_matches_torch():
    """The device-state twin of test_fused_adam_grad_clip_matches_torch: tick(); step(max_grad_norm=0.7) x 3 against clip_grad_norm_ +
    torch.optim.Adam, 2e-6 * max(1, |ref|max).  Then with a threshold no step reaches: the coefficient is exactly 1 and the
    parameters are, bit for bit, those of the same steps without clipping."""
    ps, norms, coefs, opt = _device_state_steps(0.7)
    for p, r in zip(ps, _torch_steps(0.7)):
        assert (p - r).abs().max().item() <= 2e-6 * max(1.0, r.abs().max().item())
    print("norms", norms, "coefs", coefs)
    assert all(c < 1.0 for c in coefs) and all(n > 0.7 for n in norms)
    assert opt.dev_hyper[3].item() == coefs[-1]                     # base_scale 1: what the Adam kernel multiplied the gradient with
    loose = 2.0 * max(norms)
    ps_loose, norms_loose, coefs_loose, _ = _device_state_steps(loose)
    assert norms_loose == norms                                     # same seeded gradients: the norm does not depend on the threshold
    assert coefs_loose == [1.0, 1.0, 1.0]
    ps_none, _, _, opt_none = _device_state_steps(None)
    assert opt_none.dev_clip is None                                # max_grad_norm=None: nothing allocated, nothing launched
    for a, b, r in zip(ps_loose, ps_none, _torch_steps(loose)):
        assert torch.equal(a, b)
        assert (a - r).abs().max().item() <= 2e-6 * max(1.0, r.abs().max().item())


# ---- 2. norm accuracy ------------------------------------------------------------------------------------------------------------

def _arena(kind):
    from vimo_clip_amd.optim import GradArena
    if kind == "tiny":
        return GradArena(_three_params())
    if kind == "odd":                                               # 3776 elements: 3.69 x 1024
        return GradArena([torch.nn.Parameter(torch.zeros(sh, device="cuda")) for sh in [(100, 37), (5,)]])
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    m = AMO_CLIP(d_model=768, nhead=8, num_layers=4, dim_feedforward=2048, num_classes=140, device="cuda").cuda()
    return GradArena(m.used_parameters())


def _errors(arena, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    arena.flat_grad.copy_(torch.randn(arena.numel, generator=g, device="cuda") * 0.02)
    ref = arena.flat_grad.double().norm().item()
    host = arena.grad_norm().item()
    clip, hyper = _clip_call(arena.flat_grad, 1.0, 1.0)
    return ref, abs(host - ref) / ref, abs(clip[2].item() - ref) / ref, clip, hyper


@pytest.mark.parametrize("kind", ["tiny", "odd", "tfam768"])
def test_norm_is_at_least_as_accurate_as_the_host_path(kind):
    arena = _arena(kind)
    assert arena.numel % 64 == 0 and (kind != "odd" or arena.numel % 1024)
    assert kind != "tfam768" or arena.numel > 4 * 2048 * 512       # more than one trip of the capped grid: the grid-stride loop
    ref, e_host, e_dev, clip, _ = _errors(arena, 3)
    print(f"{kind}: n {arena.numel}  ||g|| {ref:.9g}  rel err host path {e_host:.3e}  device clip {e_dev:.3e}  floor {FLOOR:.3e}")
    assert e_dev <= max(e_host, FLOOR)


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------------------

def test_same_gradient_same_bits_and_the_host_formula():
    from vimo_clip_amd.optim import clipped_grad_scale
    arena = _arena("tfam768")
    ref, e_host, _, clip0, hyper0 = _errors(arena, 4)
    clip1, hyper1 = _clip_call(arena.flat_grad, 1.0, 1.0)
    assert torch.equal(clip0, clip1) and torch.equal(hyper0, hyper1)
    assert hyper0[:3].tolist() == [-1.0, -1.0, -1.0]               # only hyper[3] is written
    tol = max(e_host, FLOOR)
    assert ref > 4.0                                                # max_norm = 1 clips for every base below
    for base in (1.0, 0.5, 0.125):
        (clip, hyper), (clip_b, hyper_b) = _clip_call(arena.flat_grad, base, 1.0), _clip_call(arena.flat_grad, base, 1.0)
        assert torch.equal(clip, clip_b) and torch.equal(hyper, hyper_b)
        want = clipped_grad_scale(ref, base, 1.0)
        got = hyper[3].item()
        print(f"base {base}: hyper[3] {got:.9g}  host formula {want:.9g}  rel diff {abs(got - want) / want:.3e}  tol {tol:.3e}")
        assert abs(got - want) <= tol * want
        assert clip[0].item() == base and clip[1].item() == 1.0 and got == base * clip[3].item()
        assert abs(clip[2].item() - ref * base) <= tol * ref * base


# ---- 4. captured trainer ---------------------------------------------------------------------------------------------------------

class _RecordCoef:
    """Wraps a GraphedTrainStep: keeps a device copy of the clip coefficient after every step (no synchronisation)."""

    def __init__(self, inner, opt):
        self.inner, self.opt, self.coefs = inner, opt, []

    def __call__(self, *inputs):
        out = self.inner(*inputs)
        self.coefs.append(self.opt.last_clip_coef.clone())
        return out


def _forward_on_padded_batches(t, bucket):
    """Make the eager trainer ``t`` see what the bucketed graph manager feeds the model: every batch zero-padded to its length bucket,
    its own length as ``pool_len`` (graphs.pad_to_bucket).  Loss, backward and the host-mode optimiser step stay the trainer's."""
    from vimo_clip_amd.graphs import pad_to_bucket, pooled_stream

    def forward(batch):
        dev, mk = t.config.device, t.config.motion_key
        rgb, mot, mr, mf, n = pad_to_bucket(batch["embeddings"].to(dev), batch[f"{mk}_embeddings"].to(dev), batch["mask_rgb"].to(dev),
                                            batch[f"mask_{mk}"].to(dev), bucket, pooled_stream(t.model))
        return t.model(rgb, mot, mask_rgb=mr, mask_flow=mf, pool_len=n), batch["labels"].to(dev)
    t._forward = forward


TRAINER_CASES = {
    # set-up of test_trainer_with_captured_steps_follows_the_uncaptured_trainer
    "exact_shapes": dict(D=256, H=8, L=2, FF=512, tmin=12, tmax=16, bucket=1, seed=77, clip=0.29),
    # the same ragged clips (12-16 RGB / 11-15 motion tokens) zero-padded to ONE 16-token bucket: one graph, pool_len per batch
    "bucket16": dict(D=256, H=8, L=2, FF=512, tmin=12, tmax=16, bucket=16, seed=77, clip=0.29),
}


@pytest.mark.parametrize("case", list(TRAINER_CASES))
def test_captured_trainer_with_clipping_follows_the_eager_trainer(case):
    """ModelTrainer(grad_clip_norm=x): the eager host-mode trainer (norm read back, factor passed as a host float) and the
    use_graphs=True trainer (vmc_grad_clip_dev inside every replay) over two epochs of 12 steps: epoch statistics within 2e-3,
    weights within 5e-3 * max(1e-3, |w|max) -- the tolerances of the unclipped twin.  The threshold is the median pre-clip norm of the
    UNCLIPPED eager trainer, so that both regimes occur; the captured run's coefficients must show it.

    Pre-clip norms of the unclipped eager trainer (the same run for both cases), 24 steps, measured on an MI355X -- the norm grows
    as the classifier sharpens, so the early steps stay below the threshold and the late ones are clipped:
      0.2394 0.2714 0.2488 0.2464 0.2363 0.2349 0.2430 0.2663 0.2506 0.2691 0.2857 0.2929
      0.2816 0.3247 0.3047 0.3129 0.3182 0.3374 0.3485 0.3279 0.3367 0.3494 0.3498 0.3500      median 0.2893 -> threshold 0.29

    bucket16: the eager trainer is fed the same zero-padded batches and pool_len as the graph manager feeds the model
    (_forward_on_padded_batches), so both runs take the same kernels and differ in the optimiser path alone: host-mode clipping with
    a read-back norm against vmc_grad_clip_dev inside the replay.  Against the eager trainer at EXACT shapes the statistics agree
    (2e-3) but one bias vector misses the weight bound on an MI355X: a padded and an unpadded batch take other kernels
    (DESIGN.md 3.5), a parameter whose true gradient is zero (the key bias of an attention) then receives other rounding noise, and
    Adam turns noise of any size into steps of +-lr -- d_model 512, 17-40 tokens: layers.0.self_attn.in_proj_bias 6.7e-4 against a
    bound of 3.3e-4; that comparison says nothing about clipping and is not made here."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer
    c = TRAINER_CASES[case]
    D, H, L, FF, C, BS = c["D"], c["H"], c["L"], c["FF"], 140, 8
    tr = SyntheticEmbeddingDataset(_labels("train", 96), D, tmin=c["tmin"], tmax=c["tmax"], seed=5, signal=0.6)
    va = SyntheticEmbeddingDataset(_labels("val", 32), D, tmin=c["tmin"], tmax=c["tmax"], seed=6, signal=0.6)
    runs = []
    for graphs in (False, True):
        ag.weights.clear()
        cfg = Config(epochs=2, batch_size=BS, d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, dropout=0.0, mlp_dropout=0.0,
                     device="cuda", checkpoint_dir=None, use_graphs=graphs, graph_bucket=c["bucket"] if graphs else 1,
                     grad_clip_norm=c["clip"])
        model = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, dropout=0.0, mlp_dropout=0.0, device="cuda").cuda()
        model.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, c["seed"]), strict=True)
        t = ModelTrainer(model, tr, va, cfg)
        assert t.grad_clip_norm == c["clip"]
        rec = None
        if not graphs and c["bucket"] > 1:
            _forward_on_padded_batches(t, c["bucket"])
        if graphs:
            rec = t._graphed_train = _RecordCoef(t._graphed_train, t.optimizer)
        stats = []
        for ep in range(2):
            stats.append(t.train_epoch(ep) + t.validate(ep))
            t.scheduler.step()
        runs.append((stats, {k: v.detach().clone() for k, v in model.state_dict().items()}, t, rec))
    (se, we, te, _), (sg, wg, tg, rec) = runs
    coefs = torch.cat(rec.coefs).tolist()
    print("eager   ", se)
    print("captured", sg)
    print("coefficients", [round(x, 4) for x in coefs], "last norm", tg.optimizer.last_grad_norm.item())
    assert te._graphed_train is None and 1 <= len(rec.inner._graphs) <= (16 if c["bucket"] == 1 else 1)
    assert rec.inner.bucket == c["bucket"]
    assert tg.optimizer.step_count == te.optimizer.step_count == 24 == int(tg.optimizer.dev_state[0].item()) == len(coefs)
    assert any(x < 1.0 for x in coefs) and any(x == 1.0 for x in coefs), coefs
    for a, b in zip(se, sg):
        assert all(abs(x - y) <= 2e-3 * max(abs(x), 1e-3) for x, y in zip(a, b)), (a, b)
    for k in we:
        d = (we[k].float() - wg[k].float()).abs().max().item()
        assert d <= 5e-3 * max(1e-3, we[k].float().abs().max().item()), (k, d)


def test_max_grad_norm_must_not_change_inside_a_capture():
    """A first clipped step, or another threshold, writes device memory from the host: inside a capture that raises (as a changed
    optimiser plan does); after one eager step with the threshold the same step captures and replays."""
    from vimo_clip_amd.optim import FusedAdam, GradArena
    ps = _three_params()
    opt = FusedAdam(GradArena(ps), lr=1e-2).enable_device_state()
    opt.arena.flat_grad.fill_(0.5)
    for thr in (0.7, 0.3):                                          # first use; then a changed threshold
        g = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            with torch.cuda.graph(g):
                opt.tick()
                opt.step(max_grad_norm=thr)
        torch.cuda.synchronize()
        opt.tick()
        opt.step(max_grad_norm=thr)                                 # eager: allowed
        torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.tick()
        opt.step(max_grad_norm=0.3)
    before = ps[0].detach().clone()
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(before, ps[0].detach())
    want = 0.5 * opt.arena.numel ** 0.5                             # fill_ wrote the alignment padding too
    assert abs(opt.last_grad_norm.item() - want) <= 1e-6 * want and opt.last_clip_coef.item() < 1.0


# ---- 5. two ranks on one GPU -----------------------------------------------------------------------------------------------------

def _ddp_clip_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from vimo_clip_amd import autograd_ops, parallel
    from vimo_clip_amd.graphs import GraphedTrainStep
    from vimo_clip_amd.losses import bce_with_logits_loss, loss_and_grad
    from vimo_clip_amd.optim import FusedAdam, GradArena, clipped_grad_scale
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    dist.init_process_group("gloo")                        # two ranks share the one GPU of the box: gloo instead of RCCL
    try:
        D, H, L, FF, C, B = 512, 8, 2, 512, 140, 4
        res, thr = {}, float(2 ** 20)                        # "probe": never clips, reads the norms of the averaged gradient
        for mode in ("probe", "plain", "all_reduce"):
            autograd_ops.grad_ready_hooks.clear()
            m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, dropout=0.1, mlp_dropout=0.1, device="cuda").cuda().train()
            m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 9), strict=True)
            arena = GradArena(m.used_parameters())
            opt = FusedAdam(arena, lr=1e-3, weight_decay=0.1, decoupled=True)
            opt.enable_device_state(base_seed=77 + rank)
            m.use_device_seeds(opt)
            red = parallel.GradientAllReducer(arena.flat_grad, bucket_bytes=256 * 1024, exchange="all_reduce")

            def fwd_bwd(rgb, mot, y):
                opt.tick()
                out = m(rgb, mot)
                loss, dl = loss_and_grad(bce_with_logits_loss, out, y)
                out.backward(dl)
                return loss, out.detach()

            def update():
                opt.step(max_grad_norm=thr)
            stepper = GraphedTrainStep(fwd_bwd, opt, exchange=red.all_reduce, opt_fn=update) if mode == "all_reduce" else None
            norms, coefs = [], []
            for step in range(4):
                Tn = 16 if step % 2 else 12                   # two shapes -> two forward/backward graphs, one optimiser graph
                rgb = synth.normal(100 * rank + step, "r", (B, Tn, D)).cuda()
                mot = synth.normal(100 * rank + step, "m", (B, Tn - 1, D)).cuda()
                y = synth.multi_hot_labels(100 * rank + step, "y", B, C).cuda()
                if stepper is None:
                    fwd_bwd(rgb, mot, y)
                    opt.sync_hyper(grad_scale=red.all_reduce())
                    update()
                else:
                    stepper(rgb, mot, y)
                norms.append(opt.last_grad_norm.item())
                coefs.append(opt.last_clip_coef.item())
            torch.cuda.synchronize()
            # the arena still holds the rank SUM of the last step: the host formula on it, base_scale = 1 / world
            total = arena.flat_grad.double().norm().item()
            want = clipped_grad_scale(total, 1.0 / world, thr)
            got = opt.dev_hyper[3].item()
            res[mode] = dict(params=arena.flat_param.detach().cpu().clone(), norms=norms, coefs=coefs, rel=abs(got - want) / want,
                             base=opt.dev_clip[0].item(), norm_rel=abs(norms[-1] - total / world) / (total / world),
                             graphs=None if stepper is None else (len(stepper._graphs), stepper._opt_graph is not None),
                             steps=int(opt.dev_state[0].item()))
            if mode == "probe":
                thr = float(torch.tensor(0.5 * min(norms), dtype=torch.float32))      # every later step clips; exact in fp32
        q.put((rank, bool(torch.equal(res["plain"]["params"], res["all_reduce"]["params"])), float(res["all_reduce"]["params"].double().abs().sum()),
               {k: {f: v for f, v in r.items() if f != "params"} for k, r in res.items()}, thr))
    finally:
        dist.destroy_process_group()


def test_two_graph_data_parallel_step_with_clipping_two_ranks_one_gpu():
    """The pattern of test_two_graph_data_parallel_step_two_ranks_one_gpu with max_grad_norm: the clip launch sits in the optimiser
    graph behind the eager exchange, sees the rank sum and base_scale = 1 / world.  The two-graph step equals the eager device-state
    step bit for bit, the replicas stay identical, and hyper[3] is the host formula on the all-reduced arena (item 2's floor)."""
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_clip_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    print(res)
    assert all(r[1] for r in res), res                              # two-graph == eager device-state, bit for bit
    assert res[0][2] == res[1][2] and res[0][4] == res[1][4]        # replicas identical (and agreed on the threshold)
    for r in res:
        for mode, d in r[3].items():
            assert d["base"] == 0.5 and d["steps"] == 4, (mode, d)
            assert d["rel"] <= FLOOR and d["norm_rel"] <= FLOOR, (mode, d)
        assert all(c == 1.0 for c in r[3]["probe"]["coefs"])
        assert all(c < 1.0 for c in r[3]["plain"]["coefs"] + r[3]["all_reduce"]["coefs"]), r[3]
        assert r[3]["all_reduce"]["graphs"] == (2, True)
        assert r[3]["all_reduce"]["coefs"] == r[3]["plain"]["coefs"] and r[3]["all_reduce"]["norms"] == r[3]["plain"]["norms"]
