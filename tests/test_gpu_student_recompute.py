"""GPU: per-block activation recomputation of the student's ViT (VisionTransformer.recompute = "block", autograd_vit._BlockFn).
The contract is bit-identity with recompute = "none": the recomputed path launches the same kernels on the same operands, so
outputs, loss and every parameter gradient are compared with torch.equal.  The byte model (autograd_vit.saved_activation_bytes)
is checked against the caching allocator, and the peak of a step against the peak of the "none" step."""
import gc

import pytest
import torch

from vimo_clip_amd import synth
from vimo_clip_amd.autograd_vit import saved_activation_bytes

pytestmark = pytest.mark.gpu


def _student(name, seed, dtype, recompute, sd=None, cls_only=True):
    from vimo_clip_amd.models import FlowStudentModel
    m = FlowStudentModel(name, device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype, recompute=recompute)
    m.load_state_dict(sd if sd is not None else synth.student_state_dict(name, seed), strict=True)
    m.visual_encoder.cls_only_last_block = cls_only
    return m.train()


def _loss(m, vids, teacher, labels):
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    emb, emb_d, logits = m(vids)
    loss = distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)
    return (emb, emb_d, logits), loss


def _inputs(seed, shape, E):
    B, T = shape[:2]
    return (synth.randint_u8(seed, "vids", shape).cuda(), synth.normal(seed, "teacher", (B, T + 1, E)).cuda(),
            synth.multi_hot_labels(seed, "labels", B, 140).cuda())


CASES = [
    # name, videos, dtype, cls_only_last_block
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.bfloat16, True),       # 640 rows: the block linears leave through the grouped queue,
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.float16, True),        # the last block's 128 class rows do not
    ("ViT-tiny/14", (2, 3, 3, 56, 56), torch.bfloat16, True),        # 102 rows: ungrouped wgrad_tn; three blocks
    ("ViT-tiny/14@336px", (1, 2, 3, 336, 336), torch.bfloat16, True),    # 577 tokens: streamed attention forward, tiled backward
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.bfloat16, False),      # every block on all rows
]


@pytest.mark.parametrize("name,shape,dtype,cls_only", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_block_recompute_is_bit_identical(name, shape, dtype, cls_only):
    from vimo_clip_amd.optim import GradArena
    sd = synth.student_state_dict(name, 31)
    E = synth.vit_geometry(name)[5]
    vids, teacher, labels = _inputs(31, shape, E)
    got = {}
    for mode in ("none", "block"):
        m = _student(name, 31, dtype, mode, sd, cls_only)
        assert m.visual_encoder.recompute == mode
        arena = GradArena(m.parameters())                      # gradients written in place: the grouped queue is on the path
        arena.flat_grad.fill_(float("nan"))
        outs, loss = _loss(m, vids, teacher, labels)
        loss.backward()
        torch.cuda.synchronize()
        got[mode] = ([o.detach().clone() for o in outs], loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()})
    for a, b in zip(got["none"][0], got["block"][0]):
        assert torch.equal(a, b)
    assert torch.equal(got["none"][1], got["block"][1]) and torch.isfinite(got["none"][1]).item()
    for k, g in got["none"][2].items():
        assert torch.isfinite(g).all().item(), k
        assert torch.equal(g, got["block"][2][k]), k


def test_block_recompute_is_bit_identical_without_an_arena():
    """Gradients returned to autograd (``.grad``) instead of written into arena slots."""
    name, shape = "ViT-tiny/14", (2, 3, 3, 56, 56)
    sd = synth.student_state_dict(name, 37)
    vids, teacher, labels = _inputs(37, shape, 96)
    grads = {}
    for mode in ("none", "block"):
        m = _student(name, 37, torch.bfloat16, mode, sd)
        _loss(m, vids, teacher, labels)[1].backward()
        grads[mode] = {k: p.grad for k, p in m.named_parameters()}
    for k, g in grads["none"].items():
        assert g is not None and torch.equal(g, grads["block"][k]), k


def test_two_training_steps_leave_identical_parameters():
    """Step 2 recomputes from the 16-bit weight copies the optimiser refreshed after step 1: stale copies would show here."""
    from vimo_clip_amd.optim import FusedAdam, GradArena
    name, shape = "ViT-tiny/32", (8, 16, 3, 64, 64)
    sd = synth.student_state_dict(name, 41)
    params = {}
    for mode in ("none", "block"):
        m = _student(name, 41, torch.bfloat16, mode, sd)
        arena = GradArena(m.parameters())
        opt = FusedAdam(arena, lr=1e-3)
        for step in range(2):
            vids, teacher, labels = _inputs(41 + step, shape, 64)
            _loss(m, vids, teacher, labels)[1].backward()
            opt.step()
        torch.cuda.synchronize()
        params[mode] = arena.flat_param.detach().clone()
    assert torch.isfinite(params["none"]).all().item()
    assert not torch.equal(params["none"][:4096], torch.zeros_like(params["none"][:4096]))
    assert torch.equal(params["none"], params["block"])


# ---- memory ---------------------------------------------------------------------------------------------------------------------
GEO = (56, 14, 128, 8, 2, 64)          # 17 rows per frame, 8 blocks
FRAMES = 64


def _tower(mode, frames=FRAMES):
    from vimo_clip_amd.clip_vit import VisionTransformer
    from vimo_clip_amd.optim import GradArena
    torch.manual_seed(5)
    m = VisionTransformer(*GEO).cuda().train()
    m.recompute = mode
    arena = GradArena(m.parameters())                          # gradients have their place before anything is measured
    x = synth.randint_u8(43, "frames", (frames, 3, GEO[0], GEO[0])).cuda()
    return m, arena, x


def _fwd_bwd(m, x):
    from vimo_clip_amd.autograd_vit import vit_forward_train
    out = vit_forward_train(m, x)
    out.backward(torch.ones_like(out))


def _clean():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", ["none", "block"])
def test_byte_model_against_the_allocator(mode):
    from vimo_clip_amd.autograd_vit import vit_forward_train
    R, p, D, L, H, E = GEO
    F, N = FRAMES, (R // p) ** 2 + 1
    rows = F * N
    m, arena, x = _tower(mode)
    _fwd_bwd(m, x)                                             # 16-bit weight copies and workspaces exist from here on
    _clean()
    # a memory pool of its own: the forward's tensors are carved from fresh segments.  In the shared pool a request of 1 MiB or more
    # (z and u here) can be handed a free block left by earlier tests whole, with up to 1 MiB it did not ask for
    pool = torch.cuda.MemPool()
    base = torch.cuda.memory_allocated()
    with torch.cuda.use_mem_pool(pool):
        out = vit_forward_train(m, x)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - base
    model = saved_activation_bytes(GEO, F, mode)
    # outside the blocks: the patch rows (K = 3 p^2 padded to 64) of the patch GEMM, ln_pre's input with (mean, rstd), ln_post's
    # input (the class rows of the last block) with (mean, rstd), the projection's 16-bit input, the embeddings
    kpad = (3 * p * p + 63) // 64 * 64
    outside = F * (N - 1) * kpad * 2 + (rows * D * 4 + 2 * rows * 4) + (F * D * 4 + 2 * F * 4) + F * D * 2 + F * E * 4
    # tensors a block saves: x, mean, rstd (twice), ln_1 output, qkv, attention output, lse, ln_2 output, z, u: 13, and the gathered
    # class rows of the last block; one in "block" mode.  Nine outside.  The allocator rounds every one up to 512 B
    tensors = (13 * L + 1 if mode == "none" else L) + 9
    print(f"recompute={mode}: forward keeps {grown} B; byte model {model} B; upper bound {model + outside + 512 * tensors} B")
    assert model <= grown <= model + outside + 512 * tensors, (mode, grown, model, outside, tensors)
    del out, pool


# block / none, measured on the MI355X (profiles/student_recompute.md).  64 frames = 1088 rows: every weight gradient is a launch of
# its own.  128 frames = 2176 rows, whole 128-row pairs: the weight gradients are parked in wgrad_queue, whose operands must not pile up
PEAK_RATIO_MEASURED = {64: 0.3335, 128: 0.3548}


@pytest.mark.parametrize("frames", [64, 128])
def test_peak_memory_of_a_recomputed_step(frames):
    """Peak minus baseline over one forward + backward, "block" against "none".  The byte model gives (4 L + 36) / (36 L) = 0.236 at
    L = 8 (one stream per block plus one live block); transient dgrad and cast buffers come on top.  Bound: the measured ratio plus a
    tenth of it, and never above 0.5 (more would mean something is retained across blocks -- as the operands of parked weight-gradient
    problems were at 128 frames before _BlockFn flushed them per block)."""
    peak = {}
    for mode in ("none", "block"):
        m, arena, x = _tower(mode, frames)
        _fwd_bwd(m, x)
        _clean()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _fwd_bwd(m, x)
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated() - base
        del m, arena, x
    ratio = peak["block"] / peak["none"]
    print(f"{frames} frames, peak over a step: none {peak['none']} B, block {peak['block']} B, ratio {ratio:.4f}")
    bound = min(0.5, 1.1 * PEAK_RATIO_MEASURED[frames])
    assert ratio <= bound, (ratio, bound, peak)


# ---- gradient-ready hooks ------------------------------------------------------------------------------------------------------
def test_gradient_ready_hooks_fire_as_often_as_without_recomputation():
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.optim import GradArena
    name, shape = "ViT-tiny/32", (8, 16, 3, 64, 64)
    sd = synth.student_state_dict(name, 47)
    vids, teacher, labels = _inputs(47, shape, 64)
    counts = {}
    for mode in ("none", "block"):
        m = _student(name, 47, torch.bfloat16, mode, sd)
        arena = GradArena(m.parameters())
        names = {id(p): k for k, p in m.named_parameters()}
        fired = {}
        hook = lambda p: fired.__setitem__(names[id(p)], fired.get(names[id(p)], 0) + 1)      # noqa: E731
        ag.grad_ready_hooks.append(hook)
        try:
            _loss(m, vids, teacher, labels)[1].backward()
        finally:
            ag.grad_ready_hooks.remove(hook)
        assert not ag.wgrad_queue.items
        counts[mode] = fired
    assert set(counts["none"]) == {k for k, _ in m.named_parameters()}          # every parameter reported
    assert counts["none"] == counts["block"]


def _ddp_recompute_worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from vimo_clip_amd import autograd_ops, parallel
    from vimo_clip_amd.optim import GradArena
    dist.init_process_group("gloo")                            # two ranks share the one GPU: gloo instead of RCCL
    try:
        name, shape = "ViT-tiny/32", (8, 16, 3, 64, 64)
        sd = synth.student_state_dict(name, 53)
        vids, teacher, labels = _inputs(53 + rank, shape, 64)
        res = {}
        for mode in ("none", "block"):
            autograd_ops.grad_ready_hooks.clear()
            m = _student(name, 53, torch.bfloat16, mode, sd)
            arena = GradArena(m.parameters())
            red = parallel.GradientAllReducer(arena.flat_grad, bucket_bytes=256 * 1024).attach(arena)
            sent = []
            launch = red._launch
            red._launch = lambda b: (sent.append(b), launch(b))[1]
            for step in range(2):                              # the first step teaches the reducer its report counts
                del sent[:]
                _loss(m, vids, teacher, labels)[1].backward()
                red.all_reduce()
            torch.cuda.synchronize()
            res[mode] = (arena.flat_grad.cpu().clone(), sorted(sent), len(red.buckets), red.overlapped_last_step, dict(red._expected))
            red.detach()
        same = torch.equal(res["none"][0], res["block"][0])
        once = all(res[k][1] == list(range(res[k][2])) for k in res)            # every bucket sent exactly once in the learned step
        early = (res["none"][3], res["block"][3])
        counts = sorted(res["none"][4].values()) == sorted(res["block"][4].values())
        q.put((rank, same, once, early, counts, float(res["block"][0].double().abs().sum())))
    finally:
        dist.destroy_process_group()


def test_data_parallel_reducer_two_ranks_one_gpu():
    """A bucket reducer attached in a 2-rank job: after all_reduce() the arena of a "block" step equals the arena of a "none" step bit
    for bit, every bucket was sent once, and at least as many buckets left during the backward pass as without recomputation (the groups of a
    recomputed block leave at the end of the block, so no parameter reports later than in the per-op path)."""
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_recompute_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert [p.exitcode for p in procs] == [0, 0]
    assert all(r[1] for r in res), res                          # block == none after the exchange
    assert all(r[2] for r in res), res                          # every bucket once
    assert all(r[3][1] >= r[3][0] >= 1 for r in res), res       # buckets leave during the backward, none later than without recomputation
    assert all(r[4] for r in res), res                          # same report counts learned
    assert res[0][5] == res[1][5] and res[0][5] > 0, res        # the replicas hold the same sums


# ---- the full towers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", [("ViT-L/14", (1, 3, 3, 224, 224)), ("ViT-L/14@336px", (1, 2, 3, 336, 336))])
def test_full_tower_student_step_with_recomputation(name, shape):
    """One full-depth student step with recomputation (24 blocks): finite loss and gradients, and the two gradients that depend on
    every recomputed block equal the "none" run's."""
    m = _student(name, 2, torch.bfloat16, "none")
    vids, teacher, labels = _inputs(2, shape, 768)
    keys = ("visual_encoder.positional_embedding", "visual_encoder.transformer.resblocks.0.attn.in_proj_weight")
    params = dict(m.named_parameters())
    _loss(m, vids, teacher, labels)[1].backward()
    want = {k: params[k].grad.clone() for k in keys}
    for p in params.values():
        p.grad = None
    m.visual_encoder.recompute = "block"
    _, loss = _loss(m, vids, teacher, labels)
    loss.backward()
    assert torch.isfinite(loss).item()
    for k, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
    for k in keys:
        assert torch.equal(params[k].grad, want[k]), k
