"""CPU: gradient accumulation over micro-batches -- the numpy reference of vmc_grad_accumulate (tests/grad_accum_ref.py), the
micro-batch split of the student trainer, the GradArena / FusedAdam state machine with the launch replaced by the reference, the
command lines, and a gloo world-2 run of the reducer's no_sync() with an arena on CPU tensors."""
import os
import re
import socket
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import grad_accum_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _data(n, seed):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(np.float32)
    acc = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(np.float32)
    return g, acc


def _round_f32(x: Fraction) -> np.float32:
    """Correctly rounded (nearest, ties to even) fp32 of an exact rational in the normal range."""
    if x == 0:
        return np.float32(0.0)
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = 0
    while x >= 2:
        x, e = x / 2, e + 1
    while x < 1:
        x, e = x * 2, e - 1
    scaled = x * 2 ** 23                                   # in [2^23, 2^24)
    q, r = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * r
    if twice > scaled.denominator or (twice == scaled.denominator and q % 2):
        q += 1
    return np.float32(sign * float(Fraction(q) * Fraction(2) ** (e - 23)))


@pytest.mark.parametrize("w", [1.0, 0.5, 0.25, -2.0])
def test_reference_power_of_two_weights_equal_sequential_fp32_and_the_exact_fma(w):
    g, acc = _data(600, 3)
    w32 = np.float32(w)
    assert R.is_power_of_two(w)
    assert np.array_equal(R.grad_accumulate_ref(g, acc, w, 0), w32 * g)
    seq = acc + w32 * g
    assert seq.dtype == np.float32
    for mode in (1, 2):
        got = R.grad_accumulate_ref(g, acc, w, mode)
        assert got.dtype == np.float32 and np.array_equal(got, seq)
    exact = np.array([_round_f32(Fraction(float(w32)) * Fraction(float(a)) + Fraction(float(b))) for a, b in zip(g, acc)])
    assert np.array_equal(seq, exact)                      # one rounding of the exact value: what fmaf returns


@pytest.mark.parametrize("w", [0.375, 1.0 / 3.0])
def test_reference_other_weights_are_float64_rounded_and_within_one_ulp_of_the_exact_fma(w):
    g, acc = _data(600, 5)
    w32 = np.float32(w)
    assert not R.is_power_of_two(w32)
    got = R.grad_accumulate_ref(g, acc, w, 1)
    assert np.array_equal(got, (acc.astype(np.float64) + np.float64(w32) * g.astype(np.float64)).astype(np.float32))
    assert np.array_equal(R.grad_accumulate_ref(g, acc, w, 0), (np.float64(w32) * g.astype(np.float64)).astype(np.float32))
    exact = np.array([_round_f32(Fraction(float(w32)) * Fraction(float(a)) + Fraction(float(b))) for a, b in zip(g, acc)])
    assert R.ulp_distance(got, exact).max() <= 1


def test_reference_propagates_inf_and_nan_and_ulp_distance():
    g = np.array([np.inf, -np.inf, np.nan, 1.0], dtype=np.float32)
    acc = np.array([1.0, np.inf, 0.0, np.nan], dtype=np.float32)
    out = R.grad_accumulate_ref(g, acc, 0.5, 2)
    assert out[0] == np.inf and np.isnan(out[1:]).all()
    one = np.float32(1.0)
    assert R.ulp_distance([one, -one, 0.0, np.nan], [np.nextafter(one, np.float32(2)), -one, -0.0, np.nan]).tolist() == [1, 0, 0, 0]
    assert R.ulp_distance([np.nan], [1.0])[0] > 1


# ---- the micro-batch split ----------------------------------------------------------------------------------------------------------
def _batch(B):
    return {"video_id": [f"v{i}" for i in range(B)], "rgb_emb": torch.arange(B * 3 * 2, dtype=torch.float32).view(B, 3, 2),
            "flow_frames": torch.arange(B * 2, dtype=torch.uint8).view(B, 2), "labels": torch.arange(B * 4.0).view(B, 4)}


@pytest.mark.parametrize("B,n", [(8, 2), (8, 4), (8, 3), (7, 4), (5, 2), (3, 8), (6, 5), (1, 4)])
def test_split_micro_batches_follows_torch_chunk(B, n):
    from vimo_clip_amd.train import split_micro_batches
    batch = _batch(B)
    micro = split_micro_batches(batch, n)
    want = torch.chunk(batch["labels"], n, dim=0)
    assert len(micro) == len(want) <= n
    assert sum(w for _, w in micro) == pytest.approx(1.0, abs=1e-12)
    start = 0
    for (sub, w), ref in zip(micro, want):
        k = ref.shape[0]
        assert w == k / B
        assert torch.equal(sub["labels"], ref)
        for key in ("rgb_emb", "flow_frames"):
            assert torch.equal(sub[key], batch[key][start:start + k])
        assert sub["video_id"] == batch["video_id"][start:start + k]
        start += k
    assert start == B


def test_split_micro_batches_edges():
    from vimo_clip_amd.train import split_micro_batches
    batch = _batch(4)
    (sub, w), = split_micro_batches(batch, 1)
    assert sub is batch and w == 1.0
    assert len(split_micro_batches(batch, 9)) == 4                      # more micro-steps than clips: one clip each
    with pytest.raises(ValueError):
        split_micro_batches(batch, 0)


def test_accum_steps_on_the_command_lines():
    from vimo_clip_amd import train, train_frame_diff_mn
    p = train.build_parser()
    assert p.parse_args([]).accum_steps == 1
    assert p.parse_args(["--accum_steps", "4", "--recompute", "block", "--grad_clip_norm", "1.0"]).accum_steps == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--accum_steps", "two"])
    for bad in ("0", "-2"):                                              # refused before anything touches a device
        with pytest.raises(ValueError, match="accum_steps"):
            train.train(p.parse_args(["--accum_steps", bad]))
    need = ["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c"]
    q = train_frame_diff_mn.build_parser()
    assert q.parse_args(need).accum_steps == 1
    assert q.parse_args(need + ["--accum_steps", "3"]).accum_steps == 3 and q.parse_args(need + ["--accum-steps", "2"]).accum_steps == 2


# ---- the arena's state machine, launch replaced by the reference ------------------------------------------------------------------
def _reference_launch(calls):
    def launch(self, mode, weight):
        calls.append((mode, float(weight)))
        g, acc = self.flat_grad.numpy(), self.flat_acc.numpy()
        res = R.grad_accumulate_ref(g.copy(), acc.copy(), weight, mode)
        (g if mode == 2 else acc)[...] = res
    return launch


@pytest.fixture
def arena_calls(monkeypatch):
    from vimo_clip_amd.optim import GradArena
    calls = []
    monkeypatch.setattr(GradArena, "_launch_accumulate", _reference_launch(calls))
    params = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i))) for i, s in enumerate([(5, 7), (130,), (3,)])]
    return GradArena(params), calls


def _fill(arena, seed):
    g = torch.randn(arena.numel, generator=torch.Generator().manual_seed(seed))
    arena.flat_grad.copy_(g)
    return g


def test_arena_first_middle_final_sequence(arena_calls):
    arena, calls = arena_calls
    assert arena.pending == 0 and arena.flat_acc is None
    ws = (0.5, 0.25, 0.25)
    gs = []
    for j, w in enumerate(ws):
        gs.append(_fill(arena, 10 + j))
        arena.accumulate(w, final=j == 2)
        assert arena.pending == (j + 1 if j < 2 else 0)
    assert calls == [(0, 0.5), (1, 0.25), (2, 0.25)]
    want = (gs[0] * 0.5 + gs[1] * 0.25) + gs[2] * 0.25                     # power-of-two weights: sequential fp32, bit for bit
    assert torch.equal(arena.flat_grad, want)
    assert torch.equal(arena.params[1].grad, want[arena.offsets[1]:arena.offsets[1] + 130])      # .grad views see the sum
    # a second round starts with mode 0 again: nothing of the first one leaks
    del calls[:]
    g0 = _fill(arena, 20)
    arena.accumulate(0.5)
    g1 = _fill(arena, 21)
    arena.accumulate(0.5, final=True)
    assert calls == [(0, 0.5), (2, 0.5)] and torch.equal(arena.flat_grad, g0 * 0.5 + g1 * 0.5)


def test_arena_final_with_nothing_pending(arena_calls):
    arena, calls = arena_calls
    g = _fill(arena, 1)
    arena.accumulate(final=True)
    arena.accumulate(1.0, final=True)
    assert calls == [] and arena.flat_acc is None and torch.equal(arena.flat_grad, g)      # the plain path: nothing launched or allocated
    arena.accumulate(0.5, final=True)                                      # a weight on a single micro-step still applies
    assert arena.pending == 0 and torch.equal(arena.flat_grad, g * 0.5)


def test_arena_zero_grad_drops_a_pending_accumulation(arena_calls):
    arena, calls = arena_calls
    _fill(arena, 1)
    arena.accumulate(0.5)
    assert arena.pending == 1
    arena.zero_grad()
    assert arena.pending == 0 and not arena.flat_grad.any()
    g = _fill(arena, 2)
    arena.accumulate(0.5)
    arena.accumulate(0.5, final=True)
    assert [m for m, _ in calls] == [0, 0, 2]                              # mode 0 again: the dropped micro-step is not in the sum
    assert torch.equal(arena.flat_grad, g * 0.5 + g * 0.5)


def test_optimizer_step_raises_on_a_pending_accumulation(arena_calls):
    from vimo_clip_amd.optim import FusedAdam
    arena, _ = arena_calls
    opt = FusedAdam(arena, lr=1e-3)
    before = arena.flat_param.clone()
    _fill(arena, 1)
    arena.accumulate(0.5)
    with pytest.raises(RuntimeError, match=r"accumulate\(.*final=True\)"):
        opt.step()
    assert opt.step_count == 0 and torch.equal(arena.flat_param, before)
    opt.zero_grad()                                                        # the optimiser's zero_grad is a no-op: still pending
    assert arena.pending == 1


def test_backward_overlap_and_accumulation_exclude_each_other(arena_calls, monkeypatch):
    from vimo_clip_amd.optim import FusedAdam
    arena, calls = arena_calls
    opt = FusedAdam(arena, lr=1e-3)
    monkeypatch.setattr(torch.cuda, "Stream", lambda **kw: object())       # no device here: only the bookkeeping is under test
    _fill(arena, 1)
    arena.accumulate(0.5)
    with pytest.raises(RuntimeError, match="pending gradient accumulation"):
        opt.enable_backward_overlap([[arena.params[0]]])
    arena.accumulate(0.5, final=True)
    opt.enable_backward_overlap([[arena.params[0]]])
    n = len(calls)
    for kw in ({}, {"final": True}):
        with pytest.raises(RuntimeError, match="enable_backward_overlap"):
            arena.accumulate(0.5, **kw)
    assert len(calls) == n and arena.pending == 0
    arena.accumulate(final=True)                                           # the no-op stays a no-op
    opt.disable_backward_overlap()
    arena.accumulate(0.5)
    assert arena.pending == 1


def test_kernel_resource_usage_reports_no_scratch():
    """The Makefile keeps hipcc's resource-usage remarks of grad_accum.hip: a streaming pass has no business spilling."""
    path = os.path.join(ROOT, "vimo_clip_amd", "csrc", "build", "grad_accum.usage.txt")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    blocks = re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]
    kernels = [b for b in blocks if "grad_accum_kernel" in b.split()[0]]
    assert len(kernels) == 3
    for b in kernels:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 0


# ---- data parallelism: no_sync() around the micro-steps, gloo, world 2 -------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _no_sync_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from vimo_clip_amd import parallel
    from vimo_clip_amd.optim import GradArena
    parallel.init_from_env("gloo")
    try:
        calls = []
        GradArena._launch_accumulate = _reference_launch(calls)
        sizes = [300, 5000, 64, 9000, 128, 4096, 700]        # as tests/test_parallel_cpu.py: parameters straddle 4096-element buckets
        arena = GradArena([torch.nn.Parameter(torch.zeros(n)) for n in sizes])
        g = arena.flat_grad
        red = parallel.GradientAllReducer(g, bucket_bytes=4096 * 4).attach(arena, register=False)
        issued = []
        issue = red._issue
        red._issue = lambda b: (issued.append(b), issue(b))[1]
        index = torch.arange(arena.numel, dtype=torch.float32) % 17

        def backward(value, skip=()):
            g.copy_(index + value)                              # rank-dependent "gradient", exact in fp32
            for i in reversed(range(len(sizes))):
                if i not in skip:
                    red.on_grad_ready(arena.params[i])

        def plain_step(step, overlapped):
            del issued[:]
            backward(float(rank + 1) * (step + 1))
            assert red.all_reduce() == 0.5
            assert torch.equal(g, 2 * index + 3.0 * (step + 1))
            early = red.overlapped_last_step
            assert (early >= len(red.buckets) - 1) if overlapped else early == 0, (step, early)
            assert sorted(issued) == list(range(len(red.buckets)))

        plain_step(0, False)                                   # learns the report counts
        plain_step(1, True)
        expected = dict(red._expected)
        weights = (0.5, 0.25, 0.25)
        for rounds in range(2):                                # two accumulated steps in a row
            del issued[:]
            for j, w in enumerate(weights):
                with red.no_sync():
                    backward(float((rank + 1) * (j + 1)))
                    assert issued == [] and red._pending == [] and red._counts == {} and red._expected == expected
                    try:
                        red.all_reduce()
                        raise AssertionError("all_reduce() inside no_sync() did not raise")
                    except RuntimeError as e:
                        assert "no_sync" in str(e)
                assert issued == []
                arena.accumulate(w, final=j == len(weights) - 1)
            assert arena.pending == 0 and [m for m, _ in calls[-3:]] == [0, 1, 2]
            assert red.all_reduce() == 0.5
            assert red.overlapped_last_step == 0 and sorted(issued) == list(range(len(red.buckets)))     # one exchange, not overlapped
            # sum over ranks r = 1, 2 of sum_j w_j (index + r (j + 1)) = 2 index + 3 * (0.5 * 1 + 0.25 * 2 + 0.25 * 3)
            assert torch.equal(g, 2 * index + 3.0 * 1.75), g[:5]
        both = [torch.empty_like(g) for _ in range(world)]
        dist.all_gather(both, g)
        assert torch.equal(both[0], both[1])                   # replicas identical
        plain_step(2, True)                                    # the steps after it overlap again
        plain_step(3, True)
        q.put((rank, True))
    finally:
        dist.destroy_process_group()


def _no_sync_first_worker(rank, world, port, q):
    """A reducer whose first backward passes all ran under no_sync() must still learn its report counts afterwards."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from vimo_clip_amd import parallel
    from vimo_clip_amd.optim import GradArena
    parallel.init_from_env("gloo")
    try:
        arena = GradArena([torch.nn.Parameter(torch.zeros(n)) for n in (5000, 9000, 4096)])
        red = parallel.GradientAllReducer(arena.flat_grad, bucket_bytes=4096 * 4).attach(arena, register=False)
        early = []
        for step in range(4):
            arena.flat_grad.fill_(float(rank + 1))
            if step == 0:
                with red.no_sync():
                    for p in reversed(arena.params):
                        red.on_grad_ready(p)
            else:
                for p in reversed(arena.params):
                    red.on_grad_ready(p)
            red.all_reduce()
            assert torch.all(arena.flat_grad == 3.0)
            early.append(red.overlapped_last_step)
        assert early[:2] == [0, 0] and min(early[2:]) >= len(red.buckets) - 1, early
        q.put((rank, True))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("worker", [_no_sync_worker, _no_sync_first_worker], ids=["accumulate", "no_sync_first"])
def test_no_sync_gloo_world2(worker):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert [p.exitcode for p in procs] == [0, 0]
    assert sorted(q.get(timeout=10) for _ in procs) == [(0, True), (1, True)]


def test_no_sync_does_not_nest_and_rearms_at_world_size_one():
    from vimo_clip_amd import parallel
    red = parallel.GradientAllReducer(torch.zeros(256))
    with red.no_sync():
        with pytest.raises(RuntimeError, match="nest"):
            with red.no_sync():
                pass
        with pytest.raises(RuntimeError, match="no_sync"):
            red.all_reduce()
    assert red.all_reduce() == 1.0
