"""GPU: the five drop-path kernels (vimo_clip_amd/csrc/drop_path.hip) against tests/drop_path_refs.py.

The sampler equals its CPU reference exactly.  The data kernels are called through the C ABI on buffers of this file's own: every
output is pre-filled with NaN and followed by a 64-element canary.  Gathered rows, dropped rows and every unscaled row are exact bits
(NaN payloads, -0 and subnormals included: those rows carry random bit patterns); a kept row is held to drop_path_refs.kept_bound,
derived there from the two-term fp32 sum and the store's half ulp."""
import numpy as np
import pytest
import torch

import drop_path_refs as R
import patch_dropout_ref as PR
from train_kernel_refs import BF16, DT_NAME, F16, F32

pytestmark = pytest.mark.gpu

E_ARG, E_ALIGN, E_SHAPE, E_DTYPE = -1, -2, -3, -4
CANARY = 64
INT_OF = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}


def _L():
    from vimo_clip_amd import _lib
    return _lib


def _call(name, *args):
    L = _L()
    rc = getattr(L.lib, name)(*args, L.stream())
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------------------------- the sampler
def _sample(seed_arg, block, F, K):
    L = _L()
    keep = torch.full((K + CANARY,), -7, dtype=torch.int32, device="cuda")
    slot = torch.full((F + CANARY,), -7, dtype=torch.int32, device="cuda")
    assert _call("vmc_drop_path_sample", seed_arg, block, F, K, L.ptr(keep), L.ptr(slot)) == 0
    assert (keep[K:] == -7).all().item() and (slot[F:] == -7).all().item()
    return keep[:K].cpu().numpy(), slot[:F].cpu().numpy()


@pytest.mark.parametrize("F", [1, 2, 17, 544, 1025, 8192])
def test_sampler_equals_the_reference(F):
    seed = 0x5EED0000 + F
    cell = torch.tensor([seed], dtype=torch.int64, device="cuda")
    for K in sorted({1, (F + 1) // 2, F}):
        for block in (0, 5):
            want_keep, want_slot = R.sample(seed, block, F, K)
            for arg in (seed, (1 << 63) | cell.data_ptr()):                # a value, and the address of one
                keep, slot = _sample(arg, block, F, K)
                assert np.array_equal(keep, want_keep) and np.array_equal(slot, want_slot), (F, K, block)
            assert (np.diff(keep) > 0).all() and keep[0] >= 0 and keep[-1] < F
            assert (slot[keep] == np.arange(K)).all() and (np.delete(slot, keep) == -1).all()


def test_sampler_is_the_ops_wrapper_and_every_call_gives_the_same_bits():
    from vimo_clip_amd import ops
    a = ops.drop_path_sample(99, 3, 544, 300, "cuda")
    b = ops.drop_path_sample(99, 3, 544, 300, "cuda")
    want = R.sample(99, 3, 544, 300)
    for got, again, w in zip(a, b, want):
        assert got.dtype == torch.int32 and torch.equal(got, again) and np.array_equal(got.cpu().numpy(), w)


def test_sampler_inclusion_is_uniform_within_the_binomial_tail():
    """256 seeds at F = 16, K = 8: every frame's inclusion count within the deviation any of the 16 counts reaches with probability
    at most 1e-6 under a uniform sampler (patch_dropout_ref.inclusion_deviation_bound)."""
    n, F, K = 256, 16, 8
    counts = np.zeros(F, dtype=np.int64)
    for i in range(n):
        counts[_sample((i + 1) * 0x9E3779B1, 1, F, K)[0]] += 1
    bound = PR.inclusion_deviation_bound(n, F, K)
    worst = np.abs(counts - n * K / F).max()
    print(f"inclusion counts {counts.tolist()}: largest deviation {worst:.0f}, bound {bound}")
    assert counts.sum() == n * K and worst < bound


def test_sampler_argument_checks():
    L = _L()
    keep = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    slot = torch.full((8200,), -7, dtype=torch.int32, device="cuda")
    call = lambda *a: _call("vmc_drop_path_sample", *a)
    assert call(1, 0, 8193, 4, L.ptr(keep), L.ptr(slot)) == E_SHAPE
    assert call(1, 0, 8, 0, L.ptr(keep), L.ptr(slot)) == E_SHAPE and call(1, 0, 8, 9, L.ptr(keep), L.ptr(slot)) == E_SHAPE
    assert call(1, 0, 8, 4, None, L.ptr(slot)) == E_ARG and call(1, 0, 8, 4, L.ptr(keep), None) == E_ARG
    assert call(1, -1, 8, 4, L.ptr(keep), L.ptr(slot)) == E_ARG
    assert (keep == -7).all().item() and (slot == -7).all().item()          # nothing was launched
    from vimo_clip_amd import ops
    with pytest.raises(ValueError, match="8192"):
        ops.drop_path_sample(1, 0, 8193, 4, "cuda")


# ---------------------------------------------------------------------------------------------- the data kernels
def _keep_for(F, K, seed):
    keep = np.sort(np.random.default_rng(seed).permutation(F)[:K]).astype(np.int32)
    return keep, R.slots(keep, F)


def _values(rows, row, dtype, gen):
    return (torch.randn(rows, row, generator=gen) * 2.0).to(dtype)


def _bits(rows, row, dtype, gen):
    """Random bit patterns: NaN payloads, infinities, -0 and subnormals among them."""
    info = torch.iinfo(INT_OF[dtype])
    return torch.randint(info.min, info.max + 1, (rows, row), generator=gen, dtype=torch.int64).to(INT_OF[dtype]).view(dtype)


def _out(rows, row, dtype, offset=0):
    """(buffer, view [rows, row] at `offset` elements): NaN where the kernel writes, a canary of 64 elements behind it."""
    buf = torch.full((offset + rows * row + CANARY,), float("nan"), dtype=dtype, device="cuda")
    buf[offset + rows * row:] = 12345.0
    return buf, buf[offset:offset + rows * row].view(rows, row)


def _canary_ok(buf, rows, row, offset=0):
    return (buf[offset + rows * row:] == 12345.0).all().item() and (offset == 0 or torch.isnan(buf[:offset]).all().item())


def _dev(t, offset=0):
    """t on the device, `offset` elements into a larger allocation (offset 1: no 16-byte alignment)."""
    buf = torch.empty(offset + t.numel(), dtype=t.dtype, device="cuda")
    buf[offset:].copy_(t.reshape(-1))
    return buf[offset:].view(t.shape)


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(INT_OF[a.dtype]), b.cpu().contiguous().view(INT_OF[b.dtype]))


def _ratio(got, want64, bound):
    err = (got.cpu().to(torch.float64) - want64).abs()
    assert torch.isfinite(err).all()
    return float((err / bound).max()) if err.numel() else 0.0


PAIRS = [(1, 1), (5, 1), (5, 4), (5, 5), (64, 1), (64, 63), (64, 64)]           # F in {1, 5, 64}, K in {1, F - 1, F}
ROWS = [8, 37, 408, 6400]          # 37: unaligned rows, the element path; 6400: a row longer than one workgroup pass
DATA_CFG = [(dt, row) for dt in (F32, BF16, F16) for row in ROWS]
DATA_ID = lambda v: DT_NAME.get(v, str(v)) if not isinstance(v, int) else str(v)


def _run_all(dtype, row, F, K, offset=0):
    """The four data kernels on one shape; returns the worst error / bound ratio of the kept rows."""
    L = _L()
    p = L.ptr
    gen = torch.Generator().manual_seed(F * 1000 + K * 10 + row)
    keep, slot = _keep_for(F, K, F * 131 + K)
    keep_d, slot_d = torch.from_numpy(keep).cuda(), torch.from_numpy(slot).cuda()
    kept = torch.from_numpy(slot >= 0)
    c, s = R.scales(F, K)
    dt = L.dt(dtype)
    worst = 0.0
    # gather: bit copies of random bit patterns
    src = _bits(F, row, dtype, gen)
    buf, dst = _out(K, row, dtype, offset)
    assert _call("vmc_frame_gather", p(_dev(src, offset)), p(keep_d), p(dst), F, K, row, dt) == 0
    assert _same_bits(dst, R.gather(src, keep)) and _canary_ok(buf, K, row, offset)
    # merge: dropped rows carry bit patterns and come out as they went in
    x, y = _values(F, row, dtype, gen), _values(K, row, dtype, gen)
    x[~kept] = _bits(int((~kept).sum()), row, dtype, gen)
    buf, out = _out(F, row, dtype, offset)
    assert _call("vmc_drop_path_merge", p(_dev(x, offset)), p(_dev(y, offset)), p(slot_d), p(out), F, row, c, s, dt) == 0
    xz = torch.where(kept[:, None], x, torch.zeros_like(x))                 # the reference never reads the dropped rows' patterns
    want, mag, _ = R.merge(xz, y, slot, c, s)
    assert _same_bits(out[~kept], x[~kept]) and _canary_ok(buf, F, row, offset)
    worst = max(worst, _ratio(out[kept], want[kept], R.kept_bound(want[kept], mag[kept], dtype)))
    # merge backward: one launch writes dx and dy
    dout = _values(F, row, dtype, gen)
    dout[~kept] = _bits(int((~kept).sum()), row, dtype, gen)
    bufx, dx = _out(F, row, dtype, offset)
    bufy, dy = _out(K, row, dtype, offset)
    assert _call("vmc_drop_path_merge_bwd", p(_dev(dout, offset)), p(keep_d), p(slot_d), p(dx), p(dy), F, K, row, c, s, dt) == 0
    dz = torch.where(kept[:, None], dout, torch.zeros_like(dout))
    wdx, mdx, _, wdy, mdy = R.merge_bwd(dz, keep, slot, c, s)
    assert _same_bits(dx[~kept], dout[~kept]) and _canary_ok(bufx, F, row, offset) and _canary_ok(bufy, K, row, offset)
    worst = max(worst, _ratio(dx[kept], wdx[kept], R.kept_bound(wdx[kept], mdx[kept], dtype)),
                _ratio(dy, wdy, R.kept_bound(wdy, mdy, dtype)))
    # scatter-add: the gather's backward
    dpass, dsub = _values(F, row, dtype, gen), _values(K, row, dtype, gen)
    dpass[~kept] = _bits(int((~kept).sum()), row, dtype, gen)
    buf, dxs = _out(F, row, dtype, offset)
    assert _call("vmc_frame_scatter_add", p(_dev(dpass, offset)), p(_dev(dsub, offset)), p(slot_d), p(dxs), F, row, dt) == 0
    pz = torch.where(kept[:, None], dpass, torch.zeros_like(dpass))
    want, mag, _ = R.scatter_add(pz, dsub, slot)
    assert _same_bits(dxs[~kept], dpass[~kept]) and _canary_ok(buf, F, row, offset)
    return max(worst, _ratio(dxs[kept], want[kept], R.kept_bound(want[kept], mag[kept], dtype)))


@pytest.mark.parametrize("dtype,row", DATA_CFG, ids=DATA_ID)
def test_data_kernels(dtype, row):
    worst = max(_run_all(dtype, row, F, K) for F, K in PAIRS)
    print(f"{DT_NAME[dtype]} row {row}: worst error / bound of a kept row {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=DATA_ID)
def test_data_kernels_on_pointers_without_16_byte_alignment(dtype):
    """Rows of 8 and 408 elements would take 16-byte accesses; one element into an allocation they may not."""
    worst = max(_run_all(dtype, row, 5, 4, offset=1) for row in (8, 408))
    print(f"{DT_NAME[dtype]} offset pointers: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_wrappers_are_the_entries_and_f32_merge_bits_do_not_depend_on_the_call():
    from vimo_clip_amd import ops
    gen = torch.Generator().manual_seed(5)
    F, K, row = 5, 3, 408
    keep, slot = _keep_for(F, K, 3)
    keep_d, slot_d = torch.from_numpy(keep).cuda(), torch.from_numpy(slot).cuda()
    x, y = _values(F, row, F32, gen).cuda(), _values(K, row, F32, gen).cuda()
    s = F / K
    c32, s32 = R.scales(F, K)
    a, b = ops.drop_path_merge(x, y, slot_d, s), ops.drop_path_merge(x, y, slot_d, s)
    want, mag, kept = R.merge(x.cpu(), y.cpu(), slot, c32, s32)
    assert torch.equal(a, b) and _ratio(a, want, R.kept_bound(want, mag, F32)) <= 1.0
    assert torch.equal(ops.frame_gather(x, keep_d), x[keep_d.long()])
    dx, dy = ops.drop_path_merge_bwd(x, keep_d, slot_d, s)
    assert dx.shape == x.shape and dy.shape == y.shape and torch.equal(dx[~kept.cuda()], x[~kept.cuda()])
    assert torch.equal(ops.frame_scatter_add(x, y, slot_d)[~kept.cuda()], x[~kept.cuda()])


def test_data_kernel_argument_checks():
    """One bad argument of each kind per entry: NULL -> ARG, a count out of range -> SHAPE, a pointer off its element size -> ALIGN, an
    unknown dtype -> DTYPE; nothing is launched (the outputs keep their NaN)."""
    L = _L()
    p = L.ptr
    F, K, row = 4, 2, 8
    x = torch.zeros((F, row), dtype=torch.float32, device="cuda")
    y = torch.zeros((K, row), dtype=torch.float32, device="cuda")
    outF = torch.full((F, row), float("nan"), dtype=torch.float32, device="cuda")
    outK = torch.full((K, row), float("nan"), dtype=torch.float32, device="cuda")
    keep, slot = torch.tensor([0, 2], dtype=torch.int32, device="cuda"), torch.tensor([0, -1, 1, -1], dtype=torch.int32, device="cuda")
    f32 = L.F32
    g = lambda *a: _call("vmc_frame_gather", *a)
    assert g(None, p(keep), p(outK), F, K, row, f32) == E_ARG and g(p(x), p(keep), p(outK), F, K, 0, f32) == E_ARG
    assert g(p(x), p(keep), p(outK), F, 0, row, f32) == E_SHAPE and g(p(x), p(keep), p(outK), F, F + 1, row, f32) == E_SHAPE
    assert g(p(x) + 2, p(keep), p(outK), F, K, row, f32) == E_ALIGN and g(p(x), p(keep), p(outK), F, K, row, 7) == E_DTYPE
    sa = lambda *a: _call("vmc_frame_scatter_add", *a)
    assert sa(p(x), None, p(slot), p(outF), F, row, f32) == E_ARG and sa(p(x), p(y), p(slot), p(outF), 0, row, f32) == E_SHAPE
    assert sa(p(x), p(y), p(slot), p(outF) + 1, F, row, f32) == E_ALIGN and sa(p(x), p(y), p(slot), p(outF), F, row, -1) == E_DTYPE
    m = lambda *a: _call("vmc_drop_path_merge", *a)
    assert m(p(x), p(y), None, p(outF), F, row, -1.0, 2.0, f32) == E_ARG and m(p(x), p(y), p(slot), p(outF), 0, row, -1.0, 2.0, f32) == E_SHAPE
    assert m(p(x), p(y) + 2, p(slot), p(outF), F, row, -1.0, 2.0, f32) == E_ALIGN
    assert m(p(x), p(y), p(slot), p(outF), F, row, -1.0, 2.0, 3) == E_DTYPE
    mb = lambda *a: _call("vmc_drop_path_merge_bwd", *a)
    assert mb(p(x), p(keep), p(slot), p(outF), None, F, K, row, -1.0, 2.0, f32) == E_ARG
    assert mb(p(x), p(keep), p(slot), p(outF), p(outK), F, F + 1, row, -1.0, 2.0, f32) == E_SHAPE
    assert mb(p(x), p(keep), p(slot), p(outF), p(outK), F, 0, row, -1.0, 2.0, f32) == E_SHAPE
    assert mb(p(x) + 1, p(keep), p(slot), p(outF), p(outK), F, K, row, -1.0, 2.0, f32) == E_ALIGN
    assert mb(p(x), p(keep), p(slot), p(outF), p(outK), F, K, row, -1.0, 2.0, 9) == E_DTYPE
    assert m(p(x), p(y), p(slot), p(outF), F, row, -1.0, 2.0, f32) == 0          # and the valid call goes through
    assert not torch.isnan(outF).any().item() and torch.isnan(outK).all().item()
