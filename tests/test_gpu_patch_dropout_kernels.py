"""GPU: the four patch-dropout stem kernels (vimo_clip_amd/csrc/patch_dropout.hip) against tests/patch_dropout_ref.py.

The sampler, the row gather, the forward assembly and the 16-bit patch gradient are integer or single-rounding operations: bit
equality.  dcls / dpos are fp32 sums over the frames: each element within F 2^-23 sum_f |addend| of the float64 sum (the fp32
reassociation bound, addends taken from the inputs), exact zeros where no frame kept the position, the same bits on a second run.
Every output is a whole allocation with sentinel rows behind it that must survive; workspaces and outputs start as NaN."""
import numpy as np
import pytest
import torch

import patch_dropout_ref as PR
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_ARG, E_ALIGN, E_SHAPE, E_DTYPE = -1, -2, -3, -4
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT16 = (BF16, F16)
GUARD = 2          # sentinel rows behind every output
SENT = -1536.0     # exact in bf16 and f16


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vimo_clip_amd import _lib
    return _lib


def _keeps(seed, F, G, Kp):
    """Per-frame different keep sets from the reference sampler (asserted different where that is possible)."""
    keep = PR.keep_sample(seed, F, G, Kp)
    if Kp < G and F > 1:
        assert len({tuple(r) for r in keep}) > 1
    return keep


def _bits(a):
    return a.contiguous().view(torch.int32 if a.dtype is F32 else torch.int16)


def _guarded(rows, cols, dtype):
    return torch.full((rows + GUARD, cols), SENT, dtype=dtype, device=DEV)


def _guard_intact(buf, rows):
    return bool((buf[rows:].float() == SENT).all().item())


# ---------------------------------------------------------------------------------------------- sampler
SAMPLER_CASES = [(3, 16, 4), (3, 49, 24), (2, 576, 144), (2, 16, 16), (2, 16, 1)]


@pytest.mark.parametrize("F,G,Kp", SAMPLER_CASES, ids=lambda v: str(v))
def test_sampler_matches_the_reference(L, F, G, Kp):
    from vimo_clip_amd import ops
    for seed in (1, 0x0123456789ABCDEF, (1 << 63) - 1):
        want = PR.keep_sample(seed, F, G, Kp)
        got = ops.patch_keep_sample(seed, F, G, Kp, DEV)
        assert got.dtype == torch.int32 and tuple(got.shape) == (F, Kp)
        assert np.array_equal(got.cpu().numpy(), want), (seed, F, G, Kp)
        # the same seed through a device address (bit 63 set): what a captured step passes
        cell = torch.tensor([seed, 0], dtype=torch.int64, device=DEV)
        buf = torch.full((F + GUARD, Kp), -7, dtype=torch.int32, device=DEV)
        assert L.lib.vmc_patch_keep_sample((1 << 63) | cell.data_ptr(), F, G, Kp, L.ptr(buf), L.stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(buf[:F].cpu().numpy(), want) and bool((buf[F:] == -7).all().item())
    # a stored seed with bit 63 set is a value like any other once it is read from memory
    big = 0xF123456789ABCDEF
    cell = torch.tensor([big - (1 << 64)], dtype=torch.int64, device=DEV)
    got = ops.patch_keep_sample((1 << 63) | cell.data_ptr(), F, G, Kp, DEV)
    assert np.array_equal(got.cpu().numpy(), PR.keep_sample(big, F, G, Kp))


def test_sampler_error_codes(L):
    keep = torch.zeros((2, 1024), dtype=torch.int32, device=DEV)
    call = lambda F, G, Kp, p=L.ptr(keep): L.lib.vmc_patch_keep_sample(5, F, G, Kp, p, L.stream())      # noqa: E731
    assert call(2, 16, 17) == E_SHAPE                  # Kp > G
    assert call(2, 1025, 4) == E_SHAPE                 # G > 1024
    assert call(2, 16, 0) == E_SHAPE
    assert call(0, 16, 4) == E_ARG
    assert call(2, 16, 4, None) == E_ARG
    assert call(2, 1024, 1024) == 0                    # the largest frame there is
    torch.cuda.synchronize()
    assert np.array_equal(keep.cpu().numpy(), np.tile(np.arange(1024, dtype=np.int32), (2, 1)))


# ---------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("cols,ld_pad", [(3072, 0), (640, 0), (1280, 0), (640, 8), (20, 0), (24, 4)], ids=lambda v: str(v))
def test_gather_rows_is_a_bit_copy(L, cols, ld_pad):
    """cols = 3072 (ViT-B/32), 640 and 2 x 640 (p = 14: kpad and the [v | v] layout); a padded source stride; and rows that are not
    16-byte pieces (cols % 8 != 0, stride % 8 != 0), which take the element-wise kernel.  The rows are raw bit patterns, NaNs included."""
    F, G, Kp = 3, 16, 4
    keep = _keeps(21, F, G, Kp)
    raw = synth.randint(cols, "gather", (F * G, cols + ld_pad), -32768, 32768).to(torch.int16)
    src = raw.view(BF16).to(DEV)[:, :cols]
    assert src.stride(0) == cols + ld_pad
    dst = _guarded(F * Kp, cols, BF16)
    keep_d = torch.from_numpy(keep).to(DEV)
    rc = L.lib.vmc_gather_rows16(L.ptr(src), src.stride(0), L.ptr(keep_d), G, L.ptr(dst), cols, cols, F, Kp, L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    want = PR.gather_rows(raw[:, :cols].numpy(), keep, G)
    assert np.array_equal(dst[:F * Kp].cpu().view(torch.int16).numpy(), want)
    assert _guard_intact(dst, F * Kp)


def test_gather_wrapper_and_error_codes(L):
    from vimo_clip_amd import ops
    F, G, Kp, cols = 2, 16, 16, 64
    src = synth.normal(3, "g", (F * G, cols)).to(F16).to(DEV)
    ident = torch.arange(G, dtype=torch.int32, device=DEV).repeat(F, 1)
    assert torch.equal(ops.gather_rows16(src, ident, G), src)                       # every patch: the identity
    p = L.ptr
    out = torch.zeros_like(src)
    call = lambda *a: L.lib.vmc_gather_rows16(*a, L.stream())                       # noqa: E731
    assert call(p(src), cols, p(ident), G, p(out), cols, cols, F, G + 1) == E_SHAPE
    assert call(p(src), cols - 8, p(ident), G, p(out), cols, cols, F, Kp) == E_SHAPE
    assert call(p(src), cols, p(ident), G, p(out), cols - 8, cols, F, Kp) == E_SHAPE
    assert call(None, cols, p(ident), G, p(out), cols, cols, F, Kp) == E_ARG
    assert call(p(src), cols, p(ident), G, p(out), cols, cols, 0, Kp) == E_ARG


# ---------------------------------------------------------------------------------------------- assembly, forward
ASM_CASES = [(D, Kp) for D in (128, 768) for Kp in (4, 9)] + [(20, 4)]      # D = 20: rows that are no 16-byte pieces


def _asm_inputs(D, Kp, dt16, F=3, G=16):
    keep = _keeps(100 + D + Kp, F, G, Kp)
    xp = synth.normal(D + Kp, "xp", (F * Kp, D)).to(dt16)
    cls = synth.normal(D + Kp, "cls", (D,), std=0.5)
    pos = synth.normal(D + Kp, "pos", (G + 1, D), std=0.5)
    return keep, xp, cls, pos


@pytest.mark.parametrize("dt16", DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("res_f32", [True, False], ids=["res32", "res16"])
@pytest.mark.parametrize("D,Kp", ASM_CASES, ids=lambda v: str(v))
def test_assemble_keep_forward_is_bit_exact(L, D, Kp, res_f32, dt16):
    F, G = 3, 16
    keep, xp, cls, pos = _asm_inputs(D, Kp, dt16)
    out_dtype = F32 if res_f32 else dt16
    want = PR.assemble_keep(xp, cls, pos, keep, out_dtype)
    x = _guarded(F * (Kp + 1), D, out_dtype)
    xp_d, cls_d, pos_d, keep_d = xp.to(DEV), cls.to(DEV), pos.to(DEV), torch.from_numpy(keep).to(DEV)      # alive until the synchronise
    rc = L.lib.vmc_assemble_tokens_keep(L.ptr(xp_d), L.ptr(cls_d), L.ptr(pos_d), L.ptr(keep_d), L.ptr(x), F, G, Kp, D, L.dt(out_dtype),
                                        L.dt(dt16), L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(_bits(x[:F * (Kp + 1)].cpu()), _bits(want))
    assert _guard_intact(x, F * (Kp + 1))


def test_assemble_keep_equals_assemble_tokens_when_everything_is_kept(L):
    """Kp = G with the identity keep: the bits of vmc_assemble_tokens."""
    from vimo_clip_amd import ops
    F, G, D = 3, 16, 128
    for dt16 in DT16:
        for out_dtype in (F32, dt16):
            xp = synth.normal(9, "xp", (F * G, D)).to(dt16).to(DEV)
            cls, pos = synth.normal(9, "cls", (D,)).to(DEV), synth.normal(9, "pos", (G + 1, D)).to(DEV)
            ref = torch.empty((F * (G + 1), D), dtype=out_dtype, device=DEV)
            assert L.lib.vmc_assemble_tokens(L.ptr(xp), L.ptr(cls), L.ptr(pos), L.ptr(ref), F, G + 1, D, L.dt(out_dtype), L.dt(dt16),
                                             L.stream()) == 0
            ident = torch.arange(G, dtype=torch.int32, device=DEV).repeat(F, 1)
            assert torch.equal(_bits(ops.assemble_tokens_keep(xp, cls, pos, ident, out_dtype)), _bits(ref))


def test_assemble_keep_error_codes(L):
    F, G, Kp, D = 2, 16, 4, 64
    xp = torch.zeros((F * Kp, D), dtype=BF16, device=DEV)
    cls, pos = torch.zeros(D, device=DEV), torch.zeros((G + 1, D), device=DEV)
    keep = torch.zeros((F, Kp), dtype=torch.int32, device=DEV)
    x = torch.zeros((F * (Kp + 1), D), device=DEV)
    p = L.ptr
    call = lambda *a: L.lib.vmc_assemble_tokens_keep(*a, L.stream())                 # noqa: E731
    assert call(p(xp), p(cls), p(pos), None, p(x), F, G, Kp, D, 0, 1) == E_ARG
    assert call(p(xp), p(cls), p(pos), p(keep), p(x), F, G, G + 1, D, 0, 1) == E_SHAPE
    assert call(p(xp), p(cls), p(pos), p(keep), p(x), F, G, 0, D, 0, 1) == E_SHAPE
    assert call(p(xp), p(cls), p(pos), p(keep), p(x), F, G, Kp, D, 0, 7) == E_DTYPE
    assert call(p(xp), p(cls), p(pos), p(keep), p(x), F, G, Kp, D, 2, 1) == E_DTYPE     # f16 stream, bf16 compute type
    assert call(p(xp), p(cls), p(pos), p(keep), p(x), F, G, Kp, D, 0, 1) == 0


# ---------------------------------------------------------------------------------------------- assembly, backward
# (F, G, Kp, D): the forward's shapes; 130 frames = two slabs of frames (the partial sums go through the workspace); D = 20: scalar rows
BWD_CASES = [(3, 16, Kp, D) for D in (128, 768) for Kp in (4, 9)] + [(130, 16, 4, 128), (3, 16, 4, 20)]


def _bwd_keep(F, G, Kp):
    """Per-frame different keeps that leave patches 5 and 11 to nobody (drawn among the other G - 2 ids)."""
    pool = np.array([n for n in range(G) if n not in (5, 11)], dtype=np.int32)
    keep = pool[PR.keep_sample(300 + F + Kp, F, G - 2, Kp)]
    assert (np.diff(keep, axis=1) > 0).all() and len({tuple(r) for r in keep}) > 1
    return keep


def _bwd_run(L, dx, keep, G, dt16):
    F, Kp = keep.shape
    D = dx.shape[1]
    dxp = _guarded(F * Kp, D, dt16)
    dcls = torch.full((D + 8,), float("nan"), device=DEV)
    dpos = torch.full((G + 1 + GUARD, D), float("nan"), device=DEV)
    dpos[G + 1:] = SENT
    nbytes = L.lib.vmc_assemble_tokens_keep_bwd_workspace_bytes(F, G, D)
    assert nbytes >= F * G * 4 and nbytes % 16 == 0
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    keep_d = torch.from_numpy(keep).to(DEV)
    rc = L.lib.vmc_assemble_tokens_keep_bwd(L.ptr(dx), L.ptr(keep_d), L.ptr(dxp), L.ptr(dcls), L.ptr(dpos), F, G, Kp, D, L.dt(dx),
                                            L.dt(dt16), L.ptr(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert _guard_intact(dxp, F * Kp) and _guard_intact(dpos, G + 1) and bool(torch.isnan(dcls[D:]).all().item())
    return dxp[:F * Kp].cpu(), dcls[:D].cpu(), dpos[:G + 1].cpu()


@pytest.mark.parametrize("dt16", DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("dx_f32", [True, False], ids=["dx32", "dx16"])
@pytest.mark.parametrize("F,G,Kp,D", BWD_CASES, ids=lambda v: str(v))
def test_assemble_keep_backward(L, F, G, Kp, D, dx_f32, dt16):
    keep = _bwd_keep(F, G, Kp)
    dx = synth.normal(F + D + Kp, "dx", (F * (Kp + 1), D), std=0.3)
    dx = dx if dx_f32 else dx.to(dt16)
    want_dxp, dpos64, mag = PR.assemble_keep_bwd(dx, keep, G, dt16)
    dxp, dcls, dpos = _bwd_run(L, dx.to(DEV), keep, G, dt16)
    assert torch.equal(_bits(dxp), _bits(want_dxp))                                  # round16 of the patch rows
    err = np.abs(dpos.double().numpy() - dpos64)
    bound = PR.reassociation_bound(F, mag)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"F={F} Kp={Kp} D={D}: max |dpos - f64| / (F 2^-23 sum|addend|) = {worst:.3e}")
    assert (err <= bound).all()
    assert torch.equal(_bits(dcls), _bits(dpos[0]))                                  # dcls is dpos[0]
    kept = np.zeros(G + 1, dtype=bool)
    kept[0] = True
    kept[keep.reshape(-1) + 1] = True
    assert not kept[6] and not kept[12]
    assert (_bits(dpos)[torch.from_numpy(~kept)] == 0).all()                         # positions nobody kept: +0.0 bit patterns
    assert (np.abs(dpos.numpy())[kept].sum(axis=1) > 0).all()                        # ... and the kept ones received something
    again = _bwd_run(L, dx.to(DEV), keep, G, dt16)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((dxp, dcls, dpos), again))      # run to run: the same bits


def test_assemble_keep_backward_error_codes(L):
    F, G, Kp, D = 2, 16, 4, 64
    dx = torch.zeros((F * (Kp + 1), D), device=DEV)
    keep = torch.zeros((F, Kp), dtype=torch.int32, device=DEV)
    dxp = torch.zeros((F * Kp, D), dtype=BF16, device=DEV)
    dcls, dpos = torch.zeros(D, device=DEV), torch.zeros((G + 1, D), device=DEV)
    nbytes = L.lib.vmc_assemble_tokens_keep_bwd_workspace_bytes(F, G, D)
    ws = torch.zeros(nbytes // 4 + 4, device=DEV)
    p = L.ptr
    call = lambda *a: L.lib.vmc_assemble_tokens_keep_bwd(*a, L.stream())             # noqa: E731
    assert call(p(dx), p(keep), p(dxp), p(dcls), p(dpos), F, G, Kp, D, 0, 1, p(ws), nbytes - 1) == E_ARG       # short workspace
    assert call(p(dx), p(keep), p(dxp), p(dcls), p(dpos), F, G, Kp, D, 0, 1, None, nbytes) == E_ARG
    assert call(p(dx), p(keep), p(dxp), p(dcls), p(dpos), F, G, Kp, D, 0, 1, p(ws) + 4, nbytes) == E_ALIGN
    assert call(p(dx), p(keep), p(dxp), p(dcls), p(dpos), F, G, G + 1, D, 0, 1, p(ws), nbytes) == E_SHAPE
    assert call(p(dx), p(keep), p(dxp), p(dcls), p(dpos), F, G, Kp, D, 2, 1, p(ws), nbytes) == E_DTYPE
    assert call(p(dx), p(keep), p(dxp), p(dcls), p(dpos), F, G, Kp, D, 0, 5, p(ws), nbytes) == E_DTYPE
    assert call(p(dx), p(keep), p(dxp), p(dcls), p(dpos), F, G, Kp, D, 0, 1, p(ws), nbytes) == 0
    assert L.lib.vmc_assemble_tokens_keep_bwd_workspace_bytes(64, 16, 64) == 64 * 16 * 4                       # one slab: the inverse only
    assert L.lib.vmc_assemble_tokens_keep_bwd_workspace_bytes(128, 16, 64) == 128 * 16 * 4 + 2 * 17 * 64 * 4   # two slabs of partial sums
