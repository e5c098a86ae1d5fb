"""GPU: the six patch-extraction entries of include/vmc.h, bit for bit, called through ``_lib.lib`` directly.

Every output buffer is pre-filled with a NaN bit pattern and followed by guard rows: data columns must carry the expected bits,
pad columns must read 0 and the guard rows must keep their pattern.  Every comparison is ``torch.equal`` on the int16 view.

Expected values are numpy float32 with IEEE division, ``((v / 255) - mean_c) * (1 / std_c)``, rounded to nearest even once.  The
normalised output depends only on (v, c), and ``arange(256)`` is planted in every (frame, channel) plane, so those entries are
checked exhaustively.  The f16 kernels may fuse the last multiply into the conversion (one rounding of the exact product instead
of two): ``test_reference_is_unique`` shows that both give the same f16 on all 768 pairs (a bf16 conversion takes an fp32
operand, there is nothing to fuse)."""
import functools

import numpy as np
import pytest
import torch

from vimo_clip_amd import _lib, synth

MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)
ISTD = np.float32(1.0) / np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)
SHAPES = [(28, 7),       # odd p (the 2-byte stores of the exact layout), pad 147 -> 192
          (56, 14),      # even p (4-byte stores), pad 588 -> 640
          (64, 16),      # no pad columns: no zeroing launch
          (64, 32)]      # g = 2
DTYPES = [torch.bfloat16, torch.float16]
F = 2
NAN16 = 0x7FC1           # a NaN in bf16 and in f16
GUARD_ROWS = 2


def _kpad(p):
    return (3 * p * p + 63) // 64 * 64


def _round16(x: np.ndarray, dtype) -> np.ndarray:
    """fp32 -> the bits (uint16) of the nearest bf16 / f16, ties to even.  Finite inputs only."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == torch.float16:
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def _widen(bits: np.ndarray, dtype) -> np.ndarray:
    """bf16 / f16 bits -> fp32 (exact)."""
    if dtype == torch.float16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _normalise(v: np.ndarray, c: np.ndarray) -> np.ndarray:
    return (v.astype(np.float32) / np.float32(255.0) - MEAN[c]) * ISTD[c]


def _im2col(x: np.ndarray, p: int) -> np.ndarray:
    """[F,3,R,R] -> [F*g*g, 3*p*p], column c*p*p + dy*p + dx."""
    f, ch, r, _ = x.shape
    g = r // p
    return np.ascontiguousarray(x.reshape(f, ch, g, p, g, p).transpose(0, 2, 4, 1, 3, 5)).reshape(f * g * g, ch * p * p)


def _expected(parts, p: int) -> np.ndarray:
    """The whole buffer: one [rows, kpad] block per part (data | zero pad) side by side, then the untouched guard rows."""
    k, kpad = 3 * p * p, _kpad(p)
    rows = parts[0].shape[0]
    buf = np.full((rows + GUARD_ROWS, len(parts) * kpad), NAN16, dtype=np.uint16)
    for i, part in enumerate(parts):
        buf[:rows, i * kpad:i * kpad + k] = part
        buf[:rows, i * kpad + k:(i + 1) * kpad] = 0
    return buf


@functools.lru_cache(maxsize=None)
def _frames(R: int) -> np.ndarray:
    a = synth.randint_u8(300 + R, "patch-frames", (F, 3, R, R)).numpy().copy()
    a.reshape(F, 3, R * R)[:, :, :256] = np.arange(256, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _pixels(R: int) -> np.ndarray:
    a = synth.normal(400 + R, "patch-pixels", (F, 3, R, R)).numpy().astype(np.float32).clip(-1.8, 2.15)      # CLIP's normalised range
    planted = [0.0, -0.0, 1.0,
               1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,       # bf16 ties: down to 1 (even), up to 1 + 2^-6
               1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11]     # f16 ties
    a.reshape(-1)[:len(planted)] = planted
    a.reshape(-1)[-len(planted):] = [-v for v in planted]
    a.setflags(write=False)
    return a


def _run(entry: str, src: np.ndarray, p: int, dtype, wrap=None) -> np.ndarray:
    """One call of lib.<entry> into a NaN-filled buffer with guard rows; the whole buffer back as uint16."""
    R = src.shape[-1]
    parts = {"vmc_patches_u8_exact": 2, "vmc_patches_gray_u8_exact": 2, "vmc_patches_f32_split": 3}.get(entry, 1)
    rows, kpad = src.shape[0] * (R // p) ** 2, _kpad(p)
    x = torch.tensor(src, device="cuda")
    out = torch.full((rows + GUARD_ROWS, parts * kpad), NAN16, dtype=torch.int16, device="cuda")
    args = (_lib.ptr(x), _lib.ptr(out), src.shape[0], R, p, kpad) + (() if wrap is None else (int(wrap),))
    _lib.check(getattr(_lib.lib, entry)(*args, _lib.dt(dtype), _lib.stream()), entry)
    return out.cpu().numpy().view(np.uint16)


def _assert_buffer(got: np.ndarray, want: np.ndarray, p: int, what: str):
    k, kpad, rows = 3 * p * p, _kpad(p), want.shape[0] - GUARD_ROWS
    g, w = torch.from_numpy(got.view(np.int16)), torch.from_numpy(want.view(np.int16))
    assert torch.equal(g[rows:], w[rows:]), f"{what}: guard rows were written"
    for i in range(want.shape[1] // kpad):
        assert torch.equal(g[:rows, i * kpad + k:(i + 1) * kpad], w[:rows, i * kpad + k:(i + 1) * kpad]), f"{what}: pad columns of part {i} are not 0"
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


def test_reference_is_unique():
    v, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(3), indexing="ij")
    val = _normalise(v, c)
    for dtype in DTYPES:                                      # torch's cast agrees with the numpy rounding
        assert np.array_equal(torch.from_numpy(val).to(dtype).view(torch.int16).numpy().view(np.uint16), _round16(val, dtype))
    # a product of two fp32 is exact in fp64, and numpy rounds fp64 -> f16 once: fused and unfused conversion give the same f16
    diff = v.astype(np.float32) / np.float32(255.0) - MEAN[c]
    exact = diff.astype(np.float64) * ISTD[c].astype(np.float64)
    assert np.array_equal(exact.astype(np.float32), val)
    assert np.array_equal(exact.astype(np.float16).view(np.uint16), _round16(val, torch.float16))
    # a reciprocal multiply instead of the division is a different fp32 on many pixel values: the division is part of the contract
    assert np.count_nonzero(np.arange(256, dtype=np.float32) * (np.float32(1.0) / np.float32(255.0))
                            != np.arange(256, dtype=np.float32) / np.float32(255.0)) == 126


@pytest.mark.gpu
@pytest.mark.parametrize("wrap", [False, True], ids=["plain", "wrap"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("R,p", SHAPES)
def test_u8_entries(R, p, dtype, wrap):
    fr = _frames(R)
    grey = np.ascontiguousarray(fr[:, :1])
    for entry, src in (("vmc_preprocess_patches_u8", fr), ("vmc_patches_u8_exact", fr),
                       ("vmc_preprocess_patches_gray_u8", grey), ("vmc_patches_gray_u8_exact", grey)):
        rgb = np.ascontiguousarray(np.broadcast_to(src, fr.shape))           # a grey plane: the RGB expectation of the plane three times
        v = ((256 - rgb.astype(np.int32)) & 255).astype(np.uint8) if wrap else rgb
        if "exact" in entry:
            bits = _im2col(_round16(v.astype(np.float32), dtype), p)        # 0..255 are exact in both types
            want = _expected([bits, bits], p)
        else:
            want = _expected([_im2col(_round16(_normalise(v, np.arange(3)[None, :, None, None]), dtype), p)], p)
        _assert_buffer(_run(entry, src, p, dtype, wrap), want, p, entry)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("R,p", SHAPES)
def test_f32_entries(R, p, dtype):
    x = _pixels(R)
    hi = _round16(x, dtype)
    lo = _round16(x - _widen(hi, dtype), dtype)      # x - hi is exact in fp32: one rounding; f16 subnormals are kept
    if dtype == torch.float16:
        assert np.count_nonzero((lo & 0x7C00 == 0) & (lo & 0x03FF != 0)) > 100
    assert hi.reshape(-1)[1] == 0x8000 and lo.reshape(-1)[1] == 0          # -0.0 -> hi -0.0, lo +0.0
    hi, lo = _im2col(hi, p), _im2col(lo, p)
    _assert_buffer(_run("vmc_patches_f32", x, p, dtype), _expected([hi], p), p, "vmc_patches_f32")
    _assert_buffer(_run("vmc_patches_f32_split", x, p, dtype), _expected([hi, lo, hi], p), p, "vmc_patches_f32_split")
