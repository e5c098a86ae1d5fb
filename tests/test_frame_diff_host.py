"""CPU: the frame-difference ABI (vmc_frame_diff_gray_u8 and the grey patch entries) is declared, exported and bound, its
argument checks answer before any launch, and the numpy reference the GPU tests compare against gives the known grey values."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import frame_diff_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vmc_frame_diff_gray_u8", "vmc_preprocess_patches_gray_u8", "vmc_patches_gray_u8_exact")
VMC_E_ARG = -1


def test_new_symbols_are_declared_exported_and_bound():
    from vimo_clip_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmc.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vmc_\w+)", nm))
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/vmc.h"
        assert name in exported, f"{name} not exported by libvmc.so"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["vmc_frame_diff_gray_u8"][1]) == 16
    assert _lib.SIGNATURES["vmc_frame_diff_gray_u8"][1][6:10] == [ctypes.c_longlong] * 4      # byte strides are 64-bit


def test_min_segment_constant_matches_the_header():
    from vimo_clip_amd import ops
    header = open(os.path.join(ROOT, "include", "vmc.h")).read()
    assert int(re.search(r"#define\s+VMC_FRAME_DIFF_MIN_SEG\s+(\d+)", header).group(1)) == ops.FRAME_DIFF_MIN_SEG
    assert ops.GRAY_WEIGHTS_CV8 == ref.CV8 and ops.GRAY_WEIGHTS_14BIT == ref.BITS14


_HOST = (ctypes.c_uint8 * 4096)()          # host memory: a launch on it would be an error, VMC_E_ARG must come first
_P = ctypes.addressof(_HOST)
_GOOD = dict(frames=_P, prev=None, out=_P, T=2, H=4, W=4, st=48, sc=1, sy=12, sx=3, wr=9798, wg=19235, wb=3735, shift=15, ch=1)

ARG_CASES = {
    "null frames": dict(frames=None),
    "null out": dict(out=None),
    "T = 0": dict(T=0),
    "H = 0": dict(H=0),
    "W = -1": dict(W=-1),
    "one frame, no prev": dict(T=1),
    "channels_out 2": dict(ch=2),
    "channels_out 0": dict(ch=0),
    "shift 0": dict(shift=0, wr=1, wg=0, wb=0),
    "shift 23": dict(shift=23, wr=1 << 23, wg=0, wb=0),
    "negative weight": dict(wr=-1, wg=19235 + 9798 + 1),
    "sum below 1 << shift": dict(wb=3734),
    "sum above 1 << shift": dict(wb=3736),
    "14-bit weights with shift 15": dict(wr=4899, wg=9617, wb=1868),
}


@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_bad_arguments_return_e_arg_before_any_launch(case):
    from vimo_clip_amd import _lib
    a = dict(_GOOD, **ARG_CASES[case])
    rc = _lib.lib.vmc_frame_diff_gray_u8(a["frames"], a["prev"], a["out"], a["T"], a["H"], a["W"], a["st"], a["sc"], a["sy"], a["sx"],
                                         a["wr"], a["wg"], a["wb"], a["shift"], a["ch"], None)
    assert rc == VMC_E_ARG, case


def test_grey_patch_entries_reject_null_pointers_and_sizes():
    from vimo_clip_amd import _lib
    for fn in (_lib.lib.vmc_preprocess_patches_gray_u8, _lib.lib.vmc_patches_gray_u8_exact):
        assert fn(None, _P, 1, 64, 16, 768, 0, _lib.BF16, None) == VMC_E_ARG
        assert fn(_P, None, 1, 64, 16, 768, 0, _lib.BF16, None) == VMC_E_ARG
        assert fn(_P, _P, 0, 64, 16, 768, 0, _lib.BF16, None) == VMC_E_ARG
        assert fn(_P, _P, 1, 64, 0, 768, 0, _lib.BF16, None) == VMC_E_ARG


def test_python_wrapper_checks_before_the_library():
    import torch
    from vimo_clip_amd import ops
    with pytest.raises(ValueError, match="layout"):
        ops.frame_diff_gray(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), layout="chwn")
    with pytest.raises(ValueError, match="3 channels"):
        ops.frame_diff_gray(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), layout="nhwc")
    with pytest.raises(ValueError, match="u8"):
        ops.frame_diff_gray(torch.zeros(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.frame_diff_gray(torch.zeros(2, 3, 4, 4, dtype=torch.uint8))
    # n_out == 0: the empty result, without a call into the library (a host tensor would raise there)
    assert tuple(ops.frame_diff_gray(torch.zeros(1, 3, 4, 5, dtype=torch.uint8), channels=3).shape) == (0, 3, 4, 5)


def test_numpy_reference_grey_values():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8)
    assert ref.gray(px).tolist() == [76, 150, 29, 255, 0]
    assert ref.gray(px[:3], ref.BITS14).tolist() == [76, 150, 29]
    assert ref.gray(px[3:], ref.BITS14).tolist() == [255, 0]
    # the difference: absolute value, prev in front, channel replication
    fr = np.stack([np.full((2, 2, 3), v, np.uint8) for v in (10, 250, 3)])
    assert ref.frame_diff(fr)[:, 0, 0, 0].tolist() == [240, 247]
    assert ref.frame_diff(fr, prev=np.full((2, 2, 3), 255, np.uint8), channels=3).shape == (3, 3, 2, 2)
    assert ref.frame_diff(fr, prev=np.full((2, 2, 3), 255, np.uint8))[0, 0, 0, 0] == 245


class _StubMotionStudent:
    """Host stand-in for the student: forward_from_rgb differences with the numpy reference and returns each motion frame's
    mean as a one-column embedding; records (frames in the chunk, prev given) per call."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def forward_from_rgb(self, rgb, prev=None):
        import torch
        self.calls.append((rgb.shape[1], prev is not None))
        fr = rgb[0].permute(0, 2, 3, 1).numpy()
        d = ref.frame_diff(fr, None if prev is None else prev[0].permute(1, 2, 0).numpy())
        return torch.from_numpy(d.astype(np.float32).mean(axis=(1, 2, 3)))[None, :, None], None, None


def test_exporter_carries_the_last_frame_across_chunks(tmp_path):
    """motion_from_rgb on the host: T - 1 rows whatever the chunk size (the seam frame is carried as `prev`), a chunk of one frame
    at the start only primes `prev`, a one-frame video ends in the empty-video branch, resume skips finished videos."""
    from vimo_clip_amd import h5lite as h5
    from vimo_clip_amd import inference as inf
    rng = np.random.default_rng(8)
    vids = {"ten": rng.integers(0, 256, (10, 6, 9, 3), dtype=np.uint8), "one": rng.integers(0, 256, (1, 6, 9, 3), dtype=np.uint8)}
    for k, v in vids.items():
        np.save(str(tmp_path / f"{k}.npy"), v)
    paths = [str(tmp_path / "ten.npy"), str(tmp_path / "one.npy")]
    want = ref.frame_diff(vids["ten"]).astype(np.float32).mean(axis=(1, 2, 3))
    # (frames in the chunk, prev given) per model call; a first chunk of one frame only primes `prev` and never reaches the model
    for chunk, calls in ((4, [(4, False), (4, True), (2, True)]), (1, [(1, True)] * 9), (256, [(10, False)])):
        model, out = _StubMotionStudent(), str(tmp_path / f"c{chunk}.h5")
        stats = inf.export_embeddings(paths, model, out, chunk_size=chunk, flush_interval_s=0, motion_from_rgb=True)
        assert stats == {"processed": 2, "skipped_existing": 0, "skipped_low_ram": 0, "errors": 0}
        assert model.calls == calls, chunk
        with h5.File(out, "r") as f:
            assert f["ten/embeddings"].shape == (9, 1) and np.array_equal(f["ten/embeddings"][:, 0], want), chunk
            assert f["one/embeddings"].shape == (0, 0)
        stats = inf.export_embeddings(paths, model, out, resume=True, chunk_size=chunk, motion_from_rgb=True)
        assert stats["skipped_existing"] == 2 and stats["processed"] == 0
