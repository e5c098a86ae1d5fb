"""CPU: the bilinear-resize recipes and the MammalNet data path around them.
  * tests/bilinear_ref.py (the numpy restatement the GPU tests compare against) equals the stored outputs of the reference's
    _resize_frames bit for bit, and equals F.interpolate on this CPU with zero differing bits.  aten's CPU kernel has TWO operation
    orders and picks by output size (OH + OW <= 128) and thread count (one thread, three channels), so the comparisons run with the
    thread count pinned, and both sides of both switches are checked;
  * the two quantise identities hold for all 256 values;
  * vmc_resize_bilinear_u8 / vmc_unit_f32_to_u8 are declared, exported and bound, and answer bad arguments before any launch;
  * dataset_frame_diff_mn: segment table, row-slice reads, fd_len rule, padding, zero fallback, item keys and shapes, collate_fn;
  * train_frame_diff_mn argument parsing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bilinear_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMC_E_ARG = -1


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "bilinear_mn.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,shape,size", [("a", (2, 3, 37, 53), (32, 48)), ("b", (1, 3, 1, 1), (16, 16)), ("c", (1, 3, 20, 30), (64, 64))])
def test_restatement_equals_the_fixture(fixture, key, shape, size):
    x = fixture[key + "_in"]
    assert x.shape == shape and tuple(fixture[key + "_size"]) == size and x.dtype == np.uint8
    got = ref.resize_f32(x, size)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(fixture[key + "_f32"]))
    assert np.array_equal(ref.to_u8(got), fixture[key + "_u8"])


@pytest.fixture
def threads():
    """Sets torch's intra-op thread count for one test: aten's choice of kernel depends on it."""
    before = torch.get_num_threads()

    def pin(n):
        torch.set_num_threads(n)
        assert torch.get_num_threads() == n

    yield pin
    torch.set_num_threads(before)


def _interpolate(x, size):
    return F.interpolate(torch.from_numpy(x).float() / 255.0, size=size, mode="bilinear", align_corners=False)


@pytest.mark.parametrize("hw,size", [((360, 640), (224, 224)), ((224, 300), (224, 224)), ((200, 224), (224, 224)), ((45, 80), (28, 31))],
                         ids=lambda v: "x".join(map(str, v)))
def test_restatement_equals_interpolate_on_this_cpu(hw, size, threads):
    threads(2)
    x = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, (2, 3) + hw, dtype=np.uint8)
    want = _interpolate(x, size)
    got = ref.resize_f32(x, size)
    assert int((_bits(got) != _bits(want.numpy())).sum()) == 0
    assert np.array_equal(ref.to_u8(got), want.mul(255).byte().numpy())


@pytest.mark.parametrize("size,recipe", [((64, 64), "weights4"), ((63, 65), "weights4"), ((100, 28), "weights4"), ((2, 126), "weights4"),
                                         ((64, 65), "separable"), ((100, 29), "separable"), ((2, 127), "separable")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_atens_switch_between_the_recipes_sits_at_oh_plus_ow_128(size, recipe, threads):
    """Both sides of the output-size switch, whatever the input size, channel count and batch; the other recipe does not match."""
    threads(2)
    assert ref.aten_recipe(size) == recipe and ref.ATEN_SMALL == 128
    other = "separable" if recipe == "weights4" else "weights4"
    for shape in ((2, 3, 37, 53), (1, 1, 150, 9), (5, 3, 101, 90)):
        x = np.random.default_rng(size[0] * 1000 + size[1] + shape[2]).integers(0, 256, shape, dtype=np.uint8)
        want = _bits(_interpolate(x, size).numpy())
        assert np.array_equal(_bits(ref.resize_f32(x, size)), want), shape
        assert np.array_equal(_bits(ref.resize_f32(x, size, recipe)), want), shape
    assert not np.array_equal(_bits(ref.resize_f32(x, size, other)), want)


def test_one_thread_takes_the_four_weight_recipe_for_three_channels(threads):
    """What a DataLoader worker of the reference computes (torch gives a worker one thread): "weights4" at every output size for
    C == 3, while one-channel frames keep the size rule."""
    threads(1)
    x = np.random.default_rng(11).integers(0, 256, (2, 3, 230, 300), dtype=np.uint8)
    want = _interpolate(x, (224, 224))
    assert np.array_equal(_bits(ref.resize_f32(x, (224, 224), "weights4")), _bits(want.numpy()))
    assert not np.array_equal(_bits(ref.resize_f32(x, (224, 224), "separable")), _bits(want.numpy()))
    assert np.array_equal(ref.resize_u8(x, (224, 224), "weights4"), want.mul(255).byte().numpy())
    g = x[:, :1]
    assert np.array_equal(_bits(ref.resize_f32(g, (224, 224), "separable")), _bits(_interpolate(g, (224, 224)).numpy()))


def test_quantise_identities_hold_for_all_256_values():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.to_u8(ref.unit(v)), v)                                   # same-size frames pass through unchanged
    assert np.array_equal(ref.to_u8(v.astype(np.float32)), ((256 - v.astype(np.int64)) % 256).astype(np.uint8))      # the wrap quirk
    t = torch.from_numpy(v)
    assert torch.equal((t.float() / 255.0).mul(255).byte(), t)
    for recipe in ("separable", "weights4"):
        assert np.array_equal(ref.resize_f32(v.reshape(1, 16, 16), (16, 16), recipe), ref.unit(v).reshape(1, 16, 16))
        assert np.array_equal(ref.resize_u8(v.reshape(1, 16, 16), (16, 16), recipe), v.reshape(1, 16, 16))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from vimo_clip_amd import _lib
    header = open(os.path.join(ROOT, "include", "vmc.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vmc_\w+)", nm))
    for name, nargs in (("vmc_resize_bilinear_u8", 14), ("vmc_unit_f32_to_u8", 4)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} not declared in include/vmc.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in exported, f"{name} not exported by libvmc.so"
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["vmc_resize_bilinear_u8"][1][8:12] == [ctypes.c_longlong] * 4          # byte strides are 64-bit
    assert _lib.SIGNATURES["vmc_unit_f32_to_u8"][1][2] is ctypes.c_longlong


def test_recipe_constants_match_the_header():
    from vimo_clip_amd import ops
    header = open(os.path.join(ROOT, "include", "vmc.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"(VMC_RESIZE_\w+) = (\d+)", header)}
    assert flags == {"VMC_RESIZE_U8": 1, "VMC_RESIZE_SEPARABLE": 2, "VMC_RESIZE_WEIGHTS4": 4}
    assert ops.RESIZE_RECIPES == {"aten": 0, "separable": flags["VMC_RESIZE_SEPARABLE"], "weights4": flags["VMC_RESIZE_WEIGHTS4"]}
    small = int(re.search(r"#define\s+VMC_RESIZE_ATEN_SMALL\s+(\d+)", header).group(1))
    assert small == ops.RESIZE_ATEN_SMALL == ref.ATEN_SMALL


_HOST = (ctypes.c_uint8 * 4096)()          # host memory: a launch on it would be an error, VMC_E_ARG must come first
_P = ctypes.addressof(_HOST)
_GOOD = dict(src=_P, dst=_P, F=1, C=3, H=4, W=4, OH=2, OW=2, sf=48, sc=16, sy=4, sx=1, mode=0)
ARG_CASES = {"null src": dict(src=None), "null dst": dict(dst=None), "F = 0": dict(F=0), "H = 0": dict(H=0), "W = -1": dict(W=-1),
             "OH = 0": dict(OH=0), "OW = 0": dict(OW=0), "C = 2": dict(C=2), "C = 0": dict(C=0), "C = 4": dict(C=4),
             "out_mode -1": dict(mode=-1), "out_mode 6 (both recipes)": dict(mode=6), "out_mode 7": dict(mode=7), "out_mode 8": dict(mode=8)}


@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_resize_bad_arguments_return_e_arg_before_any_launch(case):
    from vimo_clip_amd import _lib
    a = dict(_GOOD, **ARG_CASES[case])
    rc = _lib.lib.vmc_resize_bilinear_u8(a["src"], a["dst"], a["F"], a["C"], a["H"], a["W"], a["OH"], a["OW"], a["sf"], a["sc"], a["sy"],
                                         a["sx"], a["mode"], None)
    assert rc == VMC_E_ARG, case


def test_unit_bad_arguments_return_e_arg_before_any_launch():
    from vimo_clip_amd import _lib
    fn = _lib.lib.vmc_unit_f32_to_u8
    assert fn(None, _P, 4, None) == VMC_E_ARG
    assert fn(_P, None, 4, None) == VMC_E_ARG
    assert fn(_P, _P, 0, None) == VMC_E_ARG
    assert fn(_P, _P, -3, None) == VMC_E_ARG


def test_python_wrappers_check_before_the_library():
    from vimo_clip_amd import ops
    u8 = torch.zeros(2, 3, 4, 5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="u8"):
        ops.resize_bilinear_u8(u8.float(), (2, 2))
    with pytest.raises(ValueError, match="channels"):
        ops.resize_bilinear_u8(torch.zeros(2, 2, 4, 5, dtype=torch.uint8), (2, 2))
    with pytest.raises(ValueError, match="recipe"):
        ops.resize_bilinear_u8(u8, (2, 2), recipe="bicubic")
    with pytest.raises(ValueError, match="out must be"):
        ops.resize_bilinear_u8(u8, (2, 2), out=torch.zeros(2, 3, 2, 2), as_u8=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_bilinear_u8(u8, (2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.unit_f32_to_u8(torch.zeros(4))
    with pytest.raises(ValueError, match="float32"):
        ops.unit_f32_to_u8(torch.zeros(4, dtype=torch.float64))


# ---- dataset -----------------------------------------------------------------------------------------------------------------
L, E, NC = 10, 6, 4
LENGTHS = {"v00": 0, "v01": 1, "v05": 5, "v10": 10, "v23": 23}
SIZES = {"v01": (6, 9), "v05": (12, 8), "v10": (8, 8), "v23": (5, 7)}          # v10 is already at spatial_size
SPATIAL = (8, 8)


@pytest.fixture(scope="module")
def mn(tmp_path_factory):
    from vimo_clip_amd import h5lite as h5
    d = tmp_path_factory.mktemp("mn")
    rng = np.random.default_rng(5)
    emb = {k: rng.standard_normal((T, E)).astype(np.float32) for k, T in LENGTHS.items()}
    lab = {k: np.eye(NC, dtype=np.float32)[i % NC] for i, k in enumerate(LENGTHS)}
    vid = {k: rng.integers(0, 256, (LENGTHS[k] - (3 if k == "v23" else 0),) + hw + (3,), dtype=np.uint8) for k, hw in SIZES.items()}
    path = str(d / "emb.h5")
    with h5.File(path, "w") as f:
        g = f.create_group("trimmed_videos")
        for k in LENGTHS:
            gg = g.create_group(k)
            gg.create_dataset("embeddings", data=emb[k]) if LENGTHS[k] else gg.create_dataset("embeddings", shape=(0, E), dtype=np.float32)
            gg.create_dataset("labels", data=lab[k])
    os.makedirs(str(d / "videos"))
    for k, v in vid.items():
        np.save(str(d / "videos" / f"{k}.npy"), v[:0] if k == "v01" else v)          # v01: a video that decodes to no frame at all
    return dict(path=path, videos=str(d / "videos"), emb=emb, lab=lab, vid=vid)


def _ds(mn, **kw):
    from vimo_clip_amd.dataset_frame_diff_mn import HDF5VideoDataset
    return HDF5VideoDataset(mn["path"], mn["videos"], sequence_length=L, spatial_size=SPATIAL, **kw)


def test_segment_table(mn):
    from vimo_clip_amd.dataset_frame_diff_mn import build_segments_mn, frame_diff_len
    want = [("v01", 0, 1), ("v05", 0, 5), ("v10", 0, 10), ("v23", 0, 10), ("v23", 10, 10), ("v23", 20, 3)]
    assert _ds(mn).segments == want and len(_ds(mn)) == 6
    assert build_segments_mn(LENGTHS, L) == want
    assert build_segments_mn({"a": 4}, 2) == [("a", 0, 2), ("a", 2, 2)] and build_segments_mn({"a": 0}, 2) == []
    # fd_len: seg_len - 1 for a full segment, L - 1 for a padded one
    assert [frame_diff_len(s, L) for s in (10, 3, 1)] == [9, 9, 9] and frame_diff_len(2, 2) == 1 and frame_diff_len(1, 2) == 1
    assert frame_diff_len(7, 7) == 6 and frame_diff_len(6, 7) == 6


def test_embedding_rows_are_read_as_a_slice(mn, monkeypatch):
    from vimo_clip_amd import h5lite as h5
    seen = []
    orig = h5.Dataset._read_all_storage

    def spy(self, rows=None):
        seen.append((self.name, rows))
        return orig(self, rows)

    monkeypatch.setattr(h5.Dataset, "_read_all_storage", spy)
    item = _ds(mn)[4]                        # ("v23", 10, 10)
    assert ("/trimmed_videos/v23/embeddings", (10, 20)) in seen
    assert not any(n.endswith("embeddings") and r is None for n, r in seen)
    assert torch.equal(item["rgb_emb"], torch.from_numpy(mn["emb"]["v23"][10:20]))


def test_items_keys_shapes_padding_and_zero_fallback(mn):
    ds = _ds(mn)
    by = {(s[0], s[1]): ds[i] for i, s in enumerate(ds.segments)}
    for (k, start), it in by.items():
        assert list(it) == ["video_id", "rgb_emb", "frame_diff", "labels"] and it["video_id"] == k
        assert it["rgb_emb"].shape == (L, E) and it["frame_diff"].shape == (L - 1, 3) + SPATIAL and it["frame_diff"].dtype == torch.float32
        assert torch.equal(it["labels"], torch.from_numpy(mn["lab"][k]))
        assert 0.0 <= float(it["frame_diff"].min()) and float(it["frame_diff"].max()) <= 1.0
    # embeddings: the segment's rows, then the last row repeated
    e = by[("v23", 20)]["rgb_emb"].numpy()
    assert np.array_equal(e[:3], mn["emb"]["v23"][20:23]) and all(np.array_equal(e[j], mn["emb"]["v23"][22]) for j in range(3, L))
    assert np.array_equal(by[("v05", 0)]["rgb_emb"].numpy()[5:], np.repeat(mn["emb"]["v05"][4:5], 5, axis=0))

    def frames(k, lo, hi):
        return np.ascontiguousarray(mn["vid"][k][lo:hi].transpose(0, 3, 1, 2))

    # full segment: frames start .. start + 8, resized (the restatement is pinned against F.interpolate above)
    assert np.array_equal(by[("v23", 0)]["frame_diff"].numpy(), ref.resize_f32(frames("v23", 0, 9), SPATIAL))
    # same-size source: only divided by 255
    assert np.array_equal(by[("v10", 0)]["frame_diff"].numpy(), ref.unit(frames("v10", 0, 9)))
    # short video (20 frames decoded): frames 10..18 exist; the tail segment asks for 20..28, gets none -> zeros
    assert np.array_equal(by[("v23", 10)]["frame_diff"].numpy(), ref.resize_f32(frames("v23", 10, 19), SPATIAL))
    assert not by[("v23", 20)]["frame_diff"].any() and not by[("v01", 0)]["frame_diff"].any()
    # padded segment: 5 decoded frames, the last repeated 4 times
    fd = by[("v05", 0)]["frame_diff"].numpy()
    assert np.array_equal(fd[:5], ref.resize_f32(frames("v05", 0, 5), SPATIAL)) and all(np.array_equal(fd[j], fd[4]) for j in range(5, 9))


def test_raw_u8_items_and_slice_rules(mn):
    from vimo_clip_amd.dataset_frame_diff_mn import slice_video_segment
    ds = _ds(mn, raw_u8=True)
    it = ds[1]                               # ("v05", 0, 5)
    assert it["frame_diff"].dtype == torch.uint8 and it["frame_diff"].shape == (L - 1, 3) + SIZES["v05"]
    assert np.array_equal(it["frame_diff"][:5].numpy(), mn["vid"]["v05"].transpose(0, 3, 1, 2))
    assert all(torch.equal(it["frame_diff"][j], it["frame_diff"][4]) for j in range(5, 9))
    z = ds[0]["frame_diff"]                  # v01: nothing decoded
    assert z.shape == (L - 1, 3, 1, 1) and z.dtype == torch.uint8 and not z.any()
    v = torch.arange(4 * 2 * 2 * 3, dtype=torch.uint8).reshape(4, 2, 2, 3)
    assert torch.equal(slice_video_segment(v, 1, 2), v[1:3].permute(0, 3, 1, 2))
    assert torch.equal(slice_video_segment(v, 3, 3), v[3:4].permute(0, 3, 1, 2).repeat(3, 1, 1, 1))
    assert slice_video_segment(v, 4, 2).shape == (2, 3, 1, 1)


def test_collate_fn(mn):
    from vimo_clip_amd.dataset_frame_diff_mn import collate_fn
    ds = _ds(mn)
    b = collate_fn([ds[1], ds[3]])
    assert list(b) == ["video_id", "rgb_emb", "frame_diff", "labels"] and b["video_id"] == ["v05", "v23"]
    assert b["rgb_emb"].shape == (2, L, E) and b["frame_diff"].shape == (2, L - 1, 3) + SPATIAL and b["labels"].shape == (2, NC)
    assert torch.equal(b["frame_diff"][1], ds[3]["frame_diff"]) and torch.equal(b["rgb_emb"][0], ds[1]["rgb_emb"])
    assert b["labels"].argmax(dim=1).tolist() == [2, 0]


# ---- training entry ----------------------------------------------------------------------------------------------------------
def test_train_frame_diff_mn_argument_parsing():
    from vimo_clip_amd import train_frame_diff_mn as t
    p = t.build_parser()
    a = p.parse_args(["--train_hdf5_path", "tr.h5", "--val_hdf5_path", "va.h5", "--frame_diff_videos_dir", "vids"])
    assert (a.train_hdf5_path, a.val_hdf5_path, a.frame_diff_videos_dir) == ("tr.h5", "va.h5", "vids")
    assert (a.epochs, a.batch_size, a.num_workers, a.learning_rate, a.distillation_loss_mode) == (10, 32, 4, 1e-3, "cosine")
    assert (a.num_classes, a.sequence_length, a.residual_alpha, tuple(a.spatial_size), a.device_resize) == (12, 30, 0.1, (224, 224), False)
    # the reference's own spelling, and the device-side option
    b = p.parse_args(["--train-hdf5-path", "tr.h5", "--val-hdf5-path", "va.h5", "--frame-diff-videos-dir", "vids", "--sequence-length", "10",
                      "--batch-size", "4", "--device_resize", "--spatial_size", "64", "80"])
    assert (b.train_hdf5_path, b.sequence_length, b.batch_size, b.device_resize, tuple(b.spatial_size)) == ("tr.h5", 10, 4, True, (64, 80))
    with pytest.raises(SystemExit):
        p.parse_args(["--val_hdf5_path", "va.h5", "--frame_diff_videos_dir", "vids"])
    with pytest.raises(SystemExit):
        p.parse_args(["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c", "--distillation_loss_mode", "l1"])
