"""CPU: the device-resident embedding store (vimo_clip_amd/TFAM/data/device_store.py) built on the host holds, row for row, what
the datasets return; its padded lengths are those of pad_to_bucket(collate_fn_pad(...)); the trainer's index batches are those of
batches().  The gather kernel and the trainer path run in test_gpu_device_store.py."""
import numpy as np
import pytest
import torch

from vimo_clip_amd import h5lite as h5
from vimo_clip_amd import synth
from vimo_clip_amd.graphs import pad_to_bucket
from vimo_clip_amd.TFAM.data import DeviceClipStore
from vimo_clip_amd.TFAM.data.dataset import HDF5VideoDataset, SyntheticEmbeddingDataset, collate_fn_pad
from vimo_clip_amd.TFAM.train_and_eval import Config, batches, index_batches

LENGTHS = [5, 40, 17, 64, 9, 2, 33]


def _make_rgb_and_flow(tmp_path, lengths, E=24, C=140):
    """The file pair of tests/test_hdf5_pipeline.py: .mp4-suffixed RGB keys, motion groups named key.split('.')[0]."""
    rng = np.random.default_rng(1)
    with h5.File(str(tmp_path / "rgb.h5"), "w") as f, h5.File(str(tmp_path / "flow.h5"), "w") as g:
        for i, T in enumerate(lengths):
            vid = f"clip_{i:02d}.mp4"
            lab = np.zeros(C, np.float32)
            lab[[i % C, (3 * i + 7) % C]] = 1.0
            grp = f.create_group(vid)
            grp.create_dataset("embeddings", data=rng.standard_normal((T, E)).astype(np.float32), compression="gzip", chunks=(1, E))
            grp.create_dataset("labels", data=lab)
            g.create_group(vid.split(".")[0]).create_dataset("embeddings", data=rng.standard_normal((T - 1, E)).astype(np.float32))
    return str(tmp_path / "rgb.h5"), str(tmp_path / "flow.h5")


def _assert_store_equals_dataset(store, ds, mk="flow"):
    assert len(store) == len(ds) and store.device.type == "cpu"
    assert store.rgb.rows.dtype == torch.float32 and store.rgb.offset.dtype == torch.int64 and store.rgb.length.dtype == torch.int32
    for i in range(len(ds)):
        it = ds[i]
        for s, key in ((store.rgb, "embeddings"), (store.motion, f"{mk}_embeddings")):
            o, n = int(s.offset[i]), int(s.length[i])
            assert n == it[key].shape[0] == int(s.length_host[i])
            assert torch.equal(s.rows[o:o + n], it[key])
        assert torch.equal(store.labels[i], it["labels"].float())
        assert store.video_ids[i] == it["video_id"] and store.total_frames[i] == it["total_frames"]
    for s in (store.rgb, store.motion):                       # back to back, nothing else
        assert s.rows.shape[0] == int(s.length_host.sum()) and s.length_host.dtype == np.int32
    assert store.nbytes == sum(t.numel() * t.element_size() for s in (store.rgb, store.motion) for t in (s.rows, s.offset, s.length)) \
        + store.labels.numel() * 4


@pytest.mark.parametrize("kw", [{}, {"num_frames": 8}, {"max_frames": 40}], ids=["plain", "sparse8", "max40"])
def test_store_from_hdf5_equals_dataset_items(tmp_path, kw):
    rgb, flow = _make_rgb_and_flow(tmp_path, LENGTHS)
    ds = HDF5VideoDataset(rgb, flow, **kw)
    store = DeviceClipStore.from_hdf5(rgb, flow, device="cpu", **kw)
    assert len(store) == (5 if "max_frames" in kw else 7)          # 5, 17, 9, 2, 33 are below 40
    assert all(v.endswith(".mp4") for v in store.video_ids)
    _assert_store_equals_dataset(store, ds)
    if "num_frames" in kw:
        assert int(store.rgb.length_host.max()) == 8 and store.total_frames == [5, 8, 8, 8, 8, 2, 8]
    same = DeviceClipStore.from_dataset(ds, "cpu")
    for a, b in ((store.rgb, same.rgb), (store.motion, same.motion)):
        assert torch.equal(a.rows, b.rows) and torch.equal(a.offset, b.offset) and torch.equal(a.length, b.length)
    assert torch.equal(store.labels, same.labels) and store.video_ids == same.video_ids


def test_store_from_hdf5_applies_transform(tmp_path):
    rgb, flow = _make_rgb_and_flow(tmp_path, LENGTHS[:3])
    tf = lambda x: x * 2.0 + 1.0      # noqa: E731
    _assert_store_equals_dataset(DeviceClipStore.from_hdf5(rgb, flow, transform=tf, device="cpu"), HDF5VideoDataset(rgb, flow, transform=tf))


def _synthetic(n=13, D=16, C=10, mk="flow"):
    return SyntheticEmbeddingDataset(synth.multi_hot_labels(3, "t", n, C), D, seed=4, motion_key=mk)


def test_store_from_synthetic_dataset():
    ds = _synthetic(mk="frame_diff")
    store = DeviceClipStore.from_dataset(ds, "cpu", motion_key="frame_diff")
    _assert_store_equals_dataset(store, ds, mk="frame_diff")
    assert store.D == 16 and store.C == 10 and store.motion_key == "frame_diff"


@pytest.mark.parametrize("bucket", [1, 16, 32])
def test_padded_lengths_equal_pad_to_bucket_of_collate(bucket):
    ds = _synthetic(n=24)
    store = DeviceClipStore.from_dataset(ds, "cpu")
    g = torch.Generator().manual_seed(0)
    for _ in range(12):
        ids = torch.randint(0, len(ds), (int(torch.randint(1, 6, (1,), generator=g)),), generator=g).tolist()
        b = collate_fn_pad([ds[i] for i in ids])
        rgb, mot, mr, mf, _ = pad_to_bucket(b["embeddings"], b["flow_embeddings"], b["mask_rgb"], b["mask_flow"], bucket, "rgb")
        assert store.padded_lengths(ids, bucket) == (rgb.shape[1], mot.shape[1]) == (mr.shape[1], mf.shape[1])


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_index_batches_equal_the_loaders_batches(rank, world):
    ds = _synthetic(n=23)
    store = DeviceClipStore.from_dataset(ds, "cpu")
    order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(5)).tolist()
    for od in (None, order):
        want = [b["video_id"] for b in batches(ds, 4, rank, world, order=od)]
        got = list(index_batches(len(store), 4, rank, world, order=od))
        assert [[store.video_ids[i] for i in ids] for _, ids in got] == want and len(want) >= 2
        flat = list(range(len(ds))) if od is None else od
        assert all(flat[pos:pos + len(ids)] == ids for pos, ids in got)          # pos: where the batch sits in the epoch order
    assert [len(ids) for _, ids in index_batches(10, 4, drop_last=False)] == [4, 4, 2]


def test_cpu_store_cannot_gather_and_max_bytes_raises():
    ds = _synthetic()
    store = DeviceClipStore.from_dataset(ds, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        store.gather(torch.zeros(2, dtype=torch.int32), 64, 64)
    with pytest.raises(MemoryError, match="max_bytes"):
        DeviceClipStore.from_dataset(ds, "cpu", max_bytes=store.nbytes - 1)
    assert DeviceClipStore.from_dataset(ds, "cpu", max_bytes=store.nbytes).nbytes == store.nbytes
    with pytest.raises(ValueError, match="no token rows"):
        DeviceClipStore([torch.zeros(0, 8)], device="cpu")


def test_config_reads_device_store(tmp_path):
    yaml = pytest.importorskip("yaml")
    assert Config().device_store is False
    cfg = {"training": {"mode": "both", "seed": 1, "lr": 1e-4, "epochs": 2, "batch_size": 8, "num_workers": 4, "device": "cuda"},
           "logging": {"log_dir": "logs", "checkpoint_dir": "ck"},
           "data": {"num_classes": 140, "class_names_dir": None, "train_dataset_path": None, "val_dataset_path": None,
                    "flow_dataset_path": None},
           "model": {"d_model": 512, "nhead": 8, "num_layers": 4, "dim_feedforward": 2048, "use_cross_attention": True, "concat_dim": 1,
                     "dropout": 0.1, "mlp_dropout": 0.1, "use_pe": False, "use_only_rgb": False, "use_only_flow": False}}
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).device_store is False              # the key is optional
    cfg["training"]["device_store"] = True
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).device_store is True


def test_gather_argument_errors_are_found_on_the_host():
    """vmc_gather_clips validates its arguments before any launch, so every rejected call returns VMC_E_ARG without a device.
    Every call below must be a rejected one: the pointers are host addresses.  Should a check regress, the call would go on to
    the launch with them -- on a machine without a GPU that launch fails and the return code is a positive hipError_t, so the
    assertion still fails; this test is not marked gpu and never runs beside a device.  The same checks run on the GPU with
    device pointers in tests/test_gpu_device_store.py."""
    import ctypes

    from vimo_clip_amd import _lib
    from vimo_clip_amd.TFAM.data.device_store import ClipStream
    buf = (ctypes.c_char * 64)()                       # something non-NULL to point at; a rejected call never reads it
    p = ctypes.addressof(buf)

    def streams(**bad):
        arr = (ClipStream * 2)()
        for q in range(2):
            arr[q] = ClipStream(p, p, p, p, p, p, 8)
            for k, v in bad.items():
                setattr(arr[q], k, v)
        return arr

    def call(arr, n_streams=2, index=p, B=2, n_videos=3, D=4, labels=p, labels_out=p, C=2):
        return _lib.lib.vmc_gather_clips(ctypes.addressof(arr) if arr is not None else None, n_streams, index, B, n_videos, D, labels,
                                         labels_out, C, None, None)
    ok = streams()
    E_ARG = -1
    assert call(None) == E_ARG and call(ok, index=None) == E_ARG and call(ok, labels_out=None) == E_ARG and call(ok, C=0) == E_ARG
    assert call(ok, n_streams=0) == E_ARG and call(ok, n_streams=3) == E_ARG
    assert call(ok, B=0) == E_ARG and call(ok, D=0) == E_ARG and call(ok, n_videos=0) == E_ARG and call(ok, B=-1) == E_ARG
    for field in ("rows", "offset", "length", "out", "mask"):
        assert call(streams(**{field: None})) == E_ARG, field
    assert call(streams(T_out=0)) == E_ARG
    assert ctypes.sizeof(ClipStream) == 56
