"""GPU: batches assembled on the device from a DeviceClipStore (vmc_gather_clips, include/vmc.h K17) are, bit for bit, the batches
the host loader builds (``collate_fn_pad`` + ``graphs.pad_to_bucket``), and a trainer fed from the store computes what the trainer
fed from the loader computes.

Every comparison is ``torch.equal``: the kernel copies fp32 rows, so there is no tolerance to choose; the step and trainer
comparisons run the same kernels on the same values in both runs (same padded shapes, hence the same dropout element indices).
Output buffers are pre-filled with NaN / 0xFF so that an element the kernel leaves unwritten shows up.
"""
import ctypes
import os
import re

import pytest
import torch

from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB_LENGTHS = [2, 3, 16, 17, 33, 64, 5]


def _items(lengths, D, C, seed, motion=True):
    g = torch.Generator().manual_seed(seed)
    items = []
    for i, T in enumerate(lengths):
        it = {"video_id": f"v{i}", "embeddings": torch.randn(T, D, generator=g), "labels": (torch.rand(C, generator=g) < 0.3).float(),
              "total_frames": T}
        if motion:
            it["flow_embeddings"] = torch.randn(T - 1, D, generator=g)
        items.append(it)
    return items


def _prefilled(store, B, Tr, Tf):
    out = store.alloc_out(B, Tr, Tf)
    for k, v in out.items():
        if v.dtype == torch.float32:
            v.fill_(float("nan"))
        elif v.dtype == torch.bool:
            v.view(torch.uint8).fill_(255)
        else:
            v.fill_(-7)
    return out


def _u8(mask):
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _check_stream(got_tokens, got_mask, clips, T_out):
    """Against pad_sequence + arange < length, zero-padded to T_out (what collate_fn_pad + pad_to_bucket build)."""
    B, D = len(clips), got_tokens.shape[2]
    want = torch.zeros(B, T_out, D)
    mask = torch.zeros(B, T_out, dtype=torch.uint8)
    for b, c in enumerate(clips):
        want[b, :c.shape[0]] = c
        mask[b, :c.shape[0]] = 1
    assert got_tokens.shape == want.shape and torch.equal(got_tokens.cpu(), want)
    assert torch.equal(_u8(got_mask).cpu(), mask)


INDEX_SETS = {1: [6], 3: [4, 6, 4], 8: [0, 6, 3, 3, 5, 1, 6, 2]}


@pytest.mark.parametrize("D", [512, 768], ids=["d512", "d768"])
def test_gather_equals_collate_bit_for_bit(D):
    from vimo_clip_amd.graphs import pad_to_bucket
    from vimo_clip_amd.TFAM.data import DeviceClipStore
    from vimo_clip_amd.TFAM.data.dataset import collate_fn_pad
    C = 140
    items = _items(RGB_LENGTHS, D, C, seed=D)
    store = DeviceClipStore.from_dataset(items, "cuda")
    assert len(store) == 7 and store.motion.length_host.tolist() == [t - 1 for t in RGB_LENGTHS]
    for B, ids in INDEX_SETS.items():
        idx = torch.tensor(ids, dtype=torch.int32, device="cuda")
        b = collate_fn_pad([items[i] for i in ids])
        n_rgb, n_mot = b["embeddings"].shape[1], b["flow_embeddings"].shape[1]
        for bucket in (1, 32, 64):
            rgb, mot, mr, mf, _ = pad_to_bucket(b["embeddings"], b["flow_embeddings"], b["mask_rgb"], b["mask_flow"], bucket, "rgb")
            Tr, Tf = store.padded_lengths(ids, bucket)
            assert (Tr, Tf) == (rgb.shape[1], mot.shape[1])
            out = store.gather(idx, Tr, Tf, out=_prefilled(store, B, Tr, Tf))
            assert torch.equal(out["embeddings"].cpu(), rgb) and torch.equal(out["flow_embeddings"].cpu(), mot), (B, bucket)
            assert out["mask_rgb"].dtype == torch.bool
            assert torch.equal(_u8(out["mask_rgb"]).cpu(), mr.to(torch.uint8)) and torch.equal(_u8(out["mask_flow"]).cpu(), mf.to(torch.uint8))
            assert torch.equal(out["labels"].cpu(), b["labels"])
            assert out["max_len_rgb"].item() == n_rgb and out["max_len_flow"].item() == n_mot, (B, bucket)
        fresh = store.gather(idx, n_rgb, n_mot)                          # buffers of its own
        assert torch.equal(fresh["embeddings"].cpu(), b["embeddings"]) and torch.equal(fresh["mask_flow"].cpu(), b["mask_flow"])
    assert store.read_status() == 0


def test_gather_single_stream_scalar_path():
    """D = 6 (not a multiple of 4: 4-byte accesses), one stream, a video without rows."""
    from vimo_clip_amd.TFAM.data import DeviceClipStore
    items = _items([0, 1, 4], 6, 3, seed=2, motion=False)
    clips = [it["embeddings"] for it in items]
    store = DeviceClipStore(clips, labels=torch.stack([it["labels"] for it in items]), device="cuda")
    assert store.motion is None and store.rgb.offset.tolist() == [0, 0, 1]
    for B, ids in {1: [2], 3: [0, 2, 0], 8: [1, 0, 2, 2, 0, 1, 1, 2]}.items():
        idx = torch.tensor(ids, dtype=torch.int32, device="cuda")
        for T_out in (4, 32, 64):
            assert store.padded_lengths(ids, T_out if T_out > 4 else 1) == (T_out, None)
            out = store.gather(idx, T_out, out=_prefilled(store, B, T_out, None))
            assert set(out) == {"embeddings", "mask_rgb", "max_len_rgb", "labels"}
            _check_stream(out["embeddings"], out["mask_rgb"], [clips[i] for i in ids], T_out)
            assert torch.equal(out["labels"].cpu(), torch.stack([items[i]["labels"] for i in ids]))
            assert out["max_len_rgb"].item() == 4
    one = store.gather(torch.tensor([0, 0], dtype=torch.int32, device="cuda"), 5)        # only empty clips: max_len is at least 1
    assert one["max_len_rgb"].item() == 1 and not bool(one["mask_rgb"].any()) and not bool(one["embeddings"].any())
    assert store.read_status() == 0


def _stream_array(store, out, Tr, Tf):
    from vimo_clip_amd.TFAM.data.device_store import ClipStream
    arr = (ClipStream * 3)()
    for q, (s, ke, km, kl, T) in enumerate(((store.rgb, "embeddings", "mask_rgb", "max_len_rgb", Tr),
                                             (store.motion, "flow_embeddings", "mask_flow", "max_len_flow", Tf))):
        arr[q] = ClipStream(s.rows.data_ptr(), s.offset.data_ptr(), s.length.data_ptr(), out[ke].data_ptr(), out[km].data_ptr(),
                            out[kl].data_ptr(), T)
    arr[2] = arr[1]
    return arr


def test_out_of_range_indices_truncation_and_argument_errors():
    from vimo_clip_amd import _lib
    from vimo_clip_amd.TFAM.data import DeviceClipStore
    D, C = 512, 140
    items = _items(RGB_LENGTHS, D, C, seed=11)
    store = DeviceClipStore.from_dataset(items, "cuda")
    ids = [-1, 2, len(store), 4, 2 ** 31 - 1, -2 ** 31]
    idx = torch.tensor(ids, dtype=torch.int32, device="cuda")
    good = [i if 0 <= i < len(store) else None for i in ids]
    out = store.gather(idx, 64, 32, out=_prefilled(store, len(ids), 64, 32))
    empty = torch.zeros(0, D)
    _check_stream(out["embeddings"], out["mask_rgb"], [items[i]["embeddings"] if i is not None else empty for i in good], 64)
    _check_stream(out["flow_embeddings"], out["mask_flow"], [items[i]["flow_embeddings"] if i is not None else empty for i in good], 32)
    want_labels = torch.stack([items[i]["labels"] if i is not None else torch.zeros(C) for i in good])
    assert torch.equal(out["labels"].cpu(), want_labels)
    assert out["max_len_rgb"].item() == 33 and out["max_len_flow"].item() == 32
    assert store.read_status() == 1                               # bad indices only: nothing was truncated
    store.reset_status()
    # T_out one below a clip's length: truncated, bit 2; the status is sticky over a clean call
    idx = torch.tensor([5, 0], dtype=torch.int32, device="cuda")
    out = store.gather(idx, 63, 63, out=_prefilled(store, 2, 63, 63))
    _check_stream(out["embeddings"], out["mask_rgb"], [items[5]["embeddings"][:63], items[0]["embeddings"]], 63)
    _check_stream(out["flow_embeddings"], out["mask_flow"], [items[5]["flow_embeddings"], items[0]["flow_embeddings"]], 63)
    assert out["max_len_rgb"].item() == 63 and out["max_len_flow"].item() == 63
    assert store.read_status() == 2
    store.gather(idx, 64, 63)
    assert store.read_status() == 2
    store.reset_status()
    assert store.read_status() == 0
    # host-side argument checks, before any launch
    out = store.alloc_out(2, 64, 63)
    arr = _stream_array(store, out, 64, 63)

    def call(streams=ctypes.addressof(arr), n_streams=2, index=idx.data_ptr(), B=2, n_videos=len(store), labels_out=out["labels"].data_ptr()):
        return _lib.lib.vmc_gather_clips(streams, n_streams, index, B, n_videos, D, store.labels.data_ptr(), labels_out, C,
                                         store.status.data_ptr(), _lib.stream())
    assert call() == 0
    E_ARG = -1
    assert call(B=0) == E_ARG and call(index=None) == E_ARG and call(n_streams=3) == E_ARG and call(n_streams=0) == E_ARG
    assert call(streams=None) == E_ARG and call(n_videos=0) == E_ARG and call(labels_out=None) == E_ARG
    for field in ("rows", "offset", "length", "out", "mask"):
        bad = _stream_array(store, out, 64, 63)
        setattr(bad[1], field, None)
        assert call(streams=ctypes.addressof(bad)) == E_ARG, field
    bad = _stream_array(store, out, 64, 0)
    assert call(streams=ctypes.addressof(bad)) == E_ARG
    torch.cuda.synchronize()
    assert store.read_status() == 0


def test_clip_stream_mirrors_the_header():
    """vmc_clip_stream (include/vmc.h) is filled from Python through the ctypes.Structure mirror ClipStream: same field names in
    the same order, six pointers and one int."""
    from vimo_clip_amd.TFAM.data.device_store import ClipStream
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vmc.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vmc_clip_stream\s*\{(.*?)\}\s*vmc_clip_stream\s*;", src, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.split(r"[\s*]+", d)[-1] for d in decls]
    assert names == [f[0] for f in ClipStream._fields_]
    for d, (name, ctype) in zip(decls, ClipStream._fields_):
        assert ctype is (ctypes.c_void_p if "*" in d else ctypes.c_int), d
        assert "*" in d or re.fullmatch(r"int\s+\w+", d), d
    assert ctypes.sizeof(ClipStream) == 56 and ClipStream.T_out.offset == 48


# ---- a step fed from the store ---------------------------------------------------------------------------------------------------

def _amo(D, H, L, FF, C, seed, **kw):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, device="cuda", **kw).cuda()
    m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, seed), strict=True)
    return m


@pytest.mark.parametrize("mode", ["cross", "concat1"])
def test_eager_step_from_store_equals_step_from_loader(mode):
    """One training step (dropout 0.1, fixed seeds) on B = 4 clips of 17..40 tokens: logits, loss and every parameter gradient are
    bit-identical whether the batch comes from the store (pool_len = the store's max_len tensor; None in concat mode, which keeps
    exact T_out) or from collate_fn_pad."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.TFAM.data import DeviceClipStore
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset, collate_fn_pad
    D, H, L, FF, C = 512, 8, 2, 1024, 140
    ds = SyntheticEmbeddingDataset(synth.multi_hot_labels(3, "st", 6, C), D, tmin=17, tmax=40, seed=21)
    ids = [4, 1, 5, 2]
    assert len({int(ds.lengths[i]) for i in ids}) > 1
    kw = dict(use_cross_attention=True) if mode == "cross" else dict(use_cross_attention=False, concat_dim=1)
    store = DeviceClipStore.from_dataset(ds, "cuda")
    runs = []
    for from_store in (False, True):
        ag.weights.clear()
        m = _amo(D, H, L, FF, C, 31, dropout=0.1, mlp_dropout=0.1, **kw).train()
        m.set_dropout_seed(77)
        if from_store:
            b = store.gather(torch.tensor(ids, dtype=torch.int32, device="cuda"), *store.padded_lengths(ids, 1))
            pool_len = b["max_len_rgb"] if m.pools_padded_tokens else None
            assert (pool_len is None) == (mode == "concat1")
        else:
            b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in collate_fn_pad([ds[i] for i in ids]).items()}
            pool_len = None
        logits = m(b["embeddings"], b["flow_embeddings"], mask_rgb=b["mask_rgb"], mask_flow=b["mask_flow"], pool_len=pool_len)
        loss = bce_with_logits_loss(logits, b["labels"])
        loss.backward()
        used = {id(p) for p in m.used_parameters()}
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if id(p) in used}
        runs.append((logits.detach().clone(), loss.detach().clone(), grads))
    (lo_l, ls_l, g_l), (lo_s, ls_s, g_s) = runs
    assert bool(torch.isfinite(lo_l).all()) and torch.equal(lo_l, lo_s) and torch.equal(ls_l, ls_s)
    assert set(g_l) == set(g_s) and len(g_l) > 10
    for k in g_l:
        assert torch.equal(g_l[k], g_s[k]), k
    assert store.read_status() == 0


# ---- the trainer ----------------------------------------------------------------------------------------------------------------

def _trainer(device_store, use_graphs, tr, va, **cfg_kw):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer
    D, H, L, FF, C = 512, 8, 2, 1024, 140
    ag.weights.clear()
    cfg = Config(epochs=2, batch_size=4, d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, device="cuda", checkpoint_dir=None,
                 use_graphs=use_graphs, graph_bucket=32, device_store=device_store, **cfg_kw)
    model = _amo(D, H, L, FF, C, 83, dropout=cfg.dropout, mlp_dropout=cfg.mlp_dropout)
    model.set_dropout_seed(cfg.seed * 1000)
    return ModelTrainer(model, tr, va, cfg), model


def _sets(n_train, n_val):
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    return (SyntheticEmbeddingDataset(synth.multi_hot_labels(1, "tr", n_train, 140), 512, seed=5, signal=0.6, class_seed=5),
            SyntheticEmbeddingDataset(synth.multi_hot_labels(2, "va", n_val, 140), 512, seed=6, signal=0.6, class_seed=5))


def test_captured_trainer_from_store_equals_trainer_from_loader():
    """ModelTrainer(use_graphs, graph_bucket=32) over two epochs of 8 steps (32 videos of 17..64 tokens, B = 4, dropout 0.1): the
    per-epoch loss and metric and every parameter after the run are bit-identical with and without device_store -- the padded
    shapes, hence the dropout element indices, are the same in both runs.  The store path captures at most one graph per distinct
    (T_rgb, T_motion) bucket pair and leaves the status word at 0."""
    from vimo_clip_amd.TFAM.train_and_eval import batches
    tr, va = _sets(32, 4)
    pairs = set()
    for epoch in (0, 1):
        order = torch.randperm(len(tr), generator=torch.Generator().manual_seed(49 + epoch)).tolist()
        for b in batches(tr, 4, order=order):
            pairs.add((-(-b["embeddings"].shape[1] // 32) * 32, -(-b["flow_embeddings"].shape[1] // 32) * 32))
    runs = []
    for device_store in (False, True):
        t, model = _trainer(device_store, True, tr, va)
        assert t.config.seed == 49 and (t._train_store is not None) == device_store
        stats = [t.train_epoch(0), t.train_epoch(1)]
        runs.append((stats, {k: v.detach().clone() for k, v in model.state_dict().items()}, t))
    (sl, wl, tl), (ss, ws, ts) = runs
    print(f"trainer, loader {sl} store {ss}; graphs: loader {tl._graphed_train.n_graphs} store {ts._graphed_train.n_graphs} "
          f"for bucket pairs {sorted(pairs)}")
    assert all(torch.isfinite(torch.tensor(s)).all() for s in sl) and sl == ss
    for k in wl:
        assert torch.equal(wl[k], ws[k]), k
    assert 1 <= ts._graphed_train.n_graphs <= len(pairs)
    assert int(ts.optimizer.dev_state[0].item()) == int(tl.optimizer.dev_state[0].item()) == 16
    assert ts._train_store.read_status() == 0 and ts._val_store.read_status() == 0


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_validation_from_store_equals_validation_from_loader(use_graphs):
    tr, va = _sets(4, 16)
    got = []
    for device_store in (False, True):
        t, _ = _trainer(device_store, use_graphs, tr, va)
        got.append(t.validate(0))
    print(f"validate use_graphs={use_graphs}: loader {got[0]} store {got[1]}")
    assert all(torch.isfinite(torch.tensor(g)).all() for g in got) and got[0] == got[1]
    assert t._val_store.read_status() == 0


def test_eager_trainer_epoch_from_store_equals_loader():
    """Without graphs the store path gathers at the batch maxima and runs the existing eager step: one epoch, same statistics and
    parameters."""
    tr, va = _sets(16, 4)
    runs = []
    for device_store in (False, True):
        t, model = _trainer(device_store, False, tr, va)
        runs.append((t.train_epoch(0), {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
