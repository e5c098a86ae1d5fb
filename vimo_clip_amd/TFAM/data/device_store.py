"""Device-resident TFAM embedding store: every video's token rows in device memory, batches assembled there by one kernel
(vmc_gather_clips, include/vmc.h K17) instead of ``HDF5VideoDataset.__getitem__`` + ``collate_fn_pad`` on the host per step.

The Animal-Kingdom embedding set is 30 100 videos of at most 64 rows: both token streams take ~8 GB at 512 floats per row, on a
288 GB card.  A training step then needs B int32 indices and nothing else from the host, so a captured step
(graphs.GraphedTrainStep) can contain its own batch assembly.  ``device="cpu"`` builds and inspects a store; ``gather`` needs the
device -- there is no CPU fallback, as elsewhere in the package.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .dataset import sparse_sampling


class ClipStream(ctypes.Structure):
    """ctypes mirror of ``vmc_clip_stream`` (include/vmc.h): same fields in the same order."""
    _fields_ = [("rows", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("length", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("max_len", ctypes.c_void_p), ("T_out", ctypes.c_int)]


class _Stream:
    """One token stream of a store: ``rows`` [total_rows, D] fp32 (the videos' rows back to back), ``offset`` [N] int64 (first row
    of video i) and ``length`` [N] int32 on the store's device; ``length_host``: the lengths as a numpy array."""

    def __init__(self, clips, D):
        self.length_host = np.array([c.shape[0] for c in clips], dtype=np.int32)
        off = np.zeros(len(clips), dtype=np.int64)
        np.cumsum(self.length_host[:-1], out=off[1:])
        self.rows = torch.cat([c.reshape(-1, D) for c in clips], dim=0).contiguous() if clips else torch.zeros(0, D)
        self.offset, self.length = torch.from_numpy(off), torch.from_numpy(self.length_host.copy())

    def to(self, device):
        self.rows, self.offset, self.length = self.rows.to(device), self.offset.to(device), self.length.to(device)
        return self

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.rows, self.offset, self.length))


def _bucketed(n, bucket):
    return -(-n // bucket) * bucket if bucket > 1 else n


class DeviceClipStore:
    """``rgb`` / ``motion``: the two token streams (``_Stream``; ``motion`` is None for a single-stream store), ``labels`` [N, C]
    fp32 on the device (None without labels); on the host ``video_ids``, ``total_frames`` and the streams' ``length_host``.
    ``status``: one int32 on the device, OR-ed by every ``gather`` (bit 1: an index outside the store, bit 2: a clip longer than
    T_out was truncated); ``read_status()`` / ``reset_status()``."""

    def __init__(self, rgb_clips, motion_clips=None, labels=None, video_ids=None, total_frames=None, device="cuda", motion_key="flow",
                 max_bytes=None):
        rgb_clips = [torch.as_tensor(c).float() for c in rgb_clips]
        if not rgb_clips or sum(c.shape[0] for c in rgb_clips) == 0:
            raise ValueError("DeviceClipStore: no token rows to store")
        self.D = int(rgb_clips[0].shape[-1])
        self.motion_key, self.device = motion_key, torch.device(device)
        if motion_clips is not None:
            motion_clips = [torch.as_tensor(c).float() for c in motion_clips]
            if len(motion_clips) != len(rgb_clips):
                raise ValueError("DeviceClipStore: one motion clip per RGB clip")
        for c in rgb_clips + (motion_clips or []):
            if c.dim() != 2 or c.shape[1] != self.D:
                raise ValueError(f"DeviceClipStore: clips must be [T, {self.D}], got {tuple(c.shape)}")
        need = 4 * self.D * sum(c.shape[0] for c in rgb_clips + (motion_clips or []))
        if labels is not None:
            labels = torch.as_tensor(labels).float().reshape(len(rgb_clips), -1).contiguous()
            need += 4 * labels.numel()
        need += 12 * len(rgb_clips) * (1 if motion_clips is None else 2)
        self._check_budget(need, max_bytes)
        self.rgb = _Stream(rgb_clips, self.D).to(self.device)
        self.motion = _Stream(motion_clips, self.D).to(self.device) if motion_clips is not None else None
        if self.motion is not None and self.motion.rows.shape[0] == 0:
            raise ValueError("DeviceClipStore: the motion stream has no rows")
        self.labels = labels.to(self.device) if labels is not None else None
        self.C = int(labels.shape[1]) if labels is not None else 0
        self.video_ids = list(video_ids) if video_ids is not None else [f"v{i:06d}" for i in range(len(rgb_clips))]
        self.total_frames = list(total_frames) if total_frames is not None else self.rgb.length_host.tolist()
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    @staticmethod
    def _check_budget(need, max_bytes):
        if max_bytes is not None and need > max_bytes:
            raise MemoryError(f"DeviceClipStore: the store needs {need} bytes, max_bytes allows {max_bytes}")

    # ---- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def _from_items(cls, items, device, motion_key, max_bytes):
        rgb, mot, lab, ids, frames, need = [], [], [], [], [], 0
        for it in items:
            r, m = it["embeddings"], it[f"{motion_key}_embeddings"]
            need += 4 * (r.numel() + m.numel() + it["labels"].numel()) + 24
            cls._check_budget(need, max_bytes)                   # stop reading as soon as the budget is exceeded
            rgb.append(r), mot.append(m), lab.append(torch.as_tensor(it["labels"]).float())
            ids.append(it["video_id"]), frames.append(int(it["total_frames"]))
        return cls(rgb, mot, torch.stack(lab), ids, frames, device=device, motion_key=motion_key, max_bytes=max_bytes)

    @classmethod
    def from_dataset(cls, dataset, device, motion_key="flow", max_bytes=None):
        """Any map-style dataset returning the item dict of HDF5VideoDataset / SyntheticEmbeddingDataset; read once, in index order."""
        return cls._from_items((dataset[i] for i in range(len(dataset))), device, motion_key, max_bytes)

    @classmethod
    def from_hdf5(cls, hdf5_path, flow_path, transform=None, num_frames=None, max_frames=None, device="cuda", motion_key="flow",
                  max_bytes=None):
        """What ``HDF5VideoDataset(hdf5_path, flow_path, transform, num_frames, max_frames)[i]`` returns for every i, with each
        file opened ONCE: the motion group is ``key.split(".")[0]``, the ``max_frames`` key filter, ``sparse_sampling`` (torch.linspace
        itself), ``transform`` and ``.float()`` are all deterministic per video, so the store holds the items row for row."""
        from ... import h5lite as h5py

        def items():
            with h5py.File(hdf5_path, "r") as f, h5py.File(flow_path, "r") as g:
                keys = list(f.keys())
                if max_frames:
                    keys = [k for k in keys if f[k]["embeddings"].shape[0] < max_frames]
                for k in keys:
                    emb = torch.from_numpy(f[k]["embeddings"][:])
                    labels = torch.from_numpy(f[k]["labels"][:])
                    mot = torch.from_numpy(g[k.split(".")[0]]["embeddings"][:])
                    if num_frames:
                        emb, mot = sparse_sampling(emb, num_frames), sparse_sampling(mot, num_frames)
                    if transform:
                        emb, mot = transform(emb), transform(mot)
                    yield {"video_id": k, "embeddings": emb.float(), f"{motion_key}_embeddings": mot.float(), "labels": labels,
                           "total_frames": emb.shape[0]}

        return cls._from_items(items(), device, motion_key, max_bytes)

    # ---- inspection ---------------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.video_ids)

    @property
    def nbytes(self):
        n = self.rgb.nbytes + (self.motion.nbytes if self.motion is not None else 0)
        return n + (self.labels.numel() * 4 if self.labels is not None else 0)

    def read_status(self) -> int:
        """The sticky status word (synchronises: call it once per epoch, not per step)."""
        return int(self.status.item())

    def reset_status(self):
        self.status.zero_()

    def padded_lengths(self, index_host, bucket=1):
        """(T_rgb, T_motion) for the videos ``index_host`` (host integers): the batch maxima from the host length arrays, each
        rounded up to its own multiple of ``bucket`` -- the shapes ``graphs.pad_to_bucket(collate_fn_pad(...))`` produces."""
        idx = np.asarray(index_host, dtype=np.int64)
        tr = _bucketed(max(1, int(self.rgb.length_host[idx].max())), int(bucket))
        if self.motion is None:
            return tr, None
        return tr, _bucketed(max(1, int(self.motion.length_host[idx].max())), int(bucket))

    # ---- batch assembly -----------------------------------------------------------------------------------------------------
    def _keys(self):
        mk = self.motion_key
        return ("embeddings", "mask_rgb", "max_len_rgb"), (f"{mk}_embeddings", f"mask_{mk}", f"max_len_{mk}")

    def alloc_out(self, B, T_rgb, T_motion=None):
        """Caller-owned output buffers of one ``gather`` shape (what a captured step keeps as its static batch)."""
        dev, out = self.device, {}
        streams = [(self._keys()[0], T_rgb)] + ([(self._keys()[1], T_motion)] if self.motion is not None else [])
        for (ke, km, kl), T in streams:
            out[ke] = torch.empty(B, int(T), self.D, dtype=torch.float32, device=dev)
            out[km] = torch.empty(B, int(T), dtype=torch.bool, device=dev)          # one byte holding 0 / 1, as collate_fn_pad's masks
            out[kl] = torch.empty(1, dtype=torch.int32, device=dev)
        if self.labels is not None:
            out["labels"] = torch.empty(B, self.C, dtype=torch.float32, device=dev)
        return out

    def gather(self, index, T_rgb, T_motion=None, out=None):
        """The batch ``collate_fn_pad([dataset[i] for i in index])`` zero-padded to (T_rgb, T_motion), assembled on the device by
        one launch: ``embeddings`` [B, T_rgb, D], ``{mk}_embeddings`` [B, T_motion, D], ``mask_rgb`` / ``mask_{mk}`` (bool, True =
        real token), ``labels`` [B, C], plus ``max_len_rgb`` / ``max_len_{mk}``: one-element int32 tensors holding the batch's own
        length, what ``AMO_CLIP.forward(pool_len=...)`` takes.  ``index``: int32 device tensor [B].  ``out``: buffers from
        ``alloc_out`` to write into (a captured step); fresh ones otherwise.  Only enqueues; clips longer than T_out are
        truncated and indices outside the store give empty clips, both recorded in ``status``."""
        if self.device.type != "cuda":
            raise RuntimeError("DeviceClipStore.gather needs a store on the GPU: libvmc kernels have no CPU path")
        from ... import _lib
        if index.dtype != torch.int32 or index.dim() != 1 or not index.is_cuda or not index.is_contiguous():
            raise ValueError("DeviceClipStore.gather: index must be a contiguous int32 device tensor of shape [B]")
        B = int(index.shape[0])
        if self.motion is not None and T_motion is None:
            raise ValueError("DeviceClipStore.gather: T_motion is required for a two-stream store")
        if out is None:
            out = self.alloc_out(B, T_rgb, T_motion)
        streams = [(self.rgb, self._keys()[0], T_rgb)] + ([(self.motion, self._keys()[1], T_motion)] if self.motion is not None else [])
        arr = (ClipStream * len(streams))()
        for q, (s, (ke, km, kl), T) in enumerate(streams):
            e, m, n = out[ke], out[km], out[kl]
            if tuple(e.shape) != (B, int(T), self.D) or tuple(m.shape) != (B, int(T)) or not (e.is_contiguous() and m.is_contiguous()) \
                    or e.dtype != torch.float32 or m.element_size() != 1 or n.dtype != torch.int32:
                raise ValueError(f"DeviceClipStore.gather: output buffers do not match B = {B}, T = {T}, D = {self.D}")
            arr[q] = ClipStream(_lib.ptr(s.rows), _lib.ptr(s.offset), _lib.ptr(s.length), _lib.ptr(e), _lib.ptr(m), _lib.ptr(n), int(T))
        lab_out = out["labels"] if self.labels is not None else None
        if lab_out is not None and (tuple(lab_out.shape) != (B, self.C) or lab_out.dtype != torch.float32 or not lab_out.is_contiguous()):
            raise ValueError("DeviceClipStore.gather: labels buffer must be [B, C] fp32")
        _lib.check(_lib.lib.vmc_gather_clips(ctypes.addressof(arr), len(streams), _lib.ptr(index), B, len(self), self.D,
                                             _lib.ptr(self.labels), _lib.ptr(lab_out), self.C, _lib.ptr(self.status), _lib.stream()),
                   "gather_clips")
        return out
