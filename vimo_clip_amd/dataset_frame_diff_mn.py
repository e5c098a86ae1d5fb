"""MammalNet student dataset — drop-in for the reference's dataset_frame_diff_mn.py (HDF5VideoDataset + collate_fn).

Same constructor, item keys (``video_id, rgb_emb, frame_diff, labels``) and rules: the ``trimmed_videos/<id>`` HDF5 layout, only the
embedding rows of one segment read (h5lite reads the row slice, not the dataset), a decoded segment of frames padded by repeating
its last frame, bilinear resize to ``spatial_size``, float frames in [0,1].  The integer contracts are pure functions so they are
tested without HDF5 or a codec.  Video decode stays host-side I/O (dataset.read_video_frames, with its ``.npy`` stand-in offline).

Two additions for the device: ``raw_u8=True`` keeps the decoded u8 frames unresized, and ``collate_fn_device`` uploads them (1 B per
sample instead of 4 B per resized sample) and resizes + quantises on the GPU (ops.resize_bilinear_u8, bit-exact with the host path
followed by the student's ``to_pil_image``) into one u8 batch, consumed with ``model(batch["frame_diff"], unit_u8=True)``.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from .dataset import read_video_frames


def build_segments_mn(lengths: dict, sequence_length: int) -> list:
    """dataset_frame_diff_mn.py:40-50.  lengths: {video_id: T}.  Non-overlapping windows (vid, start, min(L, T - start)); T == 0 videos
    are skipped."""
    segments = []
    for vid, T in lengths.items():
        start = 0
        while start < T:
            seg_len = min(sequence_length, T - start)
            segments.append((vid, start, seg_len))
            start += seg_len
    return segments


def frame_diff_len(seg_len: int, sequence_length: int) -> int:
    """dataset_frame_diff_mn.py:115: seg_len - 1 frames for a full segment, L - 1 for a padded one."""
    return seg_len - 1 if seg_len == sequence_length else sequence_length - 1


def pad_rgb_segment(rgb_seq: torch.Tensor, seg_len: int, sequence_length: int, embed_dim: int) -> torch.Tensor:
    """dataset_frame_diff_mn.py:105-109: pad to sequence_length rows by repeating the last row."""
    leftover = sequence_length - seg_len
    if leftover > 0:
        pad = rgb_seq[-1:].repeat(leftover, 1) if seg_len > 0 else torch.zeros((leftover, embed_dim))
        rgb_seq = torch.cat([rgb_seq, pad], dim=0)
    return rgb_seq


def slice_video_segment(video_thwc: torch.Tensor, start_idx: int, n_frames: int) -> torch.Tensor:
    """dataset_frame_diff_mn.py:57-80 on decoded frames [T,H,W,3] u8: frames start .. start + n - 1 as a [n,3,H,W] view, padded by
    repeating the last decoded one; ``zeros(n,3,1,1)`` when there are none."""
    frames = video_thwc[start_idx:start_idx + n_frames].permute(0, 3, 1, 2)
    if frames.shape[0] == 0:
        return torch.zeros((n_frames, 3, 1, 1), dtype=torch.uint8)
    if frames.shape[0] < n_frames:
        frames = torch.cat([frames, frames[-1:].repeat(n_frames - frames.shape[0], 1, 1, 1)], dim=0)
    return frames


class HDF5VideoDataset(Dataset):
    """Same constructor, item keys and semantics as the reference class (dataset_frame_diff_mn.py:12-125)."""

    def __init__(self, clip_embeddings_dir, frame_diff_videos_dir, sequence_length=2, spatial_size=(224, 224), transform=None, *,
                 raw_u8=False):
        super().__init__()
        from . import h5lite as h5py          # native reader of the reference's HDF5 layout (h5py itself is not needed)
        self.hdf5_path, self.frame_diff_videos_dir = clip_embeddings_dir, frame_diff_videos_dir
        self.sequence_length, self.spatial_size, self.transform, self.raw_u8 = sequence_length, tuple(spatial_size), transform, raw_u8
        with h5py.File(self.hdf5_path, "r") as f:
            lengths = {vid: grp["embeddings"].shape[0] for vid, grp in f["trimmed_videos"].items()}
        self.segments = build_segments_mn(lengths, sequence_length)

    def __len__(self):
        return len(self.segments)

    @staticmethod
    def _read_video_segment(path: str, start_idx: int, n_frames: int) -> torch.Tensor:
        return slice_video_segment(read_video_frames(path), start_idx, n_frames)

    def _resize_frames(self, frames: torch.Tensor) -> torch.Tensor:
        """[T,3,H,W] u8 -> f32 in [0,1] at spatial_size (dataset_frame_diff_mn.py:82-91; a same-size input is only divided)."""
        if tuple(frames.shape[2:]) == self.spatial_size:
            return frames.to(torch.float32) / 255.0
        return F.interpolate(frames.to(torch.float32) / 255.0, size=self.spatial_size, mode="bilinear", align_corners=False)

    def __getitem__(self, idx):
        from . import h5lite as h5py
        video_id, start_idx, seg_len = self.segments[idx]
        with h5py.File(self.hdf5_path, "r") as f:
            grp = f[f"trimmed_videos/{video_id}"]
            emb_ds = grp["embeddings"]
            rgb_seq = torch.from_numpy(emb_ds[start_idx:start_idx + seg_len])          # the segment's rows only
            embed_dim = emb_ds.shape[1]
            labels = torch.from_numpy(grp["labels"][:])
        rgb_seq = pad_rgb_segment(rgb_seq, seg_len, self.sequence_length, embed_dim)
        if self.transform:
            rgb_seq = self.transform(rgb_seq)
        fd_len = frame_diff_len(seg_len, self.sequence_length)
        frame_diff = self._read_video_segment(os.path.join(self.frame_diff_videos_dir, video_id), start_idx, fd_len)
        if not self.raw_u8:
            frame_diff = self._resize_frames(frame_diff)
        return {"video_id": video_id, "rgb_emb": rgb_seq, "frame_diff": frame_diff, "labels": labels}


def collate_fn(samples):
    """dataset_frame_diff_mn.py:129-139."""
    return {"video_id": [s["video_id"] for s in samples],
            "rgb_emb": torch.stack([s["rgb_emb"] for s in samples], dim=0),
            "frame_diff": torch.stack([s["frame_diff"] for s in samples], dim=0),
            "labels": torch.stack([s["labels"] for s in samples], dim=0)}


def collate_fn_device(samples, spatial_size, device, recipe="aten"):
    """Batch of ``raw_u8`` samples (unresized u8 frames, source sizes may differ): every sample's frames are uploaded as they are and
    resized + quantised on the device into its slice of ``frame_diff`` u8 [B, L-1, 3, OH, OW] -- the pixels ``to_pil_image`` makes of
    the host path's float frames.  Consume with ``model(batch["frame_diff"], unit_u8=True)``.
    recipe: which of aten's two operation orders to reproduce (ops.resize_bilinear_u8): "aten" is what ``_resize_frames`` computes in
    this (multi-threaded) process, "weights4" what it computes in a one-thread DataLoader worker of the reference."""
    from . import ops
    OH, OW = (int(v) for v in spatial_size)
    n = samples[0]["frame_diff"].shape[0]
    batch = torch.empty((len(samples), n, 3, OH, OW), dtype=torch.uint8, device=device)
    for b, s in enumerate(samples):
        fr = s["frame_diff"]
        if fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[0] != n or fr.shape[1] != 3:
            raise ValueError(f"collate_fn_device needs raw_u8 samples of {n} frames [n,3,H,W] u8, got {tuple(fr.shape)} {fr.dtype}")
        if n:
            ops.resize_bilinear_u8(fr.to(device), (OH, OW), out=batch[b], as_u8=True, recipe=recipe)
    return {"video_id": [s["video_id"] for s in samples],
            "rgb_emb": torch.stack([s["rgb_emb"] for s in samples], dim=0),
            "frame_diff": batch,
            "labels": torch.stack([s["labels"] for s in samples], dim=0)}
