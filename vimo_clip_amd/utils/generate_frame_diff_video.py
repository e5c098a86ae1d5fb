"""Frame-difference motion frames of an RGB video — drop-in for the reference's utils/generate_frame_diff_video.py.

The reference reads a video with OpenCV on one CPU thread, takes ``cv2.absdiff`` of consecutive ``COLOR_BGR2GRAY`` frames and
writes the result through a lossy H.264 encoder.  Here the grey conversion and the difference run on the GPU
(``ops.frame_diff_gray``, vmc_frame_diff_gray_u8) in chunks, and the result is stored as an exact ``[T-1,H,W,3]`` u8 ``.npy``
stack (three identical channels, what a decoder hands back for a grey video) that ``open_video`` reads: there is no codec here.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .. import ops
from ..extract_embeddings import open_video


def npy_path(output_path: str) -> str:
    """Where the stack of ``output_path`` is stored: the path itself when it ends in ``.npy``, else ``output_path + ".npy"``
    (the first candidate ``open_video(output_path)`` looks for)."""
    return output_path if output_path.endswith(".npy") else output_path + ".npy"


@torch.no_grad()
def compute_frame_difference(video_path, output_path, frame_source=None, chunk_size=256, device="cuda"):
    """utils/generate_frame_diff_video.py:7-60: ``|gray(frame[t+1]) - gray(frame[t])|`` for every consecutive pair of frames.

    This is the reference's arithmetic BEFORE its lossy encode: the reference writes the difference frames through H.264
    (``cv2.VideoWriter(..., "avc1")``) and its consumers decode that file, so their pixels carry codec error; the stack written
    here holds the exact differences.  The grey weights are OpenCV 4.x's 8-bit ``COLOR_BGR2GRAY`` (ops.GRAY_WEIGHTS_CV8).

    Writes ``npy_path(output_path)``, a ``[T-1,H,W,3]`` u8 stack, and returns its path; a video with fewer than two frames writes
    nothing and returns ``None`` (the reference prints an error and returns)."""
    vr = (frame_source or open_video)(video_path)
    total = len(vr)
    if total < 2:
        print(f"Error: fewer than two frames in {video_path}")
        return None
    dst, stack, prev, row = npy_path(output_path), None, None, 0
    out_dir = os.path.dirname(dst)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    for lo in range(0, total, chunk_size):
        frames = vr.get_batch(np.arange(lo, min(total, lo + chunk_size)))          # [n,H,W,3] u8
        if not torch.is_tensor(frames):
            frames = torch.from_numpy(np.asarray(frames))
        frames = frames.to(device)
        diff = ops.frame_diff_gray(frames, prev, channels=1, layout="nhwc")         # [n_out,1,H,W]
        prev = frames[-1].clone()
        if diff.shape[0] == 0:
            continue
        if stack is None:
            stack = np.lib.format.open_memmap(dst, mode="w+", dtype=np.uint8, shape=(total - 1,) + tuple(frames.shape[1:3]) + (3,))
        stack[row:row + diff.shape[0]] = diff[:, 0].cpu().numpy()[..., None]
        row += diff.shape[0]
    stack.flush()
    del stack
    print(f"Successfully created frame difference stack: {dst}")
    return dst


def main():
    """Same command line as the reference script (--input_dir, --output_dir, --video_list_file)."""
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--input_dir", required=True, help="folder with the RGB videos (or their .npy frame stacks)")
    ap.add_argument("--output_dir", required=True, help="folder that receives one difference stack per video")
    ap.add_argument("--video_list_file", required=True, help="text file, one video file name per line")
    ap.add_argument("--chunk_size", type=int, default=256, help="frames per device pass")
    args = ap.parse_args()
    with open(args.video_list_file) as f:
        names = [ln.strip() for ln in f if ln.strip()]
    for name in names:
        src = os.path.join(args.input_dir, name)
        if not any(os.path.exists(c) for c in (src, src + ".npy", os.path.splitext(src)[0] + ".npy")):
            print(f"Warning: no such video, skipped: {src}")
            continue
        compute_frame_difference(src, os.path.join(args.output_dir, name), chunk_size=args.chunk_size)


if __name__ == "__main__":
    main()
