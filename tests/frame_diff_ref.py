"""numpy reference of vmc_frame_diff_gray_u8 (include/vmc.h): integer arithmetic in int64, shared by the host and the GPU tests."""
import numpy as np

CV8 = (9798, 19235, 3735, 15)        # OpenCV 4.x 8-bit COLOR_BGR2GRAY (R, G, B, shift)
BITS14 = (4899, 9617, 1868, 14)      # the 14-bit constants


def gray(rgb, weights=CV8):
    """[..., 3] u8 (channels last) -> [...] int64."""
    wr, wg, wb, shift = weights
    v = rgb.astype(np.int64)
    return (wr * v[..., 0] + wg * v[..., 1] + wb * v[..., 2] + (1 << (shift - 1))) >> shift


def frame_diff(frames_nhwc, prev=None, channels=1, weights=CV8):
    """[T,H,W,3] u8 (+ prev [H,W,3]) -> [n_out, channels, H, W] u8."""
    f = frames_nhwc if prev is None else np.concatenate([prev[None], frames_nhwc], axis=0)
    g = gray(f, weights)
    d = np.abs(g[1:] - g[:-1]).astype(np.uint8)
    return np.repeat(d[:, None], channels, axis=1)
