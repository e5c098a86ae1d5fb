"""Plain-torch restatement of vmc_concat_tokens_len's contract (include/vmc.h K19), clamps included: the reference of
tests/test_concat_buckets_host.py (CPU) and tests/test_gpu_concat_buckets.py (the kernel, bit for bit)."""
import torch


def clamp_lens(len_rgb, len_motion, T_rgb, T_motion, T_out):
    """(keep, nm, n) from the two lengths (None = the full tensor length), as the kernel clamps them."""
    nr = T_rgb if len_rgb is None else int(len_rgb)
    nm = T_motion if len_motion is None else int(len_motion)
    nr = min(max(nr, 1), T_rgb)
    nm = min(max(nm, 1), T_motion)
    keep = min(nr - 1, T_out)
    nm = min(nm, T_out - keep)
    return keep, nm, keep + nm


def concat_ref(rgb, motion, mask_rgb, mask_motion, T_out, len_rgb=None, len_motion=None):
    """(x [B, T_out, D], mask [B, T_out] uint8, n): x = [rgb rows 0..keep-1 | motion rows 0..nm-1 | zeros], the masks laid out the
    same way (1 where a source mask is None, 0 on the rows from n up)."""
    B, T_rgb, D = rgb.shape
    T_motion = motion.shape[1]
    keep, nm, n = clamp_lens(len_rgb, len_motion, T_rgb, T_motion, T_out)
    x = torch.zeros(B, T_out, D, dtype=rgb.dtype, device=rgb.device)
    x[:, :keep] = rgb[:, :keep]
    x[:, keep:n] = motion[:, :nm]
    mask = torch.zeros(B, T_out, dtype=torch.uint8, device=rgb.device)
    mask[:, :keep] = 1 if mask_rgb is None else mask_rgb[:, :keep].to(torch.uint8)
    mask[:, keep:n] = 1 if mask_motion is None else mask_motion[:, :nm].to(torch.uint8)
    return x, mask, n
