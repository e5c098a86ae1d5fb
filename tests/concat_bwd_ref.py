"""Plain-torch restatement of vmc_concat_tokens_len_bwd's contract (include/vmc.h K19, backward), clamps included: the reference of
tests/test_host_tfam_input_route.py (CPU, against autograd of tests/concat_ref.py) and tests/test_gpu_tfam_input_grads.py (the kernel)."""
import torch

from concat_ref import clamp_lens


def concat_bwd_ref(dx, T_rgb, T_motion, len_rgb=None, len_motion=None):
    """(d rgb [B, T_rgb, D], d motion [B, T_motion, D]) from dx [B, T_out, D]: rows 0..keep-1 go to rgb, rows keep..n-1 to motion, every
    other row of both (the dropped last RGB row included) is zero."""
    B, T_out, D = dx.shape
    keep, nm, n = clamp_lens(len_rgb, len_motion, T_rgb, T_motion, T_out)
    drgb = torch.zeros(B, T_rgb, D, dtype=dx.dtype, device=dx.device)
    dmotion = torch.zeros(B, T_motion, D, dtype=dx.dtype, device=dx.device)
    drgb[:, :keep] = dx[:, :keep]
    dmotion[:, :nm] = dx[:, keep:n]
    return drgb, dmotion
