"""CPU: the input-gradient section of vimo_clip_amd/csrc/tfam_route.h (tests/host/test_tfam_input_route.cpp), the library's answers
about it, the model switch, and the float64 restatement of the concatenation backward against autograd of the reference
concatenation (host only, no device)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from concat_bwd_ref import concat_bwd_ref      # noqa: E402
from concat_ref import concat_ref              # noqa: E402


def test_tfam_input_route(tmp_path):
    exe = str(tmp_path / "test_tfam_input_route")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "test_tfam_input_route.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "OK" in out.stdout


def test_new_symbols_resolve():
    from vimo_clip_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vmc_tfam_input_grad_supported", "vmc_tfam_train_input_workspace_bytes", "vmc_tfam_train_input_grad_offsets",
                 "vmc_tfam_train_bwd_inputs_len", "vmc_tfam_layer_bwd_inputs", "vmc_tfam_train_bwd_inputs_proj",
                 "vmc_tfam_layer0_bwd_proj_inputs", "vmc_concat_tokens_len_bwd"):
        assert hasattr(lib, name), name


# (D, H, ff, L, C), (B, T, Tk), cross, proj, taken
SHAPES = [
    ((512, 8, 2048, 4, 140), (8, 16, 15), True, False, True),
    ((768, 8, 512, 2, 8), (2, 16, 15), True, False, True),
    ((512, 8, 512, 2, 8), (2, 16, 0), False, False, True),
    ((768, 12, 2048, 4, 140), (8, 15, 0), False, True, True),
    ((512, 8, 512, 8, 140), (2, 16, 0), False, True, False),          # the projection mode's depth limit
    ((512, 8, 512, 1, 140), (17, 16, 15), True, False, False),        # more than 256 token rows
    ((512, 8, 512, 1, 140), (2, 65, 15), True, False, False),         # more than 64 tokens per clip
]


@pytest.mark.parametrize("cfg,batch,cross,proj,want", SHAPES)
def test_library_answers(cfg, batch, cross, proj, want):
    from vimo_clip_amd import tfam_train
    from vimo_clip_amd._lib import lib
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    D, H, ff, L, C = cfg
    B, T, Tk = batch
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=ff, num_classes=C, device="cpu", use_cross_attention=cross,
                 concat_dim=-1 if proj else 1)
    args = (B, T, Tk, D, H, ff, L, C, int(cross), int(proj))
    assert (lib.vmc_tfam_input_grad_supported(*args) == 0) == want == tfam_train.supported_inputs(m, B, T, Tk, cross, proj)
    nbytes = lib.vmc_tfam_train_input_workspace_bytes(*args)
    offs = (ctypes.c_longlong * 3)(7, 7, 7)
    rc = lib.vmc_tfam_train_input_grad_offsets(*args, offs)
    assert (nbytes > 0) == (rc == 0) == want
    if not want:
        assert list(offs) == [-1, -1, -1]
        return
    al = lambda n: (n + 255) // 256 * 256
    M, Mk = B * T, B * Tk
    if proj:      # behind the projection's extension, which is what it was
        base = lib.vmc_tfam_train_proj_workspace_bytes(B, T, D, H, ff, L, C)
        assert base > 0 and list(offs) == [-1, -1, base] and nbytes == base + al(M * 2 * D * 4)
    else:         # behind the training workspace, which is what it was
        base = lib.vmc_tfam_train_workspace_bytes(*args[:9])
        assert base > 0 and offs[0] == base and offs[2] == -1
        assert offs[1] == (base + al(M * D * 4) if cross else -1)
        assert nbytes == base + al(M * D * 4) + (al(Mk * D * 4) if cross else 0)


def test_the_switch_is_off_by_default():
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    m = AMO_CLIP(d_model=512, nhead=8, num_layers=1, dim_feedforward=512, device="cpu", use_cross_attention=False, concat_dim=1)
    assert m.fused_input_grads is False
    rgb = torch.zeros(2, 5, 512, requires_grad=True)
    with pytest.raises(ValueError, match="must not require grad"):      # off: forward(token_lens=...) refuses, as it always has
        m(rgb, torch.zeros(2, 4, 512), token_lens=(5, 4))


# (T_rgb, T_motion, T_out, n_rgb, n_motion)
CONCAT_CASES = [
    (6, 5, 10, 1, 3),          # n_rgb = 1: nothing of RGB survives
    (6, 5, 10, 4, 0),          # n_motion = 0 (the kernel's clamp makes it 1, as in the forward)
    (6, 5, 10, 6, 5),          # both at their padded maxima
    (6, 5, 16, 3, 2),          # T_out larger than the real rows
    (6, 5, 16, None, None),    # no device lengths: the tensors' own
    (6, 5, 4, 5, 5),           # T_out cuts the motion rows
]


@pytest.mark.parametrize("T_rgb,T_motion,T_out,n_rgb,n_motion", CONCAT_CASES)
def test_concat_backward_reference_is_autograd_of_the_forward_reference(T_rgb, T_motion, T_out, n_rgb, n_motion):
    g = torch.Generator().manual_seed(T_out * 100 + (n_rgb or 0) * 10 + (n_motion or 0))
    B, D = 3, 8
    rgb = torch.randn(B, T_rgb, D, dtype=torch.float64, generator=g).requires_grad_()
    motion = torch.randn(B, T_motion, D, dtype=torch.float64, generator=g).requires_grad_()
    dx = torch.randn(B, T_out, D, dtype=torch.float64, generator=g)
    x, _, _ = concat_ref(rgb, motion, None, None, T_out, n_rgb, n_motion)
    want_rgb, want_motion = torch.autograd.grad(x, (rgb, motion), dx, allow_unused=True)
    want_rgb = torch.zeros_like(rgb) if want_rgb is None else want_rgb
    want_motion = torch.zeros_like(motion) if want_motion is None else want_motion
    got_rgb, got_motion = concat_bwd_ref(dx, T_rgb, T_motion, n_rgb, n_motion)
    assert torch.equal(got_rgb, want_rgb) and torch.equal(got_motion, want_motion)
    assert not got_rgb[:, T_rgb - 1].any()                     # the dropped last RGB row
