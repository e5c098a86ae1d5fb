"""CPU: the dispatch plans of the fused TFAM chains, vimo_clip_amd/csrc/tfam_route.h (tests/host/test_tfam_route.cpp), and the
Python gates over the library's own answer (vmc_tfam_supported: host only, no device)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tfam_route(tmp_path):
    exe = str(tmp_path / "test_tfam_route")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "test_tfam_route.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "OK" in out.stdout


def _model(D, H, ff, L, C, **kw):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    return AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=ff, num_classes=C, device="cpu", **kw)


# (D, H, ff, L, C), (B, T, Tk, cross), eval chain takes it, training chains take it
SHAPES = [
    ((512, 8, 512, 1, 140), (2, 16, 16, True), True, True),
    ((512, 8, 512, 1, 140), (2, 64, 33, True), True, True),
    ((512, 8, 512, 1, 140), (2, 65, 16, True), False, False),          # more than 64 tokens per clip
    ((512, 8, 512, 1, 140), (2, 16, 65, True), False, False),
    ((512, 8, 512, 1, 140), (2, 16, 65, False), True, True),           # Tk does not matter without cross attention
    ((512, 8, 512, 1, 140), (16, 16, 16, True), True, True),
    ((512, 8, 512, 1, 140), (17, 16, 16, True), False, False),         # MAX_ROWS: the per-op path wins (the C ABI would take it)
    ((512, 8, 512, 1, 140), (33, 4, 4, True), True, False),            # more than 32 clips
    ((512, 8, 512, 1, 140), (8, 16, 33, True), True, False),           # more than 256 motion rows
    ((512, 8, 512, 1, 141), (2, 16, 16, True), True, False),           # class count not a multiple of 4
    ((512, 8, 512, 1, 480), (2, 16, 16, True), True, True),
    ((512, 8, 512, 1, 484), (2, 16, 16, True), True, False),           # the head backward's dlogits rows leave its LDS
    ((768, 12, 512, 1, 140), (2, 16, 26, True), True, True),
    ((768, 12, 512, 1, 140), (2, 16, 27, True), False, False),         # two clips' keys per row block do not fit beside the W tile
    ((768, 8, 1000, 1, 140), (2, 16, 16, True), False, False),         # dim_feedforward not a multiple of 512
    ((768, 6, 512, 1, 140), (2, 16, 16, True), False, False),          # head dim 128
]


@pytest.mark.parametrize("cfg,batch,want_eval,want_train", SHAPES)
def test_supported_is_the_library_answer_and_the_policy(cfg, batch, want_eval, want_train):
    from vimo_clip_amd import tfam_fused, tfam_train
    from vimo_clip_amd._lib import lib
    D, H, ff, L, C = cfg
    B, T, Tk, cross = batch
    m = _model(D, H, ff, L, C)
    policy = B * T <= tfam_fused.MAX_ROWS
    for train, fn, want in ((0, tfam_fused.supported, want_eval), (1, tfam_train.supported, want_train)):
        rc = lib.vmc_tfam_supported(B, T, Tk, D, H, ff, L, C, int(cross), train)
        assert fn(m, B, T, Tk, cross) == (rc == 0 and policy)
        assert fn(m, B, T, Tk, cross) == want
        # the workspace query of the training chains knows the same set
        if train:
            assert (lib.vmc_tfam_train_workspace_bytes(B, T, Tk, D, H, ff, L, C, int(cross)) > 0) == (rc == 0)
            assert (lib.vmc_tfam_train_pool_grad_offset(B, T, Tk, D, H, ff, L, C, int(cross)) >= 0) == (rc == 0)


def test_supported_needs_the_relu_feed_forward():
    from vimo_clip_amd import tfam_fused, tfam_train
    m = _model(512, 8, 512, 1, 140)
    assert tfam_fused.supported(m, 2, 16, 16, True) and tfam_train.supported(m, 2, 16, 16, True)
    m.layers[0].ffn_act = 2
    assert not tfam_fused.supported(m, 2, 16, 16, True) and not tfam_train.supported(m, 2, 16, 16, True)
