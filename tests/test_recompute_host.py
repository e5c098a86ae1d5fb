"""CPU: the recompute switch of the student's ViT and the byte model of its training forward (autograd_vit.saved_activation_bytes).
The expected integers are worked out by hand from the save_for_backward calls of autograd_ops, per token row of a block with width D
and H heads (fp32 stream, 16-bit activations):
  attention half: stream at ln_1 4 D + ln_1 output 2 D + qkv 6 D + attention output 2 D = 14 D, lse 4 H, (mean, rstd) 8
  MLP half:       stream at ln_2 4 D + ln_2 output 2 D + z 8 D + u 8 D = 22 D, (mean, rstd) 8
With the class-rows shortcut the last block keeps its attention half for all rows and, per frame, a gathered class row of the
attention output (2 D) plus the MLP half."""
import pytest
import torch

from vimo_clip_amd.autograd_vit import saved_activation_bytes, vit_tokens_train
from vimo_clip_amd.clip_vit import VisionTransformer

# name -> (rows per frame, none without the shortcut, none with it, block)
EXPECTED = {
    # B/32: D 768, H 12, 12 blocks, 50 rows.  Row: 36 * 768 + 48 + 16 = 27712; block of 50 rows: 1385600
    #   shortcut: 11 * 1385600 + 50 * (14 * 768 + 48 + 8) + (2 * 768 + 22 * 768 + 8) = 15241600 + 540400 + 18440
    "ViT-B/32": (50, 16627200, 15800440, 12 * 50 * 4 * 768),
    # L/14: D 1024, H 16, 24 blocks, 257 rows.  Row: 36864 + 64 + 16 = 36944; block: 9494608
    #   shortcut: 23 * 9494608 + 257 * (14336 + 64 + 8) + (2048 + 22528 + 8) = 218375984 + 3702856 + 24584
    "ViT-L/14": (257, 227870592, 222103424, 24 * 257 * 4 * 1024),
    # L/14@336px: 577 rows.  Block: 577 * 36944 = 21316688
    #   shortcut: 23 * 21316688 + 577 * 14408 + 24584 = 490283824 + 8313416 + 24584
    "ViT-L/14@336px": (577, 511600512, 498621824, 24 * 577 * 4 * 1024),
}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_saved_activation_bytes_against_hand_computed_integers(name):
    rows, none_full, none_cls, block = EXPECTED[name]
    assert saved_activation_bytes(name, 1, "none", cls_only=False) == none_full
    assert saved_activation_bytes(name, 1, "none", cls_only=True) == none_cls
    assert saved_activation_bytes(name, 1, "none") == none_cls                       # the shortcut is the default, as in the model
    for cls_only in (False, True):                                                   # every block's INPUT has all rows
        assert saved_activation_bytes(name, 1, "block", cls_only=cls_only) == block
    assert saved_activation_bytes(name, 7, "none") == 7 * none_cls and saved_activation_bytes(name, 7, "block") == 7 * block


def test_geometry_tuple_and_other_number_formats():
    geo = (224, 14, 1024, 24, 16, 768)
    assert saved_activation_bytes(geo, 3, "none") == saved_activation_bytes("ViT-L/14", 3, "none")
    # a 16-bit residual stream: 2 D per stream instead of 4 D
    assert saved_activation_bytes(geo, 1, "block", residual_bytes=2) == 24 * 257 * 2 * 1024
    assert saved_activation_bytes(geo, 1, "none", residual_bytes=2, cls_only=False) == 24 * 257 * (32 * 1024 + 64 + 16)


def test_block_mode_keeps_less_than_a_fifth_at_l14():
    ratio = saved_activation_bytes("ViT-L/14", 928, "block") / saved_activation_bytes("ViT-L/14", 928, "none")
    assert ratio < 0.2, ratio


def test_unknown_mode_raises_and_default_is_none():
    with pytest.raises(ValueError, match="recompute"):
        saved_activation_bytes("ViT-B/32", 1, "layer")
    m = VisionTransformer(64, 32, 128, 2, 2, 64)
    assert m.recompute == "none"
    m.recompute = "all"
    with pytest.raises(ValueError, match="recompute"):                               # before anything touches the device
        vit_tokens_train(m, torch.zeros((1, 3, 64, 64), dtype=torch.uint8))


def test_student_constructor_and_command_lines_take_the_switch():
    import inspect

    from vimo_clip_amd import train_frame_diff_mn
    from vimo_clip_amd.models import FlowStudentModel, FrameDiffStudentModel
    for cls in (FlowStudentModel, FrameDiffStudentModel):
        params = inspect.signature(cls.__init__).parameters
        assert params["recompute"].default == "none" and list(params)[-1] == "recompute"
    for value in ("none", "block"):
        m = FlowStudentModel("ViT-tiny/32", device="cpu", recompute=value)
        assert m.visual_encoder.recompute == value
    assert FlowStudentModel("ViT-tiny/32", device="cpu").visual_encoder.recompute == "none"
    need = ["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c"]
    p = train_frame_diff_mn.build_parser()
    assert p.parse_args(need).recompute == "none" and p.parse_args(need + ["--recompute", "block"]).recompute == "block"
    with pytest.raises(SystemExit):
        p.parse_args(need + ["--recompute", "layer"])
