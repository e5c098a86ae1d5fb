"""GPU: the 336-px CLIP towers (577 tokens: attention_vit_long.hip) through the encoder, the extractor and the HF-name front door,
against oracle.vit run live on the CPU.  Tolerances as in test_gpu_encoder.py: f16 1e-3, bf16 8e-3, x max(1, |ref|max)."""
import numpy as np
import pytest
import torch

from oracle import vit as ovit
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
TINY = "ViT-tiny/14@336px"


def _encoder(name, seed, dtype):
    from vimo_clip_amd.clip_vit import VisionTransformer
    m = VisionTransformer.from_name(name, compute_dtype=dtype).to("cuda")
    sd = synth.vit_state_dict(name, seed)
    m.load_state_dict(sd, strict=True)
    return m.eval(), sd


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_tiny336_encoder_vs_oracle(dtype):
    m, sd = _encoder(TINY, 31, dtype)
    H = synth.VIT_GEOMETRY[TINY][4]
    u8 = synth.randint_u8(31, "frames", (5, 3, 336, 336))
    ref = ovit.vit_forward(sd, ovit.normalize_u8(u8), H)
    y = m.encode_frames_u8(u8.cuda()).cpu()
    y2 = m.encode_pixel_values(ovit.normalize_u8(u8).cuda()).cpu()
    scale = max(1.0, ref.abs().max().item())
    err, err2 = (y - ref).abs().max().item(), (y2 - ref).abs().max().item()
    print(f"{TINY} {dtype}: max abs err {err:.3e} / {err2:.3e}, scale {scale:.2f}")
    assert err <= TOL[dtype] * scale and err2 <= TOL[dtype] * scale
    # the class-query last block (vmc_attention_vit_cls_fwd at N = 577) is the same function as the full last block
    m.cls_query_last_block = False
    y_full = m.encode_frames_u8(u8.cuda()).cpu()
    assert (y - y_full).abs().max().item() <= 1e-6 * max(1.0, y_full.abs().max().item())


def test_vit_l14_336_f16_vs_oracle():
    """The full ViT-L/14@336px tower, 2 frames, f16, at the bound of the 224-px towers (fixed before the first run)."""
    name = "ViT-L/14@336px"
    m, sd = _encoder(name, 17, torch.float16)
    u8 = synth.randint_u8(17, "frames", (2, 3, 336, 336))
    y = m.encode_frames_u8(u8.cuda()).cpu()
    ref = ovit.vit_forward(sd, ovit.normalize_u8(u8), 16)
    err = (y - ref).abs().max().item()
    print(f"{name} f16: max abs err {err:.3e}, |ref|max {ref.abs().max().item():.2f}")
    assert y.shape == (2, 768)
    assert err <= 1e-3 * max(1.0, ref.abs().max().item())


def test_frame_chunks_give_identical_bits():
    m, _ = _encoder(TINY, 5, torch.bfloat16)
    u8 = synth.randint_u8(5, "frames", (40, 3, 336, 336)).cuda()
    m.frame_chunk = 40
    a = m.encode_frames_u8(u8)
    m.frame_chunk = 16
    b = m.encode_frames_u8(u8)
    assert torch.equal(a, b)


def test_360x640_frames_resize_to_336_like_pil():
    from PIL import Image

    from oracle import pil_resize as opr
    from vimo_clip_amd.preprocess import resize_center_crop_u8
    fr = synth.randint_u8(12, "fr360x640", (2, 3, 360, 640))
    out, pending = resize_center_crop_u8(fr.cuda(), 336, "torchvision", wrap_quirk=False)
    assert not pending
    out = out.cpu()
    nh, nw = opr.shortest_edge_size(360, 640, 336)
    top, left = opr.center_crop_offsets(nh, nw, 336, "torchvision")
    crops = []
    for f in range(2):
        ref = np.asarray(Image.fromarray(np.transpose(fr[f].numpy(), (1, 2, 0))).resize((nw, nh), Image.BICUBIC))[top:top + 336, left:left + 336]
        assert np.array_equal(np.transpose(out[f].numpy(), (1, 2, 0)), ref)
        crops.append(np.transpose(ref, (2, 0, 1)))
    m, _ = _encoder(TINY, 12, torch.float16)
    y = m.encode_frames_u8(fr.cuda())
    y_pil = m.encode_frames_u8(torch.from_numpy(np.stack(crops)).cuda())
    assert torch.equal(y, y_pil)


def test_hf_id_encoder_equals_vision_transformer():
    from vimo_clip_amd.clip_vit import CLIPImageEncoder, VisionTransformer
    name = "ViT-L/14@336px"
    sd = synth.vit_state_dict(name, 3)
    enc = CLIPImageEncoder("openai/clip-vit-large-patch14-336", compute_dtype=torch.bfloat16).cuda().eval()
    enc.visual.load_state_dict(sd, strict=True)
    vt = VisionTransformer.from_name(name, compute_dtype=torch.bfloat16).cuda().eval()
    vt.load_state_dict(sd, strict=True)
    px = ovit.normalize_u8(synth.randint_u8(3, "frames", (2, 3, 336, 336))).cuda()
    assert enc.visual.input_resolution == 336
    assert torch.equal(enc.get_image_features(px), vt.encode_pixel_values(px))


def test_extractor_writes_tiny336_embeddings(tmp_path):
    from vimo_clip_amd import h5lite as h5
    from vimo_clip_amd.clip_vit import CLIPImageEncoder
    from vimo_clip_amd.extract_embeddings import create_hdf5_dataset, encode_video_frames, frames_to_nchw, sample_frame_indices
    enc = CLIPImageEncoder(TINY, compute_dtype=torch.float16).cuda().eval()
    enc.visual.load_state_dict(synth.vit_state_dict(TINY, 8), strict=True)
    root = tmp_path / "videos"
    root.mkdir()
    vids = {"AAAA.mp4": (6, 360, 640), "BBBB.mp4": (3, 336, 400)}
    for i, (vid, shape) in enumerate(vids.items()):
        np.save(str(root / (vid + ".npy")), synth.randint_u8(8 + i, "video", (shape[0], shape[1], shape[2], 3)).numpy())
    (tmp_path / "ann.txt").write_text("AAAA.mp4 3\nBBBB.mp4 0 1\n")
    (tmp_path / "classes.csv").write_text("id,name\n" + "".join(f"{i},c{i}\n" for i in range(140)))
    out = str(tmp_path / "ak.h5")
    assert create_hdf5_dataset(str(root), str(tmp_path / "ann.txt"), str(tmp_path / "classes.csv"), out, max_frames=8, encoder=enc,
                               clip_model_name=TINY) == 2
    with h5.File(out, "r") as f:
        for i, (vid, shape) in enumerate(vids.items()):
            idx = sample_frame_indices(shape[0], 8)
            frames = synth.randint_u8(8 + i, "video", (shape[0], shape[1], shape[2], 3))[torch.from_numpy(idx)]
            want = encode_video_frames(enc, frames_to_nchw(frames))
            got = f[vid]["embeddings"][:]
            assert got.shape == (len(idx), 96)
            assert np.array_equal(got, want), vid
