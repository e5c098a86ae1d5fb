"""CPU: the 336-px CLIP towers' names and geometry (synth.vit_name / vit_geometry), train.py's embedding width, and the oracle at
577 tokens against transformers.CLIPModel built from a config (the check oracle/make_golden.py runs for the 224-px geometries)."""
import pytest
import torch

from vimo_clip_amd import synth

NAMES = {
    "ViT-B/32": "ViT-B/32", "ViT-B/16": "ViT-B/16", "ViT-L/14": "ViT-L/14", "ViT-L/14@336px": "ViT-L/14@336px",
    "openai/clip-vit-base-patch32": "ViT-B/32", "openai/clip-vit-base-patch16": "ViT-B/16",
    "openai/clip-vit-large-patch14": "ViT-L/14", "openai/clip-vit-large-patch14-336": "ViT-L/14@336px",
}


@pytest.mark.parametrize("name", list(NAMES))
def test_every_name_resolves(name):
    assert synth.vit_name(name) == NAMES[name]
    R, p, D, L, H, E = synth.vit_geometry(name)
    N = (R // p) ** 2 + 1
    assert N == (577 if "336" in name else {"ViT-B/32": 50, "ViT-B/16": 197, "ViT-L/14": 257}[NAMES[name]])


def test_geometries_of_the_336_towers():
    assert synth.vit_geometry("ViT-L/14@336px") == (336, 14, 1024, 24, 16, 768)
    assert synth.vit_geometry("ViT-tiny/14@336px") == (336, 14, 128, 2, 2, 96)


@pytest.mark.parametrize("name", ["ViT-L/14@336", "openai/clip-vit-large-patch14-448", "RN50", ""])
def test_unknown_name_raises_keyerror_listing_the_known_names(name):
    with pytest.raises(KeyError, match="ViT-L/14@336px"):
        synth.vit_name(name)


@pytest.mark.parametrize("name", list(NAMES) + ["ViT-tiny/14@336px"])
def test_train_embedding_width_is_the_towers_output_width(name):
    from vimo_clip_amd.train import embed_dim
    assert embed_dim(name) == synth.vit_geometry(name)[5]


def test_oracle_matches_hf_clip_at_577_tokens():
    transformers = pytest.importorskip("transformers")
    from oracle import vit

    name, seed = "ViT-tiny/14@336px", 19
    R, p, D, L, H, E = synth.VIT_GEOMETRY[name]
    sd = synth.vit_state_dict(name, seed)
    vcfg = transformers.CLIPVisionConfig(hidden_size=D, intermediate_size=4 * D, num_hidden_layers=L, num_attention_heads=H, image_size=R,
                                         patch_size=p, projection_dim=E, hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0)
    tcfg = transformers.CLIPTextConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, projection_dim=E,
                                       vocab_size=100, max_position_embeddings=8)
    hf = transformers.CLIPModel(transformers.CLIPConfig(text_config=tcfg.to_dict(), vision_config=vcfg.to_dict(), projection_dim=E)).eval()
    missing, unexpected = hf.load_state_dict(vit.openai_to_hf_vision(sd, H), strict=False)
    assert not unexpected and all(not k.startswith(("vision_model", "visual_projection")) for k in missing)
    pix = vit.normalize_u8(synth.randint_u8(seed, "frames", (2, 3, R, R)))
    with torch.no_grad():
        ref = hf.get_image_features(pixel_values=pix)
        if not isinstance(ref, torch.Tensor):
            ref = ref.pooler_output
        tokens = vit.vit_forward(sd, pix, H, return_tokens=True)
        mine = vit.vit_forward(sd, pix, H)
    assert tokens.shape == (2, 577, D)
    err = (mine - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err
