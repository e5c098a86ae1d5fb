"""CPU: the feature-concatenation section of vimo_clip_amd/csrc/tfam_route.h (tests/host/test_tfam_proj_route.cpp), the ctypes mirror
of vmc_tfam_proj_params, and the switch from YAML / command line down to the model (host only, no device)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tfam_proj_route(tmp_path):
    exe = str(tmp_path / "test_tfam_proj_route")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "test_tfam_proj_route.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "OK" in out.stdout


def test_proj_params_mirror_the_header():
    """vmc_tfam_proj_params (include/vmc.h) against tfam_train.ProjParams: same names, same order, every field one pointer wide."""
    from vimo_clip_amd import tfam_train as tt
    src = open(os.path.join(ROOT, "include", "vmc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct vmc_tfam_proj_params\s*\{(.*?)\}\s*vmc_tfam_proj_params\s*;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert re.match(r"(const\s+)?(void|float)\s*\*", decl), decl
        names += [n.strip().lstrip("*").strip() for n in re.sub(r"^(const\s+)?(void|float)\s*", "", decl).split(",")]
    assert names == [f[0] for f in tt.ProjParams._fields_] == ["w_proj", "b_proj", "gw_proj", "gb_proj"]
    assert all(f[1] is ctypes.c_void_p for f in tt.ProjParams._fields_) and ctypes.sizeof(tt.ProjParams) == 8 * len(names)


# (D, H, ff, L, C), (B, T), the chains with the projection take it
SHAPES = [
    ((512, 8, 2048, 4, 140), (8, 15), True),
    ((768, 12, 512, 1, 140), (16, 16), True),
    ((512, 8, 512, 7, 140), (2, 16), True),
    ((512, 8, 512, 8, 140), (2, 16), False),           # 4 x 8 + 1 problems do not fit the weight-gradient table
    ((512, 8, 512, 1, 140), (17, 16), False),          # more than 256 token rows
    ((512, 8, 512, 1, 141), (2, 16), False),           # class count not a multiple of 4
    ((512, 8, 512, 1, 140), (2, 65), False),           # more than 64 tokens per clip
]


@pytest.mark.parametrize("cfg,batch,want", SHAPES)
def test_supported_proj_is_the_library_answer(cfg, batch, want):
    from vimo_clip_amd import tfam_train
    from vimo_clip_amd._lib import lib
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    D, H, ff, L, C = cfg
    B, T = batch
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=ff, num_classes=C, device="cpu", use_cross_attention=False, concat_dim=-1)
    rc = lib.vmc_tfam_proj_supported(B, T, D, H, ff, L, C)
    assert tfam_train.supported_proj(m, B, T) == (rc == 0) == want
    nbytes = lib.vmc_tfam_train_proj_workspace_bytes(B, T, D, H, ff, L, C)
    off = lib.vmc_tfam_train_proj_dx0_offset(B, T, D, H, ff, L, C)
    assert (nbytes > 0) == (off >= 0) == want
    if want:      # the extension lies behind the unchanged training workspace
        plain = lib.vmc_tfam_train_workspace_bytes(B, T, 0, D, H, ff, L, C, 0)
        al = lambda n: (n + 255) // 256 * 256
        M = B * T
        assert plain > 0 and off == plain + al(M * D * 4) + al(M * 2 * D * 2)                    # x32, xcat16 in front of dx0
        assert nbytes == off + al(M * D * 4) + al(M * D * 2) and off % 256 == 0                  # dx0, d0_16


def test_the_switch_is_off_by_default_and_reaches_the_model(tmp_path):
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, build_model
    m = AMO_CLIP(d_model=512, nhead=8, num_layers=1, dim_feedforward=512, device="cpu", use_cross_attention=False, concat_dim=-1)
    assert m.fused_feature_training is False and m.fused_training is True
    assert Config().fused_feature_training is False
    kw = dict(d_model=512, nhead=8, num_layers=1, dim_feedforward=512, device="cpu", use_cross_attention=False, concat_dim=-1)
    assert build_model(Config(**kw)).fused_feature_training is False
    assert build_model(Config(fused_feature_training=True, **kw)).fused_feature_training is True
    # the switch off: _fused_inputs declines the training step of the feature mode, as it always has
    import torch
    rgb, mot = torch.zeros(2, 5, 512), torch.zeros(2, 4, 512)
    assert m._fused_inputs(rgb, mot, None, None, True) is None


def test_yaml_key_and_cli_flag_reach_config(tmp_path, monkeypatch):
    yaml = pytest.importorskip("yaml")
    from vimo_clip_amd.TFAM import sweep
    from vimo_clip_amd.TFAM import train_and_eval as te
    cfgs = sweep.sweep_configs()
    base = cfgs["concat_feature_do11"]
    for val in (None, False, True):
        c = {k: dict(v) for k, v in base.items()}
        if val is not None:
            c["training"]["fused_feature_training"] = val
        p = tmp_path / f"c_{val}.yaml"
        p.write_text(yaml.safe_dump(c, sort_keys=False))
        assert te.Config.from_yaml(str(p)).fused_feature_training is bool(val)
    # the sweep forwards training keys into its YAML files
    on = sweep.sweep_configs({"training": {"fused_feature_training": True}})["concat_feature_do11"]
    assert on["training"]["fused_feature_training"] is True
    # the command line: main() builds its Config from the flag (the three trainers share main)
    seen = {}
    monkeypatch.setattr(te, "run", lambda cfg, *a, **k: seen.setdefault("cfg", cfg) and {})
    monkeypatch.setattr(te.parallel, "init_from_env", lambda: (1, 1, 0))      # rank 1: main prints nothing
    for flag, want in (([], False), (["--fused-feature-training"], True)):
        seen.clear()
        monkeypatch.setattr(sys, "argv", ["train_and_eval"] + flag)
        te.main()
        assert seen["cfg"].fused_feature_training is want
    from vimo_clip_amd.TFAM import train_and_eval_frame_diff_AK as ak
    from vimo_clip_amd.TFAM import train_and_eval_frame_diff_MN as mn
    assert ak.main is te.main and mn.main is te.main
