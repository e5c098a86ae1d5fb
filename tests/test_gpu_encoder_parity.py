"""GPU: the inference forward of the CLIP ViT encoder -- VisionTransformer.encode_frames_u8 / encode_pixel_values / encode_gray_u8 as
shipped, and VisionTransformer._encode_patches with its ``trace=`` hook for the residual stream -- against tests/encoder_refs.py: a
float64 forward and a float64 model of it that rounds where the path rounds.  Every recorded stage and the
embeddings, per tensor, under §5.1's measure; the runs that must be the same function bit for bit are compared with torch.equal.

VMC_ENCODER_PARITY_JSON=<path>: one line per checked tensor (case, dtype, tensor, errors, both ratios, the distance to the model)."""
import functools
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_refs as R                         # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16      # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (BF16, F16)
CONFIGS = [(c["name"], dt) for c in R.CASES for dt in DTYPES]
CFG_ID = lambda v: v if isinstance(v, str) else DT_NAME[v]


def _model(c, dtype, inp):
    from vimo_clip_amd.clip_vit import VisionTransformer
    kw = dict(residual_dtype=dtype) if c["res16"] else {}
    m = VisionTransformer(c["R"], c["p"], c["D"], c["L"], c["H"], c["E"], compute_dtype=dtype, **kw).cuda().eval()
    m.load_state_dict(inp["p32"], strict=True)
    assert (m.fuse_add_ln, m.cls_only_last_block, m.cls_query_last_block, m.exact_patch_embed, m.defer_attn_add) == (True, True, True, True, False)
    m.cls_only_last_block, m.cls_query_last_block = c["cls_only"], c["cls_query"]
    m.exact_patch_embed, m.defer_attn_add, m.frame_chunk = c["exact"], c["defer"], c["frame_chunk"]
    return m


def _encode(m, c, x):
    if c["source"] == "pix":
        return m.encode_pixel_values(x)
    return m.encode_frames_u8(x, wrap_quirk=c["wrap"])


def forward_on_gpu(name, dtype):
    """Build the case's model, load its weights, run the shipped forward and a ``trace=`` run; returns {tensor name: CPU tensor}
    under the names of encoder_refs."""
    inp = R.make_inputs(name, dtype)
    c = inp["case"]
    m = _model(c, dtype, inp)
    x = (R.pixel_values(inp) if c["source"] == "pix" else R.frames_rgb(inp)).cuda()
    got = {"E": _encode(m, c, x)}
    # the stream: the same patch operand through _encode_patches with the trace hook, all frames in one pass
    if c["source"] == "pix":
        patches, mode = m._patches(x)
    else:
        fr, wrap = m.fit_frames_u8(x, c["wrap"])
        patches, mode = m._patches(fr, wrap)
    assert mode == c["mode"] and patches.shape == (c["F"] * (c["N"] - 1), {"u8_exact": 2, "f32_split": 3, "plain": 1}[mode] * c["kpad"])
    trace = []
    got["E_trace"] = m._encode_patches(patches, c["F"], trace=trace, patch_mode=mode)
    assert [n for n, _ in trace] == R.stage_names(c)
    got.update(trace)
    if name == "h":
        # deferred attention add: the same fp32 additions in the same order, with the last block on all rows and on the class rows,
        # and the latter is case b's forward
        m.defer_attn_add = False
        assert torch.equal(got["E"], _encode(m, c, x))
        m.cls_only_last_block = True
        e_plain = _encode(m, c, x)
        m.defer_attn_add = True
        got["E_cls"] = _encode(m, c, x)
        assert torch.equal(got["E_cls"], e_plain)
        assert torch.equal(got["E_cls"], forward_on_gpu("b", dtype)["E"].cuda())
    if name == "k":
        got["E_gray"] = m.encode_gray_u8(inp["frames"].cuda())
        assert torch.equal(got["E_gray"], got["E"])
    if name == "m":
        assert c["F"] > 2 * c["frame_chunk"] and c["F"] % c["frame_chunk"]
        m.frame_chunk = 256
        assert torch.equal(got["E"], _encode(m, c, x))
    torch.cuda.synchronize()
    return {n: t.detach().float().cpu() for n, t in got.items()}


@functools.lru_cache(maxsize=None)
def _measured(name, dtype):
    c = R.BY_NAME[name]
    full, m16 = R.forward_ref64(name, dtype), R.forward_model16(name, dtype)
    r = dict({n: full[n] for n in m16}, floor=full["floor"])
    got = forward_on_gpu(name, dtype)
    assert set(got) == set(R.output_names(c)), set(got) ^ set(R.output_names(c))
    got = {n: t.reshape(r[n].shape) for n, t in got.items()}
    ms, bad = R.check(got, r, m16)
    path = os.environ.get("VMC_ENCODER_PARITY_JSON")
    if path:
        with open(path, "a") as f:
            for m in ms:
                f.write(json.dumps(dict(case=name, dtype=DT_NAME[dtype], tensor=m["name"], rms=m["rms"], max=m["max"], e_rms=m["e_rms"],
                                        e_max=m["e_max"], ratio_rms=round(m["ratio_rms"], 4), ratio_max=round(m["ratio_max"], 4),
                                        model_dist=round(m["model_dist"], 4), max_exempt=m["max_exempt"], ok=m["ok"])) + "\n")
    return ms, bad


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_forward_matches_the_float64_model(name, dtype):
    ms, bad = _measured(name, dtype)
    assert len(ms) == len(R.output_names(R.BY_NAME[name]))
    for m in ms:
        print(f"ratio {name} {DT_NAME[dtype]} {m['name']} rms {m['ratio_rms']:.3f} max {m['ratio_max']:.3f}"
              f"{' (max-exempt)' if m['max_exempt'] else ''} model_dist {m['model_dist']:.3f}")
    assert not bad, "\n".join(bad)
