"""GPU: ViT self-attention past 288 tokens (attention_vit_long.hip behind vmc_attention_vit_fwd / vmc_attention_vit_cls_fwd):
K / V streamed through LDS in 64-key tiles.  N = 577 is ViT-L/14@336px; 289 and 1025 take the runtime-N instance.

Tolerances as in test_gpu_kernels.py's test_attention_vit: 2e-2 (bf16) / 3e-3 (f16) on the output against a float64 softmax of
the same 16-bit operands, lse within 1e-3 of logsumexp."""
import os
import re

import pytest
import torch

from vimo_clip_amd import ops, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.bfloat16: 2e-2, torch.float16: 3e-3}


def _qkv(F, N, H, dtype, seed, kind="normal"):
    D = H * 64
    qkv = synth.normal(seed, "qkv", (F * N, 3 * D))
    if kind == "spike":          # one key, in the last full tile, takes almost all of every query's weight
        x = qkv.view(F, N, 3, H, 64)
        x[:, :, 0] = x[:, :, 0].abs()
        x[:, N - 2, 1] = 3.0
    elif kind == "growing":      # scores grow along the key axis: the running max rises in every tile, every tile rescales
        x = qkv.view(F, N, 3, H, 64)
        x[:, :, 0] = x[:, :, 0].abs() * 0.25 + 0.5
        ramp = torch.linspace(0.0, 1.5, N).view(1, N, 1, 1)
        x[:, :, 1] = x[:, :, 1] * 0.1 + ramp
    return qkv.to(dtype).cuda()


def _reference(qkv, F, N, H):
    D = H * 64
    x = qkv.double().cpu().view(F, N, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [F, H, N, 64]
    s = q @ k.transpose(-1, -2) * 0.125
    out = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(F * N, D)
    return out, torch.logsumexp(s, -1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("F,N,H,kind", [(2, 289, 2, "normal"), (3, 577, 2, "normal"), (1, 577, 16, "normal"), (2, 1025, 1, "normal"),
                                        (2, 577, 2, "spike"), (2, 577, 2, "growing"), (1, 1025, 2, "growing")])
def test_attention_vit_long_vs_float64(dtype, F, N, H, kind):
    qkv = _qkv(F, N, H, dtype, 11 + N, kind)
    out, lse = ops.attention_vit(qkv, F, N, H, want_lse=True)
    ref, ref_lse = _reference(qkv, F, N, H)
    err = (out.double().cpu() - ref).abs().max().item()
    lerr = (lse.double().cpu() - ref_lse).abs().max().item()
    print(f"F={F} N={N} H={H} {kind} {dtype}: out err {err:.2e}, lse err {lerr:.2e}")
    assert torch.isfinite(out).all()
    assert err <= TOL[dtype] and lerr <= 1e-3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", [577, 700])
def test_class_query_equals_row0_of_the_full_call(dtype, N):
    """The class-query call runs the keys in the same tiles through the same tile step: its row equals row 0 bit for bit."""
    F, H = 5, 16
    D = H * 64
    qkv = _qkv(F, N, H, dtype, 3 + N)
    full, _ = ops.attention_vit(qkv, F, N, H)
    q_cls = qkv.view(F, N, 3 * D)[:, 0, :D].contiguous()
    kv = qkv.view(F * N, 3 * D)[:, D:].contiguous()
    cls = ops.attention_vit_cls(q_cls, kv, F, N, H)
    assert torch.equal(cls, full.view(F, N, D)[:, 0])


def test_two_identical_calls_give_identical_bits():
    F, N, H = 4, 577, 16
    qkv = _qkv(F, N, H, torch.bfloat16, 5)
    a, la = ops.attention_vit(qkv, F, N, H, want_lse=True)
    b, lb = ops.attention_vit(qkv, F, N, H, want_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_no_scratch_and_no_spills():
    """The kept resource-usage remarks of attention_vit_long.hip: no instantiation uses scratch or spills a VGPR."""
    path = os.path.join(ROOT, "vimo_clip_amd", "csrc", "build", "attention_vit_long.usage.txt")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    blocks = re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        if "attn_vit_long" not in name:
            continue
        seen += 1
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        spills = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert seen == 8, seen        # {full, class} x {577, runtime N} x {bf16, f16}
