"""GPU: masked attention on sequences of any length (the tiled MFMA kernels of attention_long.hip behind vmc_attention_fwd /
vmc_attention_bwd), forward and the three gradients against float64 torch autograd on the CPU, and the per-op AMO_CLIP path
on a whole video longer than 2048 tokens against the fp32 oracle.

Tolerances are the attention tests' (test_gpu_kernels.py): 2e-2 bf16, 3e-3 f16, times max(1, |ref|max)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT16 = [torch.bfloat16, torch.float16]
TOL = {torch.bfloat16: 2e-2, torch.float16: 3e-3}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vimo_clip_amd import ops as _ops
    return _ops


def _mask(kind, B, Tk, g):
    """[B, Tk] bool key mask, True = attend."""
    ar = torch.arange(Tk)[None, :]
    if kind == "full":
        return torch.ones(B, Tk, dtype=torch.bool)
    if kind == "prefix":                                  # collate_fn_pad: lengths uniform in [Tk/2, Tk], the first one full
        lens = torch.randint(Tk // 2, Tk + 1, (B,), generator=g)
        lens[0] = Tk
        return ar < lens[:, None]
    if kind == "random":
        m = torch.rand(B, Tk, generator=g) < 0.7
        m[:, 0] = True
        return m
    if kind == "concat":                                  # concat_dim=1: (Tr - 1) RGB tokens then Tf flow tokens, each padded
        tr = Tk // 2
        lr = torch.randint(1, tr + 1, (B,), generator=g)
        lf = torch.randint(1, Tk - tr + 1, (B,), generator=g)
        return torch.cat([ar[:, :tr] < lr[:, None], ar[:, :Tk - tr] < lf[:, None]], dim=1)
    if kind == "tiles":                                   # whole 64-key tiles masked, live keys on both sides of them
        m = torch.ones(B, Tk, dtype=torch.bool)
        m[:, 64:192] = False
        m[1:, 200:] = False
        return m
    if kind == "len1":                                    # one clip of length 1
        m = _mask("prefix", B, Tk, g)
        m[-1] = False
        m[-1, 0] = True
        return m
    raise ValueError(kind)


def _ref(q, kv, mask, dout, B, H, Tq, Tk, dh, fac=None):
    """float64 attention with autograd: (out, lse, dq, dk, dv) in the kernels' [B*T, H*dh] layout."""
    D = H * dh
    qf = q.double().view(B, Tq, H, dh).transpose(1, 2).requires_grad_(True)
    kf = kv[:, :D].double().view(B, Tk, H, dh).transpose(1, 2).requires_grad_(True)
    vf = kv[:, D:].double().view(B, Tk, H, dh).transpose(1, 2).requires_grad_(True)
    sc = (qf @ kf.transpose(-1, -2)) / math.sqrt(dh)
    sc = sc.masked_fill(~mask[:, None, None, :], float("-inf"))
    p = torch.softmax(sc, dim=-1)
    if fac is not None:
        p = p * fac
    o = (p @ vf).transpose(1, 2).reshape(B * Tq, D)
    o.backward(dout.double())
    flat = lambda t, T_: t.detach().transpose(1, 2).reshape(B * T_, D)
    return o.detach(), torch.logsumexp(sc.detach(), -1), flat(qf.grad, Tq), flat(kf.grad, Tk), flat(vf.grad, Tk)


def _run(ops, q, kv, mask, dout, B, H, Tq, Tk, dh, p=0.0, seed=0):
    from vimo_clip_amd import autograd_ops as ag
    D = H * dh
    qd, kvd, dd = q.to(DEV), kv.to(DEV), dout.to(DEV)
    md = mask.to(torch.uint8).to(DEV) if mask is not None else None
    out, lse = ops.attention(qd, kvd[:, :D], kvd[:, D:], md, B, H, Tq, Tk, dh, want_lse=True, dropout_p=p, dropout_seed=seed)
    dq, dkv = torch.empty_like(qd), torch.empty_like(kvd)
    ag._attn_bwd(qd, kvd[:, :D], kvd[:, D:], md, out, dd, lse, dq, dkv[:, :D], dkv[:, D:], B, H, Tq, Tk, dh, p=p, seed=seed)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu(), dq.cpu(), dkv[:, :D].cpu(), dkv[:, D:].cpu()


def _inputs(B, H, Tq, Tk, dh, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * dh
    q = torch.randn(B * Tq, D, generator=g).to(dtype)
    kv = torch.randn(B * Tk, 2 * D, generator=g).to(dtype)
    dout = torch.randn(B * Tq, D, generator=g).to(dtype)
    return q, kv, dout, g


def _check(got, ref, dtype, lse_tol=None):
    tol = TOL[dtype]
    for name, a, b in zip(("out", "lse", "dq", "dk", "dv"), got, ref):
        if name == "lse":
            err = (a.double() - b).abs().max().item()
            assert err <= (lse_tol or 2 * tol) * max(1.0, b.abs().max().item()), (name, err)
            continue
        assert torch.isfinite(a.float()).all(), name
        err = (a.double() - b).abs().max().item()
        assert err <= tol * max(1.0, b.abs().max().item()), (name, err, b.abs().max().item())


# ---------------------------------------------------------------- 1. beyond the old 2048 cap
@pytest.mark.parametrize("dtype", DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("dh", [64, 96])
def test_attention_beyond_old_cap(ops, dtype, dh):
    B, H, T = 1, 2, 2500
    q, kv, dout, g = _inputs(B, H, T, T, dh, dtype, 100 + dh)
    mask = _mask("concat", B, T, g)
    got = _run(ops, q, kv, mask, dout, B, H, T, T, dh)
    _check(got, _ref(q, kv, mask, dout, B, H, T, T, dh), dtype)


# ---------------------------------------------------------------- 2. shapes the scalar kernels used to take
@pytest.mark.parametrize("dtype", DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("B,H,Tq,Tk,dh,kind", [
    (2, 2, 65, 65, 64, "prefix"),          # first length past the short-sequence forward
    (2, 2, 65, 65, 96, "random"),
    (2, 2, 300, 300, 96, "concat"),        # past the in-LDS backward at head_dim 96 (T > 192)
    (2, 2, 300, 300, 64, "prefix"),        # past it at head_dim 64 (T > 288)
    (2, 2, 700, 699, 64, "random"),        # cross shapes, Tk not a multiple of the tile
    (2, 2, 100, 333, 96, "concat"),
    (2, 2, 130, 300, 96, "tiles"),         # whole masked key tiles
    (3, 2, 100, 400, 64, "len1"),          # a clip of length 1
    (2, 8, 96, 1000, 64, "full"),          # no mask
])
def test_attention_long_shapes(ops, dtype, B, H, Tq, Tk, dh, kind):
    q, kv, dout, g = _inputs(B, H, Tq, Tk, dh, dtype, Tq * 7 + Tk)
    mask = _mask(kind, B, Tk, g)
    got = _run(ops, q, kv, None if kind == "full" else mask, dout, B, H, Tq, Tk, dh)
    _check(got, _ref(q, kv, mask, dout, B, H, Tq, Tk, dh), dtype)


# ---------------------------------------------------------------- 3. dropout on the probabilities at long T
@pytest.mark.parametrize("dtype", DT16, ids=["bf16", "f16"])
def test_attention_long_dropout_mask_matches_vmc_dropout(ops, dtype):
    """The keep mask is vmc_dropout's counter-based mask on the flat index ((b*H + h)*Tq + t)*Tk + key (obtained by running
    vmc_dropout on a tensor of ones), at a length the per-op path could not run before."""
    from vimo_clip_amd._lib import check, dt, lib, ptr, stream
    B, H, T, dh, p, seed = 1, 2, 2100, 64, 0.25, 0x2468ACE
    q, kv, dout, g = _inputs(B, H, T, T, dh, dtype, 7)
    mask = _mask("prefix", B, T, g)
    ones = torch.ones(B * H * T * T, device=DEV)
    fac = torch.empty_like(ones)
    check(lib.vmc_dropout(ptr(ones), ptr(fac), ones.numel(), p, seed, dt(ones), dt(dtype), stream()), "dropout")
    fac = fac.view(B, H, T, T).cpu().double()
    assert 0.2 < (fac == 0).double().mean().item() < 0.3
    got = _run(ops, q, kv, mask, dout, B, H, T, T, dh, p=p, seed=seed)
    _check(got, _ref(q, kv, mask, dout, B, H, T, T, dh, fac=fac), dtype)


# ---------------------------------------------------------------- 4. the online-softmax rescale
@pytest.mark.parametrize("dtype", DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("dh", [64, 96])
def test_attention_long_running_max_grows_every_tile(ops, dtype, dh):
    """Scores that rise along the key index, up to |s| ~ 50: every 64-key tile raises the running max of the even query rows
    (the rescale of the accumulated O and sum runs at every tile), while the odd rows see their max in the first tile."""
    B, H, Tq, Tk = 2, 2, 100, 777
    D = H * dh
    g = torch.Generator().manual_seed(5)
    sign = torch.where(torch.arange(Tq) % 2 == 0, 1.0, -1.0)
    q = (sign[None, :, None, None] * (1.0 + 0.05 * torch.rand(B, Tq, H, dh, generator=g))).reshape(B * Tq, D)
    ramp = 50.0 * math.sqrt(dh) / dh * (torch.arange(Tk) + 1) / Tk            # q . k / sqrt(dh) ~ 50 (key + 1) / Tk
    k = ramp[None, :, None, None] * (1.0 + 0.02 * torch.rand(B, Tk, H, dh, generator=g))
    v = torch.randn(B, Tk, H, dh, generator=g)
    kv = torch.cat([k.reshape(B * Tk, D), v.reshape(B * Tk, D)], dim=1).to(dtype)
    q = q.to(dtype)
    dout = torch.randn(B * Tq, D, generator=g).to(dtype)
    mask = _mask("prefix", B, Tk, g)
    got = _run(ops, q, kv, mask, dout, B, H, Tq, Tk, dh)
    ref = _ref(q, kv, mask, dout, B, H, Tq, Tk, dh)
    assert ref[1].abs().max().item() > 40.0            # the scores reach the intended size
    _check(got, ref, dtype, lse_tol=1e-3)


# ---------------------------------------------------------------- 5. a row whose keys are all masked
@pytest.mark.parametrize("dtype", DT16, ids=["bf16", "f16"])
def test_attention_long_all_masked_row_is_nan(ops, dtype):
    """Batch 1 has no live key: its output rows and lse are NaN, as torch; the tiled backward (T = 300 at head_dim 64 is past
    the in-LDS one) skips every key tile of it, so its dQ, dK and dV are zero, as the scalar kernels gave."""
    B, H, Tq, Tk, dh = 3, 2, 300, 300, 64
    q, kv, dout, g = _inputs(B, H, Tq, Tk, dh, dtype, 9)
    mask = _mask("prefix", B, Tk, g)
    mask[1] = False
    out, lse, dq, dk, dv = _run(ops, q, kv, mask, dout, B, H, Tq, Tk, dh)
    rows = torch.arange(B * Tq) // Tq == 1
    assert torch.isnan(out[rows].float()).all() and torch.isnan(lse[1]).all()
    assert not torch.isnan(out[~rows].float()).any() and not torch.isnan(lse[[0, 2]]).any()
    assert (dq[rows] == 0).all()
    krows = torch.arange(B * Tk) // Tk == 1
    assert (dk[krows] == 0).all() and (dv[krows] == 0).all()
    keep = [0, 2]
    sel = lambda t, T_: t.view(B, T_, -1)[keep].reshape(len(keep) * T_, -1)
    ref = _ref(sel(q, Tq), sel(kv, Tk), mask[keep], sel(dout, Tq), 2, H, Tq, Tk, dh)
    got = (sel(out, Tq), lse[keep], sel(dq, Tq), sel(dk, Tk), sel(dv, Tk))
    _check(got, ref, dtype)


# ---------------------------------------------------------------- 6. determinism, captured == eager
def test_attention_long_deterministic_and_graph_replay(ops):
    from vimo_clip_amd import autograd_ops as ag
    B, H, Tq, Tk, dh, dtype, p, seed = 2, 4, 1000, 900, 96, torch.bfloat16, 0.1, 77
    D = H * dh
    q, kv, dout, g = _inputs(B, H, Tq, Tk, dh, dtype, 11)
    md = _mask("concat", B, Tk, g).to(torch.uint8).to(DEV)
    qd, kvd, dd = q.to(DEV), kv.to(DEV), dout.to(DEV)

    def step():
        out, lse = ops.attention(qd, kvd[:, :D], kvd[:, D:], md, B, H, Tq, Tk, dh, want_lse=True, dropout_p=p, dropout_seed=seed)
        dq, dkv = torch.empty_like(qd), torch.empty_like(kvd)
        ag._attn_bwd(qd, kvd[:, :D], kvd[:, D:], md, out, dd, lse, dq, dkv[:, :D], dkv[:, D:], B, H, Tq, Tk, dh, p=p, seed=seed)
        return out, lse, dq, dkv

    a = [t.clone() for t in step()]
    b = [t.clone() for t in step()]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = step()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, cap):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- other head dims keep the scalar kernels and their cap
def test_attention_other_head_dims_keep_scalar_cap(ops):
    B, H, dh, dtype = 1, 2, 32, torch.float16
    q, kv, dout, g = _inputs(B, H, 300, 300, dh, dtype, 3)
    mask = _mask("prefix", B, 300, g)
    got = _run(ops, q, kv, mask, dout, B, H, 300, 300, dh)
    _check(got, _ref(q, kv, mask, dout, B, H, 300, 300, dh), dtype)
    qd = torch.zeros(2100, H * dh, dtype=dtype, device=DEV)
    kvd = torch.zeros(2100, 2 * H * dh, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError):
        ops.attention(qd, kvd[:, :H * dh], kvd[:, H * dh:], None, B, H, 2100, 2100, dh)


# ---------------------------------------------------------------- 7. the per-op AMO_CLIP path on a whole long video
def test_tfam_per_op_train_whole_video_concat(ops):
    """concat_dim=1 over Tr = Tf = 1100 frames: (Tr - 1) + Tf = 2199 tokens, past the old 2048 limit; train mode with no dropout
    against the fp32 oracle under autograd (logits, loss and every parameter gradient)."""
    from oracle import tfam as otfam
    from vimo_clip_amd import synth
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.losses import bce_with_logits_loss
    D, H, L, ff, C, B, Tr, Tf, seed = 512, 8, 1, 2048, 140, 2, 1100, 1100, 61
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=ff, num_classes=C, use_pe=False, dropout=0.0, mlp_dropout=0.0,
                 device="cuda", compute_dtype=torch.bfloat16, use_cross_attention=False, concat_dim=1).cuda()
    sd = synth.tfam_state_dict(D, H, L, ff, C, seed)
    m.load_state_dict(sd, strict=True)
    m.train()
    rgb = synth.normal(seed, "rgb", (B, Tr, D))
    mot = synth.normal(seed, "motion", (B, Tf, D))
    lens = torch.tensor([Tr, 700])
    mr = torch.arange(Tr)[None, :] < lens[:, None]
    mf = torch.arange(Tf)[None, :] < (lens - 1)[:, None]
    rgb, mot = rgb * mr[..., None], mot * mf[..., None]
    y = synth.multi_hot_labels(seed, "labels", B, C)
    logits = m(rgb.cuda(), mot.cuda(), mask_rgb=mr.cuda(), mask_flow=mf.cuda())
    loss = bce_with_logits_loss(logits, y.cuda())
    loss.backward()

    sd_ref = {k: v.float().clone().requires_grad_(True) for k, v in sd.items()}
    ref_logits = otfam.amo_clip_forward(sd_ref, rgb, mot, mr, mf, nhead=H, use_cross_attention=False, concat_dim=1)
    ref_loss = otfam.bce_with_logits_mean(ref_logits, y)
    ref_loss.backward()
    err = (logits.detach().cpu() - ref_logits.detach()).abs().max().item()
    assert err <= 8e-3 * max(1.0, ref_logits.abs().max().item()), err
    assert abs(loss.item() - ref_loss.item()) <= 5e-3 * abs(ref_loss.item())
    params = dict(m.named_parameters())
    used = {id(p) for p in m.used_parameters()}
    checked = 0
    for k, pr in sd_ref.items():
        if k not in params or id(params[k]) not in used:
            continue
        ref, got = pr.grad, params[k].grad.cpu()
        assert ref is not None and got is not None, k
        rel = (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
        rel_l2 = ((got - ref).norm() / (ref.norm() + 1e-20)).item()
        assert rel_l2 <= 4e-2, (k, rel_l2)
        assert rel <= (2e-1 if "ffn.0" in k else 6e-2), (k, rel)
        checked += 1
    assert checked >= 10
