"""GPU: dynamic loss scaling on the device (DESIGN.md "Dynamic loss scaling") -- vmc_loss_scale_check against its CPU reference
(tests/loss_scale_ref.py, itself pinned to torch._amp_update_scale_), the Adam entries behind the skip flag, scale invariance of the
bf16 backward, what scaling buys float16 gradients, the overflow path (eager, accumulated, captured) and the unchanged off path.

Bound of the clip norm / coefficient (item 1): that of tests/test_gpu_grad_clip.py for vmc_grad_clip_dev -- the relative error of the
host path (vmc_sumsq: fp32 partials, float atomics) measured on the same gradient, with a floor of 2 fp32 ulps (2^-22); the reference
is the float64 norm."""
import hashlib

import numpy as np
import pytest
import torch

import loss_scale_ref as R
from oracle import student as ostudent
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -22                                     # tests/test_gpu_grad_clip.py
SIZES = [1, 3, 4, 1023, 4101, (1 << 20) + 7]
BIG = 4 * 2048 * 512 + 4101                            # more than one trip of the capped grid (2048 workgroups x 512 float4)
E_ARG, E_ALIGN = -1, -2


# ---- 1. the check kernel --------------------------------------------------------------------------------------------------------------

def _record(scale=1024.0, growth=2.0, backoff=0.5, base=1.0, interval=2000, tracker=0, found=0, skipped=0):
    from vimo_clip_amd.optim import LossScaleStruct
    rec = LossScaleStruct(scale, growth, backoff, base, interval, tracker, found, skipped)
    return torch.frombuffer(bytearray(bytes(rec)), dtype=torch.int32).clone().cuda()


def _check(grad, rec, clip=None, state=None, hyper=None):
    """One vmc_loss_scale_check through the C ABI; returns hyper on the host.  rec / clip / state are updated in place."""
    from vimo_clip_amd._lib import check, lib, ptr, stream
    n = grad.numel()
    hyper = torch.full((4,), -1.0, dtype=torch.float32, device="cuda") if hyper is None else hyper
    ws = torch.empty(int(lib.vmc_loss_scale_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    check(lib.vmc_loss_scale_check(ptr(grad), n, ptr(rec), ptr(hyper), ptr(clip), ptr(state), ptr(ws), ws.numel(), stream()),
          "loss_scale_check")
    torch.cuda.synchronize()
    return hyper.cpu()


def _fields(rec):
    r = rec.cpu()
    f = r.view(torch.float32)
    return dict(scale=np.float32(f[0].item()), growth=f[1].item(), backoff=f[2].item(), base=f[3].item(), interval=int(r[4]),
                tracker=int(r[5]), found=int(r[6]), skipped=int(r[7]))


def _grad(n, seed=0):
    g = torch.Generator().manual_seed(1000 + n + seed)
    return (torch.randn(n + 8, generator=g) * 0.02).cuda()          # 8 guard elements behind n: never read as part of the gradient


def _positions(n):
    tail = (n & ~3) if (n & 3) else n - 1                             # first element of the n % 4 tail where there is one
    return sorted({0, n - 1, tail, n // 2})


@pytest.mark.parametrize("n", SIZES)
def test_check_finds_every_planted_non_finite_value(n):
    S, base = 1024.0, 0.5
    clean = _grad(n)
    clean[n:] = float("nan")                                          # a read past n would raise the flag
    cases = [(None, None)] + [(v, p) for v in (float("inf"), float("-inf"), float("nan")) for p in _positions(n)]
    for value, pos in cases:
        g = clean.clone()
        if value is not None:
            g[pos] = value
        rec = _record(scale=S, base=base, tracker=3, skipped=5)
        state = torch.tensor([7, 99], dtype=torch.int64, device="cuda")
        hyper = _check(g[:n], rec, state=state)
        f = _fields(rec)
        found = value is not None
        assert f["found"] == int(found), (n, value, pos)
        assert hyper[:3].tolist() == [-1.0, -1.0, -1.0]              # only hyper[3] is written
        assert hyper[3].item() == (0.0 if found else base / S), (n, value, pos, hyper[3].item())
        assert state.tolist() == [6 if found else 7, 99]             # the tick is taken back only on overflow
        assert f["skipped"] == 5 + int(found) and f["tracker"] == (0 if found else 4)
        assert f["scale"] == np.float32(S * 0.5 if found else S)
        assert (f["growth"], f["backoff"], f["base"], f["interval"]) == (2.0, 0.5, base, 2000)       # host-written fields stay


def test_scripted_sequence_equals_the_reference_bit_for_bit():
    n, seq = 4101, [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    for growth, backoff, interval, s0 in ((2.0, 0.5, 2, 65536.0), (2.0, 2.0 ** -8, 3, 2.0 ** 40), (1.0, 1.0, 1, 1024.0), (2.0, 0.5, 1, 3e38)):
        want = R.run(s0, seq, growth, backoff, interval)
        rec = _record(scale=s0, growth=growth, backoff=backoff, interval=interval)
        state = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
        t = 0
        for i, found in enumerate(seq):
            g = _grad(n, i)
            if found:
                g[(37 * i) % n] = float("inf") if i % 2 else float("nan")
            state[0] += 1                                             # the step's tick
            s_before = _fields(rec)["scale"]
            hyper = _check(g[:n], rec, state=state)
            f = _fields(rec)
            t += 0 if found else 1
            assert f["scale"].tobytes() == np.float32(want[i][0]).tobytes(), (i, f, want[i])
            assert (f["tracker"], f["skipped"], f["found"]) == (want[i][1], want[i][2], found), (i, f, want[i])
            assert int(state[0]) == t
            if found or float(np.log2(float(s_before))).is_integer():      # exact for a power-of-two S
                assert hyper[3].item() == (0.0 if found else float(np.float32(1.0) / s_before)), (i, hyper[3].item(), s_before)


def test_a_finite_value_whose_square_overflows_is_no_overflow():
    n = 4101
    for pos in _positions(n):
        g = _grad(n)
        g[pos] = 1e20                                                 # finite; its fp32 square is inf
        rec = _record(scale=1024.0)
        hyper = _check(g[:n], rec)                                    # train_state NULL: allowed
        f = _fields(rec)
        assert f["found"] == 0 and f["skipped"] == 0 and f["tracker"] == 1 and hyper[3].item() == 1.0 / 1024.0


def _host_norm_error(g, ref):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    check(lib.vmc_sumsq(ptr(g), g.numel(), ptr(out), stream()), "sumsq")
    return abs(out.sqrt().item() - ref) / ref


@pytest.mark.parametrize("n", [4101, (1 << 20) + 7, BIG])
def test_clip_norm_and_coefficient_against_float64(n):
    """With clip: norm = sqrt(sum) * |base| / S of the UNSCALED averaged gradient, coef = min(1, max_norm / (norm + 1e-6)),
    hyper[3] = base / S * coef -- norm and coef within the bound vmc_grad_clip_dev is held to; the same call twice gives the same
    bits; and for a power-of-two S the norm, the coefficient and hyper[3] * S are those of vmc_grad_clip_dev on the unscaled gradient."""
    from vimo_clip_amd._lib import check, lib, ptr, stream
    S = 1024.0
    unscaled = _grad(n)[:n].contiguous()
    g = (unscaled * S).contiguous()                                   # exact: a power of two
    ref_sum = g.double().norm().item()
    tol = max(_host_norm_error(g, ref_sum), FLOOR)
    for base, max_norm in ((1.0, 1.0), (0.5, 0.25), (1.0, 1e6)):
        outs = []
        for _ in range(2):
            rec, clip = _record(scale=S, base=base), torch.tensor([base, max_norm, -1.0, -1.0], dtype=torch.float32, device="cuda")
            hyper = _check(g, rec, clip=clip)
            outs.append((clip.cpu(), hyper, rec.cpu()))
        (clip, hyper, rec), (clip_b, hyper_b, rec_b) = outs
        assert torch.equal(clip, clip_b) and torch.equal(hyper, hyper_b) and torch.equal(rec, rec_b)      # same input, same state, same bits
        norm_ref = ref_sum * base / S
        coef_ref = min(1.0, max_norm / (norm_ref + 1e-6))
        norm, coef = clip[2].item(), clip[3].item()
        print(f"n {n} base {base} max {max_norm}: norm {norm:.9g} ref {norm_ref:.9g} rel {abs(norm - norm_ref) / norm_ref:.3e}  "
              f"coef {coef:.9g} ref {coef_ref:.9g} rel {abs(coef - coef_ref) / coef_ref:.3e}  tol {tol:.3e}")
        assert abs(norm - norm_ref) <= tol * norm_ref and abs(coef - coef_ref) <= tol * coef_ref
        assert (coef < 1.0) == (max_norm < 1e6) and clip[:2].tolist() == [base, max_norm]
        assert hyper[3].item() == float(np.float32(base / S) * np.float32(coef)) and _fields(rec)["found"] == 0
        old_clip = torch.tensor([base, max_norm, -1.0, -1.0], dtype=torch.float32, device="cuda")
        old_hyper = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
        ws = torch.empty(int(lib.vmc_grad_clip_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        check(lib.vmc_grad_clip_dev(ptr(unscaled), n, ptr(old_hyper), ptr(old_clip), ptr(ws), ws.numel(), stream()), "grad_clip_dev")
        torch.cuda.synchronize()
        assert torch.equal(old_clip.cpu(), clip) and old_hyper[3].item() == hyper[3].item() * S
    bad = g.clone()
    bad[n // 3] = float("inf")
    rec, clip = _record(scale=S), torch.tensor([1.0, 1.0, -1.0, -1.0], dtype=torch.float32, device="cuda")
    hyper = _check(bad, rec, clip=clip)
    assert _fields(rec)["found"] == 1 and hyper[3].item() == 0.0 and clip[2].item() == float("inf") and clip[3].item() == 0.0


def test_argument_checks_launch_nothing():
    from vimo_clip_amd._lib import lib, ptr, stream
    n = 64
    g = torch.ones(n + 4, device="cuda")
    rec, hyper = _record(), torch.full((8,), -1.0, device="cuda")
    ws = torch.empty(int(lib.vmc_loss_scale_workspace_bytes(n)) + 16, dtype=torch.uint8, device="cuda")
    state = torch.zeros(4, dtype=torch.int64, device="cuda")

    def call(grad=g, n_=n, r=rec, h=hyper, c=None, s=None, w=ws, wb=None):
        return lib.vmc_loss_scale_check(ptr(grad), n_, ptr(r), ptr(h), ptr(c), ptr(s), ptr(w), ws.numel() - 16 if wb is None else wb, stream())
    assert call(grad=None) == E_ARG and call(r=None) == E_ARG and call(h=None) == E_ARG and call(w=None) == E_ARG and call(n_=0) == E_ARG
    assert call(wb=8) == E_ARG
    assert call(grad=g[1:]) == E_ALIGN and call(h=hyper[1:]) == E_ALIGN and call(c=hyper[5:]) == E_ALIGN and call(w=ws[4:]) == E_ALIGN
    assert call(s=state.view(torch.int32)[1:]) == E_ALIGN
    assert lib.vmc_loss_scale_workspace_bytes(1) >= 16 and lib.vmc_loss_scale_workspace_bytes(BIG) % 16 == 0
    torch.cuda.synchronize()
    assert _fields(rec)["tracker"] == 0 and (hyper == -1.0).all().item()


# ---- 2. Adam behind the skip flag ---------------------------------------------------------------------------------------------------

def _adam_buffers(n, seed):
    p, g, m, v = (synth.normal(seed, k, (n,)).cuda() for k in "pgmv")
    return p, g, m * 0.1, v.abs() * 0.01


def _hyper():
    return torch.tensor([3e-3, 3.1e-3, 1.7, 0.5], dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("n", [4099, 3])
def test_adam_step_dev_skip(n):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    args = (0.9, 0.999, 1e-8, 0.1, 1)
    flag = torch.zeros(2, dtype=torch.int32, device="cuda")
    ref, hyp = _adam_buffers(n, 3), _hyper()
    check(lib.vmc_adam_step_dev(ptr(ref[0]), ptr(ref[1]), ptr(ref[2]), ptr(ref[3]), n, ptr(hyp), *args, stream()), "adam_step_dev")
    before = _adam_buffers(n, 3)
    assert not torch.equal(ref[0], before[0]) and not torch.equal(ref[2], before[2])
    for skip, wgs in ((None, 2048), (flag, 2048), (None, 3), (flag, 3)):              # NULL and flag 0, both grid geometries
        got = _adam_buffers(n, 3)
        check(lib.vmc_adam_step_dev_skip(ptr(got[0]), ptr(got[1]), ptr(got[2]), ptr(got[3]), n, ptr(hyp), *args, wgs, ptr(skip), stream()),
              "adam_step_dev_skip")
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), (skip is None, wgs)
    flag[0] = 1
    got = _adam_buffers(n, 3)
    check(lib.vmc_adam_step_dev_skip(ptr(got[0]), ptr(got[1]), ptr(got[2]), ptr(got[3]), n, ptr(hyp), *args, 2048, ptr(flag), stream()),
          "adam_step_dev_skip")
    assert all(torch.equal(a, b) for a, b in zip(got, before))                        # p, m, v (and g) keep their bytes
    assert lib.vmc_adam_step_dev_skip(ptr(got[0]), ptr(got[1]), ptr(got[2]), ptr(got[3]), n, ptr(hyp), *args, 2048,
                                      flag.data_ptr() + 2, stream()) == E_ALIGN


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_adam_cast_multi_skip(dtype):
    """vmc_adam_cast_multi_skip over a 4099-element vector (the ranges launch) and a small matrix with both 16-bit copies (the tile
    launch): NULL and flag 0 equal vmc_adam_cast_multi bit for bit; flag 1 leaves masters, moments and both copies as they were."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd._lib import check, dt, lib, ptr, stream
    from vimo_clip_amd.optim import FusedAdam, GradArena
    shapes = [(4099,), (100, 72), (5,)]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(entry, skip):
        ag.weights.clear()
        ps = [torch.nn.Parameter(synth.normal(8, f"p{i}", sh).cuda()) for i, sh in enumerate(shapes)]
        opt = FusedAdam(GradArena(ps), lr=3e-3, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=7)
        copies = (ag.weights.get(ps[1], dtype, transposed=False, pad_k=True, both=True), ag.weights.get(ps[1], dtype, transposed=True, pad_k=True, both=True))
        for step in range(2):
            for i, p in enumerate(ps):
                p._vmc_grad.copy_(synth.normal(20 + step, f"g{i}", tuple(p.shape)).cuda())
            opt.tick()
            if step == 0:
                opt.step()                                            # builds the descriptor table and the range plan
        assert opt._fused_plan is not None and opt._fused_plan[2] == 2
        a = opt.arena
        (d16, tab), = ag.weights.tables(owner=id(opt), param_ids=opt._param_ids).items()
        plan = opt._fused_plan
        before = [t.clone() for t in (a.flat_param, opt.m, opt.v) + copies]
        common = (ptr(tab[1]), tab[2], tab[3], ptr(plan[1]), plan[2], plan[3], ptr(a.flat_param), ptr(a.flat_grad), ptr(opt.m), ptr(opt.v),
                  ptr(opt.dev_hyper), 0.9, 0.999, 1e-8, 0.1, 1, dt(d16))
        if entry == "old":
            check(lib.vmc_adam_cast_multi(*common, stream()), "adam_cast_multi")
        else:
            check(lib.vmc_adam_cast_multi_skip(*common, ptr(skip), stream()), "adam_cast_multi_skip")
        torch.cuda.synchronize()
        return before, [t.clone() for t in (a.flat_param, opt.m, opt.v) + copies]

    before, ref = run("old", None)
    assert not any(torch.equal(a, b) for a, b in zip(before, ref))
    for skip in (None, flag):
        _, got = run("skip", skip)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    flag[0] = 1
    before, got = run("skip", flag)
    assert all(torch.equal(a, b) for a, b in zip(got, before))
    ag.weights.clear()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_adam_cast_multi_master_at_an_odd_float(dtype):
    """A hand-built table of one record: a 68 x 132 master at p_base + 1 float, so 4-byte aligned only, with both 16-bit copies.  The
    kernel has to take its scalar path for it.  One vmc_adam_cast_multi leaves p, m, v and both copies equal, bit for bit, to
    vmc_adam_step_dev on 16-byte aligned copies of the same values followed by vmc_cast_weight, and the floats in front of and behind
    the matrix in all four arenas (and g everywhere) as they were."""
    from vimo_clip_amd._lib import check, dt, lib, ptr, stream
    rows, cols, ld, ldt, behind = 68, 132, 192, 128, 7
    n = rows * cols
    args = (0.9, 0.999, 1e-8, 0.1, 1)
    hyp = _hyper()
    arenas = _adam_buffers(1 + n + behind, 5)
    before = [a.clone() for a in arenas]

    def copies():
        return torch.full((rows, ld), 3.0, dtype=dtype, device="cuda"), torch.full((cols, ldt), 3.0, dtype=dtype, device="cuda")

    rp, rg, rm, rv = (a[1:1 + n].clone() for a in arenas)                 # fresh allocations: aligned
    r16, r16t = copies()
    assert rp.data_ptr() % 16 == 0
    check(lib.vmc_adam_step_dev(ptr(rp), ptr(rg), ptr(rm), ptr(rv), n, ptr(hyp), *args, stream()), "adam_step_dev")
    check(lib.vmc_cast_weight(ptr(rp), ptr(r16), ptr(r16t), rows, cols, ld, ldt, dt(dtype), stream()), "cast_weight")

    w16, w16t = copies()
    p, g, m, v = arenas
    assert p.data_ptr() % 16 == 0 and (p.data_ptr() + 4) % 16 == 4
    tiles_x, tiles_y = (cols + 63) // 64, (rows + 63) // 64
    desc = torch.tensor([[p.data_ptr() + 4, w16.data_ptr(), w16t.data_ptr(), rows | (cols << 32), ld | (ldt << 32), 0 | (tiles_x << 32)]],
                        dtype=torch.int64).cuda()
    check(lib.vmc_adam_cast_multi(ptr(desc), 1, tiles_x * tiles_y, None, 0, 0, ptr(p), ptr(g), ptr(m), ptr(v), ptr(hyp), *args, dt(dtype),
                                  stream()), "adam_cast_multi")
    torch.cuda.synchronize()

    def same(a, b):                                                       # the stored bits, not the values
        as_int = torch.int32 if a.dtype == torch.float32 else torch.int16
        return torch.equal(a.view(as_int), b.view(as_int))
    assert not same(rp, before[0][1:1 + n]) and not same(rm, before[2][1:1 + n]) and not same(rv, before[3][1:1 + n])
    for got, ref in zip((p, m, v), (rp, rm, rv)):
        assert same(got[1:1 + n], ref)
    assert same(w16, r16) and same(w16t, r16t)
    assert bool((w16[:, cols:] == 3.0).all()) and bool((w16t[:, rows:] == 3.0).all())      # the pad columns are not written
    for got, was in zip(arenas, before):
        assert same(got[:1], was[:1]) and same(got[1 + n:], was[1 + n:])
    assert same(g, before[1])


# ---- models ---------------------------------------------------------------------------------------------------------------------------

TINY_TFAM = dict(D=256, H=8, L=2, ff=512, C=140, B=4, Tr=16, Tf=15, seed=77)          # the trainer tests' smallest model (test_gpu_grad_clip.py)


def _tfam(dtype, c=TINY_TFAM):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    ag.weights.clear()
    m = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=c["C"], dropout=0.0, mlp_dropout=0.0,
                 device="cuda", compute_dtype=dtype).cuda()
    m.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], c["C"], c["seed"]), strict=True)
    return m.train()


def _tfam_batch(step, c=TINY_TFAM, Tr=None):
    Tr = c["Tr"] if Tr is None else Tr
    return (synth.normal(500 + step, "rgb", (c["B"], Tr, c["D"])).cuda(), synth.normal(500 + step, "mot", (c["B"], Tr - 1, c["D"])).cuda(),
            synth.multi_hot_labels(500 + step, "y", c["B"], c["C"]).cuda())


def _student(dtype, name="ViT-tiny/32", seed=71):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.models import FlowStudentModel
    ag.weights.clear()
    m = FlowStudentModel(name, device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype)
    sd = synth.student_state_dict(name, seed)
    m.load_state_dict(sd, strict=True)
    return m.train(), sd


def _student_batch(step, B=4, T=5, name="ViT-tiny/32"):
    R_, E = synth.VIT_GEOMETRY[name][0], synth.VIT_GEOMETRY[name][5]
    return (synth.randint_u8(71 + step, "vids", (B, T, 3, R_, R_)), synth.normal(71 + step, "teacher", (B, T + 1, E)),
            synth.multi_hot_labels(71 + step, "labels", B, 140))


def _student_loss(m, vids, teacher, labels):
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    _, emb_d, logits = m(vids)
    return distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)


# ---- 3. scale invariance ------------------------------------------------------------------------------------------------------------

def _three_steps(kind, scale, max_grad_norm):
    """Three device-state training steps in bf16; scale None = no loss scaling.  Returns (parameters, clip coefficients, first norm)."""
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    if kind == "tfam":
        m = _tfam(torch.bfloat16)
        arena = GradArena(m.used_parameters())
        opt = FusedAdam(arena, lr=1e-3, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=11)
    else:
        m, _ = _student(torch.bfloat16)
        arena = GradArena(m.parameters())
        opt = FusedAdam(arena, lr=1e-3).enable_device_state(base_seed=11)
    if scale is not None:
        opt.enable_loss_scaling(init_scale=scale, growth_factor=1.0, backoff_factor=1.0)
    coefs, norms = [], []
    for step in range(3):
        opt.tick()
        if kind == "tfam":
            rgb, mot, y = _tfam_batch(step)
            loss = bce_with_logits_loss(m(rgb, mot), y)
        else:
            vids, teacher, labels = _student_batch(step)
            loss = _student_loss(m, vids.cuda(), teacher.cuda(), labels.cuda())
        opt.scale_loss(loss).backward()
        opt.step(max_grad_norm=max_grad_norm)
        if max_grad_norm is not None:
            coefs.append(opt.last_clip_coef.item())
            norms.append(opt.last_grad_norm.item())
    if scale is not None:
        assert opt.skipped_steps.item() == 0 and opt.loss_scale.item() == scale and int(opt.dev_state[0].item()) == 3
    return arena.flat_param.detach().clone(), coefs, norms


@pytest.mark.parametrize("kind", ["tfam", "student"])
def test_power_of_two_scale_leaves_bf16_training_bit_identical(kind):
    """bf16, S = 1024 fixed: the backward is linear in its upstream gradient and a power-of-two factor commutes with every rounding
    away from under / overflow, so three steps leave the parameters of the unscaled run, bit for bit -- without clipping, and with a
    threshold (half the first step's norm, read from a probe run that never clips) that clips every step."""
    plain, _, _ = _three_steps(kind, None, None)
    scaled, _, _ = _three_steps(kind, 1024.0, None)
    assert torch.isfinite(plain).all().item() and torch.equal(plain, scaled)
    _, _, norms = _three_steps(kind, None, 1e30)
    thr = float(np.float32(0.5 * min(norms)))
    plain_c, coefs, norms_c = _three_steps(kind, None, thr)
    scaled_c, coefs_s, norms_s = _three_steps(kind, 1024.0, thr)
    print(f"{kind}: norms {norms_c} coefs {coefs} | scaled norms {norms_s} coefs {coefs_s}")
    assert all(c < 1.0 for c in coefs) and not torch.equal(plain_c, plain)
    assert coefs == coefs_s and norms_c == norms_s                   # the unscaled norm and the same coefficient
    assert torch.equal(plain_c, scaled_c)


# ---- 4. what the feature is for -------------------------------------------------------------------------------------------------------

TOL_GRAD = 8e-2                                                     # tests/test_gpu_models.py::test_student_train_step_vs_oracle_autograd
WEIGHT = 2.0 ** -12                                                 # stands for a mean over 4096 x more rows


def test_f16_gradients_need_the_scale_and_meet_the_bound_with_it():
    """The construction of tests/test_gpu_models.py::test_student_train_step_vs_oracle_autograd (ViT-tiny/32, 4 clips x 5 frames, cosine
    distillation + BCE with pw 9, every parameter's gradient against torch autograd through the fp32 CPU oracle, max error relative to
    the gradient's max <= 8e-2) in float16, with the loss multiplied by 2^-12 on both sides.  With dynamic scaling from 2^16 every
    parameter gradient (arena gradient x 1 / S) meets that bound; without scaling the first block's c_fc weight violates it."""
    from vimo_clip_amd.optim import FusedAdam, GradArena
    vids, teacher, labels = _student_batch(0)
    H = synth.VIT_GEOMETRY["ViT-tiny/32"][4]
    _, sd = _student(torch.float16)
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    _, oe_d, ol = ostudent.student_forward(sdo, vids, H, alpha=0.1, wrap_quirk=True)
    ((ostudent.distillation_loss(oe_d, teacher[:, :-1, :], "cosine") + ostudent.classification_loss(ol, labels, 9)) * WEIGHT).backward()
    dv, dt_, dl = vids.cuda(), teacher.cuda(), labels.cuda()

    def errors(m, inv_scale):
        return {k: ((p.grad.cpu().double() * inv_scale - sdo[k].grad.double()).abs().max() / (sdo[k].grad.double().abs().max() + 1e-30)).item()
                for k, p in m.named_parameters()}
    key = next(k for k in sd if k.endswith("resblocks.0.mlp.c_fc.weight"))
    # without scaling
    m, _ = _student(torch.float16)
    GradArena(m.parameters())
    (_student_loss(m, dv, dt_, dl) * WEIGHT).backward()
    plain = errors(m, 1.0)
    # with dynamic scaling from 2^16: steps that overflow are skipped and halve S; the first clean one is measured
    m, _ = _student(torch.float16)
    arena = GradArena(m.parameters())
    opt = FusedAdam(arena, lr=0.0).enable_device_state().enable_loss_scaling(init_scale=65536.0)
    for attempt in range(8):
        S = opt.loss_scale.item()
        opt.tick()
        opt.scale_loss(_student_loss(m, dv, dt_, dl) * WEIGHT).backward()
        opt.step()
        if opt.last_found_inf.item() == 0:
            break
    assert opt.last_found_inf.item() == 0 and opt.skipped_steps.item() == attempt
    scaled = errors(m, 1.0 / S)
    worst = max(scaled, key=scaled.get)
    print(f"f16 x 2^-12: S {S:g} after {attempt} skipped; unscaled {key} {plain[key]:.3e}, worst unscaled {max(plain.values()):.3e}; "
          f"scaled {key} {scaled[key]:.3e}, worst scaled {scaled[worst]:.3e} at {worst}")
    assert plain[key] > TOL_GRAD, plain[key]                         # the demonstration: most of that gradient is zero in f16
    bad = {k: e for k, e in scaled.items() if not e <= TOL_GRAD}
    assert not bad, bad


# ---- 5. / 6. the overflow path, eager, accumulated and captured ---------------------------------------------------------------------

def _copies():
    from vimo_clip_amd import autograd_ops as ag
    return [hit[3] for _, hit in sorted(ag.weights._c.items(), key=lambda kv: (kv[0][0], kv[0][2], kv[0][3]))]


def _snapshot(opt):
    return [t.clone() for t in [opt.arena.flat_param, opt.m, opt.v] + _copies()]


def _overflow_run(mode, steps=8):
    """f16 tiny TFAM from S = 2^40 with backoff 2^-8.  mode: "eager" | "accumulate" (two micro-batches per step, weights 1/2; at step 6
    an inf is planted into the FIRST micro-batch's gradient) | "captured" (GraphedTrainStep; steps 1 and 5 at another clip length, so
    captures happen while S overflows -- steps 0 and 1 -- and while it does not).  Returns per step (found, S, tracker, skipped, device t,
    parameters) after checking the per-step contract."""
    from vimo_clip_amd.graphs import GraphedTrainStep
    from vimo_clip_amd.losses import bce_with_logits_loss
    from vimo_clip_amd.optim import FusedAdam, GradArena
    m = _tfam(torch.float16)
    arena = GradArena(m.used_parameters())
    opt = FusedAdam(arena, lr=1e-3, weight_decay=0.1, decoupled=True).enable_device_state(base_seed=11)
    opt.enable_loss_scaling(init_scale=2.0 ** 40, backoff_factor=2.0 ** -8)
    m.use_device_seeds(opt)

    def step(rgb, mot, y):
        opt.tick()
        loss = bce_with_logits_loss(m(rgb, mot), y)
        opt.scale_loss(loss).backward()
        opt.step()
        return loss.detach()

    run = GraphedTrainStep(step, opt) if mode == "captured" else step
    out = []
    for i in range(steps):
        rgb, mot, y = _tfam_batch(i, Tr=12 if (mode != "accumulate" and i in (1, 5)) else None)
        S, t, skipped = opt.loss_scale.item(), int(opt.dev_state[0].item()), opt.skipped_steps.item()
        if mode == "accumulate":
            opt.tick()
            for j in range(2):
                lo = 2 * j
                opt.scale_loss(bce_with_logits_loss(m(rgb[lo:lo + 2], mot[lo:lo + 2]), y[lo:lo + 2])).backward()
                if i == 6 and j == 0:
                    arena.flat_grad[arena.numel // 2] = float("inf")
                arena.accumulate(0.5, final=j == 1)
            before = _snapshot(opt)
            opt.step()
        else:
            before = _snapshot(opt)                                   # step 0: parameters and moments only, the copies do not exist yet
            run(rgb, mot, y)
        found = opt.last_found_inf.item()
        after = _snapshot(opt)
        S1, t1 = opt.loss_scale.item(), int(opt.dev_state[0].item())
        assert len(after) > 3 and (i == 0 or len(before) == len(after)), (i, len(before), len(after))
        if found:
            assert all(torch.equal(a, b) for a, b in zip(before, after)), i      # zip: the copies too wherever they existed before
            assert S1 == S * 2.0 ** -8 and t1 == t and opt.skipped_steps.item() == skipped + 1, i
        else:
            assert not torch.equal(before[0], after[0]) and (len(before) == 3 or not torch.equal(before[3], after[3])), i
            assert S1 == S and t1 == t + 1 and opt.skipped_steps.item() == skipped, i
        out.append((found, S1, opt.dev_ls[5].item(), opt.skipped_steps.item(), t1, after[0]))
    kinds = [o[0] for o in out]
    print(mode, "found", kinds, "S", [o[1] for o in out])
    assert 0 in kinds and 1 in kinds and out[-1][3] == sum(kinds) and out[-1][4] == steps - sum(kinds)
    assert torch.isfinite(out[-1][5]).all().item()
    if mode == "accumulate":
        assert kinds[6] == 1 and kinds[5] == 0                        # the planted inf of the first micro-batch survived the fp32 sum
    if mode == "captured":
        assert run.n_graphs == 2 and opt.step_count == steps          # the host mirror counts attempts
    return out


def test_overflowing_steps_are_skipped_and_the_scale_backs_off():
    _overflow_run("eager")


def test_an_inf_from_the_first_micro_batch_skips_the_accumulated_step():
    _overflow_run("accumulate")


def test_captured_steps_equal_eager_steps_bit_for_bit():
    """GraphedTrainStep over the sequence of the eager test: found flag, S, tracker, skipped count, device step count and every
    parameter after every step equal the eager run's, bit for bit -- across the captures of two shapes while S still overflows
    (steps 0 and 1) and while it does not, whose warm-up runs therefore left the scaler record as they found it."""
    eager, captured = _overflow_run("eager"), _overflow_run("captured")
    for i, (e, c) in enumerate(zip(eager, captured)):
        assert e[:5] == c[:5], (i, e[:5], c[:5])
        assert torch.equal(e[5], c[5]), i


# ---- 7. nothing changes when it is off ----------------------------------------------------------------------------------------------

def _off_path_digest(mode):
    """Three steps of a small arena with seeded gradients (elementwise kernels only: the same bits on every run) without
    enable_loss_scaling; sha256 of parameters, m and v."""
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.optim import FusedAdam, GradArena
    ag.weights.clear()
    ps = [torch.nn.Parameter(synth.normal(8, f"p{i}", sh).cuda()) for i, sh in enumerate([(100, 72), (33,), (64, 64), (4099,)])]
    opt = FusedAdam(GradArena(ps), lr=3e-3, weight_decay=0.1, decoupled=True)
    if mode != "host":
        opt.enable_device_state(base_seed=7)
    if mode == "device_fused":
        ag.weights.get(ps[0], torch.bfloat16, transposed=False, pad_k=True, both=True)
    for step in range(3):
        for i, p in enumerate(ps):
            p._vmc_grad.copy_(synth.normal(20 + step, f"g{i}", tuple(p.shape)).cuda() * 3.0)
        if mode != "host":
            opt.tick()
        opt.step(max_grad_norm=0.7 if mode == "device_clip" else None)
    torch.cuda.synchronize()
    assert getattr(opt, "dev_ls", None) is None and (mode != "device_fused" or opt._fused_plan is not None)
    h = hashlib.sha256()
    for t in (opt.arena.flat_param, opt.m, opt.v):
        h.update(t.detach().cpu().numpy().tobytes())
    ag.weights.clear()
    return h.hexdigest()


# recorded on the commit before loss scaling existed, on an MI355X, with this very function (host, device and device_fused agree:
# the three paths are the same arithmetic, element for element)
OFF_PATH_DIGESTS = {
    "host": "617173d28e55f80083d737ccaf2864f4f0c704f5e38ccfa24e3398b03f890a26",
    "device": "617173d28e55f80083d737ccaf2864f4f0c704f5e38ccfa24e3398b03f890a26",
    "device_clip": "59a8ce94b92077e1df3c29e8e40f4cfb925707ed61871d87a99e4f4f921ac28f",
    "device_fused": "617173d28e55f80083d737ccaf2864f4f0c704f5e38ccfa24e3398b03f890a26",
}


@pytest.mark.parametrize("mode", list(OFF_PATH_DIGESTS))
def test_steps_without_loss_scaling_keep_the_bits_they_had(mode):
    assert _off_path_digest(mode) == OFF_PATH_DIGESTS[mode]


# ---- 8. the trainers ----------------------------------------------------------------------------------------------------------------

def test_student_trainer_in_f16_with_dynamic_scaling(capsys):
    """train.py --compute_dtype f16 --loss_scale dynamic [--accum_steps 2] on ViT-tiny/32: the optimiser runs in device-state mode with
    the scaler, the epoch line carries S and the skipped count, the logged loss is the unscaled one (finite and of order 1)."""
    import json

    from vimo_clip_amd import autograd_ops, train as T
    from vimo_clip_amd.dataset import SyntheticSegmentDataset
    sets = (SyntheticSegmentDataset(16, 6, 64, 140, resolution=64, seed=3), SyntheticSegmentDataset(8, 6, 64, 140, resolution=64, seed=4))
    for extra in ([], ["--accum_steps", "2"], ["--loss_scale", "4096"]):
        autograd_ops.weights.clear()
        args = T.build_parser().parse_args(["--clip_model_name", "ViT-tiny/32", "--batch_size", "4", "--sequence_length", "6", "--grad_clip_norm", "1.0",
                                            "--compute_dtype", "f16", "--loss_scale", "dynamic"] + extra)
        best = T.train(args, datasets=sets)
        line = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
        print(extra, best, line)
        assert np.isfinite(best) and 0.0 < best < 100.0
        assert line["loss_scale"] in (4096.0,) if extra == ["--loss_scale", "4096"] else 0.0 < line["loss_scale"] <= 65536.0
        assert 0 <= line["skipped_steps"] <= 4
        if extra == ["--accum_steps", "2"]:
            assert np.isfinite(line["train_total"]) and 0.0 < line["train_total"] < 100.0


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_tfam_trainer_with_a_static_scale_follows_the_unscaled_trainer(graphs):
    """ModelTrainer in bf16 with Config.loss_scale = "1024" against loss_scale = "off" over one epoch of 12 steps.  Captured: both runs
    are device-state steps, and a power-of-two scale changes no bit -- identical statistics and weights.  Eager: the unscaled run is
    the host-scalar optimiser, the scaled one the device-state optimiser (tick per step); the tolerances of the captured-against-eager
    trainer tests (statistics 2e-3, weights 5e-3 * max(1e-3, |w|max)).  The logged loss is the unscaled one either way."""
    import os

    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z = np.load(os.path.join(root, "tests", "golden", "ak_labels.npz"))
    lab = lambda split, n: torch.from_numpy(np.unpackbits(z[f"{split}/labels"], axis=1)[:n, :140].astype(np.float32))      # noqa: E731
    c = TINY_TFAM
    tr = SyntheticEmbeddingDataset(lab("train", 96), c["D"], tmin=12, tmax=16, seed=5, signal=0.6)
    va = SyntheticEmbeddingDataset(lab("val", 32), c["D"], tmin=12, tmax=16, seed=6, signal=0.6)
    runs = []
    for scale in ("off", "1024"):
        ag.weights.clear()
        cfg = Config(epochs=1, batch_size=8, d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], dropout=0.0, mlp_dropout=0.0,
                     device="cuda", checkpoint_dir=None, use_graphs=graphs, grad_clip_norm=0.29, loss_scale=scale)
        model = AMO_CLIP(d_model=c["D"], nhead=c["H"], num_layers=c["L"], dim_feedforward=c["ff"], num_classes=140, dropout=0.0, mlp_dropout=0.0, device="cuda").cuda()
        model.load_state_dict(synth.tfam_state_dict(c["D"], c["H"], c["L"], c["ff"], 140, c["seed"]), strict=True)
        t = ModelTrainer(model, tr, va, cfg)
        stats = t.train_epoch(0) + t.validate(0)
        assert t.optimizer.loss_scaling == (scale != "off")
        if scale != "off":
            assert t.optimizer.loss_scale.item() == 1024.0 and t.optimizer.skipped_steps.item() == 0 and int(t.optimizer.dev_state[0].item()) == 12
        runs.append((stats, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    (so, wo), (ss, ws) = runs
    print("off", so, "scaled", ss)
    if graphs:
        assert so == ss and all(torch.equal(wo[k], ws[k]) for k in wo)
    else:
        assert all(abs(x - y) <= 2e-3 * max(abs(x), 1e-3) for x, y in zip(so, ss)), (so, ss)
        for k in wo:
            d = (wo[k].float() - ws[k].float()).abs().max().item()
            assert d <= 5e-3 * max(1e-3, wo[k].float().abs().max().item()), (k, d)
