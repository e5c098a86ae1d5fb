"""GPU: gradient accumulation over micro-batches on the gradient arena -- vmc_grad_accumulate against its numpy reference
(tests/grad_accum_ref.py), GradArena.accumulate on the student (exact plumbing, and against the CPU oracle's full-batch autograd),
the optimiser after a finalised accumulation, and the trainer's --accum_steps."""
import functools
import gc
import json

import numpy as np
import pytest
import torch

import grad_accum_ref as R
from oracle import student as ostudent
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 64, 4101, (1 << 20) + 7]          # the scalar tail alone, one float4, an odd size, and more than one grid stride
POW2 = [1.0, 0.5, 0.25]
OTHER = [0.375, 1.0 / 3.0]


@functools.lru_cache(maxsize=None)
def _host(n):
    rng = np.random.default_rng(1000 + n)
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-10, 10, n))).astype(np.float32)
    acc = (rng.standard_normal(n) * np.exp2(rng.integers(-10, 10, n))).astype(np.float32)
    g.setflags(write=False)
    acc.setflags(write=False)
    return g, acc


def _call(g, acc, out, n, w, mode):
    from vimo_clip_amd._lib import lib, stream
    return lib.vmc_grad_accumulate(g.data_ptr() if g is not None else None, acc.data_ptr() if acc is not None else None,
                                   out.data_ptr() if out is not None else None, n, float(w), mode, stream())


def _run(n, w, mode, alias):
    """Returns (result, g after, acc after) as numpy arrays, with guard elements behind every buffer checked."""
    hg, hacc = _host(n)
    pad = 8
    bufs = {}
    for name, src in (("g", hg), ("acc", hacc), ("out", None)):
        t = torch.full((n + pad,), -77.0, device="cuda")
        if src is not None:
            t[:n] = torch.from_numpy(src.copy()).cuda()
        bufs[name] = t
    out = bufs["g"] if alias else bufs["out"]
    assert _call(bufs["g"], bufs["acc"], out, n, w, mode) == 0
    torch.cuda.synchronize()
    for t in bufs.values():
        assert (t[n:] == -77.0).all().item()                                   # nothing written past n
    res = (out if mode == 2 else bufs["acc"])[:n].cpu().numpy()
    if mode != 2 or alias:
        assert (bufs["out"] == -77.0).all().item()                             # out is not touched
    return res, bufs["g"][:n].cpu().numpy(), bufs["acc"][:n].cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_the_reference(n):
    hg, hacc = _host(n)
    for mode in (0, 1, 2):
        for alias in ((False, True) if mode == 2 else (False,)):
            for w in POW2 + OTHER:
                got, g_after, acc_after = _run(n, w, mode, alias)
                want = R.grad_accumulate_ref(hg, hacc, w, mode)
                if w in POW2:
                    assert np.array_equal(got, want), (n, mode, alias, w)      # fmaf == sequential fp32, bit for bit
                else:
                    d = int(R.ulp_distance(got, want).max())
                    assert d <= 1, (n, mode, alias, w, d)                      # one more rounding in the float64 reference
                if not (mode == 2 and alias):
                    assert np.array_equal(g_after, hg)
                if mode == 2:
                    assert np.array_equal(acc_after, hacc)                     # the final pass leaves the accumulator alone


def test_kernel_propagates_inf_and_nan():
    n = 4101
    hg, hacc = (a.copy() for a in _host(n))
    hg[[0, 5, 4100]] = [np.inf, -np.inf, np.nan]                              # vector body and scalar tail
    hacc[[5, 9]] = [np.inf, np.nan]
    g, acc = torch.from_numpy(hg).cuda(), torch.from_numpy(hacc).cuda()
    out = torch.empty_like(g)
    for mode in (0, 1, 2):
        a = acc.clone()
        assert _call(g, a, out, n, 0.5, mode) == 0
        got = (out if mode == 2 else a).cpu().numpy()
        want = R.grad_accumulate_ref(hg, hacc, 0.5, mode)
        assert np.array_equal(got, want, equal_nan=True), mode
        assert np.isnan(got[4100]) and np.isinf(got[0])
        assert np.isnan(got[5]) if mode else got[5] == -np.inf                 # -inf + inf


def test_argument_checks_launch_nothing():
    from vimo_clip_amd._lib import lib
    n = 64
    g = torch.ones(n + 4, device="cuda")
    acc = torch.full((n + 4,), 2.0, device="cuda")
    out = torch.full((n + 4,), 5.0, device="cuda")                            # not w * g + acc = 3: a mode-2 launch would show
    E_ARG, E_ALIGN = -1, -2
    assert b"alignment" in lib.vmc_error_string(E_ALIGN)
    for mode in (-1, 3, 7):
        assert _call(g, acc, out, n, 1.0, mode) == E_ARG
    for mode in (0, 1, 2):                                                    # every pointer is required in every mode
        assert _call(None, acc, out, n, 1.0, mode) == E_ARG and _call(g, None, out, n, 1.0, mode) == E_ARG
        assert _call(g, acc, None, n, 1.0, mode) == E_ARG
    assert _call(g[1:], acc, out, n, 1.0, 7) == E_ARG                         # the order: arguments before alignment
    for bad in ((g[1:], acc, out), (g, acc[1:], out), (g, acc, out[1:])):     # a pointer 4 bytes off
        assert _call(*bad, n, 1.0, 2) == E_ALIGN
    assert _call(g[1:], acc, out, 0, 1.0, 2) == E_ALIGN                       # ... and alignment before the empty case
    assert _call(g, acc, out, 0, 1.0, 2) == 0
    torch.cuda.synchronize()
    assert (g == 1).all().item() and (acc == 2).all().item() and (out == 5).all().item()


# ---- the student ------------------------------------------------------------------------------------------------------------------
def _student(name, seed, dtype, recompute="none"):
    from vimo_clip_amd.models import FlowStudentModel
    m = FlowStudentModel(name, device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype, recompute=recompute)
    sd = synth.student_state_dict(name, seed)
    m.load_state_dict(sd, strict=True)
    return m.train(), sd


def _loss(m, vids, teacher, labels):
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    emb, emb_d, logits = m(vids)
    return distillation_loss(emb_d, teacher[:, :-1, :], mode="cosine") + classification_loss(logits, labels, positive_weight=9)


def _accumulated(m, arena, vids, teacher, labels, sizes):
    """Back-propagate the micro-batches of `sizes` clips one after the other; returns the clones of the arena after each backward."""
    B, lo, clones = vids.shape[0], 0, []
    assert sum(sizes) == B
    for j, k in enumerate(sizes):
        _loss(m, vids[lo:lo + k], teacher[lo:lo + k], labels[lo:lo + k]).backward()
        clones.append(arena.flat_grad.clone())
        arena.accumulate(k / B, final=j == len(sizes) - 1)
        assert arena.pending == (0 if j == len(sizes) - 1 else j + 1)
        lo += k
    return clones


PLUMBING = [
    # name, videos, dtype, clips per micro-batch, recompute
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.bfloat16, (4, 4), "none"),
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.bfloat16, (2, 2, 2, 2), "none"),
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.float16, (4, 4), "none"),
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.float16, (2, 2, 2, 2), "none"),
    ("ViT-tiny/32", (8, 16, 3, 64, 64), torch.bfloat16, (2, 2, 2, 2), "block"),
    ("ViT-tiny/14", (2, 3, 3, 56, 56), torch.bfloat16, (1, 1), "none"),       # 51 rows per micro-batch: ungrouped weight gradients
]


@pytest.mark.parametrize("name,shape,dtype,sizes,recompute", PLUMBING, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_student_accumulation_is_the_fp32_combination_of_the_micro_gradients(name, shape, dtype, sizes, recompute):
    from vimo_clip_amd.optim import GradArena
    B, T = shape[:2]
    E = synth.vit_geometry(name)[5]
    m, _ = _student(name, 31, dtype, recompute)
    arena = GradArena(m.parameters())
    vids = synth.randint_u8(31, "vids", shape).cuda()
    teacher = synth.normal(31, "teacher", (B, T + 1, E)).cuda()
    labels = synth.multi_hot_labels(31, "labels", B, 140).cuda()
    clones = _accumulated(m, arena, vids, teacher, labels, sizes)
    want = clones[0] * (sizes[0] / B)                                          # power-of-two weights: the products are exact
    for c, k in zip(clones[1:], sizes[1:]):
        want = want + c * (k / B)
    assert not any(torch.equal(clones[0], c) for c in clones[1:])              # the micro-batches do differ
    used = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
    assert torch.isfinite(used).all().item()
    assert torch.equal(arena.flat_grad, want)
    assert arena.flat_acc is not None and arena.flat_acc.numel() == arena.numel


def _rel_l2(got, ref):
    return ((got - ref).double().norm() / (ref.double().norm() + 1e-300)).item()


# (accumulated error / single-pass error - 1), largest over the parameters, measured on the MI355X (profiles/grad_accum.md).
# 4 + 4: every micro-batch scales the loss gradient by exactly 2, so all 16-bit roundings repeat and only the fp32 order of the
# weight-gradient sums differs -- 6e-6 of the error.  5 + 3: the scales 8/5 and 8/3 round the 16-bit loss gradients differently
# from the single pass; the errors (3.2e-3 against 2.3e-3 at the worst parameter, the median parameter 0.7 % BETTER) are two
# draws of the same 16-bit rounding noise, not a loss of accuracy ...
EXCESS_MEASURED = {"2x4": 6.0111e-06, "5+3": 4.0189e-01}
# ... and the margin the accumulated gradient is allowed: twice that
MARGIN = {k: 2.0 * v for k, v in EXCESS_MEASURED.items()}


def test_student_accumulated_gradient_vs_oracle_autograd():
    """The construction of tests/test_gpu_models.py::test_student_train_step_vs_oracle_autograd at 8 clips: the full-batch gradient of
    every parameter from torch autograd through the fp32 CPU oracle is the reference; (a) the single-pass GPU gradient -- what the
    engine computes without accumulation -- is the yardstick; (b) the accumulated gradients of a 4 + 4 and of an unequal 5 + 3 split
    may be further from the reference than (a), per parameter in relative L2, by the margin above and no more."""
    from vimo_clip_amd.optim import GradArena
    name, B, T = "ViT-tiny/32", 8, 5
    R_, H = synth.VIT_GEOMETRY[name][0], synth.VIT_GEOMETRY[name][4]
    m, sd = _student(name, 71, torch.bfloat16)
    vids = synth.randint_u8(71, "vids", (B, T, 3, R_, R_))
    teacher = synth.normal(71, "teacher", (B, T + 1, 64))
    labels = synth.multi_hot_labels(71, "labels", B, 140)
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    _, oe_d, ol = ostudent.student_forward(sdo, vids, H, alpha=0.1, wrap_quirk=True)
    (ostudent.distillation_loss(oe_d, teacher[:, :-1, :], "cosine") + ostudent.classification_loss(ol, labels, 9)).backward()
    arena = GradArena(m.parameters())
    dv, dt_, dl = vids.cuda(), teacher.cuda(), labels.cuda()
    names = [k for k, _ in m.named_parameters()]

    def errors():
        return {k: _rel_l2(p.grad.cpu(), sdo[k].grad) for k, p in m.named_parameters()}
    _loss(m, dv, dt_, dl).backward()
    single = errors()
    assert max(single.values()) < 8e-2                                         # the yardstick itself is sane
    report = {}
    failures = []
    for tag, sizes in (("2x4", (4, 4)), ("5+3", (5, 3))):
        arena.flat_grad.zero_()
        _accumulated(m, arena, dv, dt_, dl, sizes)
        acc = errors()
        excess = {k: acc[k] / single[k] - 1.0 for k in names}
        worst = max(excess, key=excess.get)
        report[tag] = {"worst_parameter": worst, "excess": excess[worst], "single": single[worst], "accumulated": acc[worst],
                       "median_excess": float(np.median(list(excess.values())))}
        print(f"accumulated {tag} vs single pass, rel-L2 against the oracle: worst excess {excess[worst]:+.4e} at {worst} "
              f"({acc[worst]:.4e} vs {single[worst]:.4e}); median excess {report[tag]['median_excess']:+.4e}")
        if excess[worst] > MARGIN[tag]:
            failures.append((tag, worst, excess[worst], MARGIN[tag]))
    print("GRAD_ACCUM_ORACLE " + json.dumps(report))
    assert not failures, failures


# ---- the optimiser ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_state", [True, False], ids=["device_clip", "host_no_clip"])
def test_optimizer_after_a_finalised_accumulation(device_state):
    """After accumulate(final=True) a step leaves the parameters of a second arena whose flat_grad was filled with the manual combination
    and stepped the same way, bit for bit.  With clipping (max_grad_norm = 1) that is asked of the device-state optimiser, whose norm
    (vmc_grad_clip_dev) is a fixed-order sum.  The host-side clipping path reads its norm from vmc_sumsq, which adds its workgroup
    partials with float atomics: two steps on the SAME gradient bits can differ in the last bit of the clip factor there (seen on the
    MI355X when this test ran after other tests), whatever filled the gradient -- so the host-state case steps without clipping."""
    from vimo_clip_amd.optim import FusedAdam, GradArena
    clip = 1.0 if device_state else None
    shapes = [(33, 7), (129,), (64, 64), (5,)]
    weights = (0.5, 0.25, 0.25)

    def make():
        ps = [torch.nn.Parameter(synth.normal(5, f"p{i}", s).cuda()) for i, s in enumerate(shapes)]
        arena = GradArena(ps)
        opt = FusedAdam(arena, lr=1e-2)
        return arena, (opt.enable_device_state() if device_state else opt)
    a1, o1 = make()
    a2, o2 = make()
    for step in range(2):
        gs = [synth.normal(100 + 3 * step + j, "g", (a1.numel,)).cuda() * 3.0 for j in range(3)]      # norm well above the threshold
        for j, w in enumerate(weights):
            a1.flat_grad.copy_(gs[j])
            if j == 1:
                with pytest.raises(RuntimeError, match="final=True"):
                    o1.step(max_grad_norm=clip)                                # a pending accumulation: stepping is refused
                assert o1.step_count == step
            a1.accumulate(w, final=j == 2)
        a2.flat_grad.copy_((gs[0] * 0.5 + gs[1] * 0.25) + gs[2] * 0.25)
        assert torch.equal(a1.flat_grad, a2.flat_grad)
        for o in (o1, o2):
            if device_state:
                o.tick()
            o.step(max_grad_norm=clip)
    torch.cuda.synchronize()
    assert torch.isfinite(a1.flat_param).all().item() and torch.equal(a1.flat_param, a2.flat_param)
    assert torch.equal(o1.m, o2.m) and torch.equal(o1.v, o2.v)


def test_accumulate_raises_inside_a_capture():
    from vimo_clip_amd.optim import GradArena
    arena = GradArena([torch.nn.Parameter(torch.zeros(256, device="cuda"))])
    arena.accumulate(0.5)                                                      # the accumulator exists before the capture
    arena.accumulate(0.5, final=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="capture"):                         # as tests/test_gpu_grad_clip.py raises out of a capture
        with torch.cuda.graph(graph):
            arena.flat_grad.mul_(2.0)
            arena.accumulate(0.5)
    torch.cuda.synchronize()
    assert arena.pending == 0
    arena.accumulate(0.5)                                                      # eager again: allowed
    assert arena.pending == 1


# ---- the trainer --------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_student_recompute.py::test_peak_memory_of_a_recomputed_step bounds the peak ratio by min(0.5, 1.1 * measured ratio):
# 0.367 at 64 frames and 0.390 at 128 frames (the 0.5 cap never binds), where the byte model predicts (4 L + 36) / (36 L) = 0.236
# (L = 8).  So it accepts a saving of at least 1 - 0.390 = 0.610 of the peak against a predicted saving of 0.764: 0.798 of the byte
# model's difference (0.829 at 64 frames; the looser of its two cases is taken).  The same share is asked of accumulation here.
from test_gpu_student_recompute import GEO as _RECOMPUTE_GEO, PEAK_RATIO_MEASURED  # noqa: E402

_L = _RECOMPUTE_GEO[3]
PEAK_SHARE_OF_MODEL = (1.0 - min(0.5, 1.1 * max(PEAK_RATIO_MEASURED.values()))) / (1.0 - (4 * _L + 36) / (36 * _L))


def test_trainer_accum_steps_runs_and_lowers_the_peak(capsys):
    from vimo_clip_amd import autograd_ops, train as T
    from vimo_clip_amd.autograd_vit import saved_activation_bytes
    from vimo_clip_amd.dataset import SyntheticSegmentDataset
    name, clips, seq = "ViT-tiny/32", 32, 17
    # two training steps per run; an empty validation set, so that the peak of a run is the peak of its training steps
    sets = (SyntheticSegmentDataset(64, seq, 64, 140, resolution=64, seed=3), SyntheticSegmentDataset(0, seq, 64, 140, resolution=64, seed=4))
    peak, out, numel = {}, {}, None
    # a throw-away run first: whatever the process allocates once and keeps (workspaces, cached buffers) is in `base` of BOTH measured runs
    for accum in (4, 1, 4):
        args = T.build_parser().parse_args(["--clip_model_name", name, "--batch_size", str(clips), "--sequence_length", str(seq),
                                            "--accum_steps", str(accum), "--grad_clip_norm", "1.0"])
        assert args.accum_steps == accum
        autograd_ops.weights.clear()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        best = T.train(args, datasets=sets)
        torch.cuda.synchronize()
        peak[accum] = torch.cuda.max_memory_allocated() - base
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        out[accum] = (best, lines[-1])
    assert np.isfinite(out[4][0]) and np.isfinite(out[4][1]["train_total"]) and out[4][1]["train_total"] > 0
    assert "train_total" not in out[1][1]                                      # one pass: the log line as it was
    frames = clips * (seq - 1)
    from vimo_clip_amd.models import FlowStudentModel
    numel = sum((p.numel() + 63) // 64 * 64 for p in FlowStudentModel(name, device="cpu", num_classes=140).parameters() if p.requires_grad)
    model = saved_activation_bytes(name, frames, "none") - saved_activation_bytes(name, frames // 4, "none") - 4 * numel
    saved = peak[1] - peak[4]
    print(f"trainer peak: one pass {peak[1]} B, 4 micro-batches {peak[4]} B, saved {saved} B; byte model {model} B "
          f"(needs {PEAK_SHARE_OF_MODEL:.3f} of it: {PEAK_SHARE_OF_MODEL * model:.0f} B)")
    assert model > 0
    assert saved >= PEAK_SHARE_OF_MODEL * model, (peak, model)
