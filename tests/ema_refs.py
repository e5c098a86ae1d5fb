"""Plain references, inputs and the element bound for the weight-average kernels (vmc_ema_update, vmc_ema_swap).
No GPU code: numpy on the CPU only.  tests/test_ema_refs_host.py checks the references themselves; tests/test_gpu_ema_kernels.py and
tests/test_gpu_ema_step.py compare the HIP kernels and the optimiser with them.

The rule is the one of tests/train_kernel_refs.py: the reference takes the values the kernel sees (fp32 average, fp32 parameters, the
fp32 weight) and evaluates in float64 (``r64``); the same function in float32 on the CPU is the yardstick ``e32``.  The plain rule
(max error over max value) would hide an error of the UPDATE w (p - e), which is 1e-4 of the average at decay 0.9999, so the kernel is
held to an element-wise bound, derived here and not tuned:

    |got - r64| <= 2^-24 (3 w |p - e| + |r64|) + 2^-149

  The kernel computes d = fl(p - e) and fl(w d + e) with one fused multiply-add.  d carries a relative error of at most 2^-24, which
  the multiplication by w turns into 2^-24 w |p - e|; the fma rounds once at the size of the result, 2^-24 |r64| (to first order); a
  device quotient 9 / (10 + t) that is one ulp (2^-23 relative) away from the numpy quotient moves the update by another
  2 2^-24 w |p - e|; 2^-149 is the spacing of the subnormals, where relative bounds stop.  An fp32 model of the arithmetic
  (``ema_model32``) stays inside the bound without the quotient's slack.

The inputs keep |p - e| of the order of |e|, so that the update is far above an ulp of the average even at w = 1e-4 and the comparison
is sensitive to it (the reason the Adam update has its own bound in tests/loss_optim_refs.py).
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS24 = 2.0 ** -24
TINY = 2.0 ** -149
E32_MAX = 2.0 ** -18

SIZES = [1, 3, 4, 1023, 4101, (1 << 20) + 7]           # tests/test_gpu_loss_scale.py
BIG = 4 * 2048 * 512 + 4101                             # more than one trip of the capped grid (2048 workgroups x 512 float4)
GUARD = 8
WEIGHTS = (1.0, 0.5, 1e-2, 1e-4)                        # without warm-up
WARMUP_T = (1, 2, 89, 90, 10 ** 5)                      # 9/11, 9/12, 9/99, 9/100 (an inexact and an "even" quotient), and 9e-5 < 1e-4: the floor wins


def f32v(x):
    """The float32 value of a Python number, as a Python float: what the kernel receives for a float argument."""
    return float(F32(x))


def one_minus_decay(decay):
    """1 - decay rounded ONCE to fp32 from float64, as the host does before the call."""
    return F32(1.0 - float(decay))


def weight_of(one_minus_decay_, warmup, t):
    """The fp32 weight w of step t (the step count AFTER the step's own increment, so the first step has t = 1), as numpy float32
    arithmetic gives it: 1 - decay, or with warm-up max(1 - decay, 9 / (10 + t))."""
    w = F32(one_minus_decay_)
    if not warmup:
        return w
    return max(w, F32(9.0) / F32(10 + int(t)))


def ema_ref(e, p, w, dtype=F64):
    """e + w (p - e) on the fp32 values the kernel sees, evaluated in ``dtype`` (float64: r64; float32: the plain two-rounding e32
    yardstick).  e, p: arrays; w: the fp32 weight."""
    e, p, w = np.asarray(e).astype(dtype), np.asarray(p).astype(dtype), dtype(F32(w))
    return e + w * (p - e)


def ema_model32(e, p, w):
    """fp32 model of the kernel's own arithmetic: d = fl32(p - e), then fl32 of the exact w d + e.  The product of two fp32 values is
    exact in float64; the float64 sum rounds once more before the fp32 rounding, which moves a result only in a double-rounding tie."""
    e, p = np.asarray(e, F32), np.asarray(p, F32)
    d = (p - e).astype(F32)
    return (F64(F32(w)) * d.astype(F64) + e.astype(F64)).astype(F32)


def ema_two_rounding32(e, p, w):
    """The contraction-dependent variant the kernel must NOT be: fl32(fl32(w d) + e), three roundings."""
    e, p = np.asarray(e, F32), np.asarray(p, F32)
    d = (p - e).astype(F32)
    return ((F32(w) * d).astype(F32) + e).astype(F32)


def allow(e, p, w, r64=None):
    """The element bound of the module docstring, one value per element."""
    e64, p64 = np.asarray(e, F32).astype(F64), np.asarray(p, F32).astype(F64)
    r64 = ema_ref(e, p, w) if r64 is None else r64
    return EPS24 * (3.0 * float(F32(w)) * np.abs(p64 - e64) + np.abs(r64)) + TINY


def excess(got, e, p, w):
    """max over the elements of |got - r64| / bound: <= 1 passes.  A non-finite result counts as a violation."""
    r64 = ema_ref(e, p, w)
    got = np.asarray(got, F32).astype(F64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - r64) / allow(e, p, w, r64)).max())


def e32_of(e, p, w):
    """max|f32 - r64| / max|r64| of the plain float32 evaluation: the yardstick of the plain rule."""
    r64 = ema_ref(e, p, w)
    return float(np.abs(ema_ref(e, p, w, F32).astype(F64) - r64).max() / np.abs(r64).max())


def inputs(n, seed=0):
    """(e, p): fp32, standard normal and independent, so |p - e| is of the order of |e|."""
    rng = np.random.default_rng(7000 + 13 * seed + n % 9973)
    return rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)


def planted_two_rounding_input():
    """(e, p, w) on which the fused multiply-add and the two-rounding variant differ in their bits in EVERY element: w = 1e-4 (fp32),
    e = 2^-14 and p = 1 + k 2^-10, so that d = p - e is exact and the update w d is of the size of e -- the rounding of the separate
    multiply is then of the size of the sum's own ulp and moves the result, which the fma's single rounding does not see.  The first 64
    such k (searched, not assumed)."""
    k = np.arange(1, 1024, dtype=F32)
    e = np.full(len(k), 2.0 ** -14, F32)
    p = (F32(1) + k * F32(2.0 ** -10)).astype(F32)
    exact = (p - e).astype(F32).astype(F64) == p.astype(F64) - e.astype(F64)
    keep = np.flatnonzero(exact & (ema_model32(e, p, 1e-4) != ema_two_rounding32(e, p, 1e-4)))[:64]
    assert len(keep) == 64, "no planted inputs found"
    return e[keep], p[keep], F32(1e-4)


def run(e0, ps, one_minus_decay_, warmup, skips=(), t0=0, update=None):
    """A sequence of steps as the optimiser runs them: step i ticks t, then -- unless i is in ``skips``: the loss scale found an
    overflow, the tick is taken back and the average keeps its bytes -- e = update(e, ps[i], weight_of(..., t)).  ``update`` defaults to
    the float64 reference rounded to fp32 per step.  Returns ([e after each step], [w used or None], final t)."""
    if update is None:
        update = lambda e, p, w: ema_ref(e, p, w).astype(F32)      # noqa: E731
    e, t, out, ws = np.asarray(e0, F32).copy(), int(t0), [], []
    for i, p in enumerate(ps):
        t += 1
        if i in skips:
            t -= 1
            ws.append(None)
        else:
            w = weight_of(one_minus_decay_, warmup, t)
            e = np.asarray(update(e, p, w), F32)
            ws.append(w)
        out.append(e.copy())
    return out, ws, t
