"""numpy reference of vmc_grad_accumulate (include/vmc.h K20): the three modes on fp32 arrays.

  mode 0  acc = weight * g          returns the new acc
  mode 1  acc = weight * g + acc    returns the new acc
  mode 2  out = weight * g + acc    returns out (acc is left as it is)

The kernel computes fmaf(weight, g, acc): the exact product and sum, rounded once.
- weight a power of two: weight * g is exact in fp32 (away from underflow), so sequential fp32 arithmetic ``acc + weight * g`` rounds
  the same exact value once and IS the kernel's result, bit for bit.  That is what this reference computes.
- any other weight: the product of two fp32 values is exact in float64 (24 + 24 significand bits), the float64 sum rounds once and
  the conversion to fp32 rounds a second time.  A second rounding can move the result by at most one fp32 ulp from the correctly
  rounded one, so the kernel is within ONE ULP of this reference (``ulp_distance``).
"""
import math

import numpy as np


def is_power_of_two(w: float) -> bool:
    m, _ = math.frexp(abs(float(w)))
    return m == 0.5


def grad_accumulate_ref(g, acc, weight, mode):
    g = np.asarray(g, dtype=np.float32)
    w = np.float32(weight)
    if mode not in (0, 1, 2):
        raise ValueError(mode)
    with np.errstate(all="ignore"):
        if is_power_of_two(w):
            prod = w * g                                                   # exact
            return prod if mode == 0 else (np.asarray(acc, dtype=np.float32) + prod).astype(np.float32)
        prod = np.float64(w) * g.astype(np.float64)                        # exact
        if mode == 0:
            return prod.astype(np.float32)
        return (np.asarray(acc, dtype=np.float32).astype(np.float64) + prod).astype(np.float32)


def ulp_distance(a, b):
    """Distance in units of the last place between two fp32 arrays (0 where both are NaN or the same infinity)."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)

    def ordered(x):                                                        # monotone map of the fp32 line onto the integers
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 31)) - i, i)
    d = np.abs(ordered(a) - ordered(b))
    both_nan = np.isnan(a) & np.isnan(b)
    return np.where(both_nan, 0, np.where(np.isnan(a) | np.isnan(b), np.int64(2 ** 32), d))
