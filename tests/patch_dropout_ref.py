"""CPU restatements of the patch-dropout stem kernels (vimo_clip_amd/csrc/patch_dropout.hip, include/vmc.h), written from the
header's definitions: the keep-set sampler on attention_refs.hash32, the row gather, the token assembly on the kept patches and
its backward.  No GPU code: numpy, and torch only for the 16-bit roundings."""
import math

import numpy as np
import torch

from attention_refs import hash32


def keep_count(G, p):
    """open_clip's PatchDropout rule."""
    return max(1, int(G * (1.0 - p)))


def keep_sample(seed, F, G, Kp):
    """int32 [F, Kp]: per frame the Kp patches with the smallest (hash32(seed, f G + n), n), in ascending n."""
    n = np.arange(G, dtype=np.uint64)
    out = np.empty((F, Kp), dtype=np.int32)
    for f in range(F):
        key = hash32(seed, np.uint64(f * G) + n)
        order = np.lexsort((n, key))                     # by key, ties by patch id: a strict total order
        out[f] = np.sort(order[:Kp])
    return out


def gather_rows(src, keep, G):
    """src [F*G, cols] -> [F*Kp, cols]."""
    F, Kp = keep.shape
    rows = (np.arange(F)[:, None] * G + keep).reshape(-1)
    return src[rows]


def assemble_keep(xp16, cls, pos, keep, out_dtype):
    """xp16 torch 16-bit [F*Kp, D], cls f32 [D], pos f32 [G+1, D], keep int [F, Kp] -> torch [F*(Kp+1), D] of out_dtype: one fp32
    add per element, then the rounding of the store."""
    F, Kp = keep.shape
    D = xp16.shape[1]
    k = torch.as_tensor(np.asarray(keep), dtype=torch.long)
    x = torch.empty((F, Kp + 1, D), dtype=torch.float32)
    x[:, 0] = cls.float() + pos[0].float()
    x[:, 1:] = xp16.float().view(F, Kp, D) + pos.float()[k + 1]
    return x.view(F * (Kp + 1), D).to(out_dtype)


def assemble_keep_bwd(dx, keep, G, dtype16):
    """dx torch [F*(Kp+1), D] (f32 or 16-bit) -> (dxp of dtype16 [F*Kp, D], dpos float64 [G+1, D], abs float64 [G+1, D]): dpos the
    exact sums of the stored values, abs the sums of their magnitudes (what the fp32 reassociation bound scales with).  dcls = dpos[0]."""
    F, Kp = keep.shape
    D = dx.shape[1]
    d = dx.view(F, Kp + 1, D)
    dxp = d[:, 1:].float().to(dtype16).reshape(F * Kp, D)
    d64 = d.double().numpy()
    dpos = np.zeros((G + 1, D))
    mag = np.zeros((G + 1, D))
    for f in range(F):
        dpos[0] += d64[f, 0]
        mag[0] += np.abs(d64[f, 0])
        for j in range(Kp):
            dpos[keep[f, j] + 1] += d64[f, j + 1]
            mag[keep[f, j] + 1] += np.abs(d64[f, j + 1])
    return dxp, dpos, mag


def reassociation_bound(F, mag):
    """Two fp32 sums of the same F addends in different orders (or one of them and the exact sum) differ by at most
    (F - 1) 2^-24 sum|addend| (1 + O(2^-24)) each, so by less than F 2^-23 sum|addend|."""
    return F * 2.0 ** -23 * mag


def binomial_two_sided_tail(n, p, d):
    """P(|X - n p| >= d) for X ~ Binomial(n, p), summed exactly from the mass function (log-gamma form)."""
    lo, hi = n * p - d, n * p + d
    total = 0.0
    for k in range(n + 1):
        if k <= lo or k >= hi:
            total += math.exp(math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1) + k * math.log(p) + (n - k) * math.log(1 - p))
    return total


def inclusion_deviation_bound(n_seeds, G, Kp, alpha=1e-6):
    """The smallest deviation d (in counts) with G P(|X - n Kp / G| >= d) <= alpha, X ~ Binomial(n_seeds, Kp / G): under a uniform
    sampler each patch's inclusion count is such an X, and the union bound over the G patches (they are dependent; the union bound
    does not care) makes alpha the chance that ANY patch deviates by d or more."""
    p = Kp / G
    d = 0
    while G * binomial_two_sided_tail(n_seeds, p, d) > alpha:
        d += 1
    return d
