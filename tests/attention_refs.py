"""Float64 references, the designed-rounding model, the error measure, selector inputs and the case lists for the attention
kernels (vmc_attention_vit_fwd / vmc_attention_vit_cls_fwd / vmc_attention_fwd / vmc_attention_bwd).  No GPU code: torch and numpy
on the CPU only.  tests/test_attention_refs_host.py checks everything in here on the CPU (against torch and the oracle, against
attn_route.h, and with wrong attentions that must be caught); tests/test_gpu_attention_parity.py compares the HIP kernels.

The kernels round the probabilities and dS to 16 bits on purpose, so a float64 comparison needs a
yardstick that contains those roundings and nothing else: ``attn_model16`` evaluates the operation in float64 and rounds exactly
where the kernels are designed to round.  Per output tensor, over the live rows,

    E_rms = rms(model - r64),  E_max = max|model - r64|
    out, dq, dk, dv:  rms(got - r64) <= R_RMS * E_rms   and   max|got - r64| <= R_MAX * E_max
    lse:              max|got - r64| <= R_MAX * max(E_max, 2^-23 * max(1, max|r64|))
(E_rms, E_max of the other outputs are floored the same way by one fp32 rounding of the absolute sums behind them: where a clip has a
single live key the float64 dq and dk cancel to exactly zero, the model's error is zero, and fp32 accumulation is all that is left.)

R_RMS = 2: the kernel rounds at the model's points with independent errors, so its rms over thousands of elements is that of the
model; 2 leaves room for one more source of the same size (fp32 accumulation order, exp2 at 1 ulp).  R_MAX = 4: a maximum over up to
1e5 elements fluctuates more.  Neither was calibrated on a kernel.  A bound must also mean something: every case has to satisfy
R_MAX * E_max <= 0.25 rms(r64) and R_RMS * E_rms <= 0.1 rms(r64) (``vacuity``).

The scalar fp32 kernels round nothing inside; their yardstick is train_kernel_refs' e32 (the same formulas evaluated in float32 on
the CPU) with its MARGIN, and their backward is fed CPU-made ``out`` / ``lse`` so that the reference sees the very same inputs.

Selector inputs make every query attend to exactly one known key (probability >= 1 - 2^-20 in float64, in fact far closer), so a
dropped, duplicated or mispaired key at any position shows as wrong bits: ``selector_inputs`` / ``selector_check``.
"""
import math

import numpy as np
import torch

from train_kernel_refs import BF16, DT16, DT_NAME, EPS32, F16, F32, MARGIN, bound32, max_rel, ulp, ulp16, widen  # noqa: F401

R_RMS = 2.0
R_MAX = 4.0
VAC_MAX = 0.25
VAC_RMS = 0.1
SEL_A = 16.0                 # |q| per component of a selector query: the winning score is SEL_A sqrt(dh)
SEL_SENTINEL = 1024.0        # V rows of masked keys
SEL_PROB = 1.0 - 2.0 ** -20  # the stated condition on the winner's probability
SEL_LOSS = 2.0 ** -40        # what the inputs are drawn to meet: total probability of the losers (27.7 nats), see selector_inputs
SEL_VMIN = 2.0 ** -6         # smallest |V|, |dO| component of selector inputs

OUTS = ("out", "lse", "dq", "dk", "dv")


# ---------------------------------------------------------------------------------------------- layout, rounding, dropout
def round16(x, dtype):
    """float64 -> float32 -> 16 bit -> float64: the path a kernel's fp32 value takes into a 16-bit register or store."""
    return x.to(F32).to(dtype).to(torch.float64)


def heads(x, B, T, H, dh):
    """[B*T, >= H*dh] (the kernels' layout; only the first H*dh columns count) -> float64 [B, H, T, dh]."""
    return widen(x)[:, :H * dh].reshape(B, T, H, dh).transpose(1, 2)


def flat(x):
    """[B, H, T, dh] -> [B*T, H*dh]."""
    B, H, T, dh = x.shape
    return x.transpose(1, 2).reshape(B * T, H * dh)


def hash32(seed, idx):
    """common.h hash32 on a numpy uint64 array of element indices."""
    with np.errstate(over="ignore"):
        x = (idx.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(seed)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.uint32)


def dropout_fac(p, seed, B, H, Tq, Tk, swap=False):
    """The factor tensor [B, H, Tq, Tk] of vmc_dropout's counter-based mask on the flat index ((b H + h) Tq + t) Tk + key: 0 or the
    fp32 value 1 / (1 - p).  The GPU tests check it against vmc_dropout on ones.  swap: the WRONG index with Tq and Tk exchanged."""
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    t = np.arange(Tq, dtype=np.uint64)[None, :, None]
    key = np.arange(Tk, dtype=np.uint64)[None, None, :]
    idx = (bh * np.uint64(Tk) + t) * np.uint64(Tq) + key if swap else (bh * np.uint64(Tq) + t) * np.uint64(Tk) + key
    thr = np.uint32(int(float(np.float32(p)) * 4294967296.0))
    keep = hash32(seed, idx) >= thr
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy(np.where(keep, scale, 0.0)).reshape(B, H, Tq, Tk)


# ---------------------------------------------------------------------------------------------- the operation
class Family:
    """Where a kernel family rounds (read off the kernels' code and DESIGN.md, never off their output)."""

    def __init__(self, name, sum_rounded=True, inner=True):
        self.name, self.sum_rounded, self.inner = name, sum_rounded, inner


FAM_LDS = Family("lds")            # attn_vit_kernel, attn_vit_long*, attn_small_kernel: the row sum is a ones-MFMA over the rounded p
FAM_TILED = Family("tiled", sum_rounded=False)      # attn_long_fwd_kernel: the row sum adds the fp32 exponentials
FAM_SCALAR = Family("scalar", inner=False)          # attn_generic_*: fp32 throughout, only the stores round


def _scores(q, k, mask, dh):
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    return s


def _attn(q, k, v, mask, dout, fac, shape, dtype=None, fam=None, out_lse=None, bug=None, compute=torch.float64, forward_only=False):
    """Softmax attention and its closed-form gradients on [B*T, H*dh] operands; dtype/fam None: plain `compute` arithmetic (the
    reference), else float64 with the family's roundings (the model).  out_lse: (out, lse) the backward takes as its inputs instead
    of this forward's.  bug: one of BUGS, a deliberately wrong attention for the negative controls."""
    B, H, Tq, Tk, dh = shape
    rnd = (lambda x: round16(x, dtype)) if dtype is not None else (lambda x: x)
    inner = rnd if (fam is not None and fam.inner) else (lambda x: x)
    qh, kh, vh, gh = (heads(t, B, T, H, dh).to(compute) for t, T in ((q, Tq), (k, Tk), (v, Tk), (dout, Tq)))
    scale = 1.0 / math.sqrt(dh)
    m_eff = mask
    if bug == "mask_shift":                       # the mask read one key late; without a mask, the key count one short
        m_eff = torch.ones(B, Tk, dtype=torch.bool) if mask is None else mask.clone()
        m_eff = torch.roll(m_eff, 1, dims=1)
        if mask is None:
            m_eff[:, 0] = True
            m_eff[:, Tk - 1] = Tk == 1
        else:
            m_eff[:, 0] = mask[:, 0]
    s = _scores(qh, kh, m_eff, dh)
    tile = 64 if Tk > 64 else 16
    if bug == "drop_tile" and Tk > tile:          # the second key tile never runs (the first where there are only two)
        t0 = tile if Tk > 2 * tile else 0
        s = s.clone()
        s[..., t0:t0 + tile] = float("-inf")
    dead = torch.isinf(s).all(-1, keepdim=True)                    # rows with no live key
    mx = torch.where(dead, torch.zeros_like(s[..., :1]), s.max(-1, keepdim=True).values)
    e = torch.exp(s - mx)
    pt = inner(e)
    ssum = (pt if (fam is None or fam.sum_rounded) else e).sum(-1, keepdim=True)
    f = 1.0 if fac is None else fac.to(compute)
    pv = inner(e * f)                                              # dropout acts before the rounding (kernels: pe *= factor; pack2)
    if bug == "skip_rescale" and Tk > tile:
        # the online softmax forgets to rescale what it accumulated before the tile that holds the row maximum: those keys keep the
        # weights they had against the running maximum of their own prefix
        t_of = torch.arange(Tk) // tile
        run = torch.stack([s[..., :(i + 1) * tile].max(-1).values for i in range((Tk + tile - 1) // tile)], -1)     # [.., tiles]
        tmax = s.argmax(-1, keepdim=True) // tile
        before = (t_of[None, None, None, :] < tmax) & (tmax > 0)
        prev = torch.gather(run, -1, (tmax - 1).clamp(min=0))
        pv = torch.where(before & ~torch.isinf(prev), inner(torch.exp(s - prev) * f), pv)
    o = (pv @ vh) / ssum
    lse = (mx + torch.log(ssum)).squeeze(-1)
    nan = torch.full_like(o, float("nan"))
    out = torch.where(dead, nan, rnd(o))
    lse = torch.where(dead.squeeze(-1), torch.full_like(lse, float("nan")), lse)
    if forward_only:
        res = {"out": flat(out), "lse": lse}
        if dtype is None:
            res["floor"] = {"out": EPS32 * float(vh.abs().max())}
        return res
    # backward: P from the saved lse, delta from the stored out
    if out_lse is not None:
        o_b, l_b = heads(out_lse[0], B, Tq, H, dh).to(compute), out_lse[1].to(compute)
    else:
        o_b, l_b = out, (lse.to(F32).to(compute) if dtype is not None else lse)
    o_b = torch.where(dead, torch.zeros_like(o_b), o_b)
    P = torch.where(dead | torch.isinf(s), torch.zeros_like(s), torch.exp(s - torch.where(dead.squeeze(-1), torch.zeros_like(l_b), l_b)[..., None]))
    delta = (gh * o_b).sum(-1, keepdim=True)
    if bug == "delta_wrong_row":
        delta = torch.roll(delta, 1, dims=2)
    dP = gh @ vh.transpose(-1, -2)
    dS = inner(P * (dP * f - delta))
    dv = rnd((inner(P * f)).transpose(-1, -2) @ gh)
    dq = rnd(dS @ kh * scale)
    dk = rnd(dS.transpose(-1, -2) @ qh * (1.0 if bug == "no_scale_dk" else scale))
    res = {"out": flat(out), "lse": lse, "dq": flat(dq), "dk": flat(dk), "dv": flat(dv)}
    if dtype is None and compute is torch.float64:
        # what fp32 accumulation alone may leave where the float64 value cancels exactly (a clip with one live key has dS = 0): one
        # fp32 rounding, 2^-23, of the sums of absolute values behind each output
        ag, av, pf = gh.abs(), vh.abs(), P * f
        nS = P * ((ag @ av.transpose(-1, -2)) * f + (ag * o_b.abs()).sum(-1, keepdim=True))
        res["floor"] = {"out": EPS32 * float((pf @ av).max()), "dv": EPS32 * float((pf.transpose(-1, -2) @ ag).max()),
                        "dq": EPS32 * scale * float((nS @ kh.abs()).max()), "dk": EPS32 * scale * float((nS.transpose(-1, -2) @ qh.abs()).max())}
        dq_rows = flat(dead.expand(B, H, Tq, dh)).any(-1)
        res["dead_q"] = dq_rows                                                       # query rows of clips with no live key
        res["dead_k"] = dq_rows.view(B, Tq)[:, :1].expand(B, Tk).reshape(B * Tk)      # and their key rows
    return res


# "dropout_swapped" is not a switch of _attn: the caller hands the model dropout_fac(..., swap=True)
BUGS = ("drop_tile", "mask_shift", "skip_rescale", "delta_wrong_row", "no_scale_dk", "dropout_swapped")
FWD_BUGS = ("drop_tile", "mask_shift", "skip_rescale")        # change out / lse; the others change gradients only


def attn_ref64(q, k, v, mask, dout, fac=None, *, shape, out_lse=None):
    """out, lse, dq, dk, dv of softmax attention in float64 on the 16-bit operands as the kernel sees them, in the kernels' layout
    ([B*T, H*dh]; lse [B, H, Tq]); the gradients from the closed formulas dV = (P f)^T dO, dS = P (dP f - delta),
    delta = rowsum(dO O), dQ = dS K scale, dK = dS^T Q scale.  mask [B, Tk] bool (True = attend) or None; fac [B, H, Tq, Tk]."""
    r = _attn(q, k, v, mask, dout, fac, shape, out_lse=out_lse)
    return r


def attn_ref32(q, k, v, mask, dout, fac=None, *, shape, out_lse=None):
    """The same formulas in float32 on the CPU: the e32 yardstick of the scalar kernels."""
    return _attn(q, k, v, mask, dout, fac, shape, out_lse=out_lse, compute=F32)


def attn_model16(q, k, v, mask, dout, fac=None, *, shape, dtype, fam=FAM_LDS, bug=None, out_lse=None):
    """Float64 with the roundings the kernels are designed to make: p~ = round16(exp(s - rowmax) f), row sum over round16(exp(..))
    (FAM_TILED: over the unrounded exponentials), out = round16(p~ V / sum), lse = rowmax + log(sum); backward P = exp(s - f32(lse)),
    delta from the rounded out, dV = round16(round16(P f)^T dO), dS = round16(P (dP f - delta)), dq / dk rounded."""
    return _attn(q, k, v, mask, dout, fac, shape, dtype=dtype, fam=fam, bug=bug, out_lse=out_lse)


# ---------------------------------------------------------------------------------------------- the measure
def _rms(x):
    return float(torch.sqrt((x * x).mean())) if x.numel() else 0.0


def live_rows(name, ref):
    """Rows of output `name` that carry a defined value: not those of a clip without a live key (out / lse are NaN there, and what
    the gradients hold is the family's own business: zeros from the tiled and scalar kernels, NaN dq / dk from the in-LDS one)."""
    r = ref[name]
    if name == "lse":
        return ~torch.isnan(r)
    dead = ref.get("dead_k" if name in ("dk", "dv") else "dead_q")
    return ~torch.isnan(r).any(-1) if dead is None else ~dead


def measure(name, got, ref, model):
    """One output: dict with the errors of `got` and of the model against the float64 reference over the live rows, the two ratios,
    and `ok`.  ref / model: the dicts of attn_ref64 / attn_model16.  The yardstick of every output is floored by fp32 accuracy
    (lse: 2^-23 max(1, max|r64|); the others: ref["floor"], see _attn), which only matters where the model's own error is zero."""
    rows = live_rows(name, ref)
    g, r, mo = widen(got)[rows], ref[name][rows], model[name][rows]
    d, e = g - r, mo - r
    res = dict(name=name, rms=_rms(d), max=float(d.abs().max()) if d.numel() else 0.0, e_rms=_rms(e),
               e_max=float(e.abs().max()) if e.numel() else 0.0, ref_rms=_rms(r), ref_max=float(r.abs().max()) if r.numel() else 0.0)
    finite = bool(torch.isfinite(g).all())
    if name == "lse":
        res["floor"] = EPS32 * max(1.0, res["ref_max"])
        res["allow_rms"] = float("inf")
    else:
        res["floor"] = ref.get("floor", {}).get(name, 0.0)
        res["allow_rms"] = R_RMS * max(res["e_rms"], res["floor"])
    res["allow_max"] = R_MAX * max(res["e_max"], res["floor"])
    res["ok"] = finite and res["max"] <= res["allow_max"] and res["rms"] <= res["allow_rms"]
    res["ratio_max"] = res["max"] / max(res["e_max"], res["floor"]) if max(res["e_max"], res["floor"]) > 0 else (0.0 if res["max"] == 0 else float("inf"))
    res["ratio_rms"] = res["rms"] / max(res["e_rms"], res["floor"]) if max(res["e_rms"], res["floor"]) > 0 else (0.0 if res["rms"] == 0 else float("inf"))
    return res


def measure_all(got, r64, model, names=OUTS):
    return [measure(n, got[n], r64, model) for n in names]


def failures(ms):
    return [f"{m['name']}: rms {m['rms']:.3e} (allowed {m['allow_rms']:.3e}), max {m['max']:.3e} (allowed {m['allow_max']:.3e})"
            for m in ms if not m["ok"]]


def vacuity(r64, model, names=OUTS):
    """The cases at which the bound would mean nothing: list of violations of R_MAX E_max <= 0.25 rms(r64), R_RMS E_rms <= 0.1 rms(r64)."""
    bad = []
    for n in names:
        if n == "lse":
            continue
        m = measure(n, model[n], r64, model)
        if R_MAX * m["e_max"] > VAC_MAX * m["ref_rms"] or R_RMS * m["e_rms"] > VAC_RMS * m["ref_rms"]:
            bad.append(f"{n}: E_max {m['e_max']:.3e} E_rms {m['e_rms']:.3e} rms(r64) {m['ref_rms']:.3e}")
    return bad


def scalar_excess(name, got, r64, r32, dtype):
    """The scalar kernels' criterion (train_kernel_refs): <= 1 passes.  lse (fp32): max|got - r64| / max|r64| against bound32(e32);
    16-bit outputs: |got - r64| <= ulp16(r64) + bound32(e32) max|r64| elementwise."""
    rows = live_rows(name, {name: r64})
    g, r, r3 = widen(got)[rows], r64[rows], widen(r32)[rows]
    if not r.numel():
        return 0.0
    e32 = max_rel(r3, r)
    if name == "lse":
        return max_rel(g, r) / bound32(e32)
    allow = ulp16(r, dtype) + bound32(e32) * float(r.abs().max())
    return float(((g - r).abs() / allow).max())


# ---------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


MASKS = ("none", "prefix", "first16", "first64", "first128", "last", "len1", "interior", "dead")


def make_mask(kind, B, Tk, seed=0):
    """[B, Tk] bool key mask (True = attend), or None.  Every kind but prefix / len1 masks key 0 or leaves a whole leading tile dead."""
    if kind == "none":
        return None
    ar = torch.arange(Tk)[None, :]
    g = _gen(977 + seed + Tk)
    lens = torch.randint(max(1, Tk // 2), Tk + 1, (B,), generator=g)
    lens[0] = Tk
    m = (ar < lens[:, None])
    if kind == "prefix":
        return m
    if kind in ("first16", "first64", "first128"):      # the leading keys dead: a first key tile with no live key
        n = int(kind[5:])
        assert Tk > n
        m[:, :n] = False
        m[:, Tk - 1] = True                             # (a prefix shorter than n keys keeps the last key)
        return m
    if kind == "last":                                  # clip 0: only the last key live (every leading tile dead); the others a prefix
        m[0] = False
        m[0, Tk - 1] = True
        return m
    if kind == "len1":                                  # one clip of length 1
        m[B - 1] = False
        m[B - 1, 0] = True
        return m
    if kind == "interior":                              # whole interior 64-key tiles dead, and a dead tail in the other clips
        assert Tk > 200
        m = torch.ones(B, Tk, dtype=torch.bool)
        m[:, 64:192] = False
        m[1:, 200:] = False
        return m
    if kind == "dead":                                  # clip 1 has no live key at all
        assert B >= 2
        m[1] = False
        return m
    raise ValueError(kind)


def random_inputs(shape, dtype, seed, qscale=1.0, mask=None):
    """q, k, v, dout: standard normal values (q times qscale) rounded to `dtype`, in the kernels' layout.  The dout rows of a clip
    with a single live key are divided by Tk: that key's dv row is the plain sum of the clip's Tq dout rows, and unscaled it
    would be Tk times the size of an ordinary row (sqrt(Tq) / Tk) -- half a bf16 ulp of it alone would break the non-vacuity
    condition.  (A batch in which NO clip has more than one live key of many cannot meet it in bf16 at all: no such case is listed.)"""
    B, H, Tq, Tk, dh = shape
    g = _gen(seed)
    D = H * dh
    mk = lambda T: torch.randn(B * T, D, generator=g).to(dtype)
    q = (torch.randn(B * Tq, D, generator=g) * qscale).to(dtype)
    k, v, dout = mk(Tk), mk(Tk), torch.randn(B * Tq, D, generator=g)
    if mask is not None:
        one = (mask.sum(1) == 1)[:, None, None].expand(B, Tq, D).reshape(B * Tq, D)
        dout = torch.where(one, dout / Tk, dout)
    return {"q": q, "k": k, "v": v, "dout": dout.to(dtype)}


def _away_from_zero(x):
    return torch.where(x.abs() < SEL_VMIN, torch.where(x < 0, -SEL_VMIN, SEL_VMIN).to(x.dtype), x)


def selector_inputs(shape, mask, dtype, seed, max_tries=20):
    """Inputs at which query i of every (b, h) attends to the one live key pi(i): k[j] = code(j) in {+1, -1}^dh, q[i] = SEL_A
    code(pi(i)).  pi walks a seeded permutation of the live keys (a bijection where Tq == Tk and nothing is masked; winners in every
    key tile, early and late).  Masked keys carry the code of some query's winner -- they would win were the mask off by one
    position -- and SEL_SENTINEL in V.  V and dO: normal values rounded to `dtype`, |x| >= SEL_VMIN so that half a 16-bit ulp of any
    component stays far above what the losers can add.  The codes are re-drawn until, in float64, the losers of every live query
    hold less than SEL_LOSS in all (the stated condition, winner >= 1 - 2^-20, is asserted by the host test).
    Returns the inputs plus `pi` [B, H, Tq] (-1: the clip has no live key) and `bijection`."""
    B, H, Tq, Tk, dh = shape
    D = H * dh
    for attempt in range(max_tries):
        g = _gen(seed * 131 + attempt)
        code = torch.where(torch.rand(B, H, Tk, dh, generator=g) < 0.5, -1.0, 1.0)
        pi = torch.full((B, H, Tq), -1, dtype=torch.long)
        kc = code.clone()
        for b in range(B):
            live = torch.arange(Tk) if mask is None else torch.nonzero(mask[b]).flatten()
            dead = torch.arange(0) if mask is None else torch.nonzero(~mask[b]).flatten()
            for h in range(H):
                if len(live) == 0:
                    continue
                perm = live[torch.randperm(len(live), generator=g)]
                pi[b, h] = perm[torch.arange(Tq) % len(perm)]
                if len(dead):                       # decoys: a dead key next to a winner takes that winner's code
                    src = torch.where(mask[b][(dead + 1) % Tk], (dead + 1) % Tk, torch.where(mask[b][dead - 1], dead - 1, perm[dead % len(perm)]))
                    kc[b, h, dead] = code[b, h, src]
        qc = SEL_A * torch.gather(kc, 2, pi.clamp(min=0)[..., None].expand(B, H, Tq, dh))
        v = _away_from_zero(torch.randn(B * Tk, D, generator=g)).to(dtype)
        dout = _away_from_zero(torch.randn(B * Tq, D, generator=g)).to(dtype)
        if mask is not None:
            vh = v.view(B, Tk, D)
            vh[~mask] = SEL_SENTINEL
        t = {"q": flat(qc).to(dtype), "k": flat(kc).to(dtype), "v": v, "dout": dout, "pi": pi,
             "bijection": bool(mask is None and Tq == Tk)}
        if selector_loss(t, mask, shape) <= SEL_LOSS:
            return t
    raise AssertionError(f"no selector inputs for {shape} within {max_tries} draws")


def _winner_prob(t, mask, shape):
    B, H, Tq, Tk, dh = shape
    s = _scores(heads(t["q"], B, Tq, H, dh), heads(t["k"], B, Tk, H, dh), mask, dh)
    p = torch.softmax(s, -1)
    pw = torch.gather(p, 3, t["pi"].clamp(min=0)[..., None]).squeeze(-1)
    # 1 - pw without cancellation: the losers' mass
    lose = p.masked_fill(torch.nn.functional.one_hot(t["pi"].clamp(min=0), Tk).bool(), 0.0).sum(-1)
    livec = (t["pi"] >= 0)
    return pw, lose, livec


def selector_loss(t, mask, shape):
    """Largest total probability of the losing keys over the live queries (float64)."""
    _, lose, livec = _winner_prob(t, mask, shape)
    return float(lose[livec].max()) if livec.any() else 0.0


def selector_min_prob(t, mask, shape):
    pw, _, livec = _winner_prob(t, mask, shape)
    return float(pw[livec].min()) if livec.any() else 1.0


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int16) == b.view(torch.int16)).all())


def selector_check(got, t, mask, shape, dtype, fac=None, r64=None, model=None, backward=True, scalar_fwd=False):
    """The exact check on selector inputs; returns the list of violations (empty passes).
      out[i]   = f v[pi(i)] bit for bit (f the dropout factor of the pair: 1, or exactly 2 / 0 at p = 0.5)
      lse[i]   = the winning score SEL_A sqrt(dh) to fp32 accuracy
      dv       = bit for bit dout[i] f at row pi(i) where pi is a bijection; else the model bound (several queries share a key)
      dk, dv of masked keys exactly zero
      |dq|, |dk| below a bound from the losers' probabilities in the reference plus the fp32 error of dP - delta at the winner."""
    B, H, Tq, Tk, dh = shape
    D = H * dh
    bad = []
    pi = t["pi"]
    livec = pi >= 0
    f = None if fac is None else torch.gather(fac, 3, pi.clamp(min=0)[..., None]).squeeze(-1)          # [B, H, Tq]
    vh = heads(t["v"], B, Tk, H, dh)
    want = torch.gather(vh, 2, pi.clamp(min=0)[..., None].expand(B, H, Tq, dh))
    if f is not None:
        want = want * f[..., None]
    want16 = flat(want).to(dtype)
    rows = flat(livec[..., None].expand(B, H, Tq, dh))
    go = got["out"].detach().cpu().to(dtype)          # a model's float64 values are 16-bit values already
    # a dropped winner leaves the losers: at most 2 SEL_LOSS max|v|, not always below the smallest bf16 value
    tiny = 2.0 * SEL_LOSS * float(vh.abs().max() if mask is None else (vh * mask[:, None, :, None]).abs().max())
    same = (go.view(torch.int16) == want16.view(torch.int16)) | ((want16 == 0) & (go.abs() <= tiny))
    if not bool(same[rows].all()):
        n = int((~same & rows).sum())
        r_, c_ = torch.nonzero(~same & rows)[0].tolist()
        bad.append(f"out: {n} elements differ from f v[pi(i)], first at row {r_} col {c_}: got {float(go[r_, c_])} want {float(want16[r_, c_])}")
    if bool(torch.isnan(go.float()[~rows]).logical_not().any()):
        bad.append("out: a row of a clip with no live key is not NaN")
    if got.get("lse") is not None:
        lse = widen(got["lse"])
        win = SEL_A * math.sqrt(dh)
        err = (lse[livec] - win).abs().max().item() if livec.any() else 0.0
        # MFMA families: every q . k product and partial sum is an integer of at most 2048, exact in fp32; what rounds is scale (not
        # a power of two at dh 96), the product with it, log and the final add: R_MAX 2^-23 relative.  The scalar kernel multiplies q
        # by scale first and then adds dh inexact terms one after the other: dh 2^-24 of the sum of their absolute values (= win) more
        tol = (R_MAX * EPS32 + (dh * 2.0 ** -24 if scalar_fwd else 0.0)) * win
        if not err <= tol:
            bad.append(f"lse: {err:.3e} off the winning score {win}")
        if not bool(torch.isnan(lse[~livec]).all()):
            bad.append("lse: a row of a clip with no live key is not NaN")
    if not backward:
        return bad
    gdv, gdk, gdq = widen(got["dv"]), widen(got["dk"]), widen(got["dq"])
    if mask is not None:
        deadk = (~mask)[:, :, None].expand(B, Tk, D).reshape(B * Tk, D)
        inlive = (mask.any(1)[:, None, None]).expand(B, Tk, D).reshape(B * Tk, D)       # dk of a clip with no live key: see live_rows
        for n_, g_, dk_ in (("dk", gdk, deadk & inlive), ("dv", gdv, deadk)):
            if not bool((g_[dk_] == 0).all()):
                bad.append(f"{n_}: a masked key's row is not exactly zero")
    if t["bijection"]:
        gh = heads(t["dout"], B, Tq, H, dh)
        if f is not None:
            gh = gh * f[..., None]
        wdv = torch.zeros(B, H, Tk, dh, dtype=torch.float64)
        wdv.scatter_(2, pi[..., None].expand(B, H, Tq, dh), gh)
        wdv16 = flat(wdv).to(dtype)
        gd = got["dv"].detach().cpu().to(dtype)
        same = (gd.view(torch.int16) == wdv16.view(torch.int16)) | ((wdv16 == 0) & (gd.abs() <= 2.0 * SEL_LOSS * float(gh.abs().max())))
        if not bool(same.all()):
            bad.append(f"dv: {int((~same).sum())} elements differ from f dout[i] at row pi(i)")
    else:
        m = measure("dv", got["dv"], r64, model)
        if not m["ok"]:
            bad += failures([m])
    # dq, dk: |dS_ij| <= P_ij f (|dP_ij| + |delta_i| / f) for the losers; at the winner dP f - delta cancels up to the losers' mass and
    # the fp32 error of the two dot products over dh terms, each at most dh 2^-24 sum_d |dO_d| |v_d| f
    qh, kh, gh = heads(t["q"], B, Tq, H, dh), heads(t["k"], B, Tk, H, dh), heads(t["dout"], B, Tq, H, dh)
    p = torch.softmax(_scores(qh, kh, mask, dh), -1)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)
    fmax = 1.0 if fac is None else float(fac.max())
    vlive = vh if mask is None else vh * mask[:, None, :, None]
    adp = gh.abs() @ vlive.abs().transpose(-1, -2) * fmax                                            # >= |dP_ij| f, [B, H, Tq, Tk]
    onehot = torch.nn.functional.one_hot(pi.clamp(min=0), Tk).bool()
    lose = p.masked_fill(onehot, 0.0)
    amax = adp.max(-1, keepdim=True).values
    bds = lose * 2.0 * amax + onehot * (lose.sum(-1, keepdim=True) * 2.0 * amax + 2.0 * dh * 2.0 ** -24 * amax)
    bds = bds * livec[..., None]
    scale = 1.0 / math.sqrt(dh)
    slack = 1.0 + 2.0 ** -7                                                                          # the 16-bit store
    bq = flat((bds.sum(-1, keepdim=True) * scale * slack).expand(B, H, Tq, dh))
    bk = flat((bds.sum(2)[..., None] * SEL_A * scale * slack).expand(B, H, Tk, dh))
    clipdead = (~livec[:, 0, 0])[:, None]                   # clips with no live key: their gradient rows are not this check's business
    for n_, g_, b_, T_ in (("dq", gdq, bq, Tq), ("dk", gdk, bk, Tk)):
        keep = ~clipdead.expand(B, T_).reshape(B * T_)
        g_, b_ = g_[keep], b_[keep]
        over = g_.abs() > b_
        if bool(over.any()) or not bool(torch.isfinite(g_).all()):
            r_, c_ = torch.nonzero(over | ~torch.isfinite(g_))[0].tolist()
            bad.append(f"{n_}: |{float(g_[r_, c_]):.3e}| above its bound {float(b_[r_, c_]):.3e} at row {r_} col {c_}")
    return bad


# ---------------------------------------------------------------------------------------------- attn_route.h in Python
# A port of attn_vit_route / attn_fwd_route / attn_bwd_route for well-formed calls (no error paths but the 2048 cap), so that every
# case can assert the family it is meant for; the host test runs the C++ header on every case and compares.
LDS_MAX = 160 * 1024


def bwd_lds_bytes(Tq, Tk, RS):
    TQP, TKP = (Tq + 31) & ~31, (Tk + 31) & ~31
    return 2 * (TQP + TKP) * RS + 2 * TQP * 4


def route_vit(N, NQ, F, H, variant=1):
    """(kernel, kAttnVitInsts entry or NC, grid)."""
    if N <= 288:
        vit = 4
        if N == 257 and NQ == N:
            v = variant
            vit = 0 if v == 1 else 1 if v == 2 else 2 if 10 <= v < 20 else 3 if 20 <= v < 30 else 4
        elif N != 257:
            vit = 5 if N == 197 else 6 if N == 50 else 7 if N <= 32 else 8 if N <= 64 else 9 if N <= 128 else 10 if N <= 224 else 11
        persist = vit in (2, 3)
        return ("ATTN_VIT", vit, 512 if persist and F * H >= 512 else F * H)
    nc = 577 if N == 577 else 0
    if NQ == 1:
        return ("ATTN_VIT_LONG_CLS", nc, (F * H + 3) // 4)
    return ("ATTN_VIT_LONG", nc, F * H * ((N + 127) // 128))


def route_fwd(Tq, Tk, dh, out_off=0):
    """Kernel of a vmc_attention_fwd call whose `out` lies out_off bytes past a 16-byte boundary; 'E_SHAPE' past the scalar cap."""
    mfma = dh in (64, 96)
    if mfma and Tk <= 64:
        return "ATTN_SMALL"
    if mfma and out_off % 8 == 0:
        return "ATTN_LONG_FWD"
    return "E_SHAPE" if (Tk > 2048 or Tq > 2048) else "ATTN_GENERIC_FWD"


def route_bwd(Tq, Tk, dh, ldd=0, ldo=0, grad_off=0, out_off=0):
    """(kernel, block, row stride) of a vmc_attention_bwd call; ldd / ldo: the gradient and out row strides (0: a multiple of 4)."""
    if dh in (64, 96) and ldd % 4 == 0 and ldo % 4 == 0:
        if bwd_lds_bytes(Tq, Tk, 2 * dh) <= LDS_MAX:
            rs = 2 * dh + 16 if bwd_lds_bytes(Tq, Tk, 2 * dh + 16) <= LDS_MAX else 2 * dh
            return ("ATTN_BWD_MFMA", 64 * min(4, (Tk + 15) // 16 + (Tq + 15) // 16), rs)
        if grad_off % 8 == 0 and out_off % 16 == 0:
            return ("ATTN_LONG_BWD", 256, 0)
    return ("E_SHAPE", 0, 0) if (Tk > 2048 or Tq > 2048) else ("ATTN_GENERIC_BWD", 64, 0)


# ---------------------------------------------------------------------------------------------- case lists
def case(B, H, Tq, Tk, dh, mask="none", fwd=None, bwd=None, block=None, rs=None, pad=0, out_off=0, grad_off=0, lddq_pad=0, drop=True, tag="",
         qscale=1.0, p25=True):
    """One masked-attention case.  fwd / bwd: the kernels it must take; block / rs: the in-LDS backward's workgroup and row stride;
    pad: every row stride is H*dh + pad with a sentinel in the gap; out_off / grad_off: bytes by which out / dq, dk, dv are moved
    off their 16-byte boundary; lddq_pad: extra elements of lddq only; drop: also runs with dropout (p25 False: p = 0.5 on selector inputs only, see P25_EXCLUDED); qscale: the random q's are
    scaled by it (a flatter softmax where one query row alone would make dk too heavy-tailed for the non-vacuity condition)."""
    return dict(qscale=qscale, p25=p25, B=B, H=H, Tq=Tq, Tk=Tk, dh=dh, mask=mask, fwd=fwd, bwd=bwd, block=block, rs=rs, pad=pad, out_off=out_off,
                grad_off=grad_off, lddq_pad=lddq_pad, drop=drop, tag=tag)


def case_id(c):
    s = f"{c['Tq']}x{c['Tk']}-dh{c['dh']}-{c['mask']}"
    for k in ("pad", "out_off", "grad_off", "lddq_pad"):
        if c[k]:
            s += f"-{k}{c[k]}"
    return s + (f"-{c['tag']}" if c["tag"] else "")


def shape_of(c):
    return (c["B"], c["H"], c["Tq"], c["Tk"], c["dh"])


# P25_EXCLUDED: in these three cases EVERY clip has a single live key.  Then P = 1, dS = dP f - delta, and in float64 delta = dO . (f v)
# cancels dP f exactly: dq = dk = 0, while the kernel (and the model) take delta from the stored round16(f v), which for f = 4/3 is not
# f v: the non-vacuity condition cannot hold at p = 0.25 (it does at p = 0.5, f = 2, which they run on selector inputs).
SM, LF, GF, BM, LB, GB = "ATTN_SMALL", "ATTN_LONG_FWD", "ATTN_GENERIC_FWD", "ATTN_BWD_MFMA", "ATTN_LONG_BWD", "ATTN_GENERIC_BWD"

# attn_small_kernel (Tk <= 64; NT = 2 up to 32 keys, 4 past them); their backward is the in-LDS one with 2, 3 or 4 waves
SMALL_CASES = [
    case(3, 2, 1, 1, 64, "none", SM, BM, 128, 144, p25=False),
    case(3, 2, 16, 15, 64, "prefix", SM, BM, 128, 144),
    case(3, 2, 16, 16, 96, "len1", SM, BM, 128, 208),
    case(3, 2, 17, 17, 64, "first16", SM, BM, 256, 144, p25=False),
    case(3, 2, 16, 32, 96, "first16", SM, BM, 192, 208),
    case(3, 2, 32, 16, 64, "last", SM, BM, 192, 144),
    case(3, 2, 40, 33, 64, "first16", SM, BM, 256, 144),
    case(3, 2, 150, 48, 96, "prefix", SM, BM, 256, 208),
    case(3, 2, 17, 63, 64, "last", SM, BM, 256, 144),
    case(3, 2, 40, 64, 96, "first16", SM, BM, 256, 208),
    case(3, 2, 1, 64, 64, "len1", SM, BM, 256, 144, qscale=0.5),
    case(3, 2, 150, 17, 64, "none", SM, BM, 256, 144),
    case(3, 2, 16, 33, 96, "dead", SM, BM, 256, 208),
    case(2, 2, 40, 48, 64, "prefix", SM, BM, 256, 144, pad=8, tag="strided"),
]

# attn_long_fwd_kernel (Tk > 64); the backward each shape takes is asserted too
LONG_FWD_CASES = [
    case(2, 2, 1, 65, 64, "first64", LF, BM, 256, 144, p25=False),
    case(2, 2, 63, 127, 96, "prefix", LF, BM, 256, 208),
    case(2, 2, 64, 193, 64, "first128", LF, BM, 256, 144),
    case(2, 2, 65, 129, 96, "first64", LF, BM, 256, 208),
    case(2, 2, 130, 193, 64, "last", LF, BM, 256, 144, qscale=0.5),
    case(2, 2, 65, 700, 64, "first128", LF, LB, qscale=0.5),
    case(2, 2, 130, 700, 96, "interior", LF, LB, qscale=0.5),
    case(3, 2, 64, 128, 64, "len1", LF, BM, 256, 144),
    case(2, 2, 63, 129, 64, "none", LF, BM, 256, 144),
    case(2, 2, 65, 128, 96, "prefix", LF, BM, 256, 208, pad=8, tag="strided"),
]

# attn_bwd_mfma_kernel: wave counts, the prologue's remainder loops (more rows than the register prefetch holds), the delta
# remainder (4 TQP > 2 blockDim), padded / unpadded row strides on both sides of the 160 KB limit
BWD_LDS_CASES = [
    case(3, 2, 16, 16, 64, "prefix", SM, BM, 128, 144, tag="2waves"),
    case(3, 2, 9, 5, 96, "none", SM, BM, 128, 208, tag="2waves"),
    case(2, 2, 129, 150, 64, "prefix", LF, BM, 256, 144),
    case(2, 2, 200, 129, 64, "first64", LF, BM, 256, 144),
    case(2, 2, 150, 200, 64, "len1", LF, BM, 256, 144, qscale=0.5),
    case(2, 2, 90, 130, 96, "first64", LF, BM, 256, 208),
    case(2, 2, 130, 90, 96, "prefix", LF, BM, 256, 208),
    case(2, 1, 256, 256, 64, "prefix", LF, BM, 256, 144, tag="padded-edge"),
    case(2, 1, 257, 257, 64, "first64", LF, BM, 256, 128, tag="unpadded"),
    case(2, 1, 288, 288, 64, "none", LF, BM, 256, 128, tag="unpadded-edge"),
    case(2, 1, 192, 192, 96, "first16", LF, BM, 256, 208, tag="padded-edge"),
    case(2, 1, 64, 352, 96, "prefix", LF, BM, 256, 192, tag="unpadded"),
    case(2, 2, 150, 129, 64, "prefix", LF, BM, 256, 144, pad=8, tag="strided"),
]

# the tiled passes of attention_long.hip: first lengths past the LDS limit, ragged and whole tiles, one-row and long shapes
BWD_TILED_CASES = [
    case(2, 1, 289, 289, 64, "first64", LF, LB),
    case(2, 1, 193, 193, 96, "prefix", LF, LB),
    case(1, 2, 1, 2100, 64, "interior", LF, LB, qscale=0.125),
    case(2, 2, 65, 640, 96, "first64", LF, LB, qscale=0.5),
    case(2, 1, 130, 641, 64, "interior", LF, LB, qscale=0.5),
    case(2, 2, 700, 65, 64, "none", LF, LB),
    case(3, 1, 290, 300, 64, "dead", LF, LB),
    case(2, 1, 130, 320, 96, "prefix", LF, LB, pad=8, tag="strided"),
]

# the scalar kernels: other head dims, and head dim 64 / 96 calls whose alignment the MFMA kernels refuse
SCALAR_CASES = [
    case(2, 2, 5, 7, 8, "prefix", GF, GB),
    case(2, 2, 40, 70, 32, "first16", GF, GB),
    case(2, 1, 33, 65, 128, "len1", GF, GB),
    case(2, 2, 40, 70, 64, "prefix", GF, BM, 256, 144, out_off=4, tag="fwd-fallback"),
    case(2, 2, 40, 70, 64, "prefix", LF, GB, lddq_pad=2, tag="bwd-fallback"),
    case(2, 1, 290, 300, 64, "first64", LF, GB, grad_off=4, tag="bwd-fallback-tiled"),
    case(2, 2, 40, 70, 32, "prefix", GF, GB, pad=8, tag="strided"),
]

MASKED_LISTS = {"small": SMALL_CASES, "long_fwd": LONG_FWD_CASES, "bwd_lds": BWD_LDS_CASES, "bwd_tiled": BWD_TILED_CASES,
                "scalar": SCALAR_CASES}
# calls past the scalar cap, each on a fallback: they return an error and write nothing
CAP_CASES = [
    case(1, 1, 2049, 8, 32, "none", "E_SHAPE", "E_SHAPE"),
    case(1, 1, 8, 2049, 64, "none", "E_SHAPE", "E_SHAPE", out_off=4, lddq_pad=2),
    case(1, 1, 2049, 300, 64, "none", LF, "E_SHAPE", grad_off=4),          # a tiled length: only the backward falls back
]

VIT_N = (1, 5, 16, 17, 32, 33, 50, 64, 65, 128, 129, 197, 224, 225, 257, 288)
VIT_INST = {1: 7, 5: 7, 16: 7, 17: 7, 32: 7, 33: 8, 50: 6, 64: 8, 65: 9, 128: 9, 129: 10, 197: 5, 224: 10, 225: 11, 257: 0, 288: 11}
VIT_F, VIT_H = 3, 2
VIT_LONG_N = (289, 320, 577, 640, 641, 1025)
VIT_LONG_F, VIT_LONG_H = 2, 2
CLS_N = (1, 17, 50, 197, 257, 288, 289, 577, 641)
CLS_F, CLS_H = 5, 2                       # five (frame, head) pairs per ... 10 pairs: three workgroups of the streamed kernel, the last ragged
VARIANTS = (2, 9, 10, 13, 20, 23)
VARIANT_INST = {2: 1, 9: 4, 10: 2, 13: 2, 20: 3, 23: 3}
VARIANT_F, VARIANT_H, VARIANT_N = 65, 8, 257      # F H = 520 >= 512: the persistent walks give eight workgroups two heads, the others one


def vit_random(F, N, H, dtype, seed):
    """Packed qkv [F*N, 3 H 64] of standard normal values rounded to `dtype`."""
    return torch.randn(F * N, 3 * H * 64, generator=_gen(seed)).to(dtype)


def vit_split(qkv, H):
    D = H * 64
    return qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]


def vit_selector(F, N, H, dtype, seed):
    """Selector inputs of a ViT call: (packed qkv, the selector dict)."""
    t = selector_inputs((F, H, N, N, 64), None, dtype, seed)
    return torch.cat([t["q"], t["k"], t["v"]], dim=1).contiguous(), t


# ---------------------------------------------------------------------------------------------- one case, prepared
WAYS = ("rand", "sel", "rand-p25", "sel-p50")
DROP_SEED = {"rand-p25": 0x2468ACE, "sel-p50": 0x13579BDF}
DROP_P = {"rand-p25": 0.25, "sel-p50": 0.5}


def ways_of(c):
    """dh = 8 has only 256 codes and a winning score of 45: no selector inputs; it runs the measure alone."""
    w = tuple(x for x in WAYS if c["p25"] or x != "rand-p25") if c["drop"] else WAYS[:2]
    return tuple(x for x in w if c["dh"] > 8 or x.startswith("rand"))


def family_of(c):
    return {SM: FAM_LDS, LF: FAM_TILED, GF: FAM_SCALAR}[c["fwd"]]


def bwd_family_of(c):
    return FAM_SCALAR if c["bwd"] == GB else FAM_LDS


_PREP = {}


def prepare(c, dtype, way):
    """Inputs, mask, dropout factors, float64 reference and model of one (case, dtype, way); computed once and shared (read only)."""
    key = (case_id(c), c["B"], c["H"], dtype, way)
    if key in _PREP:
        return _PREP[key]
    shape = shape_of(c)
    B, H, Tq, Tk, dh = shape
    mask = make_mask(c["mask"], B, Tk)
    seed = Tq * 7 + Tk + dh
    p = DROP_P.get(way, 0.0)
    fac = dropout_fac(p, DROP_SEED[way], B, H, Tq, Tk) if p else None
    sel = way.startswith("sel")
    t = selector_inputs(shape, mask, dtype, seed) if sel else random_inputs(shape, dtype, seed, c["qscale"], mask)
    r64 = attn_ref64(t["q"], t["k"], t["v"], mask, t["dout"], fac, shape=shape)
    ff, fb = family_of(c), bwd_family_of(c)
    args = (t["q"], t["k"], t["v"], mask, t["dout"], fac)
    model = attn_model16(*args, shape=shape, dtype=dtype, fam=ff)
    res = dict(t=t, mask=mask, fac=fac, p=p, seed=DROP_SEED.get(way, 0), r64=r64, model=model, shape=shape, sel=sel)
    if ff is FAM_SCALAR:                       # forward yardstick of the scalar kernel
        res["r32"] = attn_ref32(*args, shape=shape)
    if fb is FAM_SCALAR:
        # the scalar backward is given CPU-made out / lse (the reference's, rounded as the forward stores them), and its reference is
        # the float64 backward of exactly those inputs
        out16 = r64["out"].to(F32).to(dtype)
        lse32 = r64["lse"].to(F32)
        res["bwd_in"] = (out16, lse32)
        res["r64_b"] = attn_ref64(*args, shape=shape, out_lse=(out16, lse32))
        res["r32_b"] = attn_ref32(*args, shape=shape, out_lse=(out16, lse32))
        res["model_b"] = attn_model16(*args, shape=shape, dtype=dtype, fam=FAM_SCALAR, out_lse=(out16, lse32))
    elif ff is FAM_SCALAR:                     # scalar forward, MFMA backward: the backward's own roundings
        res["model_b"] = attn_model16(*args, shape=shape, dtype=dtype, fam=FAM_LDS)
    _PREP[key] = res
    return res


def vit_forward(q, k, v, shape, dtype=None, bug=None, chunk=16):
    """out, lse of a ViT call (no mask, no gradients) in float64 (dtype None) or as the model, a few frames at a time."""
    F, H, NQ, N, dh = shape
    outs, lses = [], []
    for f0 in range(0, F, chunk):
        f1 = min(F, f0 + chunk)
        r = _attn(q[f0 * NQ:f1 * NQ], k[f0 * N:f1 * N], v[f0 * N:f1 * N], None, q[f0 * NQ:f1 * NQ], None, (f1 - f0, H, NQ, N, dh),
                  dtype=dtype, fam=FAM_LDS if dtype is not None else None, bug=bug, forward_only=True)
        outs.append(r["out"])
        lses.append(r["lse"])
    return {"out": torch.cat(outs), "lse": torch.cat(lses)}


def prepare_vit(F, N, H, dtype, way, cls=False):
    """One ViT call: packed qkv [F*N, 3 H 64] (random or selector inputs), and for the class query q_cls [F, H 64] = the rows of
    token 0 and kv [F*N, 2 H 64]; float64 reference and model of the full call (cls: of the class rows only)."""
    key = ("vit", F, N, H, dtype, way, cls)
    if key in _PREP:
        return _PREP[key]
    D = H * 64
    sel = way == "sel"
    t = None
    if sel:
        qkv, t = vit_selector(F, N, H, dtype, 17 + N)
    else:
        qkv = vit_random(F, N, H, dtype, 17 + N)
    q, k, v = vit_split(qkv, H)
    shape = (F, H, N, N, 64)
    if cls:
        q = q.reshape(F, N, D)[:, 0].contiguous()
        shape = (F, H, 1, N, 64)
        if sel:
            t = dict(t, q=q, pi=t["pi"][:, :, :1], bijection=False)
    res = dict(qkv=qkv, q=q, k=k, v=v, t=t, shape=shape, sel=sel, r64=vit_forward(q, k, v, shape), model=vit_forward(q, k, v, shape, dtype))
    _PREP[key] = res
    return res
