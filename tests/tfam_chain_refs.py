"""Float64 reference, designed-rounding model, measure, inputs and case list for the fused TFAM training and eval chains
(tfam_kernels.h, tfam_train.hip, tfam_fused.hip; the vmc_tfam_* entries of include/vmc.h).  No GPU code: torch and numpy on the CPU.
tests/test_tfam_chain_refs_host.py checks everything in here on the CPU (against the oracle and attention_refs, the conditions on
the inputs, the measure on itself and eight mutants); tests/test_gpu_tfam_chain_parity.py compares what the C ABI returns.

``chain_ref64`` is one training step of AMO_CLIP (oracle/tfam.py's graph in train mode) in float64 with the upstream ``dlogits`` given,
on the values the kernels see (16-bit compute copies widened, fp32 biases / LayerNorm parameters / tokens), with the chain's own
dropout masks.  ``chain_model16`` is the same graph with the roundings the chains are designed to make (DESIGN.md §5.3 lists each
with its line in the kernels; none is taken from kernel output).  Two small autograd functions carry them: ``_RoundFwd`` rounds a
forward value to the compute dtype and passes the gradient through (a 16-bit store that a later GEMM reads), ``_RoundGrad`` is the
identity forward and rounds the gradient (a 16-bit gradient buffer: dgrad operand and weight-gradient dY at once).

Measure (DESIGN.md §5.1's, constants imported): per output tensor, E = model16 - r64,
    rms(got - r64) <= R_RMS max(rms(E), floor)   and   max|got - r64| <= R_MAX max(max|E|, floor),    every element finite,
floor = one fp32 rounding (2^-23) of the largest sum of absolute values behind an element of the output.
"""
import functools
import math

import numpy as np
import torch

import attention_refs as AR
from attention_refs import R_MAX, R_RMS, VAC_MAX, VAC_RMS, dropout_fac, hash32
from train_kernel_refs import BF16, EPS32, F16, F32, LN_EPS

F64 = torch.float64
P_DROP, P_MLP = 0.1, 0.3
DROPS = ((0.0, 0.0), (P_DROP, P_MLP))
LAYER_W = ("w_self_in", "w_self_out", "w_cross_in", "w_cross_out", "w_ffn0", "w_ffn3")
LAYER_B = ("b_self_in", "b_self_out", "b_cross_in", "b_cross_out", "b_ffn0", "b_ffn3")
LAYER_LN = ("ln_self_g", "ln_self_b", "ln_cross_g", "ln_cross_b", "ln_ffn_g", "ln_ffn_b")
HEAD_W = ("w_cls1", "w_cls4")
HEAD_F = ("cls_ln_g", "cls_ln_b", "b_cls1", "b_cls4")
# |dlogits| = N(0, 1) times this power of two.  f16: chosen (on the CPU, from model16 alone) so that no stored 16-bit gradient
# exceeds 2^14 and fewer than 1 % of the non-zero elements of any of them are f16-subnormal; the host test asserts both.
DL_SCALE = {BF16: 1.0, F16: 2.0 ** 9}
MUTANTS = ("ln_last_row", "bias_last_tile", "branch_keep", "relu_predrop", "no_residual_grad", "pool_div_T", "dropout_swapped",
           "dmotion_overwrite")


# ---------------------------------------------------------------------------------------------- cases
def _case(name, mode, B, T, Tk, D, H, L, C=8, pool_len=None, seed=0):
    return dict(name=name, mode=mode, B=B, T=T, Tk=Tk if mode == "cross" else 0, D=D, H=H, L=L, C=C, ff=512, pool_len=pool_len, seed=seed)


CASES = [
    _case("a", "cross", 3, 16, 15, 512, 8, 2, seed=11),
    _case("b", "cross", 2, 24, 23, 512, 8, 1, seed=12),
    _case("c", "cross", 2, 40, 39, 512, 8, 1, seed=13),
    _case("d", "cross", 2, 16, 15, 768, 8, 2, seed=14),
    _case("e", "cross", 2, 20, 50, 768, 12, 1, seed=15),
    _case("f", "self", 2, 16, 0, 512, 8, 2, seed=16),
    _case("g1", "feature", 2, 16, 0, 512, 8, 2, seed=17),
    _case("g2", "feature", 2, 16, 0, 768, 8, 1, seed=18),
    _case("h", "cross", 3, 16, 15, 512, 8, 2, pool_len=11, seed=11),
    _case("i", "cross", 1, 7, 6, 512, 8, 1, seed=19),
    _case("j", "cross", 2, 24, 23, 512, 8, 1, C=140, seed=12),
]
BY_NAME = {c["name"]: c for c in CASES}
# the case each mutant of the float32 evaluation must fail (test_tfam_chain_refs_host.py); bias_last_tile needs a token count that
# is no multiple of 16 (case e: 40 token rows, 100 motion rows), dropout_swapped a cross attention with T != Tk
MUTANT_CASE = {"ln_last_row": "a", "bias_last_tile": "e", "branch_keep": "a", "relu_predrop": "a", "no_residual_grad": "b",
               "pool_div_T": "h", "dropout_swapped": "a", "dmotion_overwrite": "a"}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def key_mask(B, T, seed, limit=None):
    """[B, T] bool, ragged: clip b keeps its first T - 1 - (seed + 3 b) mod (T / 2) keys (at least one), never all T."""
    lens = torch.tensor([max(1, T - 1 - (seed + 3 * b) % max(1, T // 2)) for b in range(B)])
    if limit is not None:
        lens = lens.clamp(max=limit)
    return torch.arange(T)[None, :] < lens[:, None]


@functools.lru_cache(maxsize=None)
def make_inputs(name, dtype, drop=(0.0, 0.0)):
    """Everything one step reads: fp32 masters, their 16-bit copies, tokens, masks, seeds, dlogits.  Weights N(0, 1) / sqrt(K), biases
    N(0, 1) / 4, LayerNorm 1 + N / 4 and N / 4, tokens N(0, 1): LayerNorm outputs and pre-activations of order one everywhere.

    The ffn.0 biases are then moved off the ReLU edge (``_relu_gap_bias``), layer by layer, in a float64 forward under the dropout
    setting the inputs are for: ReLU' is the one discontinuity of the step, and a pre-activation whose sign differs between two
    evaluations puts a whole gradient element into a row of dW, far above any rounding error, whichever of the two is right."""
    c = BY_NAME[name]
    B, T, Tk, D, L, C, ff = c["B"], c["T"], c["Tk"], c["D"], c["L"], c["C"], c["ff"]
    g = _gen(7000 + c["seed"])
    rn = lambda *s, scale=1.0, shift=0.0: torch.randn(*s, generator=g) * scale + shift
    p = {}
    for l in range(L):
        pre = f"L{l}."
        for w, (n, k) in zip(LAYER_W, ((3 * D, D), (D, D), (3 * D, D), (D, D), (ff, D), (D, ff))):
            p[pre + w] = rn(n, k, scale=k ** -0.5)
            p[pre + "b" + w[1:]] = rn(n, scale=0.25)
        for ln in ("ln_self", "ln_cross", "ln_ffn"):
            p[pre + ln + "_g"] = rn(D, scale=0.25, shift=1.0)
            p[pre + ln + "_b"] = rn(D, scale=0.25)
    p["head.cls_ln_g"], p["head.cls_ln_b"] = rn(D, scale=0.25, shift=1.0), rn(D, scale=0.25)
    p["head.w_cls1"], p["head.b_cls1"] = rn(D // 2, D, scale=D ** -0.5), rn(D // 2, scale=0.25)
    p["head.w_cls4"], p["head.b_cls4"] = rn(C, D // 2, scale=(D // 2) ** -0.5), rn(C, scale=0.25)
    p["proj.w_proj"], p["proj.b_proj"] = rn(D, 2 * D, scale=(2 * D) ** -0.5), rn(D, scale=0.25)
    w16 = {k: v.to(dtype) for k, v in p.items() if k.split(".")[1].startswith("w_")}
    inp = dict(case=c, dtype=dtype, p32=p, w16=w16)
    inp["x"] = rn(B * T, D)
    inp["motion"] = rn(B * Tk, D) if Tk else None
    inp["xcat"] = rn(B * T, 2 * D)
    inp["mask"] = key_mask(B, T, c["seed"], c["pool_len"])
    inp["mask_kv"] = key_mask(B, Tk, c["seed"] + 1) if Tk else None
    inp["dlogits"] = rn(B, C) * DL_SCALE[dtype]
    inp["seeds"] = [int(v) for v in torch.randint(1, 2 ** 62, (7 * L + 1,), generator=g)]
    inp["relu_margin"] = {}
    with torch.no_grad():
        run_chain(inp, Policy(), drop, calibrate=True)
    return inp


def _relu_gap_bias(z0, b0):
    """Per column j of the bias-free pre-activations z0 [M, N]: b0[j] shifted so that zero lies in the middle of the widest gap
    between two neighbouring values of the column's middle half (between its quartiles: both signs stay populated).
    Returns (bias as fp32 values, the smallest |z| that results)."""
    M = z0.shape[0]
    srt = torch.sort(z0 + b0, 0).values                      # [M, N]
    if M < 4:
        lo, hi = 0, M - 1
    else:
        lo, hi = M // 4, M - 1 - M // 4
    gaps = srt[lo + 1:hi + 1] - srt[lo:hi]                   # [hi - lo, N]
    i = gaps.argmax(0)
    mid = 0.5 * (torch.gather(srt, 0, (lo + i)[None])[0] + torch.gather(srt, 0, (lo + i + 1)[None])[0])
    b = (b0 - mid).to(F32)
    return b, float((z0 + b.to(z0.dtype)).abs().min())


# ---------------------------------------------------------------------------------------------- dropout masks on the CPU
def fac2d(p, seed, M, N):
    """vmc_dropout's factor on an [M, N] tensor (flat index row N + col): 0 or the fp32 value 1 / (1 - p); None for p = 0."""
    if p <= 0.0:
        return None
    idx = np.arange(M * N, dtype=np.uint64)
    thr = np.uint32(int(float(np.float32(p)) * 4294967296.0))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy(np.where(hash32(seed, idx) >= thr, scale, 0.0)).reshape(M, N)


def inv_keep(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0.0 else 1.0


# ---------------------------------------------------------------------------------------------- the rounding policy
class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        return x.to(F32).to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pol, tag):
        ctx.pol, ctx.tag = pol, tag
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        r = g.to(F32).to(ctx.pol.dtype).to(g.dtype)
        ctx.pol.note(ctx.tag, r)
        return r, None, None


class Policy:
    """dtype None: the reference (nothing rounds).  compute: float64, or float32 for the measure's self-test.  mutant: one of MUTANTS."""

    def __init__(self, dtype=None, compute=F64, mutant=None, folded=False):
        self.dtype, self.compute, self.mutant, self.folded = dtype, compute, mutant, folded
        self.stored = {}          # tag -> (max |g|, subnormal share of the non-zero elements) of every stored 16-bit gradient

    def r(self, x):
        return x if self.dtype is None else _RoundFwd.apply(x, self.dtype)

    def g(self, x, tag):
        return x if self.dtype is None else _RoundGrad.apply(x, self, tag)

    def note(self, tag, r):
        a = r.abs()
        nz = a[a > 0]
        sub = float((nz < 2.0 ** -14).double().mean()) if nz.numel() else 0.0
        self.stored[tag] = (float(a.max()) if a.numel() else 0.0, sub)


class _AttnFn(torch.autograd.Function):
    """tf_pro_attn forward and vmc_attention_bwd (attn_bwd_mfma_kernel: what attn_route.h picks for T, Tk <= 64 at head dim 64 / 96)
    through attention_refs' model: the in-LDS family's roundings (FAM_LDS)."""

    @staticmethod
    def forward(ctx, q, k, v, pol, mask, fac, shape, tag):
        # attention_refs' model rounds through float64, so it is evaluated in float64 under either compute type: the float32
        # self-test has float32 arithmetic everywhere but inside the two attentions
        B, H, Tq, Tk, dh = shape
        zero = torch.zeros(B * Tq, H * dh, dtype=F64)
        r = AR._attn(q, k, v, mask, zero, fac, shape, dtype=pol.dtype, fam=AR.FAM_LDS, forward_only=True)
        ctx.save_for_backward(q, k, v, r["out"], r["lse"])
        ctx.args = (pol, mask, fac, shape, tag)
        return r["out"].to(pol.compute)

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, lse = ctx.saved_tensors
        pol, mask, fac, shape, tag = ctx.args
        r = AR._attn(q, k, v, mask, g, fac, shape, dtype=pol.dtype, fam=AR.FAM_LDS, out_lse=(out, lse.to(F32)))
        for n in ("dq", "dk", "dv"):
            pol.note(f"{tag}.{n}", r[n])
        return r["dq"].to(g.dtype), r["dk"].to(g.dtype), r["dv"].to(g.dtype), None, None, None, None, None


def _attn_plain(q, k, v, mask, fac, shape):
    """Softmax attention under autograd on [B*T, H*dh] operands (the reference; dropout on the normalised probabilities)."""
    B, H, Tq, Tk, dh = shape
    qh, kh, vh = (t.reshape(B, n, H, dh).transpose(1, 2) for t, n in ((q, Tq), (k, Tk), (v, Tk)))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    if fac is not None:
        p = p * fac.to(p.dtype)
    return (p @ vh).transpose(1, 2).reshape(B * Tq, H * dh)


class _FfnAct(torch.autograd.Function):
    """h = round16(drop(relu(z))) (tf_epilogue_train, EPI_ACT16); backward g (h > 0 ? gate_scale : 0) from the SAVED h."""

    @staticmethod
    def forward(ctx, z, fac, pol, inv):
        a = torch.relu(z)
        h = a if fac is None else a * fac.to(z.dtype)
        h = h.to(F32).to(pol.dtype).to(z.dtype)
        ctx.save_for_backward(a if pol.mutant == "relu_predrop" else h)
        ctx.inv = inv
        return h

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        return g * (h > 0).to(g.dtype) * ctx.inv, None, None, None


class _DropNoMask(torch.autograd.Function):
    """mutant branch_keep: the forward's dropout, a backward that scales by 1 / (1 - p) without the keep mask."""

    @staticmethod
    def forward(ctx, x, fac, inv):
        ctx.inv = inv
        return x * fac.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.inv, None, None


class _ScaleFwd(torch.autograd.Function):
    """x * s in the forward, the gradient passed through unscaled (mutant pool_div_T)."""

    @staticmethod
    def forward(ctx, x, s):
        return x * s

    @staticmethod
    def backward(ctx, g):
        return g, None


class _LinMaster(torch.autograd.Function):
    """The head's linears: forward on the 16-bit copy, dgrad on the fp32 master (tr_head_bwd1 / 2), dW = dY^T X."""

    @staticmethod
    def forward(ctx, x, w16, w32):
        ctx.save_for_backward(x, w32)
        return x @ w16.t()

    @staticmethod
    def backward(ctx, g):
        x, w32 = ctx.saved_tensors
        return g @ w32, g.t() @ x, None


def _gelu_grad(a):
    return 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


class _GeluHead(torch.autograd.Function):
    """g = gelu(a) on the fp32 pre-activation; the backward evaluates gelu' at the STORED 16-bit a (tr_head_bwd1_kernel reads a16)."""

    @staticmethod
    def forward(ctx, a, dtype):
        ctx.save_for_backward(a.to(F32).to(dtype).to(a.dtype))
        return torch.nn.functional.gelu(a)

    @staticmethod
    def backward(ctx, g):
        (a16,) = ctx.saved_tensors
        return g * _gelu_grad(a16), None


# ---------------------------------------------------------------------------------------------- the chain
def _layer_norm(y, gam, bet, pol, rows_off=None):
    """LayerNorm over the last axis.  rows_off: rows whose contribution to the gamma / beta gradients is cut (mutant ln_last_row)."""
    mean = y.mean(-1, keepdim=True)
    yc = y - mean
    xhat = yc / torch.sqrt((yc * yc).mean(-1, keepdim=True) + LN_EPS)
    G, Bt = gam.expand_as(y), bet.expand_as(y)
    if rows_off is not None:
        keep = torch.ones(y.shape[0], 1, dtype=torch.bool)
        keep[rows_off] = False
        G, Bt = torch.where(keep, G, G.detach()), torch.where(keep, Bt, Bt.detach())
    return xhat * G + Bt


def run_chain(inp, pol, drop, calibrate=False):
    """One step.  Returns {"logits", "pool_grad", "dX" | "dXcat", "dMotion", "g.<param>": float64 tensors} and, for the reference
    (pol.dtype None), "floor": {name: 2^-23 of the largest sum of absolute values behind an element}."""
    c, dtype = inp["case"], inp["dtype"]
    B, T, Tk, D, H, L, C, ff = c["B"], c["T"], c["Tk"], c["D"], c["H"], c["L"], c["C"], c["ff"]
    cd, mode, mut = pol.compute, c["mode"], pol.mutant
    p_drop, p_mlp = drop
    dh, M, Mk = D // H, B * T, B * Tk
    seeds = inp["seeds"]
    leaves, absrec, neg_share = {}, [], []

    def leaf(name):
        if name not in leaves:
            src = inp["w16"][name] if name in inp["w16"] else inp["p32"][name]
            leaves[name] = src.to(F64).to(cd).clone().requires_grad_(True)
        return leaves[name]

    def master(name):
        return inp["p32"][name].to(F64).to(cd)

    def lin(x, wname, bname, rows=None, tok_rows=True):
        """x W^T + b on a row window of a packed weight; records |dY|, |X| for the floors of the reference."""
        W, b = leaf(wname), leaf(bname)
        if rows is not None:
            W, b = W[rows[0]:rows[1]], b[rows[0]:rows[1]]
        bb = b.expand(x.shape[0], -1)
        if mut == "bias_last_tile" and tok_rows and x.shape[0] % 16:
            live = (torch.arange(x.shape[0]) < 16 * (x.shape[0] // 16))[:, None]
            bb = torch.where(live, bb, bb.detach())
        y = x @ W.t() + bb
        if pol.dtype is None and y.requires_grad:
            y.register_hook(lambda g, x=x.detach(), W=W.detach(), k=(wname, bname, rows): absrec.append((k, g.abs(), x.abs(), W.abs())))
        return y

    def attn(q, k, v, mask, fac, shape, tag):
        if pol.dtype is None:
            return _attn_plain(q, k, v, mask, fac, shape)
        return _AttnFn.apply(q, k, v, pol, mask, fac, shape, tag)

    def branch(br, fac, inv, no_mask=False):
        if fac is None:
            return br
        return _DropNoMask.apply(br, fac, inv) if no_mask else br * fac.to(cd)

    inv = inv_keep(p_drop)
    x_leaf = mo_leaf = None
    if mode == "feature":
        x_leaf = inp["xcat"].to(F64).to(cd).clone().requires_grad_(True)
        xin = pol.g(lin(pol.r(x_leaf), "proj.w_proj", "proj.b_proj"), "d0_16")      # F0; L8's y16out on the way back
    else:
        x_leaf = inp["x"].to(F64).to(cd).clone().requires_grad_(True)
        xin = x_leaf
    if mode == "cross":
        mo_leaf = inp["motion"].to(F64).to(cd).clone().requires_grad_(True)
    mask, mask_kv = inp["mask"], inp["mask_kv"]
    last = torch.tensor([M - 1]) if mut == "ln_last_row" else None
    for l in range(L):
        pre, s = f"L{l}.", seeds[7 * l:7 * l + 7]
        # F1 / F2: self attention
        qkv = pol.r(lin(pol.r(xin), pre + "w_self_in", pre + "b_self_in"))
        fac = dropout_fac(p_drop, s[0], B, H, T, T) if p_drop > 0 else None
        o = pol.g(attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], mask, fac, (B, H, T, T, dh), pre + "self"), pre + "dos16")
        br = pol.g(lin(o, pre + "w_self_out", pre + "b_self_out"), pre + "d1_16")
        y = xin + branch(br, fac2d(p_drop, s[1], M, D), inv, no_mask=(mut == "branch_keep" and l == 0))
        xc = _layer_norm(y, leaf(pre + "ln_self_g"), leaf(pre + "ln_self_b"), pol, last)
        if mode == "cross":
            # F3 / F4: cross attention; K|V of the raw motion tokens, once per layer
            qc = pol.r(lin(pol.r(xc), pre + "w_cross_in", pre + "b_cross_in", rows=(0, D)))
            mo = mo_leaf.detach() if (mut == "dmotion_overwrite" and l > 0) else mo_leaf
            kv = pol.r(lin(pol.r(mo), pre + "w_cross_in", pre + "b_cross_in", rows=(D, 3 * D)))
            fac = dropout_fac(p_drop, s[2], B, H, T, Tk, swap=(mut == "dropout_swapped")) if p_drop > 0 else None
            o = pol.g(attn(qc, kv[:, :D], kv[:, D:], mask_kv, fac, (B, H, T, Tk, dh), pre + "cross"), pre + "doc16")
            br = pol.g(lin(o, pre + "w_cross_out", pre + "b_cross_out"), pre + "d2_16")
            y = xc + branch(br, fac2d(p_drop, s[3], M, D), inv)
            xc = _layer_norm(y, leaf(pre + "ln_cross_g"), leaf(pre + "ln_cross_b"), pol, last)
        # F5 / F6: FFN
        if calibrate:      # make_inputs only: move this layer's ffn.0 bias off the ReLU edge before anything reads it
            b, margin = _relu_gap_bias(xc @ leaf(pre + "w_ffn0").t(), inp["p32"][pre + "b_ffn0"].to(cd))
            inp["p32"][pre + "b_ffn0"] = b
            inp["relu_margin"][l] = margin
        z = pol.g(lin(pol.r(xc), pre + "w_ffn0", pre + "b_ffn0"), pre + "dh16")
        f4 = fac2d(p_drop, s[4], M, ff)
        if pol.dtype is None:
            h = torch.relu(z) if f4 is None else torch.relu(z) * f4.to(cd)
        else:
            h = _FfnAct.apply(z, f4, pol, inv)
        neg_share.append(float((z.detach() < 0).double().mean()))
        br = pol.g(lin(h, pre + "w_ffn3", pre + "b_ffn3"), pre + "d3_16")
        f56 = None
        if p_drop > 0:
            f56 = fac2d(p_drop, s[5], M, D) * fac2d(p_drop, s[6], M, D)
        res = xc.detach() if (mut == "no_residual_grad" and l == L - 1) else xc      # L2's epilogue without dy3
        y = res + branch(br, f56, inv * inv)
        xin = _layer_norm(y, leaf(pre + "ln_ffn_g"), leaf(pre + "ln_ffn_b"), pol, last)
    if calibrate:
        return None
    xin.retain_grad()
    # head: pool over the first n rows, LayerNorm, Linear + GELU + dropout, Linear
    n = T if c["pool_len"] is None else c["pool_len"]
    pooled = xin.reshape(B, T, D)[:, :n].sum(1) / n
    if mut == "pool_div_T":
        # tf_pool_kernel dividing by T while tr_head_bwd3_kernel keeps 1 / n.  (Both dividing by T is no defect the step can show:
        # classifier.0's LayerNorm cancels a common factor of its input, forward and backward.)
        pooled = _ScaleFwd.apply(pooled, n / T)
    p16 = pol.r(_layer_norm(pooled, leaf("head.cls_ln_g"), leaf("head.cls_ln_b"), pol))
    fm = fac2d(p_mlp, seeds[7 * L], B, D // 2)
    if pol.dtype is None:
        a = lin(p16, "head.w_cls1", "head.b_cls1", tok_rows=False)
        gl = torch.nn.functional.gelu(a)
        gl = gl if fm is None else gl * fm.to(cd)
        logits = lin(gl, "head.w_cls4", "head.b_cls4", tok_rows=False)
    else:
        a = _LinMaster.apply(p16, leaf("head.w_cls1"), master("head.w_cls1")) + leaf("head.b_cls1")
        gl = _GeluHead.apply(a, pol.dtype)
        gl = pol.r(gl if fm is None else gl * fm.to(cd))
        logits = _LinMaster.apply(gl, leaf("head.w_cls4"), master("head.w_cls4")) + leaf("head.b_cls4")
    dl = inp["dlogits"].to(F64).to(cd)
    logits.backward(dl)
    out = {"logits": logits.detach().to(F64), "pool_grad": xin.grad.to(F64), "relu_negative_share": neg_share}
    out["dXcat" if mode == "feature" else "dX"] = x_leaf.grad.to(F64)
    if mode == "cross":
        out["dMotion"] = mo_leaf.grad.to(F64)
    for name, t in leaves.items():
        if mode != "cross" and ("cross" in name):
            continue
        out["g." + name] = (t.grad if t.grad is not None else torch.zeros_like(t)).to(F64)
    if pol.dtype is None:
        out["floor"] = _floors(out, absrec, logits, dl)
    return out


def _floors(out, absrec, logits, dl):
    """2^-23 of the largest sum of absolute values behind an element, per output (what fp32 accumulation alone may leave where the
    model's error is exactly zero: classifier.4's bias gradient is a plain sum of dlogits in both references)."""
    fl = {}
    acc = {}
    for (wname, bname, rows), g, x, W in absrec:
        gw, gb = g.t() @ x, g.sum(0)
        acc[wname] = max(acc.get(wname, 0.0), float(gw.max()))
        acc[bname] = max(acc.get(bname, 0.0), float(gb.max()))
        acc["dgrad:" + wname + str(rows)] = float((g @ W).max())
    for k, v in acc.items():
        if not k.startswith("dgrad:"):
            fl["g." + k] = EPS32 * v
    for k, t in out.items():
        if isinstance(t, torch.Tensor) and k not in fl:      # LayerNorm parameters, token gradients, pool gradient, logits
            fl[k] = EPS32 * float(t.abs().max())
    for k, tag in (("dX", "L0.w_self_inNone"), ("dXcat", "proj.w_projNone")):
        if k in out:
            fl[k] = max(fl[k], EPS32 * acc.get("dgrad:" + tag, 0.0))
    return fl


@functools.lru_cache(maxsize=None)
def chain_ref64(name, dtype, drop):
    return run_chain(make_inputs(name, dtype, drop), Policy(), drop)


@functools.lru_cache(maxsize=None)
def chain_model16(name, dtype, drop):
    pol = Policy(dtype)
    out = run_chain(make_inputs(name, dtype, drop), pol, drop)
    out["stored"] = dict(pol.stored)
    return out


def chain_eval32(name, dtype, drop, mutant=None):
    """model16 evaluated in float32 with round-to-nearest stores: what a faithful kernel computes (the measure's self-test), or one
    of the MUTANTS of it."""
    return run_chain(make_inputs(name, dtype, drop), Policy(dtype, compute=F32, mutant=mutant), drop)


def tensor_names(out):
    return [k for k, v in out.items() if isinstance(v, torch.Tensor)]


# ---------------------------------------------------------------------------------------------- the measure
def _rms(x):
    return float(torch.sqrt((x * x).mean())) if x.numel() else 0.0


def measure(name, got, r64, m16):
    """One output tensor: the errors of `got` and of the model against the reference, both ratios, the distance to the model in
    units of rms(E) (reported, not asserted) and `ok`.  A tensor whose model error misses the max condition of `vacuity` (bf16
    only; the host test asserts that, and that they are at most a quarter of a case's tensors) is held to the rms rule alone."""
    g, r, mo = got.detach().to("cpu").to(F64).reshape(-1), r64[name].reshape(-1), m16[name].reshape(-1)
    d, e = g - r, mo - r
    floor = r64["floor"].get(name, 0.0)
    e_rms, e_max = max(_rms(e), floor), max(float(e.abs().max()), floor)
    finite = bool(torch.isfinite(g).all())
    res = dict(name=name, rms=_rms(d), max=float(d.abs().max()), e_rms=e_rms, e_max=e_max, ref_rms=_rms(r), floor=floor, finite=finite)
    res["ratio_rms"] = res["rms"] / e_rms if e_rms > 0 else (0.0 if res["rms"] == 0 else float("inf"))
    res["ratio_max"] = res["max"] / e_max if e_max > 0 else (0.0 if res["max"] == 0 else float("inf"))
    res["model_dist"] = _rms(g - mo) / e_rms if e_rms > 0 else 0.0
    res["max_exempt"] = R_MAX * e_max > VAC_MAX * res["ref_rms"]
    res["ok"] = finite and res["rms"] <= R_RMS * e_rms and (res["max_exempt"] or res["max"] <= R_MAX * e_max)
    return res


def measure_all(got, r64, m16):
    return [measure(n, got[n], r64, m16) for n in tensor_names(r64) if n in got]


def failures(ms):
    return [f"{m['name']}: rms ratio {m['ratio_rms']:.2f} (<= {R_RMS}), max ratio {m['ratio_max']:.2f} (<= {R_MAX}), finite {m['finite']}"
            for m in ms if not m["ok"]]


def vacuity(r64, m16):
    """(tensors that miss 2 rms(E) <= 0.1 rms(r64), tensors that miss 4 max|E| <= 0.25 rms(r64))."""
    bad_rms, bad_max = [], []
    for n in tensor_names(r64):
        m = measure(n, m16[n], r64, m16)
        if R_RMS * m["e_rms"] > VAC_RMS * m["ref_rms"]:
            bad_rms.append(n)
        if m["max_exempt"]:
            bad_max.append(n)
    return bad_rms, bad_max


# ---------------------------------------------------------------------------------------------- the eval chain (tfam_fused.hip)
EVAL_CASES = ("a", "c", "d", "f", "h")


def fold_ref(W, bias, gamma, beta, compute=F64):
    """vmc_tfam_fold_layernorm in `compute`: (W . gamma [rows, cols], bias + W beta [rows]) on the fp32 values given."""
    W, bias, gamma, beta = (t.to(F64).to(compute) for t in (W, bias, gamma, beta))
    return W * gamma, bias + W @ beta


def run_eval(inp, dtype=None):
    """Logits of the eval chain, float64.  dtype None: the reference -- the oracle's eval forward on the 16-bit weight copies, with the
    exact W . gamma and b + W beta where the pack folds a LayerNorm.  dtype: the `folded` model -- round16(W . gamma) as
    vmc_tfam_fold_layernorm stores it, a prologue that only standardises (tf_pro_ln without TR: round16 of (y - mean) rstd is the A
    operand, LN(y) in fp32 the residual), 16-bit q / k / v / h / attention outputs / pooled and classifier rows, no dropout."""
    c = inp["case"]
    B, T, Tk, D, H, L = c["B"], c["T"], c["Tk"], c["D"], c["H"], c["L"]
    dh, cross = D // H, c["mode"] == "cross"
    rnd = (lambda t: AR.round16(t, dtype)) if dtype is not None else (lambda t: t)
    P = lambda n: inp["p32"][n].to(F64)
    W = lambda n: inp["w16"][n].to(F64)

    def std(y):
        yc = y - y.mean(-1, keepdim=True)
        return yc / torch.sqrt((yc * yc).mean(-1, keepdim=True) + LN_EPS)

    def folded(z, wname, bname, gname, rows=None):
        """[standardised rows] x [the linear `wname` with LayerNorm `gname` folded in]."""
        w32, b = P(wname), P(bname)
        if rows is not None:
            w32, b = w32[rows[0]:rows[1]], b[rows[0]:rows[1]]
        wf, bf = fold_ref(w32, b, P(gname + "_g"), P(gname + "_b"))
        return rnd(z) @ rnd(wf).t() + bf

    def attn(q, k, v, mask, shape):
        if dtype is None:
            return _attn_plain(q, k, v, mask, None, shape)
        zero = torch.zeros(q.shape[0], D, dtype=F64)
        return AR._attn(q, k, v, mask, zero, None, shape, dtype=dtype, fam=AR.FAM_LDS, forward_only=True)["out"]

    x = inp["x"].to(F64)
    y = None
    for l in range(L):
        pre = f"L{l}."
        if l == 0:
            xin, qkv = x, rnd(rnd(x) @ W(pre + "w_self_in").t() + P(pre + "b_self_in"))
        else:
            z = std(y)
            xin = z * P(f"L{l - 1}.ln_ffn_g") + P(f"L{l - 1}.ln_ffn_b")
            qkv = rnd(folded(z, pre + "w_self_in", pre + "b_self_in", f"L{l - 1}.ln_ffn"))
        o = attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], inp["mask"], (B, H, T, T, dh))
        y = xin + o @ W(pre + "w_self_out").t() + P(pre + "b_self_out")
        z, ln = std(y), "ln_self"
        if cross:
            xb = z * P(pre + "ln_self_g") + P(pre + "ln_self_b")
            q = rnd(folded(z, pre + "w_cross_in", pre + "b_cross_in", pre + "ln_self", rows=(0, D)))
            kv = rnd(rnd(inp["motion"].to(F64)) @ W(pre + "w_cross_in")[D:].t() + P(pre + "b_cross_in")[D:])
            o = attn(q, kv[:, :D], kv[:, D:], inp["mask_kv"], (B, H, T, Tk, dh))
            y = xb + o @ W(pre + "w_cross_out").t() + P(pre + "b_cross_out")
            z, ln = std(y), "ln_cross"
        xa = z * P(pre + ln + "_g") + P(pre + ln + "_b")
        h = rnd(torch.relu(folded(z, pre + "w_ffn0", pre + "b_ffn0", pre + ln)))
        y = xa + h @ W(pre + "w_ffn3").t() + P(pre + "b_ffn3")
    xo = std(y) * P(f"L{L - 1}.ln_ffn_g") + P(f"L{L - 1}.ln_ffn_b")
    n = T if c["pool_len"] is None else c["pool_len"]
    pooled = xo.reshape(B, T, D)[:, :n].mean(1)
    p16 = rnd(std(pooled) * P("head.cls_ln_g") + P("head.cls_ln_b"))
    g = rnd(torch.nn.functional.gelu(p16 @ W("head.w_cls1").t() + P("head.b_cls1")))
    logits = g @ W("head.w_cls4").t() + P("head.b_cls4")
    out = {"logits": logits}
    if dtype is None:
        out["floor"] = {"logits": EPS32 * float((g.abs() @ W("head.w_cls4").abs().t() + P("head.b_cls4").abs()).max())}
    return out
