"""GPU: the fused TFAM chains through the C ABI (include/vmc.h, vmc_tfam_*) against tests/tfam_chain_refs.py: a float64 training step
and a float64 model of it that rounds where the chains round.  Whole one- and two-layer chains, every output the ABI
returns: logits, the pool gradient at its exported offset, every parameter gradient, dX / dMotion / dXcat at theirs.  No intermediate
buffer is read.

Every call gets a workspace of exactly the advertised size whose bytes are all 0xFF (NaN in every type the chains store) with a
guard behind it; logits and every gradient destination are pre-filled with a sentinel and followed by guard elements that must
survive bit for bit, and every element in front of them must have been written.

VMC_TFAM_PARITY_JSON=<path>: one line per checked output (case, dtype, dropout, tensor, both ratios, the distance to the model)."""
import ctypes
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_refs as G                            # noqa: E402
import tfam_chain_refs as R                      # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16, F32      # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (BF16, F16)
CFG_ID = lambda v: v if isinstance(v, str) else (DT_NAME[v] if isinstance(v, torch.dtype) else f"p{v[0]}")
CONFIGS = [(c["name"], dt, drop) for c in R.CASES for dt in DTYPES for drop in R.DROPS]
SENT = 0x7149F2CA        # the bits of a float near 1e30: no gradient of these cases comes near it
GUARD = 64               # sentinel elements behind every output
WS_GUARD = 256           # bytes behind the workspace
WANT_DX, WANT_DMOTION = 1, 2


def _lib():
    from vimo_clip_amd import _lib as L
    return L


def _record(case, dtype, drop, route, m):
    path = os.environ.get("VMC_TFAM_PARITY_JSON")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=case, dtype=DT_NAME[dtype], p_drop=drop[0], route=route, tensor=m["name"], ratio_rms=round(m["ratio_rms"], 4),
                                    ratio_max=round(m["ratio_max"], 4), model_dist=round(m["model_dist"], 4), max_exempt=m["max_exempt"], ok=m["ok"])) + "\n")


class Out:
    """An fp32 output of n elements with GUARD sentinel elements behind it."""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.n = int(torch.tensor(self.shape).prod())
        self.buf = torch.full((self.n + GUARD,), SENT, dtype=torch.int32, device="cuda")

    def ptr(self):
        return self.buf.data_ptr()

    def value(self):
        """The output on the CPU; asserts that the guard survived and that every element was written."""
        b = self.buf.cpu()
        assert bool((b[self.n:] == SENT).all()), "guard elements behind an output were overwritten"
        assert bool((b[:self.n] != SENT).all()), "an output element was not written"
        return b[:self.n].view(F32).reshape(self.shape).clone()


class Step:
    """Device buffers and parameter structs of one (case, dtype, dropout) and the calls on them."""

    def __init__(self, name, dtype, drop, inp=None):
        from vimo_clip_amd import tfam_train as TT
        self.TT, self.L_ = TT, _lib()
        self.lib = self.L_.lib
        self.inp = inp if inp is not None else R.make_inputs(name, dtype, drop)
        c = self.c = self.inp["case"]
        self.name, self.dtype, self.drop = name, dtype, drop
        self.cross, self.proj = c["mode"] == "cross", c["mode"] == "feature"
        self.dims = (c["B"], c["T"], c["Tk"], c["D"], c["H"], c["ff"], c["L"], c["C"], int(self.cross))
        self.pdims = self.dims[:2] + self.dims[3:8]
        self.keep = []
        dev = lambda t: self._keep(t.contiguous().cuda())
        p32, w16 = self.inp["p32"], self.inp["w16"]
        self.f = {k: dev(v) for k, v in p32.items()}                     # fp32 masters, biases, LayerNorm parameters
        self.w = {k: dev(v) for k, v in w16.items()}                     # 16-bit [N, K]
        self.wt = {k: dev(v.t()) for k, v in w16.items()}                # 16-bit [K, N]
        self.x = dev(self.inp["xcat"] if self.proj else self.inp["x"])
        self.motion = dev(self.inp["motion"]) if self.cross else None
        self.mask = dev(self.inp["mask"].to(torch.uint8))
        self.mask_kv = dev(self.inp["mask_kv"].to(torch.uint8)) if self.cross else None
        self.dlogits = dev(self.inp["dlogits"])
        self.pool_len = dev(torch.tensor([c["pool_len"]], dtype=torch.int32)) if c["pool_len"] is not None else None
        self.seeds = (ctypes.c_uint64 * len(self.inp["seeds"]))(*self.inp["seeds"])
        self.nbytes = int(self.lib.vmc_tfam_train_input_workspace_bytes(*self.dims, int(self.proj)))
        assert self.nbytes > 0, "unsupported shape"
        self.want = WANT_DX | (WANT_DMOTION if self.cross else 0)
        self.fresh()

    def _keep(self, t):
        self.keep.append(t)
        return t

    def grad_names(self):
        c, names = self.c, []
        for l in range(c["L"]):
            for n in R.LAYER_W + R.LAYER_B + R.LAYER_LN:
                if self.cross or "cross" not in n:
                    names.append(f"L{l}.{n}")
        names += ["head." + n for n in R.HEAD_W + R.HEAD_F]
        if self.proj:
            names += ["proj.w_proj", "proj.b_proj"]
        return names

    def fresh(self, null=()):
        """New workspace (0xFF), logits and gradient destinations (sentinel) and the structs that point at them.  null: gradient
        names whose pointer stays NULL."""
        TT, c = self.TT, self.c
        self.ws = torch.full((self.nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.ws[self.nbytes:] = 0xA5
        assert self.ws.data_ptr() % 256 == 0
        self.logits = Out((c["B"], c["C"]))
        self.grads = {n: Out(self.inp["p32"][n].shape) for n in self.grad_names() if n not in null}
        gp = lambda n: self.grads[n].ptr() if n in self.grads else None
        self.layers = (TT.LayerParams * c["L"])()
        for l in range(c["L"]):
            s, pre = self.layers[l], f"L{l}."
            for n in R.LAYER_W:
                if self.cross or "cross" not in n:
                    setattr(s, n, self.w[pre + n].data_ptr())
                    setattr(s, "wt" + n[1:], self.wt[pre + n].data_ptr())
                    setattr(s, "g" + n, gp(pre + n))
            for n in R.LAYER_B:
                if self.cross or "cross" not in n:
                    setattr(s, n, self.f[pre + n].data_ptr())
                    setattr(s, "g" + n, gp(pre + n))
            for n in R.LAYER_LN:
                if self.cross or "cross" not in n:
                    setattr(s, n, self.f[pre + n].data_ptr())
                    setattr(s, "g_" + n, gp(pre + n))
        h = self.head = TT.HeadParams()
        h.w_cls1, h.w_cls4 = self.w["head.w_cls1"].data_ptr(), self.w["head.w_cls4"].data_ptr()
        h.w32_cls1, h.w32_cls4 = self.f["head.w_cls1"].data_ptr(), self.f["head.w_cls4"].data_ptr()
        for n in R.HEAD_F:
            setattr(h, n, self.f["head." + n].data_ptr())
        h.g_cls_ln_g, h.g_cls_ln_b = gp("head.cls_ln_g"), gp("head.cls_ln_b")
        h.gw_cls1, h.gb_cls1, h.gw_cls4, h.gb_cls4 = gp("head.w_cls1"), gp("head.b_cls1"), gp("head.w_cls4"), gp("head.b_cls4")
        pp = self.projp = TT.ProjParams()
        if self.proj:
            pp.w_proj, pp.b_proj = self.w["proj.w_proj"].data_ptr(), self.f["proj.b_proj"].data_ptr()
            pp.gw_proj, pp.gb_proj = gp("proj.w_proj"), gp("proj.b_proj")

    # ---- calls --------------------------------------------------------------------------------------------------------------
    def _p(self, t):
        return None if t is None else t.data_ptr()

    def _seed_at(self, i):
        return ctypes.cast(ctypes.addressof(self.seeds) + 8 * i, ctypes.c_void_p)

    def _common(self):
        return (float(self.drop[0]), float(self.drop[1]), self.seeds, self._p(self.pool_len), self.L_.dt(self.dtype), self.L_.stream())

    def forward(self):
        lib, ck = self.lib, self.L_.check
        ws = (self.ws.data_ptr(), self.nbytes)
        if self.proj:
            ck(lib.vmc_tfam_train_fwd_proj(self.x.data_ptr(), ctypes.byref(self.projp), self.mask.data_ptr(), self.layers, ctypes.byref(self.head),
                                           self.logits.ptr(), *ws, *self.pdims, *self._common()), "train_fwd_proj")
        else:
            ck(lib.vmc_tfam_train_fwd_len(self.x.data_ptr(), self._p(self.motion), self.mask.data_ptr(), self._p(self.mask_kv), self.layers,
                                          ctypes.byref(self.head), self.logits.ptr(), *ws, *self.dims, *self._common()), "train_fwd_len")

    def backward(self, want=None):
        lib, ck = self.lib, self.L_.check
        ws = (self.ws.data_ptr(), self.nbytes)
        p_drop, p_mlp, seeds, pl, dt, st = self._common()
        if self.proj:
            ck(lib.vmc_tfam_train_bwd_inputs_proj(self.dlogits.data_ptr(), ctypes.byref(self.projp), self.wt["proj.w_proj"].data_ptr(), self.mask.data_ptr(),
                                                  self.layers, ctypes.byref(self.head), *ws, *self.pdims, p_drop, p_mlp, seeds, pl, dt, st), "bwd_inputs_proj")
        else:
            ck(lib.vmc_tfam_train_bwd_inputs_len(self.dlogits.data_ptr(), self.mask.data_ptr(), self._p(self.mask_kv), self.layers, ctypes.byref(self.head),
                                                 *ws, *self.dims, p_drop, p_mlp, seeds, pl, self.want if want is None else want, dt, st), "bwd_inputs_len")

    def backward_plain(self):
        """vmc_tfam_train_bwd_len: no input gradients."""
        p_drop, p_mlp, seeds, pl, dt, st = self._common()
        self.L_.check(self.lib.vmc_tfam_train_bwd_len(self.dlogits.data_ptr(), self.mask.data_ptr(), self._p(self.mask_kv), self.layers,
                                                      ctypes.byref(self.head), self.ws.data_ptr(), self.nbytes, *self.dims, p_drop, p_mlp, seeds, pl, dt, st),
                      "train_bwd_len")

    def per_layer(self):
        """The same step through the per-layer entries (the feature mode has no per-layer forward: its F0 launch belongs to
        vmc_tfam_train_fwd_proj; its backward runs head, layers L-1..1 and vmc_tfam_layer0_bwd_proj_inputs)."""
        lib, ck, c = self.lib, self.L_.check, self.c
        ws = (self.ws.data_ptr(), self.nbytes)
        p_drop, p_mlp, seeds, pl, dt, st = self._common()
        L = c["L"]
        hseed = int(self.inp["seeds"][7 * L])
        if self.proj:
            self.forward()
        else:
            for l in range(L):
                ck(lib.vmc_tfam_layer_train_fwd(self.x.data_ptr() if l == 0 else None, self._p(self.motion), self.mask.data_ptr(), self._p(self.mask_kv),
                                                self.layers, l, *ws, *self.dims, p_drop, self._seed_at(7 * l), dt, st), "layer_train_fwd")
            if pl is None:
                ck(lib.vmc_tfam_head_train_fwd(self.layers, ctypes.byref(self.head), self.logits.ptr(), *ws, *self.dims, p_mlp, hseed, dt, st), "head_train_fwd")
            else:
                ck(lib.vmc_tfam_head_train_fwd_len(self.layers, ctypes.byref(self.head), self.logits.ptr(), *ws, *self.dims, p_mlp, hseed, pl, dt, st),
                   "head_train_fwd_len")
        if pl is None and not self.proj:
            ck(lib.vmc_tfam_head_bwd(self.dlogits.data_ptr(), self.layers, ctypes.byref(self.head), *ws, *self.dims, p_mlp, hseed, dt, st), "head_bwd")
        else:
            ck(lib.vmc_tfam_head_bwd_len(self.dlogits.data_ptr(), self.layers, ctypes.byref(self.head), *ws, *self.dims, p_mlp, hseed, pl, dt, st), "head_bwd_len")
        for l in range(L - 1, -1, -1):
            if self.proj and l == 0:
                ck(lib.vmc_tfam_layer0_bwd_proj_inputs(ctypes.byref(self.projp), self.wt["proj.w_proj"].data_ptr(), self.mask.data_ptr(), self.layers, *ws,
                                                       *self.pdims, p_drop, self._seed_at(0), dt, st), "layer0_bwd_proj_inputs")
            elif self.proj:
                ck(lib.vmc_tfam_layer_bwd(self.mask.data_ptr(), None, self.layers, l, *ws, *self.dims, p_drop, self._seed_at(7 * l), dt, st), "layer_bwd")
            else:
                ck(lib.vmc_tfam_layer_bwd_inputs(self.mask.data_ptr(), self._p(self.mask_kv), self.layers, l, *ws, *self.dims, p_drop, self._seed_at(7 * l),
                                                 self.want, dt, st), "layer_bwd_inputs")

    # ---- results ------------------------------------------------------------------------------------------------------------
    def _at(self, off, rows, cols):
        assert off >= 0 and off + rows * cols * 4 <= self.nbytes
        return self.ws[off:off + rows * cols * 4].view(F32).reshape(rows, cols).cpu().clone()

    def outputs(self, inputs=True):
        """Everything the ABI returns, on the CPU; checks the guards and that every element was written."""
        torch.cuda.synchronize()
        c = self.c
        M, Mk, D = c["B"] * c["T"], c["B"] * c["Tk"], c["D"]
        assert bool((self.ws[self.nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
        out = {"logits": self.logits.value()}
        out["pool_grad"] = self._at(int(self.lib.vmc_tfam_train_pool_grad_offset(*self.dims)), M, D)
        for n, o in self.grads.items():
            out["g." + n] = o.value()
        if inputs:
            offs = (ctypes.c_longlong * 3)()
            self.L_.check(self.lib.vmc_tfam_train_input_grad_offsets(*self.dims, int(self.proj), offs), "input_grad_offsets")
            if self.proj:
                out["dXcat"] = self._at(offs[2], M, 2 * D)
            else:
                out["dX"] = self._at(offs[0], M, D)
                if self.cross:
                    out["dMotion"] = self._at(offs[1], Mk, D)
        return out

    def run(self, route="chain"):
        self.fresh()
        if route == "chain":
            self.forward()
            self.backward()
        else:
            self.per_layer()
        return self.outputs()


def _same_bits(a, b, what=""):
    assert set(a) == set(b), (set(a) ^ set(b))
    for k in a:
        assert a[k].shape == b[k].shape and bool((a[k].view(torch.int32) == b[k].view(torch.int32)).all()), f"{what}{k} differs"


# ---------------------------------------------------------------------------------------------- the measure
@pytest.mark.parametrize("name,dtype,drop", CONFIGS, ids=CFG_ID)
def test_whole_chain_outputs_under_the_measure(name, dtype, drop):
    """vmc_tfam_train_fwd_len + vmc_tfam_train_bwd_inputs_len (both WANT bits), or vmc_tfam_train_fwd_proj + vmc_tfam_train_bwd_inputs_proj:
    every output within 2 rms(E) / 4 max|E| of the float64 step, E = model16 - r64."""
    r, m = R.chain_ref64(name, dtype, drop), R.chain_model16(name, dtype, drop)
    got = Step(name, dtype, drop).run()
    assert set(R.tensor_names(r)) == set(got), set(R.tensor_names(r)) ^ set(got)
    ms = R.measure_all(got, r, m)
    for x in ms:
        _record(name, dtype, drop, "chain", x)
        print(f"{name} {DT_NAME[dtype]} p{drop[0]} {x['name']}: rms {x['ratio_rms']:.2f} max {x['ratio_max']:.2f} model {x['model_dist']:.2f}")
    assert not R.failures(ms), R.failures(ms)


# ---------------------------------------------------------------------------------------------- the per-layer route
@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("name", ["a", "g1", "h"])
def test_per_layer_entries_equal_the_whole_chain_bit_for_bit(name, dtype):
    """vmc_tfam_layer_train_fwd, vmc_tfam_head_train_fwd / _len, vmc_tfam_head_bwd / _len, vmc_tfam_layer_bwd_inputs (vmc_tfam_layer_bwd and
    vmc_tfam_layer0_bwd_proj_inputs in the feature mode): logits and every gradient of the one-call step.  The launches are the same
    ones in the same order; the weight gradients run as one grouped launch per layer instead of one per step, tile by tile the same."""
    st = Step(name, dtype, R.DROPS[1])
    _same_bits(st.run("chain"), st.run("layers"))


# ---------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
def test_masked_motion_tokens_are_never_read_into_a_result(dtype):
    """Case a, dropout on: other finite values (1024, and random ones) in the motion tokens that mask_kv masks change no output bit,
    and their dMotion rows are exact zeros."""
    drop = R.DROPS[1]
    base = Step("a", dtype, drop).run()
    inp = dict(R.make_inputs("a", dtype, drop))
    dead = ~inp["mask_kv"].reshape(-1)
    assert dead.any() and not base["dMotion"][dead].any()
    for fill in (1024.0, None):
        mo = inp["motion"].clone()
        mo[dead] = 1024.0 if fill is not None else torch.randn(int(dead.sum()), mo.shape[1], generator=torch.Generator().manual_seed(3)) * 8
        _same_bits(base, Step("a", dtype, drop, dict(inp, motion=mo)).run(), f"fill {fill}: ")


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
def test_rows_behind_the_pool_length_are_never_read_into_a_result(dtype):
    """Case h, dropout on: other finite values in the token rows at and behind pool_len (masked as keys, not pooled) change no
    output bit; their dX and pool-gradient rows are exact zeros."""
    drop = R.DROPS[1]
    base = Step("h", dtype, drop).run()
    inp = dict(R.make_inputs("h", dtype, drop))
    c = inp["case"]
    pad = (torch.arange(c["T"]) >= c["pool_len"]).repeat(c["B"])
    assert not base["dX"][pad].any() and not base["pool_grad"][pad].any() and base["dX"][~pad].any()
    x = inp["x"].clone()
    x[pad] = torch.randn(int(pad.sum()), c["D"], generator=torch.Generator().manual_seed(4)) * 8
    x[c["pool_len"]] = 1024.0
    _same_bits(base, Step("h", dtype, drop, dict(inp, x=x)).run())


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("name", ["a", "g1"])
def test_null_gradient_pointers_leave_the_others_unchanged(name, dtype):
    """Dropout on.  A weight gradient's NULL takes its bias gradient along (the grouped launch refuses a bias gradient on its own)."""
    st = Step(name, dtype, R.DROPS[1])
    base = st.run()
    names = st.grad_names()
    subsets = [[n for n in names if ".ln_" in n or "cls_ln" in n],                                   # every LayerNorm parameter
               [n for n in names if n.split(".")[1][1:] in ("_self_in", "_ffn3", "_cls1", "_proj")],      # some linears, weight and bias
               [n for n in names if n.split(".")[1].startswith("b_")]]                                # every bias
    for null in subsets:
        assert null
        st.fresh(null=set(null))
        st.forward()
        st.backward()
        got = st.outputs()
        _same_bits({k: v for k, v in base.items() if k[2:] not in null}, got, "with NULLs: ")


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
def test_inputs_entry_with_want_0_is_the_plain_backward(dtype):
    st = Step("a", dtype, R.DROPS[1])
    st.fresh()
    st.forward()
    st.backward(want=0)
    a = st.outputs(inputs=False)
    st.fresh()
    st.forward()
    st.backward_plain()
    _same_bits(a, st.outputs(inputs=False))


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("name", ["a", "g1"])
def test_entries_without_input_gradients_on_their_own_workspace(name, dtype):
    """vmc_tfam_train_fwd + vmc_tfam_train_bwd on exactly vmc_tfam_train_workspace_bytes, and vmc_tfam_train_fwd_proj + vmc_tfam_train_bwd_proj
    (then head + vmc_tfam_layer_bwd + vmc_tfam_layer0_bwd_proj) on exactly vmc_tfam_train_proj_workspace_bytes: logits, the pool gradient
    and every parameter gradient of the `_inputs` step on the larger workspace, bit for bit.  Dropout on."""
    st = Step(name, dtype, R.DROPS[1])
    lib, ck = st.lib, st.L_.check
    assert lib.vmc_tfam_input_grad_supported(*st.dims, int(st.proj)) == 0
    base = {k: v for k, v in st.run().items() if k not in ("dX", "dMotion", "dXcat")}
    small = int(lib.vmc_tfam_train_proj_workspace_bytes(*st.pdims)) if st.proj else int(lib.vmc_tfam_train_workspace_bytes(*st.dims))
    if st.proj:
        assert lib.vmc_tfam_proj_supported(*st.pdims) == 0
    assert 0 < small < st.nbytes
    st.nbytes = small
    p_drop, p_mlp, seeds, pl, dt, sm = st._common()
    assert pl is None
    for route in (("chain", "layers") if st.proj else ("chain",)):
        st.fresh()
        ws = (st.ws.data_ptr(), st.nbytes)
        if not st.proj:
            ck(lib.vmc_tfam_train_fwd(st.x.data_ptr(), st._p(st.motion), st.mask.data_ptr(), st._p(st.mask_kv), st.layers, ctypes.byref(st.head),
                                      st.logits.ptr(), *ws, *st.dims, p_drop, p_mlp, seeds, dt, sm), "train_fwd")
            ck(lib.vmc_tfam_train_bwd(st.dlogits.data_ptr(), st.mask.data_ptr(), st._p(st.mask_kv), st.layers, ctypes.byref(st.head), *ws, *st.dims,
                                      p_drop, p_mlp, seeds, dt, sm), "train_bwd")
        else:
            st.forward()
            if route == "chain":
                ck(lib.vmc_tfam_train_bwd_proj(st.dlogits.data_ptr(), ctypes.byref(st.projp), st.mask.data_ptr(), st.layers, ctypes.byref(st.head), *ws,
                                               *st.pdims, p_drop, p_mlp, seeds, pl, dt, sm), "train_bwd_proj")
            else:
                L = st.c["L"]
                ck(lib.vmc_tfam_head_bwd_len(st.dlogits.data_ptr(), st.layers, ctypes.byref(st.head), *ws, *st.dims, p_mlp, int(st.inp["seeds"][7 * L]),
                                             pl, dt, sm), "head_bwd_len")
                for l in range(L - 1, 0, -1):
                    ck(lib.vmc_tfam_layer_bwd(st.mask.data_ptr(), None, st.layers, l, *ws, *st.dims, p_drop, st._seed_at(7 * l), dt, sm), "layer_bwd")
                ck(lib.vmc_tfam_layer0_bwd_proj(ctypes.byref(st.projp), st.mask.data_ptr(), st.layers, *ws, *st.pdims, p_drop, st._seed_at(0), dt, sm),
                   "layer0_bwd_proj")
        _same_bits(base, st.outputs(inputs=False), route + ": ")


# ---------------------------------------------------------------------------------------------- the eval chain
W_SELF_IN, W_SELF_OUT, W_CROSS_Q, W_CROSS_OUT, W_FFN0, W_FFN3, W_KV_ALL, W_CLS1, W_CLS4, W_END = range(10)
(P_SELF_IN_B, P_SELF_OUT_B, P_CROSS_Q_B, P_CROSS_OUT_B, P_FFN0_B, P_FFN3_B, P_NORM_SELF, P_NORM_CROSS, P_NORM_FFN,
 P_KV_ALL_B, P_CLS_LN, P_CLS1_B, P_CLS4_B, P_END) = range(16, 30)


def _packs(inp):
    """wpack / ppack of include/vmc.h from the case's parameters: plain copies of the 16-bit weights, vmc_tfam_fold_layernorm for
    the three linears that consume a LayerNorm output."""
    L_ = _lib()
    lib, c, dtype = L_.lib, inp["case"], inp["dtype"]
    D, ff, L, C = c["D"], c["ff"], c["L"], c["C"]
    cross = c["mode"] == "cross"
    off = lambda slot, l=0: int(lib.vmc_tfam_pack_offset(slot, l, D, ff, L, C))
    wpack = torch.zeros(off(W_END), dtype=dtype, device="cuda")
    ppack = torch.zeros(off(P_END), dtype=F32, device="cuda")
    p32, w16 = inp["p32"], inp["w16"]

    def put_w(slot, l, w):
        wpack[off(slot, l):off(slot, l) + w.numel()] = w.reshape(-1).cuda()

    def put_p(slot, l, *vals):
        o = off(slot, l)
        for v in vals:
            ppack[o:o + v.numel()] = v.reshape(-1).cuda()
            o += v.numel()

    def put_folded(wslot, bslot, l, w, b, ln):
        w, b = w.contiguous().cuda(), b.contiguous().cuda()
        g, be = p32[ln + "_g"].cuda(), p32[ln + "_b"].cuda()
        rows, cols = w.shape
        wo, bo = off(wslot, l), off(bslot, l)
        L_.check(lib.vmc_tfam_fold_layernorm(w.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(), wpack[wo:wo + rows * cols].data_ptr(),
                                             ppack[bo:bo + rows].data_ptr(), rows, cols, L_.dt(dtype), L_.stream()), "fold_layernorm")
        torch.cuda.synchronize()

    for l in range(L):
        pre = f"L{l}."
        if l == 0:
            put_w(W_SELF_IN, l, w16[pre + "w_self_in"])
            put_p(P_SELF_IN_B, l, p32[pre + "b_self_in"])
        else:
            put_folded(W_SELF_IN, P_SELF_IN_B, l, p32[pre + "w_self_in"], p32[pre + "b_self_in"], f"L{l - 1}.ln_ffn")
        put_w(W_SELF_OUT, l, w16[pre + "w_self_out"])
        put_p(P_SELF_OUT_B, l, p32[pre + "b_self_out"])
        if cross:
            put_folded(W_CROSS_Q, P_CROSS_Q_B, l, p32[pre + "w_cross_in"][:D], p32[pre + "b_cross_in"][:D], pre + "ln_self")
            put_w(W_CROSS_OUT, l, w16[pre + "w_cross_out"])
            put_w(W_KV_ALL, l, w16[pre + "w_cross_in"][D:])
            put_p(P_CROSS_OUT_B, l, p32[pre + "b_cross_out"])
            put_p(P_KV_ALL_B, l, p32[pre + "b_cross_in"][D:])
            put_p(P_NORM_CROSS, l, p32[pre + "ln_cross_g"], p32[pre + "ln_cross_b"])
        put_folded(W_FFN0, P_FFN0_B, l, p32[pre + "w_ffn0"], p32[pre + "b_ffn0"], pre + ("ln_cross" if cross else "ln_self"))
        put_w(W_FFN3, l, w16[pre + "w_ffn3"])
        put_p(P_FFN3_B, l, p32[pre + "b_ffn3"])
        put_p(P_NORM_SELF, l, p32[pre + "ln_self_g"], p32[pre + "ln_self_b"])
        put_p(P_NORM_FFN, l, p32[pre + "ln_ffn_g"], p32[pre + "ln_ffn_b"])
    put_w(W_CLS1, 0, w16["head.w_cls1"])
    put_w(W_CLS4, 0, w16["head.w_cls4"])
    put_p(P_CLS_LN, 0, p32["head.cls_ln_g"], p32["head.cls_ln_b"])
    put_p(P_CLS1_B, 0, p32["head.b_cls1"])
    put_p(P_CLS4_B, 0, p32["head.b_cls4"])
    return wpack, ppack


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("name", R.EVAL_CASES)
def test_eval_chain_logits_under_the_measure_and_both_routes_agree(name, dtype):
    """vmc_tfam_forward_len against the `folded` model, and vmc_tfam_kv_fwd + vmc_tfam_layer_fwd + vmc_tfam_head_fwd_len bit-equal to it."""
    L_ = _lib()
    lib, ck = L_.lib, L_.check
    inp = R.make_inputs(name, dtype, R.DROPS[0])
    c = inp["case"]
    cross = c["mode"] == "cross"
    dims = (c["B"], c["T"], c["Tk"], c["D"], c["H"], c["ff"], c["L"], c["C"], int(cross))
    assert lib.vmc_tfam_supported(*dims, 0) == 0
    wpack, ppack = _packs(inp)
    x = inp["x"].cuda()
    motion = inp["motion"].cuda() if cross else None
    mask = inp["mask"].to(torch.uint8).cuda()
    mask_kv = inp["mask_kv"].to(torch.uint8).cuda() if cross else None
    pool_len = torch.tensor([c["pool_len"]], dtype=torch.int32, device="cuda") if c["pool_len"] is not None else None
    p = lambda t: None if t is None else t.data_ptr()
    nbytes = int(lib.vmc_tfam_workspace_bytes(dims[0], dims[1], dims[2], dims[3], dims[5], dims[6], dims[7], dims[8]))
    outs = []
    for route in ("forward", "layers"):
        ws = torch.full((nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        ws[nbytes:] = 0xA5
        logits = Out((c["B"], c["C"]))
        tail = (L_.dt(dtype), L_.stream())
        if route == "forward":
            ck(lib.vmc_tfam_forward_len(x.data_ptr(), p(motion), mask.data_ptr(), p(mask_kv), wpack.data_ptr(), ppack.data_ptr(), logits.ptr(),
                                        ws.data_ptr(), nbytes, *dims, p(pool_len), *tail), "forward_len")
        else:
            if cross:
                ck(lib.vmc_tfam_kv_fwd(motion.data_ptr(), wpack.data_ptr(), ppack.data_ptr(), ws.data_ptr(), nbytes, *dims[:8], *tail), "kv_fwd")
            for l in range(c["L"]):
                ck(lib.vmc_tfam_layer_fwd(x.data_ptr() if l == 0 else None, mask.data_ptr(), p(mask_kv), wpack.data_ptr(), ppack.data_ptr(), l,
                                          ws.data_ptr(), nbytes, *dims, *tail), "layer_fwd")
            ck(lib.vmc_tfam_head_fwd_len(wpack.data_ptr(), ppack.data_ptr(), logits.ptr(), ws.data_ptr(), nbytes, *dims, p(pool_len), *tail), "head_fwd_len")
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all())
        outs.append({"logits": logits.value()})
    _same_bits(outs[0], outs[1])
    r, m = R.run_eval(inp), R.run_eval(inp, dtype)
    x_ = R.measure("logits", outs[0]["logits"], r, m)
    _record(name, dtype, R.DROPS[0], "eval", x_)
    print(f"eval {name} {DT_NAME[dtype]}: rms {x_['ratio_rms']:.2f} max {x_['ratio_max']:.2f} model {x_['model_dist']:.2f}")
    assert x_["ok"], R.failures([x_])


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("rows,cols", [(1536, 512), (512, 768)])
def test_fold_layernorm_against_float64(rows, cols, dtype):
    """w16 = round16(W . gamma) under the interval rule of the GEMM family, bias + W beta under §5's 8 max(e32, 2^-23)."""
    L_ = _lib()
    g = torch.Generator().manual_seed(rows + cols)
    W = torch.randn(rows, cols, generator=g) * cols ** -0.5
    b, gamma, beta = torch.randn(rows, generator=g), torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    w64, b64 = R.fold_ref(W, b, gamma, beta)
    w32, b32 = R.fold_ref(W, b, gamma, beta, compute=F32)
    e_w, e_b = G.e32_of(w32, w64), G.e32_of(b32, b64)
    ends = G.interval16(w64, e_w, dtype)
    assert G.pinned_share(*ends) >= G.SHARE_MIN[dtype]
    w16 = torch.full((rows * cols + GUARD,), -1, dtype=torch.int16, device="cuda")
    bout = Out((rows,))
    dev = [t.cuda() for t in (W, b, gamma, beta)]
    L_.check(L_.lib.vmc_tfam_fold_layernorm(*(t.data_ptr() for t in dev), w16.data_ptr(), bout.ptr(), rows, cols, L_.dt(dtype), L_.stream()), "fold")
    torch.cuda.synchronize()
    assert bool((w16[rows * cols:] == -1).all())
    mw = G.measure16(w16[:rows * cols].view(dtype).reshape(rows, cols), w64, e_w, dtype, ends)
    mb = G.measure32(bout.value(), b64, e_b)
    print(f"fold {rows}x{cols} {DT_NAME[dtype]}: weights pinned {mw['pinned']:.3f} outside {mw['bad']} ratio {mw['ratio']:.2f}; bias ratio {mb['ratio']:.2f}")
    assert mw["ok"] and mb["ok"], (mw, mb)
