"""GPU: every attention kernel family behind attn_route.h against the float64 references and the designed-rounding model of
tests/attention_refs.py (the conditions on the cases themselves are checked on the CPU by tests/test_attention_refs_host.py).

Each case runs on random-normal inputs under the measure
    rms(got - r64) <= 2 E_rms  and  max|got - r64| <= 4 E_max     (E: the model's own error against float64; lse: see the module)
and on selector inputs, where every query attends to one known key, under the exact check (out = v[pi(i)] bit for bit, ...); the
masked entry points also with dropout p = 0.25 (measure) and p = 0.5 (factor exactly 2; exact check).  The scalar fp32 kernels
are held to train_kernel_refs' e32 yardstick instead.  Every case first asserts the kernel family attn_route.h gives it (through the
port the host test pins to the header), with the alignment of the buffers actually passed.  Output buffers carry a sentinel in
their gap columns and around them, which must survive bit for bit.

With VMC_ATTN_PARITY_JSON=<path> the ratios of every case against the model are written there (profiles/attention_parity.jsonl)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import attention_refs as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_IDS = {A.BF16: "bf16", A.F16: "f16"}
SENT_IN, SENT_OUT = 7.0, -1536.0        # gap columns of the inputs / every element of an output buffer before the call
E_SHAPE = -3

L = None
_REC = []


@pytest.fixture(scope="module", autouse=True)
def _lib_module():
    global L
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vimo_clip_amd import _lib
    L = _lib
    yield
    A._PREP.clear()             # the shared references (half a gigabyte with the 520-head variant runs) end with this module
    out = os.environ.get("VMC_ATTN_PARITY_JSON", "")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps({"R_RMS": A.R_RMS, "R_MAX": A.R_MAX}) + "\n")
            f.writelines(json.dumps(r) + "\n" for r in _REC)


def rec(family, case, dtype, way, ms):
    for m in ms:
        print(f"{family} {case} {DT_IDS[dtype]} {way} {m['name']}: rms {m['rms']:.3e} / E_rms {m['e_rms']:.3e} = {m['ratio_rms']:.2f}, "
              f"max {m['max']:.3e} / E_max {m['e_max']:.3e} = {m['ratio_max']:.2f}")
        _REC.append(dict(family=family, case=case, dtype=DT_IDS[dtype], way=way, output=m["name"], rms=m["rms"], e_rms=m["e_rms"],
                         max=m["max"], e_max=m["e_max"], ratio_rms=m["ratio_rms"], ratio_max=m["ratio_max"], ok=m["ok"]))


# ---------------------------------------------------------------------------------------------- buffers
class Buf:
    """A [rows, D] view with row stride ld, `off` bytes past a 256-byte boundary, inside a flat buffer filled with `fill`."""

    def __init__(self, rows, D, dtype, ld=None, off=0, fill=SENT_OUT, src=None):
        ld = ld or D
        assert off % 2 == 0
        self.flat = torch.full((rows * ld + 64,), fill, dtype=dtype, device=DEV)
        self.view = self.flat[off // 2: off // 2 + rows * ld].view(rows, ld)[:, :D]
        self.fill, self.ld = fill, ld
        if src is not None:
            self.view.copy_(src.to(DEV))
        self.inside = torch.zeros(rows * ld + 64, dtype=torch.bool)
        self.inside[off // 2: off // 2 + rows * ld].view(rows, ld)[:, :D] = True

    def untouched(self):
        """Everything outside the view still holds the fill, bit for bit."""
        f = self.flat.cpu()
        want = torch.full_like(f, self.fill)
        return bool((f.view(torch.int16) == want.view(torch.int16))[~self.inside].all())

    def all_fill(self):
        f = self.flat.cpu()
        return bool((f.view(torch.int16) == torch.full_like(f, self.fill).view(torch.int16)).all())


def _off16(t):
    return t.data_ptr() % 16


def run_masked(c, P, dtype, check_route=True, bwd=True):
    """One vmc_attention_fwd + vmc_attention_bwd on the case's buffers; returns the outputs on the CPU and the output buffers."""
    B, H, Tq, Tk, dh = P["shape"]
    D = H * dh
    ld = D + c["pad"]
    t = P["t"]
    q, k, v, dout = (Buf(x.shape[0], D, dtype, ld, fill=SENT_IN, src=x) for x in (t["q"], t["k"], t["v"], t["dout"]))
    mask = None if P["mask"] is None else P["mask"].to(torch.uint8).to(DEV)
    out = Buf(B * Tq, D, dtype, ld, off=c["out_off"])
    lse = torch.full((B, H, Tq), SENT_OUT, dtype=torch.float32, device=DEV)
    dq = Buf(B * Tq, D, dtype, ld + c["lddq_pad"], off=c["grad_off"])
    dk, dv = Buf(B * Tk, D, dtype, ld, off=c["grad_off"]), Buf(B * Tk, D, dtype, ld, off=c["grad_off"])
    if check_route:
        assert A.route_fwd(Tq, Tk, dh, _off16(out.view)) == c["fwd"]
    rc = L.lib.vmc_attention_fwd(L.ptr(q.view), L.ptr(k.view), L.ptr(v.view), L.ptr(mask), L.ptr(out.view), L.ptr(lse), B, H, Tq, Tk, dh,
                                 ld, ld, ld, ld, float(P["p"]), int(P["seed"]), L.dt(dtype), L.stream())
    bufs = dict(out=out, dq=dq, dk=dk, dv=dv)
    if rc != 0 or not bwd:
        torch.cuda.synchronize()
        return rc, dict(out=out.view.cpu(), lse=lse.cpu()), bufs
    if "bwd_in" in P:            # the scalar backward takes CPU-made out / lse
        out_in = Buf(B * Tq, D, dtype, ld, fill=SENT_IN, src=P["bwd_in"][0]).view
        lse_in = P["bwd_in"][1].to(DEV).contiguous()
    elif c["out_off"]:           # the MFMA backward reads out in 16-byte words: give it the forward's result on an aligned base
        assert c["pad"] == 0
        out_in, lse_in = out.view.clone(), lse
    else:
        out_in, lse_in = out.view, lse
    if check_route:
        got = A.route_bwd(Tq, Tk, dh, ldd=dq.ld, ldo=ld, grad_off=max(_off16(x.view) for x in (dq, dk, dv)), out_off=_off16(out_in))
        assert got[0] == c["bwd"] and (c["block"] is None or got[1:] == (c["block"], c["rs"])), got
    nbytes = L.lib.vmc_attention_bwd_workspace_bytes(B, H, Tq)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=DEV)
    rc = L.lib.vmc_attention_bwd(L.ptr(q.view), L.ptr(k.view), L.ptr(v.view), L.ptr(mask), L.ptr(out_in), L.ptr(dout.view), L.ptr(lse_in),
                                 L.ptr(dq.view), L.ptr(dk.view), L.ptr(dv.view), B, H, Tq, Tk, dh, ld, ld, ld, ld, dq.ld, ld, ld,
                                 float(P["p"]), int(P["seed"]), L.ptr(ws), nbytes, L.dt(dtype), L.stream())
    torch.cuda.synchronize()
    got = dict(out=out.view.cpu(), lse=lse.cpu(), dq=dq.view.cpu(), dk=dk.view.cpu(), dv=dv.view.cpu())
    return rc, got, bufs


def check_masked(family, c, dtype, way):
    P = A.prepare(c, dtype, way)
    rc, got, bufs = run_masked(c, P, dtype)
    assert rc == 0, rc
    for n, b in bufs.items():
        assert b.untouched(), f"{n}: an element outside the [rows, H dh] view was written"
    cid = A.case_id(c)
    r64 = P["r64"]
    r64_b, model_b = P.get("r64_b", r64), P.get("model_b", P["model"])
    bad = []
    if P["sel"]:
        ref = dict(r64_b, out=r64["out"], lse=r64["lse"])
        bad += A.selector_check(got, P["t"], P["mask"], P["shape"], dtype, P["fac"], ref, dict(model_b, out=P["model"]["out"]),
                                scalar_fwd=A.family_of(c) is A.FAM_SCALAR)
    else:
        fwd_scalar, bwd_scalar = A.family_of(c) is A.FAM_SCALAR, A.bwd_family_of(c) is A.FAM_SCALAR
        for names, scalar, ref, r32, model in ((("out", "lse"), fwd_scalar, r64, P.get("r32"), P["model"]),
                                               (("dq", "dk", "dv"), bwd_scalar, r64_b, P.get("r32_b"), model_b)):
            if scalar:
                for n in names:
                    x = A.scalar_excess(n, got[n], ref[n], r32[n], dtype)
                    print(f"{family} {cid} {DT_IDS[dtype]} {way} {n}: scalar excess {x:.3f}")
                    _REC.append(dict(family=family + "/scalar", case=cid, dtype=DT_IDS[dtype], way=way, output=n, excess=x, ok=x <= 1))
                    if not x <= 1:
                        bad.append(f"{n}: {x:.3f} times the e32 bound")
            else:
                ms = A.measure_all(got, ref, model, names)
                rec(family, cid, dtype, way, ms)
                bad += A.failures(ms)
    # rows of a clip without a live key: NaN forward and zero dv everywhere; zero dq / dk from the tiled and the scalar backward, NaN
    # dq / dk from the in-LDS backward (its zero probabilities times the NaN delta, what torch's autograd gives too): both pinned
    dead = torch.isnan(r64["lse"])
    if dead.any():
        rows, krows = r64["dead_q"], r64["dead_k"]
        assert torch.isnan(got["out"].float()[rows]).all() and torch.isnan(got["lse"][dead]).all()
        assert not torch.isnan(got["out"].float()[~rows]).any() and not torch.isnan(got["lse"][~dead]).any()
        assert (got["dv"][krows] == 0).all()
        if c["bwd"] == A.BM:
            assert torch.isnan(got["dq"].float()[rows]).all() and torch.isnan(got["dk"].float()[krows]).all()
        else:
            assert (got["dq"][rows] == 0).all() and (got["dk"][krows] == 0).all()
        for n, r_ in (("dq", rows), ("dk", krows), ("dv", krows)):
            assert torch.isfinite(got[n].float()[~r_]).all(), n
    assert not bad, "\n".join(bad)


def _params(lst):
    return [pytest.param(c, dtype, way, id=f"{A.case_id(c)}-{DT_IDS[dtype]}-{way}") for c in lst for dtype in A.DT16 for way in A.ways_of(c)]


# ---------------------------------------------------------------------------------------------- the dropout mask the references use
def test_dropout_factor_port_equals_vmc_dropout():
    for p, seed, (B, H, Tq, Tk) in ((0.25, A.DROP_SEED["rand-p25"], (2, 2, 63, 127)), (0.5, A.DROP_SEED["sel-p50"], (2, 1, 289, 289))):
        ones = torch.ones(B * H * Tq * Tk, device=DEV)
        fac = torch.empty_like(ones)
        L.check(L.lib.vmc_dropout(L.ptr(ones), L.ptr(fac), ones.numel(), p, seed, L.dt(ones), L.dt(A.BF16), L.stream()), "dropout")
        assert torch.equal(fac.cpu().double().view(B, H, Tq, Tk), A.dropout_fac(p, seed, B, H, Tq, Tk))


# ---------------------------------------------------------------------------------------------- the masked entry points
@pytest.mark.parametrize("c,dtype,way", _params(A.SMALL_CASES))
def test_attn_small_kernel(c, dtype, way):
    check_masked("attn_small_kernel", c, dtype, way)


@pytest.mark.parametrize("c,dtype,way", _params(A.LONG_FWD_CASES))
def test_attn_long_fwd_kernel(c, dtype, way):
    check_masked("attn_long_fwd_kernel", c, dtype, way)


@pytest.mark.parametrize("c,dtype,way", _params(A.BWD_LDS_CASES))
def test_attn_bwd_mfma_kernel(c, dtype, way):
    check_masked("attn_bwd_mfma_kernel", c, dtype, way)


@pytest.mark.parametrize("c,dtype,way", _params(A.BWD_TILED_CASES))
def test_attn_long_bwd_kernels(c, dtype, way):
    check_masked("attn_long_bwd", c, dtype, way)


@pytest.mark.parametrize("c,dtype,way", _params(A.SCALAR_CASES))
def test_attn_generic_kernels_and_the_fallbacks_onto_them(c, dtype, way):
    check_masked("attn_generic", c, dtype, way)


@pytest.mark.parametrize("c", A.CAP_CASES, ids=A.case_id)
def test_scalar_cap_returns_an_error_and_writes_nothing(c):
    shape = A.shape_of(c)
    B, H, Tq, Tk, dh = shape
    D = H * dh
    z = lambda T: torch.zeros(B * T, D, dtype=A.F16)
    P = dict(shape=shape, t=dict(q=z(Tq), k=z(Tk), v=z(Tk), dout=z(Tq)), mask=None, p=0.0, seed=0)
    if c["fwd"] == "E_SHAPE":
        rc, got, bufs = run_masked(c, P, A.F16, bwd=False)
        assert rc == E_SHAPE and bufs["out"].all_fill() and (got["lse"] == SENT_OUT).all()
    # the backward on its own fallback (lddq % 4 != 0, another head dim, or dq / dk / dv 4 bytes off at a tiled length), past the cap
    q, k, v, dout, out_in = (Buf(x.shape[0], D, A.F16, src=x) for x in (z(Tq), z(Tk), z(Tk), z(Tq), z(Tq)))
    lse = torch.zeros(B, H, Tq, device=DEV)
    g = c["grad_off"]
    dq, dk, dv = Buf(B * Tq, D, A.F16, D + c["lddq_pad"], off=g), Buf(B * Tk, D, A.F16, off=g), Buf(B * Tk, D, A.F16, off=g)
    assert A.route_bwd(Tq, Tk, dh, ldd=dq.ld, grad_off=max(_off16(x.view) for x in (dq, dk, dv)), out_off=_off16(out_in.view))[0] == "E_SHAPE"
    nbytes = L.lib.vmc_attention_bwd_workspace_bytes(B, H, Tq)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=DEV)
    rc = L.lib.vmc_attention_bwd(L.ptr(q.view), L.ptr(k.view), L.ptr(v.view), None, L.ptr(out_in.view), L.ptr(dout.view), L.ptr(lse),
                                 L.ptr(dq.view), L.ptr(dk.view), L.ptr(dv.view), B, H, Tq, Tk, dh, D, D, D, D, dq.ld, D, D,
                                 0.0, 0, L.ptr(ws), nbytes, L.dt(A.F16), L.stream())
    torch.cuda.synchronize()
    assert rc == E_SHAPE and dq.all_fill() and dk.all_fill() and dv.all_fill()


DETERMINISM = [("small", A.SMALL_CASES[7]), ("long_fwd", A.LONG_FWD_CASES[1]), ("bwd_lds", A.BWD_LDS_CASES[2]),
               ("bwd_tiled", A.BWD_TILED_CASES[0]), ("scalar", A.SCALAR_CASES[1]),
               ("bwd_lds_2waves", A.BWD_LDS_CASES[0]), ("bwd_lds_3waves", A.SMALL_CASES[4]), ("bwd_lds_3waves_b", A.SMALL_CASES[5])]
assert [c["block"] for _, c in DETERMINISM[5:]] == [128, 192, 192]


@pytest.mark.parametrize("name,c", DETERMINISM, ids=[n for n, _ in DETERMINISM])
def test_two_calls_give_identical_bits(name, c):
    P = A.prepare(c, A.BF16, "rand-p25")
    _, a, _ = run_masked(c, P, A.BF16, check_route=False)
    _, b, _ = run_masked(c, P, A.BF16, check_route=False)
    for n in A.OUTS:
        assert torch.equal(a[n], b[n]), n


# ---------------------------------------------------------------------------------------------- ViT
def run_vit(P, F, N, H, cls=False):
    from vimo_clip_amd import ops
    D = H * 64
    if cls:
        kv = P["qkv"][:, D:].contiguous().to(DEV)
        out = ops.attention_vit_cls(P["q"].to(DEV), kv, F, N, H)
        torch.cuda.synchronize()
        return dict(out=out.cpu(), lse=None)
    out, lse = ops.attention_vit(P["qkv"].to(DEV), F, N, H, want_lse=True)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), lse=lse.cpu())


def check_vit(family, P, got, dtype, way, case):
    names = ("out", "lse") if got["lse"] is not None else ("out",)
    if P["sel"]:
        bad = A.selector_check(got, P["t"], None, P["shape"], dtype, backward=False)
    else:
        ms = A.measure_all(got, P["r64"], P["model"], names)
        rec(family, case, dtype, way, ms)
        bad = A.failures(ms)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("way", ["rand", "sel"])
@pytest.mark.parametrize("dtype", A.DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("N", A.VIT_N)
def test_attn_vit_kernel(N, dtype, way):
    F, H = A.VIT_F, A.VIT_H
    assert A.route_vit(N, N, F, H) == ("ATTN_VIT", A.VIT_INST[N], F * H)
    P = A.prepare_vit(F, N, H, dtype, way)
    check_vit("attn_vit_kernel", P, run_vit(P, F, N, H), dtype, way, f"N{N}")


@pytest.mark.parametrize("way", ["rand", "sel"])
@pytest.mark.parametrize("dtype", A.DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("N", A.VIT_LONG_N)
def test_attn_vit_long_kernel(N, dtype, way):
    F, H = A.VIT_LONG_F, A.VIT_LONG_H
    assert A.route_vit(N, N, F, H) == ("ATTN_VIT_LONG", 577 if N == 577 else 0, F * H * ((N + 127) // 128))
    P = A.prepare_vit(F, N, H, dtype, way)
    check_vit("attn_vit_long_kernel", P, run_vit(P, F, N, H), dtype, way, f"N{N}")


@pytest.mark.parametrize("way", ["rand", "sel"])
@pytest.mark.parametrize("dtype", A.DT16, ids=["bf16", "f16"])
@pytest.mark.parametrize("N", A.CLS_N)
def test_class_query_against_float64_and_row0_of_the_full_call(N, dtype, way):
    F, H = A.CLS_F, A.CLS_H
    D = H * 64
    k = A.route_vit(N, 1, F, H)
    assert k[0] == ("ATTN_VIT" if N <= 288 else "ATTN_VIT_LONG_CLS") and (N > 288 or k[1] == (4 if N == 257 else A.route_vit(N, N, F, H)[1]))
    P = A.prepare_vit(F, N, H, dtype, way, cls=True)
    got = run_vit(P, F, N, H, cls=True)
    check_vit("attn_vit_cls", P, got, dtype, way, f"N{N}")
    full = run_vit(P, F, N, H)
    assert torch.equal(got["out"], full["out"].view(F, N, D)[:, 0])


def test_vit_two_calls_give_identical_bits():
    for N, cls in ((257, False), (577, False), (641, True), (197, True)):
        P = A.prepare_vit(A.CLS_F, N, A.CLS_H, A.BF16, "rand", cls=cls)
        a, b = run_vit(P, A.CLS_F, N, A.CLS_H, cls), run_vit(P, A.CLS_F, N, A.CLS_H, cls)
        assert torch.equal(a["out"], b["out"]) and (cls or torch.equal(a["lse"], b["lse"]))


# ---------------------------------------------------------------------------------------------- VMC_ATTN_VARIANT
_CHILD = r'''
import sys, torch
from vimo_clip_amd import ops
src, dst, F, N, H = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
res = {}
for key, qkv in torch.load(src).items():
    x = qkv.cuda()
    out, lse = ops.attention_vit(x, F, N, H, want_lse=True)
    out2, lse2 = ops.attention_vit(x, F, N, H, want_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "two calls differ: " + key
    res[key] = (out.cpu(), lse.cpu())
torch.save(res, dst)
print("variant ok")
'''


@pytest.fixture(scope="module")
def variant_inputs(tmp_path_factory):
    """The packed qkv of the four (dtype, way) runs at N = 257, F H = 520, in one file every child reads."""
    F, N, H = A.VARIANT_F, A.VARIANT_N, A.VARIANT_H
    path = str(tmp_path_factory.mktemp("attn_variant") / "qkv.pt")
    torch.save({f"{DT_IDS[d]}-{w}": A.prepare_vit(F, N, H, d, w)["qkv"] for d in A.DT16 for w in ("rand", "sel")}, path)
    yield path
    os.remove(path)


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_attn_variant_in_a_subprocess(variant, variant_inputs, tmp_path):
    """VMC_ATTN_VARIANT is read once per process: each value runs the N = 257 call in a fresh child (one GPU process at a time),
    which only runs the kernel (twice: the two calls must agree bit for bit) and stores out / lse; the measure and the selector check are applied here, on the references the
    other children share.  F H = 520 >= 512: the persistent walks (10..29) give eight workgroups two heads and the others one."""
    F, N, H = A.VARIANT_F, A.VARIANT_N, A.VARIANT_H
    inst = A.VARIANT_INST[variant]
    assert A.route_vit(N, N, F, H, variant) == ("ATTN_VIT", inst, 512 if inst in (2, 3) else F * H)
    dst = str(tmp_path / "out.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD, variant_inputs, dst, str(F), str(N), str(H)], env=dict(os.environ, VMC_ATTN_VARIANT=str(variant)),
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "variant ok" in r.stdout, r.stderr[-2000:]
    res = torch.load(dst)
    os.remove(dst)
    for d in A.DT16:
        for w in ("rand", "sel"):
            out, lse = res[f"{DT_IDS[d]}-{w}"]
            check_vit(f"attn_vit_kernel/variant{variant}", A.prepare_vit(F, N, H, d, w), dict(out=out, lse=lse), d, w, f"N{N}")
