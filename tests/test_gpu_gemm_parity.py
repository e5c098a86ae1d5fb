"""GPU: every GEMM kernel behind gemm_route.h (gemm.hip, gemm8.hip, gemm_tn.hip, gemm_tn256.hip) against the float64 references of
tests/gemm_refs.py on random operands (the conditions on the cases themselves, and the kernel each one reaches, are checked on the
CPU by tests/test_gemm_refs_host.py).

  f32 outputs:     max|got - r64| / max|r64| <= 8 max(e32, 2^-23)
  16-bit outputs:  round16(r64 - B) <= got <= round16(r64 + B) for every element, B = 8 max(e32, 2^-23) max|r64|

Operands with a padded leading dimension carry NaN in the padding (so does a residual); every output buffer is pre-filled with a
sentinel, which must survive bit for bit in the padding columns, in the rows after the last output row and in the class rows that
out_row_group skips.  Every buffer is a whole rows x ld allocation.  The VMC_GEMM_* switches are read once per process, so those
cases run in a child process per setting (this file, run as a script), which prints its figures; the parent applies the rule.

With VMC_GEMM_PARITY_JSON=<path> the figures of every case are written there (profiles/gemm_parity.jsonl)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_refs as G
from gemm_refs import F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -1536.0              # every element of an output buffer before the call (exact in f32, bf16 and f16)
GUARD_ROWS = 2
NAN = float("nan")

L = None
_REC = []


def _load():
    global L
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vimo_clip_amd import _lib
    L = _lib


@pytest.fixture(scope="module", autouse=True)
def _lib_module():
    _load()
    yield
    G.clear()
    out = os.environ.get("VMC_GEMM_PARITY_JSON", "")
    if out:
        with open(out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in _REC)


# ---------------------------------------------------------------------------------------------- buffers
def operand(t, ld, col0=0):
    """t [rows, D] on the device inside a whole [rows, ld] allocation, starting at column col0; every other column holds NaN."""
    rows, D = t.shape
    if col0:
        t = torch.cat([torch.full((rows, col0), NAN, dtype=t.dtype), t], 1)
    buf = G.padded(t, ld, NAN)[0].to(DEV)
    return buf, buf[:, col0:col0 + D]


class Out:
    """[rows + GUARD_ROWS, ld] of the sentinel; the call may write columns 0 .. D-1 of the rows it is told to."""

    def __init__(self, rows, D, ld, dtype):
        self.buf = torch.full((rows + GUARD_ROWS, ld), SENT, dtype=dtype, device=DEV)
        self.rows, self.D = rows, D

    def read(self, written_rows=None):
        """(the written rows, in the order given; whether everything else still holds the sentinel bit for bit)."""
        cpu = self.buf.cpu()
        idx = torch.arange(self.rows) if written_rows is None else written_rows
        free = torch.ones(cpu.shape, dtype=torch.bool)
        free[idx, :self.D] = False
        iv = torch.int32 if cpu.dtype is F32 else torch.int16
        kept = bool((cpu.view(iv) == torch.full_like(cpu, SENT).view(iv))[free].all())
        return cpu[idx, :self.D].contiguous(), kept


def family(c):
    if c["kind"] == "splitk":
        return "SPLITK"
    if c["kind"] == "tn":
        return c["plan"][0]
    f = c["plan"].split()
    if f[0] == "2":
        return "G8P+TILE"                 # the tail split
    if f[1] == "TILE":
        return f"TILE{f[2]}"              # gemm_kernel, by kGemmTileCfgs entry
    return f[1] + ("32" if f[1] == "G8P" and int(f[2]) >= 5 else "")


# ---------------------------------------------------------------------------------------------- one call per case
def run_linear(c, dt):
    """-> [(output name, got in GEMM row order, sentinel kept)]"""
    P = G.prepare(c, dt)
    M, N, K, p = c["M"], c["N"], c["K"], c["pad"]
    a, _ = operand(P["a"], K + p["lda"])
    w, _ = operand(P["b"], K + p["ldw"])
    bias = None if P["bias"] is None else P["bias"].to(DEV)
    res = None if P["res"] is None else operand(P["res"], N + p["ldres"])[0]
    odt = P["outs"]["C"]["dtype"]
    C = Out(P["out_rows"], N, N + p["ldc"], odt)
    Z = Out(M, N, N + p["ldz"], dt) if c["z"] else None
    dims = (M, N, K, a.stride(0), w.stride(0), C.buf.stride(0), res.stride(0) if res is not None else 0)
    tail = (c["act"], float(c["alpha"]), L.dt(odt), L.dt(res) if res is not None else 0, c["org"], c["rrm"], L.dt(dt))
    ptrs = (L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(res), L.ptr(C.buf))
    if Z is not None:
        assert c["variant"] is None
        rc = L.lib.vmc_linear_preact(*ptrs, L.ptr(Z.buf), *dims, Z.buf.stride(0), *tail, L.stream())
    elif c["variant"] is not None:
        rc = L.lib.vmc_linear_variant(*ptrs, *dims, *tail, int(c["variant"]), L.stream())
    else:
        rc = L.lib.vmc_linear(*ptrs, *dims, *tail, L.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    outs = [("C",) + C.read(P["orow"])]
    if Z is not None:
        outs.append(("Z",) + Z.read())
    return outs


def run_splitk(c, dt):
    P = G.prepare(c, dt)
    M, N, K = c["M"], c["N"], c["K"]
    a, _ = operand(P["a"], K + c["pad"][0])
    w, _ = operand(P["b"], K + c["pad"][1])
    C = Out(M, N, N, F32)
    nbytes = L.lib.vmc_linear_splitk_workspace_bytes(M, N, K)
    assert (nbytes > 0) == (c["plan"][0] > 1) and nbytes == (c["plan"][0] * M * N * 4 if c["plan"][0] > 1 else 0)
    ws = torch.full((nbytes // 4,), NAN, dtype=F32, device=DEV) if nbytes else None
    rc = L.lib.vmc_linear_splitk_f32(L.ptr(a), L.ptr(w), L.ptr(C.buf), M, N, K, a.stride(0), w.stride(0), L.ptr(ws), nbytes, L.dt(dt), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return [("C",) + C.read()]


def tn_buffers(c, P):
    """dY / X as column windows (16 bytes in) of NaN-filled tensors where the case asks for it; C [N, K] and dbias [1, N] outputs."""
    N, K = c["N"], c["K"]
    dy = operand(P["a"], N + c["win"][0], 8 if c["win"][0] else 0)[1]
    x = operand(P["b"], K + c["win"][1], 8 if c["win"][1] else 0)[1]
    return dy, x, Out(N, K, K, F32), Out(1, N, N, F32)


def run_tn(c, dt):
    """Both entry points: vmc_linear_wgrad_tn (C), then vmc_linear_wgrad_bias_tn (C and dbias)."""
    P = G.prepare(c, dt)
    M, N, K = c["M"], c["N"], c["K"]
    outs = []
    for with_b in (False, True):
        dy, x, C, db = tn_buffers(c, P)
        nbytes = L.lib.vmc_linear_wgrad_tn_workspace_bytes(M, N, K)
        ws = torch.full((nbytes // 4,), NAN, dtype=F32, device=DEV) if nbytes else None
        if with_b:
            rc = L.lib.vmc_linear_wgrad_bias_tn(L.ptr(dy), L.ptr(x), L.ptr(C.buf), L.ptr(db.buf), M, N, K, dy.stride(0), x.stride(0), L.ptr(ws),
                                                nbytes, L.dt(dt), L.stream())
        else:
            rc = L.lib.vmc_linear_wgrad_tn(L.ptr(dy), L.ptr(x), L.ptr(C.buf), M, N, K, dy.stride(0), x.stride(0), L.ptr(ws), nbytes, L.dt(dt),
                                           L.stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        outs.append(("C" if with_b else "C-nobias",) + C.read())
        g, kept = db.read()
        outs.append(("dbias",) + (g[0], kept) if with_b else ("dbias-untouched", None, kept and bool((g == SENT).all())))
    return outs


def figures(c, dt, outs, fam=None):
    """The rule's figures for every output of one call, as plain records."""
    P = G.prepare(c, dt)
    recs = []
    for name, got, kept in outs:
        r = dict(family=fam or family(c), case=c["name"], dtype=G.DT_NAME[dt], output=name, sentinel_kept=bool(kept))
        if got is not None:
            o = P["outs"][name.split("-")[0]]
            m = G.judge(got, o)
            r.update(out_dtype=G.DT_NAME[o["dtype"]], **m)
        recs.append(r)
    return recs


def apply_rule(recs):
    """Print and record every figure, then assert."""
    bad = []
    for r in recs:
        if "ratio" in r:
            what = f"err {r['err']:.3e}" if "err" in r else f"outside {r['bad']} pinned {r['pinned']:.3f}"
            print(f"{r['family']} {r['case']} {r['dtype']} {r['output']}[{r['out_dtype']}]: {what} e32 {r['e32']:.3e} ratio {r['ratio']:.2f}")
        _REC.append(r)
        if not r["sentinel_kept"]:
            bad.append((r["case"], r["dtype"], r["output"], "an element outside the output was written"))
        if "ratio" in r and not (r["ratio"] <= G.MARGIN if "err" in r else r["bad"] == 0):
            bad.append((r["case"], r["dtype"], r["output"], {k: r[k] for k in ("err", "bad", "e32", "ratio") if k in r}))
    assert not bad, bad


def _ids(pairs):
    return [G.case_id(c, dt) for c, dt in pairs]


# ---------------------------------------------------------------------------------------------- the tests
_LINEAR = G.flat(G.LINEAR_CASES)
_EPI_SMALL, _EPI_G8 = G.flat(G.EPI_SMALL), G.flat(G.EPI_G8)
_SPLITK, _TN = G.flat(G.SPLITK_CASES), G.flat(G.TN_CASES)


@pytest.mark.parametrize("c,dt", _LINEAR, ids=_ids(_LINEAR))
def test_linear_kernels(c, dt):
    """One case per routed kernel: tile configurations 0-3, 6, 7, the one-tile 8-phase kernel, every persistent instantiation, the
    tail split (its seam rows under the same rule), the row maps, and f16 subnormal operands."""
    apply_rule(figures(c, dt, run_linear(c, dt)))


@pytest.mark.parametrize("c,dt", _EPI_SMALL, ids=_ids(_EPI_SMALL))
def test_linear_epilogue_matrix_small_tiles(c, dt):
    apply_rule(figures(c, dt, run_linear(c, dt)))


@pytest.mark.parametrize("c,dt", _EPI_G8, ids=_ids(_EPI_G8))
def test_linear_epilogue_matrix_8_phase(c, dt):
    apply_rule(figures(c, dt, run_linear(c, dt)))


@pytest.mark.parametrize("c,dt", _SPLITK, ids=_ids(_SPLITK))
def test_splitk(c, dt):
    apply_rule(figures(c, dt, run_splitk(c, dt)))


@pytest.mark.parametrize("c,dt", _TN, ids=_ids(_TN))
def test_wgrad_tn(c, dt):
    apply_rule(figures(c, dt, run_tn(c, dt)))


@pytest.mark.parametrize("dt", G.DT16, ids=[G.DT_NAME[d] for d in G.DT16])
def test_wgrad_tn_group(dt):
    """vmc_linear_wgrad_tn_group: four problems from one launch, with and without dbias, one as a column window."""
    from vimo_clip_amd import ops
    bufs, probs = [], []
    for c in G.GROUP_CASES:
        P = G.prepare(c, dt)
        dy, x, C, db = tn_buffers(c, P)
        assert ops.wgrad_group_ok(dy, x, C.buf[:c["N"]])
        bufs.append((C, db))
        probs.append((dy, x, C.buf, db.buf if c["dbias"] else None))
    ops.wgrad_tn_group(probs, dt)
    torch.cuda.synchronize()
    recs = []
    for c, (C, db) in zip(G.GROUP_CASES, bufs):
        g, kept = db.read()
        outs = [("C",) + C.read(), ("dbias", g[0], kept) if c["dbias"] else ("dbias-untouched", None, kept and bool((g == SENT).all()))]
        recs += figures(c, dt, outs, fam="TN_GROUP")
    apply_rule(recs)


@pytest.mark.parametrize("env", G.ENV_SETTINGS, ids=[f"{n}={v}" for n, v in G.ENV_SETTINGS])
def test_linear_under_a_switch_in_a_child_process(env):
    """VMC_GEMM_U=2 (configurations 4 and 8), VMC_GEMM_KS=1 (5 and 9), VMC_GEMM_CFG=1..11 (10-18, and 2 / 1 again)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), env[0], env[1]], env=dict(os.environ, **{env[0]: env[1]}),
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    recs = [json.loads(ln[len("FIGURES "):]) for ln in r.stdout.splitlines() if ln.startswith("FIGURES ")]
    want = sum(len(c["dts"]) for c in G.ENV_CASES if c["env"] == env)
    assert len(recs) == want, (len(recs), want, r.stdout[-2000:])
    apply_rule(recs)


def _child(name, value):
    """Run the cases of one switch setting (already in the environment) and print their figures; the parent judges them."""
    assert os.environ.get(name) == value
    _load()
    for c, dt in G.flat([c for c in G.ENV_CASES if c["env"] == (name, value)]):
        for r in figures(c, dt, run_linear(c, dt)):
            print("FIGURES " + json.dumps(r), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(sys.argv[1], sys.argv[2])
