"""GPU: vmc_lora_down_concat and vmc_lora_wgrad_tn (vimo_clip_amd/csrc/lora.hip) against the float64 references of tests/lora_refs.py
(the conditions on the cases themselves are asserted on the CPU by tests/test_lora_refs_host.py).

Guard bands as in DESIGN.md §5.2: operands with a padded leading dimension carry NaN in the padding, every output buffer is a whole
allocation pre-filled with a sentinel that must survive bit for bit wherever the call may not write (columns past col0 + 64, the two
rows after M, the first col0 columns when copy_x is off), the workspace is pre-filled with NaN."""
import pytest
import torch

import lora_refs as LR
from lora_refs import F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -1536.0
NAN = float("nan")
GUARD_ROWS = 2
E_ARG, E_ALIGN, E_SHAPE, E_DTYPE = -1, -2, -3, -4

_DOWN = [(c, dt) for c in LR.DOWN_CASES for dt in LR.DT16]
_WGRAD = [(c, dt, tr) for c in LR.WGRAD_CASES for dt in LR.DT16 for tr in (0, 1)]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vimo_clip_amd import _lib
    return _lib


def window(t, ld, col0=0):
    """t [rows, D] on the device as a column window of a whole [rows, ld] allocation whose other columns hold NaN."""
    rows, D = t.shape
    buf = torch.full((rows, ld), NAN, dtype=t.dtype)
    buf[:, col0:col0 + D] = t
    buf = buf.to(DEV)
    return buf[:, col0:col0 + D]


def sentinel_kept(cpu, written):
    """Everything outside the boolean mask `written` still holds the sentinel bit for bit."""
    iv = torch.int32 if cpu.dtype is F32 else torch.int16
    return bool((cpu.view(iv) == torch.full_like(cpu, SENT).view(iv))[~written].all())


def down_call(L, x, a, out, M, K, r, col0, s, copy_x, dt):
    rc = L.lib.vmc_lora_down_concat(L.ptr(x), x.stride(0), L.ptr(a), a.stride(0), L.ptr(out), out.stride(0), M, K, r, col0, float(s),
                                    int(copy_x), L.dt(dt), L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("c,dt", _DOWN, ids=[LR.case_id(c, dt) for c, dt in _DOWN])
def test_down_concat(L, c, dt):
    P = LR.down_prepared(c["name"], dt)
    M, K, r, s = c["M"], c["K"], c["r"], c["s"]
    a = window(P["a"], K + 8)
    # ---- copy_x on, x with ldx = K + 8 and NaN in the padding, col0 = K, 8 sentinel columns behind the tail
    x = window(P["x"], K + 8)
    out = torch.full((M + GUARD_ROWS, K + 64 + 8), SENT, dtype=dt, device=DEV)
    assert down_call(L, x, a, out, M, K, r, K, s, 1, dt) == 0
    cpu = out.cpu()
    m, bad = LR.check_down(c, dt, cpu[:M, :K + 64].contiguous())
    print(f"down {LR.case_id(c, dt)}: outside {m['bad']} pinned {m['pinned']:.3f} e32 {m['e32']:.3e} ratio {m['ratio']:.2f}")
    written = torch.zeros(cpu.shape, dtype=torch.bool)
    written[:M, :K + 64] = True
    assert not bad, bad
    assert sentinel_kept(cpu, written), "an element outside [M, K + 64] was written"
    # ---- copy_x off, contiguous x, col0 = K + 8: only the 64 tail columns are written
    x2 = P["x"].to(DEV)
    out2 = torch.full((M + GUARD_ROWS, K + 8 + 64 + 8), SENT, dtype=dt, device=DEV)
    assert down_call(L, x2, a, out2, M, K, r, K + 8, s, 0, dt) == 0
    cpu2 = out2.cpu()
    written = torch.zeros(cpu2.shape, dtype=torch.bool)
    written[:M, K + 8:K + 8 + 64] = True
    assert sentinel_kept(cpu2, written), "copy_x = 0 wrote outside the tail columns"
    assert torch.equal(cpu2[:M, K + 8:K + 8 + 64].view(torch.int16), cpu[:M, K:K + 64].view(torch.int16)), "the tail depends on copy_x / col0"


def test_down_concat_refuses_bad_arguments_before_a_launch(L):
    dt = torch.bfloat16
    M, K, r = 16, 128, 16
    x = torch.zeros((M, K + 8), dtype=dt, device=DEV)
    a = torch.zeros((64, K + 8), dtype=dt, device=DEV)
    out = torch.full((M, K + 128), SENT, dtype=dt, device=DEV)

    def call(xp=None, ap=None, op=None, ldx=K + 8, lda=K + 8, ldo=K + 128, M=M, K=K, r=r, col0=K, dtype=None):
        return L.lib.vmc_lora_down_concat(L.ptr(x) if xp is None else xp, ldx, L.ptr(a) if ap is None else ap, lda,
                                          L.ptr(out) if op is None else op, ldo, M, K, r, col0, 1.0, 1, L.dt(dt) if dtype is None else dtype,
                                          L.stream())
    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(SENT)
    for kw, want in ((dict(K=96), E_SHAPE), (dict(r=12), E_SHAPE), (dict(r=0), E_SHAPE), (dict(r=72), E_SHAPE), (dict(M=0), E_SHAPE),
                     (dict(col0=K - 8), E_SHAPE), (dict(col0=K + 4), E_SHAPE), (dict(ldo=K + 56), E_SHAPE), (dict(ldx=K - 8), E_SHAPE),
                     (dict(xp=L.ptr(x) + 2), E_ALIGN), (dict(ap=L.ptr(a) + 8), E_ALIGN), (dict(op=L.ptr(out) + 4), E_ALIGN),
                     (dict(ldx=K + 4), E_ALIGN), (dict(lda=K + 2), E_ALIGN), (dict(ldo=K + 132), E_ALIGN), (dict(xp=0), E_ARG),
                     (dict(op=0), E_ARG), (dict(dtype=0), E_DTYPE)):
        assert call(**kw) == want, (kw, want)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote its output"


def wgrad_call(L, t, x, out, M, r, C, tr, ws, nbytes, dt):
    rc = L.lib.vmc_lora_wgrad_tn(L.ptr(t), t.stride(0), L.ptr(x), x.stride(0), L.ptr(out), M, r, C, tr, L.ptr(ws), nbytes, L.dt(dt), L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("c,dt,tr", _WGRAD, ids=[LR.case_id(c, dt) + ("-T" if tr else "") for c, dt, tr in _WGRAD])
def test_wgrad_tn(L, c, dt, tr):
    P = LR.wgrad_prepared(c["name"], dt)
    M, r, C = c["M"], c["r"], c["C"]
    # t and x as the strided views the training step passes: the 64-column tail of [M, N + 64] and the first C columns of [M, C + 64]
    t = window(P["t"], 72 + 64, 72)
    x = window(P["x"], C + 64)
    nbytes = L.lib.vmc_lora_wgrad_tn_workspace_bytes(M, r, C)
    rows, cols = (C, r) if tr else (r, C)
    got = []
    for _ in range(2):
        ws = torch.full((nbytes // 4,), NAN, dtype=F32, device=DEV) if nbytes else None
        out = torch.full((rows + GUARD_ROWS, cols), SENT, dtype=F32, device=DEV)
        assert wgrad_call(L, t, x, out, M, r, C, tr, ws, nbytes, dt) == 0
        got.append(out.cpu())
    written = torch.zeros(got[0].shape, dtype=torch.bool)
    written[:rows] = True
    assert sentinel_kept(got[0], written), "a row behind the output was written"
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), "two calls gave different bits"
    res = got[0][:rows].t() if tr else got[0][:rows]
    m = LR.measure32(res, P["r64"], P["e32"])
    print(f"wgrad {LR.case_id(c, dt)}{' T' if tr else ''} ({c['purpose']}): err {m['err']:.3e} e32 {m['e32']:.3e} ratio {m['ratio']:.2f}")
    assert m["ok"], m


def test_wgrad_tn_refuses_bad_arguments_before_a_launch(L):
    dt = torch.float16
    M, r, C = 600, 16, 136
    t = torch.zeros((M, 64), dtype=dt, device=DEV)
    x = torch.zeros((M, C + 8), dtype=dt, device=DEV)
    out = torch.full((r, C), SENT, dtype=F32, device=DEV)
    nbytes = L.lib.vmc_lora_wgrad_tn_workspace_bytes(M, r, C)
    assert nbytes > 0 and L.lib.vmc_lora_wgrad_tn_workspace_bytes(M, 12, C) == 0
    ws = torch.empty(nbytes // 4, dtype=F32, device=DEV)

    def call(tp=None, xp=None, ldt=64, ldx=C + 8, M=M, r=r, C=C, wsp=None, wsb=nbytes, dtype=None):
        return L.lib.vmc_lora_wgrad_tn(L.ptr(t) if tp is None else tp, ldt, L.ptr(x) if xp is None else xp, ldx, L.ptr(out), M, r, C, 0,
                                       L.ptr(ws) if wsp is None else wsp, wsb, L.dt(dt) if dtype is None else dtype, L.stream())
    for kw, want in ((dict(r=12), E_SHAPE), (dict(r=72), E_SHAPE), (dict(C=132), E_SHAPE), (dict(M=0), E_SHAPE), (dict(ldx=C - 8), E_SHAPE),
                     (dict(ldt=8), E_SHAPE), (dict(tp=L.ptr(t) + 2), E_ALIGN), (dict(ldx=C + 4), E_ALIGN), (dict(xp=0), E_ARG),
                     (dict(wsp=0), E_ARG), (dict(wsb=nbytes - 4), E_ARG), (dict(dtype=0), E_DTYPE)):
        assert call(**kw) == want, (kw, want)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote its output"
