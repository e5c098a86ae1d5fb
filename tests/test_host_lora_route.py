"""CPU: vimo_clip_amd/csrc/lora_route.h (tests/host/test_lora_route.cpp, plain g++) and what the library answers from it without a
device: the workspace size of vmc_lora_wgrad_tn and the refusals of both entries, which come before any launch."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_ALIGN, E_SHAPE = -1, -2, -3


def test_lora_route(tmp_path):
    exe = str(tmp_path / "test_lora_route")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "test_lora_route.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "OK" in out.stdout


def test_workspace_bytes_is_the_plan():
    from vimo_clip_amd._lib import lib
    assert lib.vmc_lora_wgrad_tn_workspace_bytes(65, 64, 64) == 0                       # one slice: straight to out
    assert lib.vmc_lora_wgrad_tn_workspace_bytes(1100, 16, 136) == 5 * 16 * 136 * 4
    assert lib.vmc_lora_wgrad_tn_workspace_bytes(2500, 8, 520) == 10 * 8 * 520 * 4
    assert lib.vmc_lora_wgrad_tn_workspace_bytes(25600, 16, 768) == 80 * 16 * 768 * 4
    assert lib.vmc_lora_wgrad_tn_workspace_bytes(2500, 12, 520) == 0 == lib.vmc_lora_wgrad_tn_workspace_bytes(2500, 8, 516)


def test_refusals_need_no_device():
    """Host memory stands in for the operands: a refused call launches nothing, so nothing dereferences it.  Dtype code 9 is refused
    last of all (VMC_E_DTYPE), still before a launch: a call that passes every other check returns it."""
    from vimo_clip_amd._lib import lib
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def down(**kw):
        a = dict(x=p, ldx=128, a16=p, lda=128, out=p, ldo=192, M=4, K=128, r=16, col0=128)
        a.update(kw)
        return lib.vmc_lora_down_concat(a["x"], a["ldx"], a["a16"], a["lda"], a["out"], a["ldo"], a["M"], a["K"], a["r"], a["col0"], 1.0, 1, 9, None)

    def wgrad(**kw):
        a = dict(t=p, ldt=64, x=p, ldx=136, out=p, M=600, r=16, C=136, ws=p, wsb=1 << 20)
        a.update(kw)
        return lib.vmc_lora_wgrad_tn(a["t"], a["ldt"], a["x"], a["ldx"], a["out"], a["M"], a["r"], a["C"], 0, a["ws"], a["wsb"], 9, None)
    assert down() == -4 and wgrad() == -4
    for kw, want in ((dict(x=None), E_ARG), (dict(K=96), E_SHAPE), (dict(r=12), E_SHAPE), (dict(col0=120), E_SHAPE), (dict(ldo=184), E_SHAPE),
                     (dict(x=p + 2), E_ALIGN), (dict(lda=132), E_ALIGN)):
        assert down(**kw) == want, kw
    for kw, want in ((dict(out=None), E_ARG), (dict(ws=None), E_ARG), (dict(wsb=64), E_ARG), (dict(C=132), E_SHAPE), (dict(r=72), E_SHAPE),
                     (dict(ldt=8), E_SHAPE), (dict(t=p + 4), E_ALIGN), (dict(ldx=140), E_ALIGN)):
        assert wgrad(**kw) == want, kw
