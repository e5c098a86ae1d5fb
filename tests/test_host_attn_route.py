"""CPU: the attention dispatch plans of vimo_clip_amd/csrc/attn_route.h (tests/host/test_attn_route.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attn_route(tmp_path):
    exe = str(tmp_path / "test_attn_route")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "test_attn_route.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "OK" in out.stdout
