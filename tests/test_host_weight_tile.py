"""CPU: the records, owner search and vector-path predicate of vimo_clip_amd/csrc/weight_tile.h (tests/host/test_weight_tile.cpp), and
the resource-usage remarks the Makefile keeps for elementwise.hip, where the three weight-copy kernels share one tile body."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_tile(tmp_path):
    exe = str(tmp_path / "test_weight_tile")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "test_weight_tile.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "OK" in out.stdout


def test_kernel_resource_usage_reports_no_scratch():
    """Both 16-bit types of cast_weight_kernel, cast_weights_multi_kernel and adam_cast_multi_kernel: no scratch, no spill, the one
    padded LDS tile, and the occupancy the separate bodies had (8 waves per SIMD for the casts, 4 for AdamW) or more."""
    path = os.path.join(ROOT, "vimo_clip_amd", "csrc", "build", "elementwise.usage.txt")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    blocks = re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]
    for kernel, occupancy in (("cast_weight_kernel", 8), ("cast_weights_multi_kernel", 8), ("adam_cast_multi_kernel", 4)):
        found = [b for b in blocks if kernel in b.split()[0]]
        assert len(found) == 2, kernel
        for b in found:
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0
            assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0
            assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 64 * 68 * 2
            assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= occupancy
