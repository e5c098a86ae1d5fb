"""CPU: the resource-usage remarks the Makefile keeps for layernorm.hip, where ln_fwd_kernel, add_ln_kernel and postnorm_kernel share
the row body of vimo_clip_amd/csrc/ln_row.h.  Every instantiation, both 16-bit types: no scratch, no spill, and at least the
occupancy (waves per SIMD) the separate bodies had (profiles/ln_row_body.md)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> {float4 chunks per lane: occupancy before the shared body}; None: an instantiation that did not exist then, held to
# the occupancy of the next larger chunk count of the same kernel
BEFORE = {
    "ln_fwd_kernel": {2: 8, 3: 5, 4: 4, 8: 2, 16: 1},
    "add_ln_kernel": {1: 8, 2: 8, 3: 7, 4: 5, 5: 4, 6: 4, 7: None, 8: 3},
    "postnorm_kernel": {1: 8, 2: 6, 3: 5, 4: 4, 5: None, 6: 3, 7: None, 8: 3},
    "ln_bwd_kernel": {2: 3, 3: 2, 4: 2, 8: 1},
}


@pytest.fixture(scope="module")
def usage():
    """{(kernel, 16-bit type or None, chunks or None): the remark block of that instantiation}"""
    path = os.path.join(ROOT, "vimo_clip_amd", "csrc", "build", "layernorm.usage.txt")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]:
        name = b.split()[0]
        m = re.match(r"_Z\d+(\w+_kernel)I\d+(BF16|F16)Li(\d+)E", name)            # _Z13add_ln_kernelI4BF16Li3EEv...
        key = (m.group(1), m.group(2), int(m.group(3))) if m else (re.match(r"_Z\d+(\w+_kernel)", name).group(1), None, None)
        assert key not in out, name
        out[key] = b
    return out


def field(block, name):
    return int(re.search(re.escape(name) + r": (\d+)", block).group(1))


def test_every_instantiation_is_reported(usage):
    want = {(k, t, n) for k, per in BEFORE.items() for n in per for t in ("BF16", "F16")} | {("ln_reduce_strided_kernel", None, None)}
    assert set(usage) == want


def test_no_scratch_no_spill(usage):
    for key, b in usage.items():
        assert field(b, "ScratchSize [bytes/lane]") == 0, key
        assert field(b, "SGPRs Spill") == 0 and field(b, "VGPRs Spill") == 0, key


def test_occupancy_not_below_the_separate_bodies(usage):
    assert field(usage[("ln_reduce_strided_kernel", None, None)], "Occupancy [waves/SIMD]") >= 8
    for kernel, per in BEFORE.items():
        for t in ("BF16", "F16"):
            occ = {n: field(usage[(kernel, t, n)], "Occupancy [waves/SIMD]") for n in per}
            for n, before in per.items():
                floor = occ[min(m for m in per if m > n)] if before is None else before
                assert occ[n] >= floor, (kernel, t, n, occ[n], floor)
