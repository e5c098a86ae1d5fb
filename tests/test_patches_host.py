"""CPU: the argument checks of the six patch-extraction entries (include/vmc.h) answer in the order ARG, SHAPE, ALIGN, DTYPE and
before any launch.  The pointers are host memory and no stream is given: a launch on them would be an error of its own."""
import ctypes

import pytest

from vimo_clip_amd import _lib

VMC_E_ARG, VMC_E_ALIGN, VMC_E_SHAPE, VMC_E_DTYPE = -1, -2, -3, -4
_HOST = (ctypes.c_uint8 * 4096)()
_P = (ctypes.addressof(_HOST) + 15) & ~15           # 16-byte aligned

U8_ENTRIES = ("vmc_preprocess_patches_u8", "vmc_preprocess_patches_gray_u8", "vmc_patches_u8_exact", "vmc_patches_gray_u8_exact")
F32_ENTRIES = ("vmc_patches_f32", "vmc_patches_f32_split")
GOOD = dict(src=_P, dst=_P, F=1, R=56, p=14, kpad=640, dtype16=_lib.BF16)       # a shape WITH pad columns (588 -> 640)


def _call(entry, **changes):
    a = dict(GOOD, **changes)
    wrap = (0,) if entry in U8_ENTRIES else ()
    return getattr(_lib.lib, entry)(a["src"], a["dst"], a["F"], a["R"], a["p"], a["kpad"], *wrap, a["dtype16"], None)


CASES = {
    "null source": (dict(src=None), VMC_E_ARG),
    "null patches": (dict(dst=None), VMC_E_ARG),
    "F = 0": (dict(F=0), VMC_E_ARG),
    "p = 0": (dict(p=0), VMC_E_ARG),
    "R % p": (dict(R=60), VMC_E_SHAPE),
    "R % 4": (dict(R=42), VMC_E_SHAPE),
    "kpad < 3 p^2": (dict(kpad=576), VMC_E_SHAPE),
    "kpad % 8": (dict(kpad=644), VMC_E_SHAPE),
    "dtype16 = VMC_F32": (dict(dtype16=_lib.F32), VMC_E_DTYPE),
    "dtype16 unknown": (dict(dtype16=7), VMC_E_DTYPE),
    # the order of the checks
    "p = 0 and bad kpad": (dict(p=0, kpad=644), VMC_E_ARG),
    "bad kpad and unaligned": (dict(kpad=644, src=_P + 1), VMC_E_SHAPE),
    "unaligned and bad dtype": (dict(src=_P + 1, dtype16=7), VMC_E_ALIGN),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("entry", U8_ENTRIES + F32_ENTRIES)
def test_bad_arguments_answer_before_any_launch(entry, case):
    changes, want = CASES[case]
    assert _call(entry, **changes) == want


def test_source_alignment():
    for entry in U8_ENTRIES:             # 4-byte loads
        for off in (1, 2, 3):
            assert _call(entry, src=_P + off) == VMC_E_ALIGN, (entry, off)
    for entry in F32_ENTRIES:            # 16-byte loads: 4-aligned is not enough
        for off in (4, 8, 12):
            assert _call(entry, src=_P + off) == VMC_E_ALIGN, (entry, off)
