"""Round 10 on the GPU: the run-time compiled pooled kernel forms a table index from a float in two instructions (detmath.hip.h:
clamp_index_of, v_cvt_u32_f32 + v_min_u32 with the bound as a literal) where it took three (v_cvt_i32_f32, v_mov_b32 of the bound,
v_med3_i32).  That both give clamp((int)f, 0, bound) for EVERY float rests on what the hardware's two conversions do with negative
values, NaN and values beyond the integer range, so it is tested, not argued: clsimhip_check_math_exhaustive(20) compares the two
forms on all 2^32 bit patterns x the bounds 0, 1, 0xa8, 0xaa, 0x1ff and 0x3fff on the device (index_clamp_check_kernel.hip)."""
import ctypes as C

import numpy as np
import pytest

from clsim_amd import _lib

pytestmark = pytest.mark.gpu


def test_two_instruction_clamp_equals_the_spelled_out_one_on_every_bit_pattern():
    lib = _lib.load()
    cap = 64
    res = np.zeros(cap, dtype=np.uint32)
    rc = lib.clsimhip_check_math_exhaustive(0, 20, 0, 0, res.ctypes.data_as(C.c_void_p), cap)
    assert rc == 0, lib.clsimhip_last_error(None)
    bad = int(res[0])
    first = res[1:1 + min(bad, cap - 1)]
    assert bad == 0, "%d mismatches, first arguments %s" % (bad, ["0x%08x (%s)" % (int(v), float.hex(float(np.uint32(v).view(np.float32))))
                                                                  for v in first[:8]])


def test_unknown_exhaustive_modes_are_still_refused():
    lib = _lib.load()
    res = np.zeros(4, dtype=np.uint32)
    for what in (14, 15, 21):
        assert lib.clsimhip_check_math_exhaustive(0, what, 0, 0, res.ctypes.data_as(C.c_void_p), 4) != 0
