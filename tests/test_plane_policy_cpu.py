"""CPU: the two format decisions of the cascade's planes (otters_amd/csrc/ott_plane_policy.h).  The header is compiled on its own
with the host compiler behind a small extern "C" driver, as test_query_policy_cpu.py does for ott_policy.h: the code under test
is the code libotters_hip.so ships.
  1. hi_plane_format against a transcription of the expressions ensure_hi_plane carried before the header existed (`parent_format`
     below, in float32), over every option value and the norms listed at NORMS, and against values written out by hand;
  2. format_rejected: more than 1 row in 64, in 64-bit arithmetic.
The function's input is the float bits of the smallest inverse norm, 1 / max_norm; `inv_bits` finds the bits whose reciprocal IS
the norm wanted.  Near 1e6 an ulp of the norm is half an ulp of its inverse, so not every norm has one: there the inverse's own
neighbours are walked, and both sides of the threshold must turn up among their reciprocals.
The GPU half: test_gpu_plane_lifecycle.py (both formats rejected on real stores)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include "ott_plane_policy.h"
extern "C" int pp_hi_format(int hi_fmt, unsigned bits, float* scale) {
    const ott::HiFormat f = ott::hi_plane_format(hi_fmt, bits);
    *scale = f.scale;
    return f.f16 ? 1 : 0;
}
extern "C" int pp_rejected(unsigned long long marked, unsigned long long converted) { return ott::format_rejected(marked, converted) ? 1 : 0; }
extern "C" float pp_i8_rel_flag() { return ott::I8_REL_FLAG; }
extern "C" float pp_half_rel_flag() { return ott::HALF_REL_FLAG; }
"""

f32 = np.float32
NO_REGULAR_ROW = 0x7F800000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("plane_policy")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.pp_hi_format.argtypes = [C.c_int, C.c_uint, C.POINTER(C.c_float)]
    L.pp_rejected.argtypes = [C.c_ulonglong, C.c_ulonglong]
    L.pp_i8_rel_flag.restype = C.c_float
    L.pp_half_rel_flag.restype = C.c_float
    return L


def hi_format(lib, hi_fmt, bits):
    scale = C.c_float(-1.0)
    f16 = lib.pp_hi_format(hi_fmt, int(bits), C.byref(scale))
    return bool(f16), float(scale.value)


def bits_of(x):
    return int(np.array(x, f32).view(np.uint32))


def from_bits(b):
    return np.array(b, np.uint32).view(f32)[()]


def parent_format(hi_fmt, got):
    """ensure_hi_plane's own lines: imgh_f16 = hi_fmt != 0; the store's smallest regular inverse norm -> max_norm -> the factor"""
    f16, scale = hi_fmt != 0, f32(1.0)
    if f16:
        min_inv = from_bits(got)
        with np.errstate(divide="ignore"):
            max_norm = f32(1.0) / min_inv if (got != NO_REGULAR_ROW and min_inv > 0.0) else f32(1.0)
        e = math.frexp(float(max_norm))[1] if math.isfinite(float(max_norm)) else 0  # max_norm = m * 2^e, m in [0.5, 1)
        scale = f32(math.ldexp(1.0, -int(e / 4)))  # (C's integer division truncates)
        if not (scale > 0.0) or not (scale < np.inf) or max_norm > f32(1e6) or max_norm < f32(1e-3):
            f16, scale = False, f32(1.0)
    return f16, float(scale)


def inv_bits(max_norm):
    """bits of an inverse norm whose float32 reciprocal is exactly max_norm (None: there is none)"""
    centre = bits_of(f32(1.0) / f32(max_norm))
    for b in range(centre - 4, centre + 5):
        if f32(1.0) / from_bits(b) == f32(max_norm):
            return b
    return None


def norms():
    out = [f32(2.0) ** e for e in range(-12, 23)]  # every power of two from 2^-12 to 2^22
    for edge in (f32(1e-3), f32(1e6)):
        out += [np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(np.inf))]
    return out


def test_hi_plane_format_is_the_parents(lib):
    cases = [NO_REGULAR_ROW, 0, bits_of(-0.25), bits_of(-0.0)]  # no regular row, zero, negative values: all count as a norm of 1
    reached = []
    for nm in norms():
        b = inv_bits(nm)
        if b is not None:
            cases.append(b)
            reached.append(float(nm))
    for e in range(-12, 23):
        assert 2.0 ** e in reached  # (a power of two always has its inverse)
    for edge in (f32(1e-3), f32(1e6)):  # the inverse's own neighbours around each threshold; their reciprocals land on both sides of it
        centre = bits_of(f32(1.0) / edge)
        around = list(range(centre - 8, centre + 9))
        sides = {bool(f32(1.0) / from_bits(b) > edge) for b in around} | {not bool(f32(1.0) / from_bits(b) < edge) for b in around}
        assert sides == {True, False}
        cases += around
    assert float(np.nextafter(f32(1e-3), f32(0))) in reached and float(np.nextafter(f32(1e-3), f32(1))) in reached
    for hi_fmt in (0, 1, 2, -1):
        for b in cases:
            assert hi_format(lib, hi_fmt, b) == parent_format(hi_fmt, b), (hi_fmt, hex(b), from_bits(b))


def test_hi_plane_format_by_hand(lib):
    for hi_fmt in (1, 2, -1):
        # max_norm = 1 = 0.5 * 2^1: factor 2^-(1 / 4) = 1.  A store without a regular row, or whose word reads zero or negative, counts as that
        for b in (inv_bits(1.0), NO_REGULAR_ROW, 0, bits_of(-3.0)):
            assert hi_format(lib, hi_fmt, b) == (True, 1.0)
        # max_norm = 1000 = 0.977 * 2^10: factor 2^-(10 / 4) = 2^-2 (the float32 nearest 1 / 1000 has the reciprocal 999.99994)
        b = bits_of(f32(1.0) / f32(1000.0))
        assert abs(float(f32(1.0) / from_bits(b)) - 1000.0) < 1e-3
        assert hi_format(lib, hi_fmt, b) == (True, 0.25)
        # max_norm = 1e6 = 0.954 * 2^20: factor 2^-5, and the last norm that takes half; an inverse a little smaller is a norm above 1e6: bf16
        centre, seen = bits_of(f32(1.0) / f32(1e6)), set()
        for b in range(centre - 8, centre + 9):
            half = bool(f32(1.0) / from_bits(b) <= f32(1e6))
            assert abs(float(f32(1.0) / from_bits(b)) - 1e6) < 2.0
            assert hi_format(lib, hi_fmt, b) == ((True, 0.03125) if half else (False, 1.0))
            seen.add(half)
        assert seen == {True, False}
        # below 1e-3: bf16; at 2^-9 = 0.00195 = 0.5 * 2^-8: factor 2^(8 / 4) = 4
        assert hi_format(lib, hi_fmt, inv_bits(2.0 ** -10)) == (False, 1.0)
        assert hi_format(lib, hi_fmt, inv_bits(2.0 ** -9)) == (True, 4.0)
        # an inverse norm so small that its reciprocal overflows
        assert hi_format(lib, hi_fmt, 1) == (False, 1.0)
    for b in (inv_bits(1.0), bits_of(1e-3), NO_REGULAR_ROW, 1):  # the store asks for bf16
        assert hi_format(lib, 0, b) == (False, 1.0)
    assert lib.pp_i8_rel_flag() == 2.0 ** -5 and lib.pp_half_rel_flag() == 2.0 ** -10


def test_format_rejected_is_more_than_one_row_in_64(lib):
    rej = lambda marked, converted: bool(lib.pp_rejected(marked, converted))  # noqa: E731
    assert not rej(0, 0)
    assert not rej(1, 64)
    assert rej(1, 63)
    assert not rej(2, 128)
    n = 3000
    assert not rej(n // 64, n)
    assert rej(n // 64 + 1, n)
    # the counts are 32-bit device words and rows of a store of up to 2^32 - 16: the product needs 64 bits
    top = 2 ** 32 - 1
    assert rej(top, top)
    assert not rej(2 ** 26, 2 ** 32) and rej(2 ** 26 + 1, 2 ** 32)
    assert not rej(2 ** 26 - 1, 2 ** 32 - 16) and rej(2 ** 26, 2 ** 32 - 16)
    assert not rej(top, 64 * top) and rej(top, 64 * top - 1)
