"""CPU: when the pruned sweep takes the head form of the four-bit sketch (otters_amd/csrc/ott_exact_plan.h: prune_plan_head; DESIGN.md
3.1b, "no f32 stage in front").  The header is compiled on its own with the host compiler, as in test_exact_plan_cpu.py.  The head
form runs exactly when the plan is the four-bit sketch form, the quantiser accepted the query, the store's head covers every row and
the option exact_sketch_head is not 0 — a table over all of these — and the list has at most four entries per lane (k <= 256); it changes nothing of the plan itself: checkpoint, form and
seed are prune_plan's."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include "ott_exact_plan.h"
#include "ott_prune.h"
using namespace ott;
// a store of `rows` rows x dim that keeps a sketch of `bits` bits for every row (sk_covers) and a head as told; exact_prune as given.
// o: c, sketch, seed of the plan the call takes (after the quantiser's answer); returns the head decision
extern "C" int head_plan(unsigned dim, unsigned long long rows, unsigned bits, int sk_covers, int exact_prune, int present, int covers, int option, int quant_ok,
                         int E, unsigned long long* o) {
    const unsigned ld = (dim + 3) / 4 * 4, nst = (ld + 31) / 32, s0 = prune_sketchb_stage0(nst, bits);
    const PruneIn in{dim, ld, OTT_METRIC_COSINE, false, true, false, 0, exact_prune, 1, SketchState{true, sk_covers != 0, bits, bits * (nst - s0), s0}, rows, E};
    PrunePlan pp = prune_plan(in);
    if (prune_plan_needs_quant(in, pp) && !quant_ok) pp = prune_plan_quant_refused(in);
    o[0] = pp.c; o[1] = pp.sketch; o[2] = pp.seed;
    return prune_plan_head(in, pp, quant_ok != 0, HeadState{present != 0, covers != 0, option});
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("planhead")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.head_plan.argtypes = [C.c_uint, C.c_ulonglong, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    L.head_plan.restype = C.c_int
    return L


def plan(lib, dim=768, rows=1 << 21, bits=4, sk_covers=1, exact_prune=-1, present=1, covers=1, option=-1, quant_ok=1, E=1):
    o = (C.c_ulonglong * 3)()
    head = lib.head_plan(dim, rows, bits, sk_covers, exact_prune, present, covers, option, quant_ok, E, o)
    return bool(head), (int(o[0]), int(o[1]), int(o[2]))


def test_the_table(lib):
    """head present or not x covering every row or not x option -1 / 0 / 1 x bits 1 / 3 / 4 x the quantiser refusing or accepting"""
    n = 0
    for present, covers, option, bits, quant_ok in itertools.product((0, 1), (0, 1), (-1, 0, 1), (1, 3, 4), (0, 1)):
        head, pp = plan(lib, bits=bits, present=present, covers=covers, option=option, quant_ok=quant_ok)
        want = bool(present and covers and option != 0 and bits == 4 and quant_ok)
        assert head == want, (present, covers, option, bits, quant_ok, head, pp)
        # the plan itself does not depend on the head: the same store without one
        assert pp == plan(lib, bits=bits, present=0, covers=0, option=0, quant_ok=quant_ok)[1]
        if bits == 4:  # stage 1 and the small seed with the quantiser's yes, the 7/8 form and the tenth with its no
            assert pp == ((1, 1, 131072) if quant_ok else (21, 0, ((1 << 21) // 10 + 63) // 64 * 64)), pp
        n += 1
    assert n == 72


@pytest.mark.parametrize("dim", [225, 256, 768, 773, 896])
def test_every_dim_of_a_four_bit_store(lib, dim):
    assert plan(lib, dim=dim) == (True, (1, 1, 131072))
    assert plan(lib, dim=dim, option=0) == (False, (1, 1, 131072))


def test_list_widths(lib):
    """up to four list entries per lane (k <= 256) take the head form; eight (k <= 512) keep the c = 1 form: the head kernel runs one
    wave per SIMD there and measured slower.  The seed follows prune_plan's own rule for the longer lists: the tenth"""
    tenth = ((1 << 21) // 10 + 63) // 64 * 64
    for E, want in ((1, True), (2, True), (4, True), (8, False)):
        assert plan(lib, E=E) == (want, (1, 1, 131072 if E == 1 else tenth)), E


def test_no_head_form_without_the_four_bit_plan(lib):
    """lines that do not cover every row, a store too small for the automatic sweep, the sweep switched off: no plan, no head form"""
    assert plan(lib, sk_covers=0) == (False, (21, 0, ((1 << 21) // 10 + 63) // 64 * 64))
    assert plan(lib, rows=20_000) == (False, (0, 0, 0))
    assert plan(lib, rows=20_000, exact_prune=1) == (True, (1, 1, 2048))
    assert plan(lib, exact_prune=0) == (False, (0, 0, 0))
