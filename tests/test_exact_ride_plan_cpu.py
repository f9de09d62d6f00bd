"""CPU: when the pruned exact sweep's counters ride in the result block (otters_amd/csrc/ott_exact_plan.h: prune_plan_ride).
The header is compiled on its own with the host compiler behind a small extern "C" driver, as test_exact_plan_cpu.py does: the
rule under test is the one libotters_hip.so ships.  The whole table over the rule's inputs is held to the sentences of the
header's comment, written out here by hand; a second build with -DOTT_X_RIDE=0 never plans it; and the rule is composed with
prune_plan_seed_est at the sizes where the estimate pass starts."""
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
using namespace ott;
extern "C" int xr_ride(unsigned long long est_rows, int E, int fetch, int merge_rank1, int merge_walk) {
    return prune_plan_ride(est_rows, E, fetch != 0, MergeOptions{merge_rank1, merge_walk != 0}) ? 1 : 0;
}
// the estimate pass's rows for a head-form plan of checkpoint 1 over `rows` rows, and whether the counters ride behind it
extern "C" void xr_chain(unsigned long long rows, int E, int head, int filtered, int fetch, unsigned long long* o) {
    const PruneIn in{768, 768, OTT_METRIC_COSINE, false, true, false, 0, 1, 1, SketchState{true, true, 4, 96, 1}, rows, E};
    const PrunePlan pp = prune_plan(in);
    const unsigned long long est = prune_plan_seed_est(in, pp, head != 0, filtered != 0);
    o[0] = est;
    o[1] = prune_plan_ride(est, E, fetch != 0, MergeOptions{-1, false}) ? 1 : 0;
}
"""


def build(tmp_path_factory, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp(name)
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR] + extra + [str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.xr_ride.argtypes, L.xr_ride.restype = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int], C.c_int
    L.xr_chain.argtypes, L.xr_chain.restype = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)], None
    return L


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build(tmp_path_factory, "ride_plan", [])


@pytest.fixture(scope="module")
def lib_off(tmp_path_factory):
    return build(tmp_path_factory, "ride_plan_off", ["-DOTT_X_RIDE=0"])


EST = (0, 64, 131072, 312512, 1 << 40)
ES = (1, 2, 4, 8)
RANK1 = (-1, 0, 1)
WALK = (0, 1)


def test_the_table(lib):
    """on exactly when the estimate pass runs, with one list entry per lane, on host output, and both merge options have their defaults"""
    on = 0
    for est, E, fetch, r1, walk in itertools.product(EST, ES, (0, 1), RANK1, WALK):
        want = est != 0 and E == 1 and fetch == 1 and r1 != 0 and walk == 0
        assert lib.xr_ride(est, E, fetch, r1, walk) == int(want), (est, E, fetch, r1, walk)
        on += want
    assert on == 4 * 2  # four estimate sizes x merge_rank1 in {-1, 1}


def test_rows_written_out_by_hand(lib):
    rows = [  # est_rows, E, fetch, merge_rank1, merge_walk -> riding
        ((312512, 1, 1, -1, 0), 1),  # the headline: 10M rows, k = 10
        ((131072, 1, 1, 1, 0), 1),
        ((131072, 1, 0, -1, 0), 0),  # device output: nobody reads the counters
        ((0, 1, 1, -1, 0), 0),       # no estimate pass: a filter, a small store, the full seed
        ((312512, 2, 1, -1, 0), 0),  # k > 64 (the estimate pass never runs there; the rule says so itself)
        ((312512, 1, 1, 0, 0), 0),   # force_fallback bit 2: round 2's merge for k <= 64
        ((312512, 1, 1, -1, 1), 0),  # force_fallback bit 1: lists merged by insertion
    ]
    for args, want in rows:
        assert lib.xr_ride(*args) == want, args


def test_the_experiment_switch_never_plans_it(lib_off):
    for est, E, fetch, r1, walk in itertools.product(EST, ES, (0, 1), RANK1, WALK):
        assert lib_off.xr_ride(est, E, fetch, r1, walk) == 0, (est, E, fetch, r1, walk)


def test_behind_the_estimate_pass(lib):
    """stores from 1 310 720 rows, head form, k <= 64, no score filter: the estimate pass, and on host output the riding counters"""
    o = (C.c_ulonglong * 2)()
    for rows, E, head, filtered, fetch, want_est in (
            (1_310_719, 1, 1, 0, 1, False), (1_310_720, 1, 1, 0, 1, True), (1_310_784, 1, 1, 0, 1, True), (10_000_000, 1, 1, 0, 1, True),
            (10_000_000, 1, 0, 0, 1, False), (10_000_000, 1, 1, 1, 1, False), (10_000_000, 2, 1, 0, 1, False), (10_000_000, 1, 1, 0, 0, True)):
        lib.xr_chain(rows, E, head, filtered, fetch, o)
        assert (o[0] != 0) == want_est, (rows, E, head, filtered, fetch, o[0])
        assert o[1] == int(want_est and fetch == 1), (rows, E, head, filtered, fetch, o[1])
    lib.xr_chain(10_000_000, 1, 1, 0, 1, o)
    assert o[0] == 312512
