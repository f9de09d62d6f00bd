"""CPU: candidate id lists (include/otters_hip.h: ott_query_ids, ott_store_score_rows) as far as they show
without a GPU — with_row_ids checks its list at validate(), resolve() carries it, a plan without a list is what it was, the
header declares the two calls (tests/test_abi_symbols.py and tests/test_rust_binding.py then hold the library and the crate to
it), the product library and the audit build export them, and their argument checks come before any device work."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from otters_amd import MetaStore, Metric, OttersError, VecQueryPlan, VecStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO = {
    "ott_query_ids": "int ott_query_ids(ott_store* s, const ott_query_desc* d, const uint64_t* ids, uint64_t n_ids, ott_hit* out, uint64_t cap, "
                     "uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);",
    "ott_store_score_rows": "int ott_store_score_rows(ott_store* s, const float* queries, uint32_t nq, uint32_t metric, const uint64_t* ids, "
                            "uint64_t n_ids, float* out_scores);",
}


def plan(ids=None):
    p = VecStore(4).query([1.0, 0.0, 0.0, 0.0], Metric.Cosine)
    return p if ids is None else p.with_row_ids(ids)


@pytest.mark.parametrize("bad", [[-1], [3, -7, 2], np.array([1.5]), [0.25, 1], ["a"], [True, False], [float("nan")], [float("inf")],
                                 np.array([2.0 ** 70])])
def test_with_row_ids_rejects_negative_and_non_integer_ids_at_validate(bad):
    p = plan(bad)  # the builder itself does not raise: errors surface at validate() / collect()
    with pytest.raises(OttersError):
        p.validate()
    with pytest.raises(OttersError):
        p.resolve()


@pytest.mark.parametrize("ids, want", [([3, 1, 1], [3, 1, 1]), ((5,), [5]), (np.array([7, 2], np.int32), [7, 2]), (range(3), [0, 1, 2]),
                                       (np.array([4.0, 0.0]), [4, 0]), ([], []), (np.array([2 ** 63 + 1], np.uint64), [2 ** 63 + 1])])
def test_resolve_carries_the_list_in_the_callers_order(ids, want):
    rq = plan(ids).resolve()
    assert rq.row_ids is not None and rq.row_ids.dtype == np.uint64 and rq.row_ids.flags["C_CONTIGUOUS"]
    assert rq.row_ids.tolist() == want


def test_a_plan_without_a_list_is_unchanged():
    rq = plan().resolve()
    assert rq.row_ids is None and rq.row_mask is None
    p = VecQueryPlan.new()
    assert p.row_ids is None
    # one plan object, used with and without a list: the list belongs to the plan that named it
    a, b = plan([1, 2]), plan()
    assert a.resolve().row_ids.tolist() == [1, 2] and b.resolve().row_ids is None
    assert callable(getattr(VecStore, "score_rows")) and callable(getattr(MetaStore, "query"))


def test_header_declares_the_two_calls_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for name, decl in TWO.items():
        assert re.sub(r"\s+", " ", decl) in flat, name
    assert "#define OTT_ABI_VERSION 4" in src
    assert '"id_gather"' in src  # the option is documented where the others are
    mk = open(os.path.join(ROOT, "otters_amd", "csrc", "Makefile")).read()
    assert "ott_gather.hip" in mk  # one source list for the product and the audit build


def test_library_exports_them_and_checks_arguments_without_a_device():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    for name in TWO:
        assert hasattr(L, name), name
    ids = np.array([0, 1], dtype=np.uint64)
    out = np.zeros(4, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)
    d = N.QueryDesc()
    assert L.ott_query_ids(None, C.byref(d), N.ptr(ids), 2, N.ptr(out), 4, C.byref(n_out), None, None) == -1
    assert b"NULL" in L.ott_last_error()
    sc = np.zeros(2, dtype=np.float32)
    q = np.zeros(4, dtype=np.float32)
    assert L.ott_store_score_rows(None, N.ptr(q), 1, 0, N.ptr(ids), 2, N.ptr(sc)) == -1
    assert b"ott_store_score_rows" in L.ott_last_error()


def test_audit_build_exports_them():
    csrc = os.path.join(ROOT, "otters_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-j", "8", "-s", "audit"])
    # (loaded in a child: two builds of one library do not belong in one process)
    code = "import ctypes, sys; A = ctypes.CDLL(sys.argv[1]); [getattr(A, n) for n in sys.argv[2:]]"
    subprocess.check_call([sys.executable, "-c", code, os.path.join(csrc, "libotters_hip_audit.so")] + list(TWO))
