"""CPU: the host side of MaxSim re-ranking over a listed set of groups (VecQueryPlan.with_groups, ott_query_maxsim_groups; DESIGN.md
3.1h) — the plan's refusals and label mapping, what resolve() carries, the header's prototype and option, the symbol in both builds
of the library with its argument checks before any device work, and the plan header (otters_amd/csrc/ott_maxsim_gather_plan.h)
compiled on its own with the host compiler and held to a plain Python restatement over a grid, as test_sort_plan_cpu.py holds
ott_sort_plan.h.  The GPU half: test_gpu_maxsim_groups.py, test_gpu_maxsim_groups_concurrent.py."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from otters_amd import Metric, Mode, OttersError, Path, VecQueryPlan, VecStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")

PROTOTYPE = ("int ott_query_maxsim_groups(ott_store* s, const ott_query_desc* d, const void* groups, uint64_t n_groups_listed, ott_hit* out, "
             "uint64_t cap, uint64_t* n_out, ott_stats* stats);")


# ---- plans --------------------------------------------------------------------------------------------------------------------

def host_store(labels=None):
    store = VecStore(4)
    store._n, store._n_groups = 100, 7  # (no GPU: lengths as set_groups would leave them)
    if labels is not None:
        store._group_labels = np.unique(np.asarray(labels))
        store._n_groups = int(store._group_labels.size)
    return store


Q = np.eye(4, dtype=np.float32)[:3]


def test_with_groups_refusals_at_validate():
    store = host_store()
    with pytest.raises(OttersError, match="with_groups cannot be combined with one_per_group in this version; use with_row_mask"):
        store.query(Q[:1], Metric.Cosine).one_per_group().with_groups([1]).validate()
    with pytest.raises(OttersError, match="with_groups cannot be combined with per_group in this version; use with_row_mask"):
        store.query(Q[:1], Metric.Cosine).per_group(2).with_groups([1]).validate()
    with pytest.raises(OttersError, match="with_groups cannot be combined with with_row_ids in this version; use with_row_mask"):
        store.query(Q, Metric.Cosine).with_groups([1]).with_row_ids([3]).validate()
    with pytest.raises(OttersError, match="with_groups needs max_sim in this version; use with_row_mask"):
        store.query(Q, Metric.Cosine).with_groups([1]).validate()
    store.query(Q, Metric.Cosine).max_sim().with_groups([1]).with_row_mask(np.ones(100, bool)).validate()
    # the refusals that were there stay word for word
    with pytest.raises(OttersError, match="^max_sim cannot be combined with with_row_ids in this version; use with_row_mask$"):
        store.query(Q, Metric.Cosine).max_sim().with_row_ids([1, 2]).validate()
    with pytest.raises(OttersError, match="^one_per_group cannot be combined with with_row_ids in this version; use with_row_mask$"):
        store.query(Q[:1], Metric.Cosine).one_per_group().with_row_ids([1, 2]).validate()
    with pytest.raises(OttersError, match="^per_group cannot be combined with with_row_ids in this version; use with_row_mask$"):
        store.query(Q[:1], Metric.Cosine).per_group(2).with_row_ids([1, 2]).validate()
    with pytest.raises(OttersError, match="group labels must be integers"):
        store.query(Q, Metric.Cosine).max_sim().with_groups([1.5]).validate()


def test_labels_map_through_the_stores_sorted_labels():
    labels = np.array([40, -3, 40, 7, 7, 2 ** 40], dtype=np.int64)  # dense: -3 -> 0, 7 -> 1, 40 -> 2, 2^40 -> 3
    store = host_store(labels)
    rq = store.query(Q, Metric.Cosine).max_sim().with_groups([2 ** 40, -3, 40, -3, 40]).resolve()
    assert rq.group_list.dtype == np.uint32 and rq.group_list.flags["C_CONTIGUOUS"]
    assert rq.group_list.tolist() == [3, 0, 2, 0, 2]      # the caller's order, duplicates kept: the library sorts and dedupes
    assert rq.k == 3 and rq.max_sim                       # the default take: the distinct listed groups
    assert store.query(Q, Metric.Cosine).max_sim().with_groups([7, 7]).take(5).resolve().k == 5
    for unknown in (8, -4, 2 ** 41, 0):
        with pytest.raises(OttersError, match=f"no row carries the group label {unknown}$"):
            store.query(Q, Metric.Cosine).max_sim().with_groups([7, unknown]).validate()
    rq = store.query(Q, Metric.Cosine).max_sim().with_groups([]).resolve()
    assert rq.group_list.size == 0 and rq.k == 0
    rq = store.query(Q, Metric.Cosine).max_sim().with_groups(np.array([7], np.uint8)).resolve()
    assert rq.group_list.tolist() == [1]


def test_dense_ids_are_their_own_labels():
    store = host_store()  # _set_dense_groups: 7 groups, no labels
    rq = store.query(Q, Metric.Euclidean).max_sim().with_groups([6, 0, 6]).take(2).resolve()
    assert rq.group_list.tolist() == [6, 0, 6] and rq.k == 2 and rq.take == 0
    for bad in (7, -1):
        with pytest.raises(OttersError, match=f"group {bad} is not one of the store's 7 groups"):
            store.query(Q, Metric.Cosine).max_sim().with_groups([1, bad]).validate()


def test_a_plan_without_a_list_resolves_to_what_it_did():
    store = host_store()
    rq = store.query(Q, Metric.Cosine).max_sim().resolve()
    assert rq.group_list is None and rq.max_sim and rq.k == 7 and rq.mode == int(Mode.Merged) and rq.path == int(Path.Auto)
    rq = store.query(Q, Metric.Cosine).take(3).resolve()
    assert rq.group_list is None and not rq.max_sim and rq.k == 3
    assert store.query(Q, Metric.Cosine).resolve().k == 100
    assert store.query(Q[:1], Metric.Cosine).one_per_group().resolve().k == 7
    assert VecQueryPlan.new().group_list is None


# ---- the header and the library -------------------------------------------------------------------------------------------------

def test_header_declares_the_call_and_the_option_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert "#define OTT_ABI_VERSION 4" in src
    assert '"group_gather"' in src and "OTT_GROUP_GATHER" in src  # documented where "id_gather" is
    assert src.index('"id_gather"') < src.index('"group_gather"') < src.index('"large_k_from"')
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ott_maxsim_gather.hip" in mk  # one source list for the product and the audit build


def test_library_exports_it_and_refuses_before_any_device_work():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    assert hasattr(L, "ott_query_maxsim_groups") and hasattr(L, "ott_store_group_index_builds")
    out = np.zeros(4, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)
    q = np.zeros(8, np.float32)
    g = np.array([0, 1], np.uint32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, 2, int(Metric.Cosine), 1, 4
    d.mode = int(Mode.PerQuery)
    assert L.ott_query_maxsim_groups(None, C.byref(d), N.ptr(g), 2, N.ptr(out), 4, C.byref(n_out), None) == -4
    assert b"ott_query_maxsim_groups: the query vectors are the tokens of ONE query" in L.ott_last_error()
    d.mode, d.path = int(Mode.Merged), int(Path.Mfma)
    assert L.ott_query_maxsim_groups(None, C.byref(d), N.ptr(g), 2, N.ptr(out), 4, C.byref(n_out), None) == -4
    assert b"ott_query_maxsim_groups: the MFMA path does not serve late-interaction" in L.ott_last_error()
    d.path = int(Path.Auto)
    assert L.ott_query_maxsim_groups(None, C.byref(d), N.ptr(g), 2, N.ptr(out), 4, C.byref(n_out), None) == -1
    assert b"ott_query_maxsim_groups: store is NULL" in L.ott_last_error()
    assert n_out.value == 9  # nothing was touched
    assert L.ott_store_group_index_builds(None) == 0
    assert L.ott_store_set_option(None, b"group_gather", 1) != 0 and b"NULL" in L.ott_last_error()


def test_audit_build_exports_it():
    subprocess.check_call(["make", "-C", CSRC, "-j", "8", "-s", "audit"])
    # (loaded in a child: two builds of one library do not belong in one process)
    code = "import ctypes, sys; A = ctypes.CDLL(sys.argv[1]); [getattr(A, n) for n in sys.argv[2:]]"
    subprocess.check_call([sys.executable, "-c", code, os.path.join(CSRC, "libotters_hip_audit.so"), "ott_query_maxsim_groups", "ott_store_group_index_builds"])


# ---- the plan header ----------------------------------------------------------------------------------------------------------------

DRIVER = r"""
#include "ott_maxsim_gather_plan.h"
using namespace ott;
extern "C" void mg_consts(unsigned long long* o) {
    o[0] = MG_WAVES; o[1] = MG_STEP_ROWS; o[2] = MG_DIMQ_MAX; o[3] = MG_PAD; o[4] = MG_LDS_MAX; o[5] = MG_TABLE_MAX; o[6] = MG_INDEX_MAX_GROUPS;
    o[7] = MG_MAX_SLOTS; o[8] = MG_MAX_ROWS; o[9] = MG_AUTO_MAX_ROWS;
}
extern "C" unsigned mg_cap(unsigned dimq) { return mg_tokens_cap(dimq); }
extern "C" unsigned mg_nt(unsigned dimq, unsigned nq) { return mg_tokens_per_pass(dimq, nq); }
extern "C" unsigned mg_np(unsigned dimq, unsigned nq) { return mg_passes(dimq, nq); }
extern "C" unsigned long long mg_lds(unsigned dimq, unsigned nt) { return mg_lds_bytes(dimq, nt); }
extern "C" unsigned long long mg_table(unsigned nq, unsigned long long n_slots, unsigned passes) { return mg_table_bytes(nq, n_slots, passes); }
extern "C" unsigned long long mg_keys(unsigned long long n_slots) { return mg_key_bytes(n_slots); }
extern "C" int mg_fits(unsigned nq, unsigned n_groups) { return mg_sweep_table_fits(nq, n_groups) ? 1 : 0; }
extern "C" int mg_wants(int multi, int mfma, unsigned dimq, int opt) { return mg_wants_index(multi != 0, mfma != 0, dimq, opt) ? 1 : 0; }
extern "C" int mg_gather(int wants, int have, int opt, unsigned long long n_slots, unsigned long long rows) { return mg_takes_gather(wants != 0, have != 0, opt, n_slots, rows) ? 1 : 0; }
// gid / start / count: room for n_listed entries; returns the number of slots, *rows = the listed rows
extern "C" unsigned long long mg_slot_arrays(const unsigned* groups, unsigned long long n_listed, unsigned n_groups, const unsigned* starts, unsigned* gid, unsigned* start,
                                             unsigned* count, unsigned long long* rows) {
    MgSlots sl;
    mg_slots(groups, n_listed, n_groups, starts, sl);
    if (starts && (sl.start.size() != sl.gid.size() || sl.count.size() != sl.gid.size())) return ~0ull;
    if (!starts && (!sl.start.empty() || !sl.count.empty())) return ~0ull;
    for (size_t i = 0; i < sl.gid.size(); i++) { gid[i] = sl.gid[i]; if (starts) { start[i] = sl.start[i]; count[i] = sl.count[i]; } }
    *rows = sl.rows;
    return sl.gid.size();
}
"""

DIMQS = (8, 16, 128, 504, 512, 520, 1024, 1032, 2048, 2056, 4096)
NQS = (1, 3, 8, 9, 16, 17, 32, 33, 64, 65, 1000)


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("maxsim_gather_plan")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    up, ullp, ull, u, i = C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong), C.c_ulonglong, C.c_uint, C.c_int
    for name, args, res in (("mg_consts", [ullp], None), ("mg_cap", [u], u), ("mg_nt", [u, u], u), ("mg_np", [u, u], u), ("mg_lds", [u, u], ull),
                            ("mg_table", [u, ull, u], ull), ("mg_keys", [ull], ull), ("mg_fits", [u, u], i), ("mg_wants", [i, i, u, i], i),
                            ("mg_gather", [i, i, i, ull, ull], i), ("mg_slot_arrays", [up, ull, u, up, up, up, up, ullp], ull)):
        f = getattr(L, name)
        f.argtypes, f.restype = args, res
    return L


def consts(L):
    o = (C.c_ulonglong * 10)()
    L.mg_consts(o)
    return dict(zip(("waves", "step_rows", "dimq_max", "pad", "lds_max", "table_max", "index_max_groups", "max_slots", "max_rows", "auto_max_rows"), list(o)))


# the restatement: DESIGN.md 3.1h in plain Python
def py_cap(dimq):
    return 32 if dimq <= 512 else 16 if dimq <= 1024 else 8 if dimq <= 2048 else 0


def py_tokens_per_pass(dimq, nq):
    """the narrowest of 8, 16, 32 that holds the query, no wider than the dim allows"""
    for w in (8, 16, 32):
        if w >= py_cap(dimq) or w >= nq:
            return min(w, py_cap(dimq))
    return py_cap(dimq)


def test_constants_and_the_lds_they_imply(plan_lib):
    k = consts(plan_lib)
    assert k["waves"] == 4 and k["step_rows"] == 32 and k["dimq_max"] == 2048 and k["pad"] == 4
    assert k["table_max"] == 2 ** 31 and k["index_max_groups"] == 2 ** 26 and k["max_slots"] == 2 ** 24 and k["max_rows"] == 2 ** 30
    # the token floats themselves stay within 64 KB at every width; with the padding and the two small arrays the kernel's opt-in covers all
    for dimq, nt in ((512, 32), (1024, 16), (2048, 8)):
        assert dimq * nt * 4 == 65536
        assert plan_lib.mg_lds(dimq, nt) == (dimq * (nt + 4) + nt + 4 * nt) * 4 <= k["lds_max"] <= 160 * 1024
    assert plan_lib.mg_lds(128, 32) == 128 * 36 * 4 + 32 * 4 + 4 * 32 * 4  # a ColBERT-sized query: 19 072 B


def test_tokens_per_pass_and_passes_over_the_grid(plan_lib):
    for dimq, nq in itertools.product(DIMQS, NQS):
        nt = py_tokens_per_pass(dimq, nq)
        assert plan_lib.mg_cap(dimq) == py_cap(dimq), dimq
        assert plan_lib.mg_nt(dimq, nq) == nt, (dimq, nq)
        assert plan_lib.mg_np(dimq, nq) == (0 if nt == 0 else -(-nq // nt)), (dimq, nq)
        if nt:
            assert plan_lib.mg_lds(dimq, nt) == (dimq * (nt + 4) + 5 * nt) * 4
    # the cases the GPU tests name
    assert (plan_lib.mg_nt(40, 33), plan_lib.mg_np(40, 33)) == (32, 2)
    assert (plan_lib.mg_nt(520, 17), plan_lib.mg_np(520, 17)) == (16, 2)
    assert (plan_lib.mg_nt(1032, 9), plan_lib.mg_np(1032, 9)) == (8, 2)
    assert plan_lib.mg_nt(2056, 3) == 0
    assert (plan_lib.mg_nt(128, 32), plan_lib.mg_np(128, 32)) == (32, 1)  # 32 x 128: every listed row is read once
    assert (plan_lib.mg_nt(128, 3), plan_lib.mg_np(128, 3)) == (8, 1)


def test_table_bytes_and_the_2_gib_refusal(plan_lib):
    for nq, n_slots in itertools.product(NQS, (0, 1, 100, 50_000, 2 ** 24)):
        for passes in (1, 2, 5):
            assert plan_lib.mg_table(nq, n_slots, passes) == (nq * n_slots * 4 if passes > 1 else 0), (nq, n_slots, passes)
        assert plan_lib.mg_keys(n_slots) == 8 * n_slots
    for nq, ng in itertools.product(NQS, (1, 1000, 2 ** 24, 2 ** 26, 2 ** 29, 2 ** 30, 2 ** 32 - 1)):
        assert plan_lib.mg_fits(nq, ng) == (1 if nq * ng * 4 <= 2 ** 31 else 0), (nq, ng)
    assert plan_lib.mg_fits(1, 2 ** 29) == 1 and plan_lib.mg_fits(3, 2 ** 30) == 0 and plan_lib.mg_fits(32, 2 ** 24) == 1 and plan_lib.mg_fits(33, 2 ** 24) == 0
    # a gather table never needs more than the sweep's: the listed slots are at most the store's groups, so only the mask route refuses


def test_route_over_the_grid(plan_lib):
    k = consts(plan_lib)
    for multi, mfma, dimq, opt in itertools.product((0, 1), (0, 1), DIMQS, (-1, 0, 1)):
        want = not multi and not mfma and dimq <= 2048 and opt != 0
        assert plan_lib.mg_wants(multi, mfma, dimq, opt) == int(want), (multi, mfma, dimq, opt)
    sizes = (0, 1, k["auto_max_rows"], k["auto_max_rows"] + 1, k["max_rows"], k["max_rows"] + 1)
    for wants, have, opt, n_slots, rows in itertools.product((0, 1), (0, 1), (-1, 1), (1, k["max_slots"], k["max_slots"] + 1), sizes):
        want = bool(wants and have) and n_slots <= k["max_slots"] and rows <= k["max_rows"] and (opt == 1 or rows <= k["auto_max_rows"])
        assert plan_lib.mg_gather(wants, have, opt, n_slots, rows) == int(want), (wants, have, opt, n_slots, rows)


def test_slot_arrays_are_sorted_distinct_and_carry_the_extents(plan_lib):
    rng = np.random.default_rng(3181)
    ng = 700  # lists of fewer than 700 / 64 = 11 ids are sorted, longer ones go through the bitmap over the groups: both sides of the switch
    counts = rng.integers(0, 6, ng).astype(np.uint32)  # (a group id may have no row)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    up = C.POINTER(C.c_uint)
    for listed in ([], [7], [7, 7, 7], list(range(ng)), [699, 0, 13, 0, 699, 2], [5] * 10 + [4], [5] * 10 + [4, 3], rng.integers(0, ng, 10).tolist(),
                   rng.integers(0, ng, 11).tolist(), rng.integers(0, ng, 200).tolist(), rng.integers(0, ng, 3000).tolist()):
        g = np.array(listed, np.uint32)
        want = np.unique(g)
        for with_starts in (True, False):
            gid, st, ct = (np.full(max(g.size, 1), 0xFFFFFFFF, np.uint32) for _ in range(3))
            rows = C.c_ulonglong(77)
            n = plan_lib.mg_slot_arrays(g.ctypes.data_as(up), g.size, ng, starts.ctypes.data_as(up) if with_starts else None, gid.ctypes.data_as(up), st.ctypes.data_as(up),
                                        ct.ctypes.data_as(up), C.byref(rows))
            assert n == want.size and gid[:n].tolist() == want.tolist(), listed
            if with_starts:
                assert st[:n].tolist() == starts[want].tolist() and ct[:n].tolist() == counts[want].tolist()
                assert rows.value == int(counts[want].sum())
            else:
                assert rows.value == 0
