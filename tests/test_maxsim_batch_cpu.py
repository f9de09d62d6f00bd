"""CPU: the host side of MaxSim re-ranking in batches (VecStore.max_sim_batch, ott_query_maxsim_groups_batch) — the
header's prototype and define, the symbol in both builds of the library with the refusals that need no store, MaxSimBatchPlan's
validation, label mapping and default take on a host-only store, and the batch part of the plan header
(otters_amd/csrc/ott_maxsim_gather_plan.h: MgBatch, the route, mg_batch_split) compiled on its own with the host compiler and held
to a plain Python restatement over a grid, as test_maxsim_groups_cpu.py holds the single call's part.  The split and the slot
building also run in a small stand-alone program under AddressSanitizer and UBSan.  The GPU half: test_gpu_maxsim_batch.py,
test_gpu_maxsim_batch_concurrent.py."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from otters_amd import Cmp, MaxSimBatchPlan, Metric, Mode, OttersError, Path, VecStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")

PROTOTYPE = ("int ott_query_maxsim_groups_batch(ott_store* s, const ott_query_desc* d, const void* tokens_per_query, const uint64_t* listed_per_query, "
             "uint32_t n_queries, const void* groups, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);")


# ---- the header and the library -------------------------------------------------------------------------------------------------

def test_header_declares_the_call_and_the_define_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert "#define OTT_MAXSIM_BATCH_MAX 4096" in src
    assert "#define OTT_ABI_VERSION 4" in src  # an added function: the version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ott_maxsim_batch.hip" in mk  # one source list for the product and the audit build
    assert len(re.findall(r"^SRCS\s*:?=", mk, flags=re.M)) == 1


def call(L, N, d, tokens, listed, n_queries, groups, out, cap, n_out, per):
    return L.ott_query_maxsim_groups_batch(None, C.byref(d) if d is not None else None, N.ptr(tokens) if tokens is not None else None,
                                           N.ptr(listed) if listed is not None else None, n_queries, N.ptr(groups) if groups is not None else None, N.ptr(out), cap,
                                           C.byref(n_out), N.ptr(per), None)


def test_library_exports_it_and_refuses_before_it_looks_at_the_store():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    assert hasattr(L, "ott_query_maxsim_groups_batch")
    out = np.zeros(4, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)
    per = np.full(2, 7, np.uint64)
    q = np.zeros(12, np.float32)
    g = np.array([0, 1, 1], np.uint32)
    tokens, listed = np.array([2, 1], np.uint32), np.array([2, 1], np.uint64)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, 3, int(Metric.Cosine), 1, 4
    last = lambda: L.ott_last_error()  # noqa: E731

    d.mode = int(Mode.PerQuery)
    assert call(L, N, d, tokens, listed, 2, g, out, 4, n_out, per) == -4
    assert b"ott_query_maxsim_groups_batch: tokens_per_query says which query vectors belong to which query; PER_QUERY is not served" in last()
    d.mode, d.path = int(Mode.Merged), int(Path.Mfma)
    assert call(L, N, d, tokens, listed, 2, g, out, 4, n_out, per) == -4
    assert b"ott_query_maxsim_groups_batch: the MFMA path does not serve late-interaction" in last()
    d.path = int(Path.Auto)
    assert call(L, N, d, tokens, listed, 0, g, out, 4, n_out, per) == -1 and b"ott_query_maxsim_groups_batch: n_queries is 0" in last()
    assert call(L, N, d, tokens, listed, 4097, g, out, 4, n_out, per) == -1
    assert b"ott_query_maxsim_groups_batch: n_queries 4097 is above OTT_MAXSIM_BATCH_MAX (4096)" in last()
    assert call(L, N, d, None, listed, 2, g, out, 4, n_out, per) == -1 and b"ott_query_maxsim_groups_batch: tokens_per_query is NULL" in last()
    assert call(L, N, d, tokens, None, 2, g, out, 4, n_out, per) == -1 and b"ott_query_maxsim_groups_batch: listed_per_query is NULL" in last()
    assert call(L, N, d, tokens, listed, 2, None, out, 4, n_out, per) == -1 and b"ott_query_maxsim_groups_batch: groups is NULL" in last()
    assert call(L, N, d, np.array([3, 0], np.uint32), listed, 2, g, out, 4, n_out, per) == -1
    assert b"ott_query_maxsim_groups_batch: query 1 has no tokens" in last()
    assert call(L, N, d, np.array([2, 2], np.uint32), listed, 2, g, out, 4, n_out, per) == -1
    assert b"ott_query_maxsim_groups_batch: tokens_per_query sums to 4, the descriptor holds 3 query vectors" in last()
    # every argument in order: only the store is missing.  Empty lists need no groups array.
    assert call(L, N, d, tokens, listed, 2, g, out, 4, n_out, per) == -1 and b"ott_query_maxsim_groups_batch: store is NULL" in last()
    assert call(L, N, d, tokens, np.zeros(2, np.uint64), 2, None, out, 4, n_out, per) == -1 and b"store is NULL" in last()
    assert n_out.value == 9 and per.tolist() == [7, 7] and not out["index"].any()  # nothing was written


def test_audit_build_exports_it():
    subprocess.check_call(["make", "-C", CSRC, "-j", "8", "-s", "audit"])
    # (loaded in a child: two builds of one library do not belong in one process)
    code = "import ctypes, sys; A = ctypes.CDLL(sys.argv[1]); [getattr(A, n) for n in sys.argv[2:]]"
    subprocess.check_call([sys.executable, "-c", code, os.path.join(CSRC, "libotters_hip_audit.so"), "ott_query_maxsim_groups_batch", "ott_query_maxsim_groups"])


# ---- plans --------------------------------------------------------------------------------------------------------------------

def host_store(labels=None):
    store = VecStore(4)
    store._n, store._n_groups = 100, 7  # (no GPU: lengths as set_groups would leave them)
    if labels is not None:
        store._group_labels = np.unique(np.asarray(labels))
        store._n_groups = int(store._group_labels.size)
    return store


Q = np.eye(4, dtype=np.float32)


def test_plan_refusals_at_validate():
    store = host_store()
    assert isinstance(store.max_sim_batch([Q[:2]], Metric.Cosine), MaxSimBatchPlan)
    with pytest.raises(OttersError, match="max_sim_batch: no token sets provided"):
        store.max_sim_batch([], Metric.Cosine).with_groups([]).validate()
    with pytest.raises(OttersError, match="max_sim_batch needs with_groups in this version: one list of groups per token set"):
        store.max_sim_batch([Q[:2]], Metric.Cosine).validate()
    with pytest.raises(OttersError, match="max_sim_batch: with_groups got 1 lists for 2 token sets"):
        store.max_sim_batch([Q[:2], Q[:1]], Metric.Cosine).with_groups([[1]]).validate()
    with pytest.raises(OttersError, match="max_sim_batch: token set 1 is empty"):
        store.max_sim_batch([Q[:2], np.zeros((0, 4), np.float32)], Metric.Cosine).with_groups([[1], [2]]).validate()
    with pytest.raises(OttersError, match="Query vector length 3 does not match expected dimension 4"):
        store.max_sim_batch([Q[:2], np.zeros((2, 3), np.float32)], Metric.Cosine).with_groups([[1], [2]]).validate()
    with pytest.raises(OttersError, match="max_sim_batch: 4097 token sets; a batch holds at most 4096"):
        store.max_sim_batch([Q[:1]] * 4097, Metric.Cosine).with_groups([[1]] * 4097).validate()
    with pytest.raises(OttersError, match="group labels must be integers"):
        store.max_sim_batch([Q[:2]], Metric.Cosine).with_groups([[1.5]]).validate()
    for bad in (7, -1):
        with pytest.raises(OttersError, match=f"with_groups: group {bad} is not one of the store's 7 groups"):
            store.max_sim_batch([Q[:2], Q[:1]], Metric.Cosine).with_groups([[1], [0, bad]]).validate()
    store.max_sim_batch([Q[:2], Q[0]], Metric.Cosine).with_groups([[1], []]).with_row_mask(np.ones(100, bool)).filter(0.5, Cmp.Gt).take(3).validate()


def test_labels_map_per_query_and_the_default_take_is_the_largest_distinct_count():
    labels = np.array([40, -3, 40, 7, 7, 2 ** 40], dtype=np.int64)  # dense: -3 -> 0, 7 -> 1, 40 -> 2, 2^40 -> 3
    store = host_store(labels)
    rb = store.max_sim_batch([Q[:3], Q[1], Q[2:]], Metric.Cosine).with_groups([[2 ** 40, -3, 40, -3], [], np.array([7, 7], np.int16)]).resolve()
    assert rb.queries.dtype == np.float32 and rb.queries.shape == (6, 4) and rb.queries.flags["C_CONTIGUOUS"]
    assert np.array_equal(rb.queries, np.concatenate([Q[:3], Q[1:2], Q[2:]]))      # the tokens of query 0, then 1, then 2
    assert rb.tokens_per_query.dtype == np.uint32 and rb.tokens_per_query.tolist() == [3, 1, 2]
    assert rb.listed_per_query.dtype == np.uint64 and rb.listed_per_query.tolist() == [4, 0, 2]
    assert rb.groups.dtype == np.uint32 and rb.groups.tolist() == [3, 0, 2, 0, 1, 1]  # the caller's order, duplicates kept
    assert rb.distinct_per_query == [3, 0, 1] and rb.k == 3 and rb.take == 1          # no take: Max, the largest distinct count
    for unknown in (8, 0, 2 ** 41):
        with pytest.raises(OttersError, match=f"no row carries the group label {unknown}$"):
            store.max_sim_batch([Q[:1], Q[:1]], Metric.Cosine).with_groups([[7], [7, unknown]]).validate()
    rb = store.max_sim_batch([Q[:1], Q[:1]], Metric.Euclidean).with_groups([[7], [7, 40]]).take(5).resolve()
    assert rb.k == 5 and rb.take == 0  # take infers Min from the metric, as VecQueryPlan does
    assert store.max_sim_batch([Q[:1]], Metric.Euclidean).with_groups([[7]]).take_max(2).resolve().take == 1
    assert store.max_sim_batch([Q[:1]], Metric.Cosine).with_groups([[7]]).take_min(2).resolve().take == 0
    rb = store.max_sim_batch([Q[:1], Q[:2]], Metric.Cosine).with_groups([[], []]).filter(0.25, Cmp.Lt).resolve()
    assert rb.groups.size == 0 and rb.k == 0 and (rb.filter_cmp, rb.filter_thr) == (int(Cmp.Lt), 0.25)


# ---- the plan header ----------------------------------------------------------------------------------------------------------------

DRIVER = r"""
#include "ott_maxsim_gather_plan.h"
using namespace ott;
extern "C" void mgb_split(const unsigned* counts, unsigned long long T, unsigned n_wg, unsigned* first) { mg_batch_split(counts, T, n_wg, first); }
// slot arrays: room for the sum of the lists; per-query arrays: room for B.  Returns T; scal = {S, NT, max_tokens, rows, compared, takes}
extern "C" unsigned long long mgb_build(const unsigned* groups, const unsigned* tokens, const unsigned long long* listed, unsigned B, unsigned n_groups,
                                        const unsigned* starts, unsigned dimq, int wants, int have, int opt, unsigned* gid, unsigned* start, unsigned* count,
                                        unsigned* query, unsigned* pos, unsigned* distinct, unsigned long long* rows_of, unsigned long long* scal) {
    MgBatch mb;
    mg_batch_build(groups, tokens, (const uint64_t*)listed, B, n_groups, starts, dimq, mb);
    const size_t T = mb.gid.size();
    if (mb.query.size() != T || mb.pos.size() != T || mb.tokens.size() != B || mb.distinct.size() != B || mb.rows_of.size() != B) return ~0ull;
    if (starts ? (mb.start.size() != T || mb.count.size() != T) : (!mb.start.empty() || !mb.count.empty())) return ~0ull;
    for (size_t i = 0; i < T; i++) { gid[i] = mb.gid[i]; query[i] = mb.query[i]; pos[i] = mb.pos[i]; if (starts) { start[i] = mb.start[i]; count[i] = mb.count[i]; } }
    for (unsigned b = 0; b < B; b++) { if (mb.tokens[b] != tokens[b]) return ~0ull; distinct[b] = mb.distinct[b]; rows_of[b] = mb.rows_of[b]; }
    scal[0] = mb.S; scal[1] = mb.NT; scal[2] = mb.max_tokens; scal[3] = mb.rows; scal[4] = mb.compared;
    scal[5] = mg_batch_takes_gather(wants != 0, have != 0, opt, dimq, mb) ? 1 : 0;
    return T;
}
// the route alone, from sizes no list could be built for here
extern "C" int mgb_route(int wants, int have, int opt, unsigned dimq, unsigned B, unsigned S, unsigned max_tokens, unsigned long long rows, unsigned long long big_query_rows) {
    MgBatch mb;
    mb.tokens.assign(B, max_tokens);
    mb.rows_of.assign(B, 0);
    mb.rows_of[B - 1] = big_query_rows;
    mb.S = S; mb.max_tokens = max_tokens; mb.rows = rows;
    return mg_batch_takes_gather(wants != 0, have != 0, opt, dimq, mb) ? 1 : 0;
}
"""

# the stand-alone program: the same grid of lists and splits as the tests below, with nothing but its own asserts (the sanitizers
# watch the vectors and the `first` array, whose end is the end of its allocation)
MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "ott_maxsim_gather_plan.h"
using namespace ott;
static unsigned long long state = 88172645463325252ull;
static unsigned rnd(unsigned n) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state % n); }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    const unsigned ngs[] = {1, 7, 64, 65, 700};
    const unsigned Bs[] = {1, 2, 5, 40};
    unsigned long long checked = 0;
    for (unsigned ng : ngs) for (unsigned B : Bs) for (unsigned longest : {0u, 1u, 9u, 200u, 3000u}) {
        std::vector<uint32_t> starts(ng + 1, 0);
        for (unsigned g = 0; g < ng; g++) starts[g + 1] = starts[g] + rnd(6);
        std::vector<uint32_t> tokens(B), groups;
        std::vector<uint64_t> listed(B);
        for (unsigned b = 0; b < B; b++) {
            tokens[b] = 1 + rnd(40);
            listed[b] = longest ? rnd(longest + 1) : 0;
            for (uint64_t i = 0; i < listed[b]; i++) groups.push_back(rnd(ng));
        }
        for (int with_starts = 0; with_starts < 2; with_starts++) {
            MgBatch mb;
            mg_batch_build(groups.data(), tokens.data(), listed.data(), B, ng, with_starts ? starts.data() : nullptr, 128, mb);
            const size_t T = mb.gid.size();
            CHECK(mb.query.size() == T && mb.pos.size() == T && mb.distinct.size() == B);
            uint64_t rows = 0, at = 0;
            for (unsigned b = 0; b < B; b++) {
                CHECK(mb.distinct[b] <= mb.S && mb.distinct[b] <= listed[b]);
                for (unsigned i = 0; i < mb.distinct[b]; i++, at++) {
                    CHECK(mb.query[at] == b && mb.pos[at] == i && mb.gid[at] < ng && (i == 0 || mb.gid[at - 1] < mb.gid[at]));
                    if (with_starts) { CHECK(mb.start[at] == starts[mb.gid[at]] && mb.count[at] == starts[mb.gid[at] + 1] - starts[mb.gid[at]]); rows += mb.count[at]; }
                }
            }
            CHECK(at == T && rows == mb.rows);
            if (!with_starts) continue;
            for (unsigned n_wg : {1u, 2u, 3u, 64u, 2048u}) {
                if (T == 0 && n_wg > 1) continue;
                const unsigned n = n_wg < T ? n_wg : (unsigned)(T ? T : 1);
                uint32_t* first = (uint32_t*)malloc((n + 1) * sizeof(uint32_t));  // exactly n + 1 entries: a write past them is seen
                mg_batch_split(mb.count.data(), T, n, first);
                CHECK(first[0] == 0 && first[n] == T);
                for (unsigned w = 0; w < n; w++) CHECK(first[w] <= first[w + 1]);
                free(first);
                checked++;
            }
        }
    }
    printf("ok %llu\n", checked);
    return 0;
}
"""

DIMQS = (8, 128, 512, 520, 1024, 1032, 2048, 2056)


def host_cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("maxsim_batch_plan")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([host_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    up, ullp, ull, u, i = C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong), C.c_ulonglong, C.c_uint, C.c_int
    L.mgb_split.argtypes, L.mgb_split.restype = [up, ull, u, up], None
    L.mgb_build.argtypes, L.mgb_build.restype = [up, up, ullp, u, u, up, u, i, i, i, up, up, up, up, up, up, ullp, ullp], ull
    L.mgb_route.argtypes, L.mgb_route.restype = [i, i, i, u, u, u, u, ull, ull], i
    return L


UP, ULLP = C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)
MAX_SLOTS, MAX_ROWS, AUTO_MAX_ROWS = 2 ** 24, 2 ** 30, 1_000_000  # ott_maxsim_gather_plan.h (held by test_maxsim_groups_cpu.py)


# the restatement: the issue's words in plain Python
def py_cap(dimq):
    return 32 if dimq <= 512 else 16 if dimq <= 1024 else 8 if dimq <= 2048 else 0


def py_nt(dimq, max_tokens):
    for w in (8, 16, 32):
        if w >= py_cap(dimq) or w >= max_tokens:
            return min(w, py_cap(dimq))
    return py_cap(dimq)


def py_route(wants, have, opt, dimq, B, S, max_tokens, rows, rows_of):
    if not (wants and have):
        return False
    if max_tokens > py_cap(dimq):
        return False
    if B * S > MAX_SLOTS or rows > MAX_ROWS:
        return False
    return opt == 1 or all(r <= AUTO_MAX_ROWS for r in rows_of)


def py_split(counts, n_wg):
    """first[w] = how many slots start before w / n_wg of the total weight, a slot weighing its rows + 1"""
    weight = [int(c) + 1 for c in counts]
    before = np.concatenate([[0], np.cumsum(weight)])[:-1].astype(object) if weight else []
    W = sum(weight)
    return [sum(1 for p in before if p * n_wg < w * W) for w in range(n_wg + 1)]


def build(L, lists, tokens, ng, starts, dimq, wants=1, have=1, opt=-1):
    B = len(lists)
    groups = np.array([g for l in lists for g in l], np.uint32)
    listed = np.array([len(l) for l in lists], np.uint64)
    tok = np.array(tokens, np.uint32)
    room = max(groups.size, 1)
    gid, start, count, query, pos = (np.full(room, 0xFFFFFFFF, np.uint32) for _ in range(5))
    distinct, rows_of, scal = np.zeros(B, np.uint32), np.zeros(B, np.uint64), np.zeros(6, np.uint64)
    T = L.mgb_build(groups.ctypes.data_as(UP), tok.ctypes.data_as(UP), listed.ctypes.data_as(ULLP), B, ng, None if starts is None else starts.ctypes.data_as(UP), dimq, wants, have, opt,
                    gid.ctypes.data_as(UP), start.ctypes.data_as(UP), count.ctypes.data_as(UP), query.ctypes.data_as(UP), pos.ctypes.data_as(UP), distinct.ctypes.data_as(UP),
                    rows_of.ctypes.data_as(ULLP), scal.ctypes.data_as(ULLP))
    assert T != 2 ** 64 - 1
    return dict(T=T, gid=gid[:T], start=start[:T], count=count[:T], query=query[:T], pos=pos[:T], distinct=distinct, rows_of=rows_of, S=int(scal[0]), NT=int(scal[1]),
                max_tokens=int(scal[2]), rows=int(scal[3]), compared=int(scal[4]), takes=int(scal[5]))


def test_batch_slots_stride_and_token_width_over_the_grid(plan_lib):
    rng = np.random.default_rng(3191)
    ng = 700
    counts = rng.integers(0, 6, ng).astype(np.uint32)  # (a group id may have no row)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    batches = ([[]], [[7]], [[], [7, 7, 7], []], [list(range(ng)), [699, 0, 13, 0, 699, 2]], [rng.integers(0, ng, n).tolist() for n in (10, 11, 200, 0, 3000, 1)],
               [[5] * 10 + [4], [5] * 10 + [4, 3], [4, 5]])
    for lists, dimq, with_starts in itertools.product(batches, DIMQS, (True, False)):
        tokens = rng.choice([1, 3, 8, 9, 16, 17, 32, 33], len(lists)).tolist()
        got = build(plan_lib, lists, tokens, ng, starts if with_starts else None, dimq)
        want = [np.unique(np.array(l, np.int64)) for l in lists]
        assert got["distinct"].tolist() == [w.size for w in want]
        assert got["S"] == max(w.size for w in want) and got["max_tokens"] == max(tokens) and got["NT"] == py_nt(dimq, max(tokens))
        assert got["gid"].tolist() == [g for w in want for g in w.tolist()]                       # per query ascending and duplicate-free, back to back
        assert got["query"].tolist() == [b for b, w in enumerate(want) for _ in range(w.size)]
        assert got["pos"].tolist() == [i for w in want for i in range(w.size)]
        if with_starts:
            assert got["start"].tolist() == [int(starts[g]) for w in want for g in w] and got["count"].tolist() == [int(counts[g]) for w in want for g in w]
            rows_of = [int(counts[w].sum()) for w in want]
            assert got["rows_of"].tolist() == rows_of and got["rows"] == sum(rows_of) and got["compared"] == sum(r * t for r, t in zip(rows_of, tokens))
            assert got["takes"] == int(py_route(1, 1, -1, dimq, len(lists), got["S"], max(tokens), sum(rows_of), rows_of))
        else:
            assert got["rows"] == 0 and got["compared"] == 0 and not got["rows_of"].any()
    # the cases the GPU tests name: 1, 3, 8, 9 and 32 tokens share NT = 32; 33 tokens at dim 40 and 17 at 520 leave the batched gather
    assert build(plan_lib, [[1]] * 5, [1, 3, 8, 9, 32], ng, starts, 40)["NT"] == 32
    assert build(plan_lib, [[1]] * 2, [3, 33], ng, starts, 40, opt=1)["takes"] == 0
    assert build(plan_lib, [[1]] * 2, [3, 17], ng, starts, 520, opt=1)["takes"] == 0
    assert build(plan_lib, [[1]] * 2, [3, 16], ng, starts, 520, opt=1)["takes"] == 1
    assert build(plan_lib, [[1]] * 2, [3, 3], ng, starts, 2056, wants=0, opt=1)["takes"] == 0


def test_route_over_the_grid_including_the_auto_rule(plan_lib):
    for wants, have, opt, dimq, B, S, max_tokens in itertools.product((0, 1), (0, 1), (-1, 1), (128, 520, 2048), (1, 4096), (1, 4096, 4097), (8, 9, 16, 17, 32, 33)):
        for rows, big in ((0, 0), (AUTO_MAX_ROWS, AUTO_MAX_ROWS), (AUTO_MAX_ROWS + 1, AUTO_MAX_ROWS + 1), (5 * AUTO_MAX_ROWS, AUTO_MAX_ROWS), (MAX_ROWS, 1), (MAX_ROWS + 1, 1)):
            want = py_route(wants, have, opt, dimq, B, S, max_tokens, rows, [0] * (B - 1) + [big])
            assert plan_lib.mgb_route(wants, have, opt, dimq, B, S, max_tokens, rows, big) == int(want), (wants, have, opt, dimq, B, S, max_tokens, rows, big)
    # AUTO: a batch of queries that each prefer the gather takes it however many rows they list together; one query above the line sends it to the loop
    assert plan_lib.mgb_route(1, 1, -1, 128, 64, 1000, 32, 64 * AUTO_MAX_ROWS, AUTO_MAX_ROWS) == 1
    assert plan_lib.mgb_route(1, 1, -1, 128, 64, 1000, 32, AUTO_MAX_ROWS + 1, AUTO_MAX_ROWS + 1) == 0
    assert plan_lib.mgb_route(1, 1, 1, 128, 64, 1000, 32, AUTO_MAX_ROWS + 1, AUTO_MAX_ROWS + 1) == 1
    assert plan_lib.mgb_route(1, 1, 1, 128, 4096, 4096, 32, 0, 0) == 1 and plan_lib.mgb_route(1, 1, 1, 128, 4096, 4097, 32, 0, 0) == 0  # B x S against 2^24


def test_split_is_a_monotone_partition_balanced_to_within_one_group(plan_lib):
    rng = np.random.default_rng(3192)
    shapes = [np.zeros(0, np.uint32), np.array([0], np.uint32), np.array([5], np.uint32), np.zeros(100, np.uint32), np.full(6000, 20, np.uint32),
              rng.integers(0, 6, 700).astype(np.uint32), rng.integers(0, 300, 6000).astype(np.uint32),
              np.concatenate([np.full(10, 100000), np.zeros(500)]).astype(np.uint32), np.array([0, 0, 0, 2 ** 30 - 5], np.uint32)]
    for counts, n_wg in itertools.product(shapes, (1, 2, 3, 7, 64, 2048)):
        first = np.full(n_wg + 2, 0xFFFFFFFF, np.uint32)
        plan_lib.mgb_split(counts.ctypes.data_as(UP), counts.size, n_wg, first.ctypes.data_as(UP))
        assert first[n_wg + 1] == 0xFFFFFFFF                                    # n_wg + 1 entries and no more
        f = first[: n_wg + 1].astype(np.int64)
        assert f[0] == 0 and f[-1] == counts.size and (np.diff(f) >= 0).all()   # a partition into contiguous ranges; first never decreases
        if counts.size * n_wg <= 700 * 64:
            assert f.tolist() == py_split(counts, n_wg), (counts[:8], n_wg)
        weight = counts.astype(np.int64) + 1
        cum = np.concatenate([[0], np.cumsum(weight)])
        load = cum[f[1:]] - cum[f[:-1]]
        if counts.size:
            assert (np.abs(load * n_wg - cum[-1]) < int(weight.max()) * n_wg).all(), (counts[:8], n_wg)  # |load - W / n_wg| < the heaviest slot
    # empty groups still cost something: 100 empty groups over 4 workgroups are 25 each, not all on one
    first = np.zeros(5, np.uint32)
    plan_lib.mgb_split(np.zeros(100, np.uint32).ctypes.data_as(UP), 100, 4, first.ctypes.data_as(UP))
    assert first.tolist() == [0, 25, 50, 75, 100]


def test_split_and_slot_building_under_asan_and_ubsan(tmp_path):
    """a stand-alone program with its own main, compiled with the host compiler and the sanitizers' own runtime: nothing is preloaded and
    nothing is loaded into python"""
    src, exe = tmp_path / "mgb_main.cpp", tmp_path / "mgb_main"
    src.write_text(MAIN)
    # clang where there is one, as tests/host/Makefile: it links the sanitizers' runtime into the program itself
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    cxx = clang if os.path.exists(clang) else host_cxx()
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, str(src), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 300, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
