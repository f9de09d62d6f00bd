"""CPU: MMR diversity re-ranking (ott_query_mmr, VecQueryPlan.mmr) without a GPU — the host model's own
self-checks (tests/mmr_ref.py), the planner's refusals and defaults, the ABI's device-free argument checks, and a walk of the
HIP-free plan header (ott_mmr_plan.h) by a stand-alone C++ program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mmr_ref as R
from otters_amd import Cmp, Metric, Mode, OttersError, VecStore
from otters_amd.vec import VecQueryPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")
f32 = np.float32


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


# ---- the host model ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(7)
    return rng.uniform(-1, 1, (300, 13)).astype(np.float32), rng.uniform(-1, 1, (2, 13)).astype(np.float32)


@pytest.mark.parametrize("metric,take", [(Metric.Cosine, 1), (Metric.DotProduct, 1), (Metric.Euclidean, 0), (Metric.Manhattan, 0), (Metric.DotProduct, 0)])
def test_lambda_one_returns_the_candidate_prefix(oracle, corpus, metric, take):
    rows, q = corpus
    hits, counts, vals = R.mmr(oracle, rows, q[0], metric, take, 7, 40, 1.0)
    cand = R.candidates(oracle, rows, q[0], metric, take, 40)
    assert counts == [7] and hits["index"].tolist() == cand["index"][:7].tolist()
    assert bits(hits["score"]) == bits(cand["score"][:7])
    g = cand["score"][:7] if take == 1 else -cand["score"][:7]
    assert bits(vals) == bits(g)  # pick 0: 1 * g(rel_0); later picks: 1 * g(rel) - 0 * red with a finite red and a non-zero g(rel)


@pytest.mark.parametrize("metric,take", [(Metric.Cosine, 1), (Metric.Euclidean, 0)])
def test_fetch_k_equal_k_returns_the_plain_set(oracle, corpus, metric, take):
    rows, q = corpus
    hits, _, _ = R.mmr(oracle, rows, q[1], metric, take, 12, 12, 0.3)
    cand = R.candidates(oracle, rows, q[1], metric, take, 12)
    assert sorted(hits["index"].tolist()) == sorted(cand["index"].tolist())
    assert hits["index"].tolist() != cand["index"].tolist()  # ... in MMR order, which on random rows is another one
    assert hits["index"][0] == cand["index"][0]


HAND_ROWS = np.array([[1, 0], [0.96, 0.28], [0, 1]], np.float32)


def test_hand_computed_case_differs_from_plain_top_k(oracle):
    """Rows [1, 0], [0.96, 0.28], [0, 1], dot, take_max(2), fetch_k = 3, lam = 0.5: plain top-2 is rows 0 and 1, MMR returns rows 0
    and 2, the pick values are literals computed by hand.  The query is [1, 0.1].  (The case was first written down with the query
    [1, 0.2]; the hand computation behind it had dropped the 0.2 * 0.28 of row 1's relevance — with it row 1 scores 1.016 > 1 and
    leads the candidates, see the next test.  0.1 is the mended query: every assertion of the case stands.)"""
    q = np.array([1, 0.1], np.float32)
    plain = R.candidates(oracle, HAND_ROWS, q, Metric.DotProduct, 1, 2)
    assert plain["index"].tolist() == [0, 1]
    hits, counts, vals = R.mmr(oracle, HAND_ROWS, q, Metric.DotProduct, 1, 2, 3, 0.5)
    assert hits["index"].tolist() == [0, 2] and counts == [2]
    # by hand; dim 2 = no full chunk of eight, two remainder terms summed in order from 0 (0 + x == x):
    #   rel = q . rows = [1*1 + 0.1*0, 1*0.96 + 0.1*0.28, 1*0 + 0.1*1] = [1, 0.988, 0.1]
    #   pick 0 = row 0, value 0.5 * 1 = 0.5;  red = P[row 0][c] = rows[0] . rows[c] = [., 0.96, 0]
    #   value(row 1) = 0.5 * 0.988 - 0.5 * 0.96 = 0.014;  value(row 2) = 0.5 * 0.1 - 0.5 * 0 = 0.05  -> row 2
    rel1 = f32(f32(1) * f32(0.96)) + f32(f32(0.1) * f32(0.28))
    rel2 = f32(f32(1) * f32(0)) + f32(f32(0.1) * f32(1))
    v1 = f32(0.5) * rel1 - f32(0.5) * (f32(f32(1) * f32(0.96)) + f32(f32(0) * f32(0.28)))
    v2 = f32(0.5) * rel2 - f32(0.5) * f32(0)
    assert abs(float(v1) - 0.014) < 1e-6 and abs(float(v2) - 0.05) < 1e-7 and v2 > v1
    assert bits(vals) == bits([f32(0.5), v2])
    assert bits(hits["score"]) == bits([f32(1), rel2])


def test_hand_computed_case_where_the_second_row_leads(oracle):
    """the same store and settings with the query [1, 0.2]: row 1 is the most relevant (0.96 + 0.2 * 0.28 = 1.016 > 1), so it is
    candidate 0 and pick 0; measured against IT row 0 (0.96) is still worth more than row 2 (0.28 away, but relevance 0.2): MMR
    returns rows 1, 0 — here the plain top-2 in the plain order"""
    q = np.array([1, 0.2], np.float32)
    plain = R.candidates(oracle, HAND_ROWS, q, Metric.DotProduct, 1, 2)
    assert plain["index"].tolist() == [1, 0]
    hits, counts, vals = R.mmr(oracle, HAND_ROWS, q, Metric.DotProduct, 1, 2, 3, 0.5)
    assert hits["index"].tolist() == [1, 0] and counts == [2]
    #   rel = [1, 0.96 + 0.056, 0.2];  pick 0 = row 1, value 0.5 * 1.016 = 0.508;  red = P[row 1][c] = [0.96*1 + 0.28*0, ., 0.96*0 + 0.28*1]
    #   value(row 0) = 0.5 * 1 - 0.5 * 0.96 = 0.02;  value(row 2) = 0.5 * 0.2 - 0.5 * 0.28 = -0.04  -> row 0
    rel1 = f32(f32(1) * f32(0.96)) + f32(f32(0.2) * f32(0.28))
    v0 = f32(0.5) * f32(1) - f32(0.5) * (f32(f32(0.96) * f32(1)) + f32(f32(0.28) * f32(0)))
    v2 = f32(0.5) * f32(f32(0.2) * f32(1)) - f32(0.5) * (f32(f32(0.96) * f32(0)) + f32(f32(0.28) * f32(1)))
    assert abs(float(v0) - 0.02) < 1e-6 and abs(float(v2) + 0.04) < 1e-6
    assert bits(vals) == bits([f32(0.5) * rel1, v0])
    assert bits(hits["score"]) == bits([rel1, f32(1)])


def test_duplicated_rows_tie_to_the_lower_position(oracle):
    rng = np.random.default_rng(3)
    base = rng.uniform(-1, 1, (20, 8)).astype(np.float32)
    rows = np.repeat(base, 3, axis=0)  # rows 3i, 3i+1, 3i+2 are one vector
    q = rng.uniform(-1, 1, 8).astype(np.float32)
    cand = R.candidates(oracle, rows, q, Metric.DotProduct, 1, 30)
    assert cand["index"][:3].tolist() == sorted(cand["index"][:3].tolist())  # equal scores: lower row first
    hits, _, vals = R.mmr(oracle, rows, q, Metric.DotProduct, 1, 12, 30, 0.5)
    pos = {int(i): p for p, i in enumerate(cand["index"])}
    # whenever a copy of a vector is picked, every copy at a lower position was picked before it
    seen = set()
    for i in hits["index"].tolist():
        twins = [t for t in range(i - i % 3, i - i % 3 + 3) if t in pos and pos[t] < pos[i]]
        assert all(t in seen for t in twins), (i, twins, seen)
        seen.add(i)
    # and directly on the loop: two candidates with the same relevance and the same pair scores
    picks, _ = R.greedy(np.array([3, 2, 2, 2], np.float32), lambda s: np.array([9, 1, 1, 1], np.float32), 3, 0.5, 1)
    assert picks.tolist() == [0, 1, 2]


def test_nan_and_infinite_pair_scores():
    inf, nan = f32(np.inf), f32(np.nan)
    rel = np.array([5, 4, 3, 2, 1], np.float32)
    P = np.array([[0, nan, inf, -inf, 1],   # after pick 0: red = [., NaN, inf, -inf, 1]
                  [0, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0],
                  [0, 7, 0, 0, nan],        # pick 3 -> red[1]: NaN becomes 7; red[4]: NaN x, stays 1
                  [0, 0, 0, 0, 0]], np.float32)
    picks, vals = R.greedy(rel, lambda s: P[s], 5, 0.5, 1)
    # round 1: values [., NaN, 1.5 - inf = -inf, 1 + inf = +inf, 0.5 - 0.5 = 0] -> 3 (+inf); NaN ranks below -inf
    # round 2: red = [., 7, inf, ., 1] -> values [., 2 - 3.5 = -1.5, -inf, ., 0] -> 4
    # round 3: P[4] = 0: red[1] = max(7, 0) = 7, red[2] = inf -> 1 (-1.5), then 2 (-inf)
    assert picks.tolist() == [0, 3, 4, 1, 2]
    assert bits(vals) == bits([f32(2.5), inf, f32(0), f32(-1.5), -inf])
    # a NaN value is picked last, after -inf, and is reported as one bit pattern
    P2 = np.array([[0, nan, inf], [0, 0, 0], [0, nan, 0]], np.float32)  # (a NaN pair score never replaces a NaN redundancy)
    picks, vals = R.greedy(np.array([3, 2, 1], np.float32), lambda s: P2[s], 3, 0.5, 1)
    assert picks.tolist() == [0, 2, 1] and bits(vals) == bits([f32(1.5), -inf]) + [0x7FC00000]
    # take Min: g flips the sign of relevances and pair scores alike (distances: the nearest picked row is the redundancy)
    picks, vals = R.greedy(np.array([1, 2, 3], np.float32), lambda s: np.array([[0, 1, 9], [1, 0, 9], [9, 9, 0]], np.float32)[s], 2, 0.5, 0)
    assert picks.tolist() == [0, 2] and bits(vals) == bits([f32(-0.5), f32(-1.5) - f32(-4.5)])
    # signed zeros: +0.0 ranks above -0.0, and "x > red" keeps the first of two equal zeros
    picks, vals = R.greedy(np.array([0.0, -0.0, 0.0], np.float32), lambda s: np.zeros(3, np.float32), 3, 1.0, 1)
    assert picks.tolist() == [0, 2, 1] and bits(vals) == bits([f32(0.0), f32(0.0), f32(-0.0) - f32(0.0)])


def test_pair_rows_are_the_oracles_scores_with_the_selected_row_as_the_query(oracle):
    rng = np.random.default_rng(11)
    rows = rng.uniform(-1, 1, (9, 13)).astype(np.float32)
    inv = oracle.inv_norms(rows)
    for mode in (oracle.REDUCE_AVX, oracle.REDUCE_SEQ4):
        for s in (0, 4):
            assert bits(R.pair_row(oracle, rows, inv, s, Metric.Cosine, mode)) == bits([oracle.cosine(rows[s], rows[c], inv[s], inv[c], mode) for c in range(9)])
            assert bits(R.pair_row(oracle, rows, inv, s, Metric.DotProduct, mode)) == bits([oracle.dot(rows[s], rows[c], mode) for c in range(9)])
            assert bits(R.pair_row(oracle, rows, inv, s, Metric.Euclidean, mode)) == bits([oracle.l2sq(rows[s], rows[c], mode) for c in range(9)])


# ---- the planner ---------------------------------------------------------------------------------------------------------------------

def plan(k=5, nq=1):
    store = VecStore.__new__(VecStore)  # validate() reads dim only: no device is touched
    store.dim = 4
    p = VecQueryPlan()
    p.vector_store = store
    p.query_vectors = np.zeros((nq, 4), np.float32) if nq > 1 else [np.zeros(4, np.float32)]
    p.search_metric = Metric.Cosine
    return p.take(k) if k is not None else p


def refused(p, text):
    with pytest.raises(OttersError) as e:
        p.validate()
    assert text in str(e.value), str(e.value)


def test_default_fetch_k():
    from otters_amd.vec import MMR_MAX_FETCH, mmr_default_fetch_k  # (here: the model's self-checks above need neither)
    assert [mmr_default_fetch_k(k) for k in (1, 3, 4, 5, 10, 204, 205, 1024)] == [20, 20, 20, 25, 50, 1020, 1024, 1024]
    assert MMR_MAX_FETCH == 1024
    p = plan(10).mmr()
    p.validate()
    assert p._mmr_args() == (f32(0.5), 50)
    lam, fk = plan(10).mmr(0.25, 10)._mmr_args()
    assert lam.dtype == np.float32 and lam == f32(0.25) and fk == 10


def test_validate_refusals_and_messages():
    refused(plan().mmr().one_per_group(), "mmr cannot be combined with one_per_group in this version")
    refused(plan().mmr().per_group(2), "mmr cannot be combined with per_group in this version")
    refused(plan(5, nq=2).mmr().max_sim(), "mmr cannot be combined with max_sim: a hit of max_sim is a group, not a row")
    refused(plan(5, nq=3).mmr(), "mmr takes one query; a batch needs per_query() (one MMR per query)")
    plan(5, nq=3).mmr().per_query().validate()
    refused(plan(30).mmr(0.5, 29), "mmr: take(30) asks for more picks than fetch_k = 29 candidates")
    refused(plan(2000).mmr(), "mmr: take(2000) asks for more picks than fetch_k = 1024 candidates")
    refused(plan(5).mmr(0.5, 1025), "mmr: fetch_k 1025 is above the limit of 1024 candidates")
    refused(plan(None).mmr(), "mmr needs an explicit take: the number of picks (take, take_min or take_max)")
    refused(plan(0).mmr(), "mmr: take must be at least 1, not 0")
    for bad in (-0.1, 1.5, float("nan"), "x", True):
        refused(plan().mmr(bad), "mmr: lambda_mult must be a number in [0, 1]")
    refused(plan().mmr(0.5, 7.5), "mmr: fetch_k must be an integer")
    # what it combines with
    p = plan(5).mmr(0.3, 40).filter(0.1, Cmp.Gt).with_row_mask([True] * 3).with_row_ids([1, 2, 3])
    p.validate()
    plan(5).take_min(5).mmr().validate()
    plan(None).take_max(5).mmr().validate()


def test_a_plan_without_mmr_resolves_to_what_it_did():
    store = VecStore.__new__(VecStore)
    store.dim, store._n, store._n_groups = 4, 9, 0
    store.len = lambda: 9
    store.group_count = lambda: 0
    p = VecQueryPlan()
    p.vector_store, p.query_vectors, p.search_metric = store, [np.zeros(4, np.float32)], Metric.Cosine
    rq = p.take(3).resolve()
    assert rq.mmr is None and rq.mmr_values is None and rq.k == 3
    rq = p.mmr(1, 7).resolve()
    assert rq.mmr == (f32(1), 7) and rq.k == 3 and rq.mode == int(Mode.Merged)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------

PROTOTYPE = """int ott_query_mmr(ott_store* s, const ott_query_desc* d, const uint64_t* ids, uint64_t n_ids,
                  uint64_t fetch_k, float lambda, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                  float* out_values , ott_stats* stats);"""


def test_header_declares_the_call_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert "#define OTT_ABI_VERSION 4" in src and "#define OTT_MMR_MAX_FETCH 1024" in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ott_mmr.hip" in mk  # one source list for the product and the audit build


def test_library_exports_it_and_checks_its_arguments_without_a_device():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    assert hasattr(L, "ott_query_mmr")
    out = np.zeros(4, dtype=N.HIT_DTYPE)
    vals = np.zeros(4, np.float32)
    n_out = C.c_uint64(9)
    q = np.zeros(4, np.float32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, 1, int(Metric.Cosine), 1, 4

    def call(fetch_k, lam, desc=d):
        return L.ott_query_mmr(None, C.byref(desc) if desc is not None else None, None, 0, fetch_k, lam, N.ptr(out), 4, C.byref(n_out), None, N.ptr(vals), None)

    assert call(8, float("nan")) == -1 and b"ott_query_mmr: lambda must lie in [0, 1]" in L.ott_last_error()
    assert call(8, 1.25) == -1 and b"lambda" in L.ott_last_error()
    assert call(8, -0.5) == -1 and b"lambda" in L.ott_last_error()
    assert call(3, 0.5) == -1 and b"ott_query_mmr: fetch_k must lie between k and OTT_MMR_MAX_FETCH" in L.ott_last_error()  # k = 4 > fetch_k
    assert call(1025, 0.5) == -1 and b"fetch_k" in L.ott_last_error()
    d.k = 0
    assert call(8, 0.5) == -1 and b"ott_query_mmr: k must be at least 1" in L.ott_last_error()
    d.k = 4
    assert call(8, 0.5, None) == -1 and b"desc is NULL" in L.ott_last_error()
    assert call(8, 0.5) == -1 and b"store is NULL" in L.ott_last_error()  # valid arguments: the NULL store is what is left to refuse
    assert n_out.value == 9 and not out["index"].any() and not vals.any()  # nothing was touched


def test_audit_build_exports_it():
    import sys
    subprocess.check_call(["make", "-C", CSRC, "-j", "8", "-s", "audit"])
    # (loaded in a child: two builds of one library do not belong in one process)
    code = "import ctypes, sys; A = ctypes.CDLL(sys.argv[1]); [getattr(A, n) for n in sys.argv[2:]]"
    subprocess.check_call([sys.executable, "-c", code, os.path.join(CSRC, "libotters_hip_audit.so"), "ott_query_mmr"])


# ---- the plan header: a stand-alone program under ASan + UBSan -----------------------------------------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <vector>
#include "ott_mmr_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (n %u nq %u)\n", __LINE__, #c, n, nq); return 1; } } while (0)
int main() {
    unsigned n = 0, nq = 0;
    CHECK(MMR_MAX_FETCH == 1024 && MMR_DIMQ_MAX == 2048 && MMR_PAIR_MAX == (256ull << 20) && MMR_SEL == 8 && MMR_COLS == 64 && MMR_PAIR_THREADS == 512);
    // the scalar arguments
    CHECK(mmr_check_args(0, 5, 0.5f) == MMR_BAD_K);
    CHECK(mmr_check_args(6, 5, 0.5f) == MMR_BAD_FETCH && mmr_check_args(1, 1025, 0.5f) == MMR_BAD_FETCH && mmr_check_args(1024, 1024, 0.5f) == MMR_OK);
    CHECK(mmr_check_args(1, 1, NAN) == MMR_BAD_LAMBDA && mmr_check_args(1, 1, -0.001f) == MMR_BAD_LAMBDA && mmr_check_args(1, 1, 1.001f) == MMR_BAD_LAMBDA);
    CHECK(mmr_check_args(1, 1, 0.0f) == MMR_OK && mmr_check_args(1, 1, 1.0f) == MMR_OK && mmr_check_args(1, 1, -0.0f) == MMR_OK);
    CHECK(mmr_refusal_is_invalid(MMR_BAD_K) && mmr_refusal_is_invalid(MMR_BAD_FETCH) && mmr_refusal_is_invalid(MMR_BAD_LAMBDA));
    CHECK(!mmr_refusal_is_invalid(MMR_MERGED_BATCH) && !mmr_refusal_is_invalid(MMR_MULTI_GPU) && !mmr_refusal_is_invalid(MMR_ROW_TOO_LONG) && !mmr_refusal_is_invalid(MMR_PAIRS_TOO_BIG));
    // the store's refusals, in their order
    CHECK(mmr_check_store(false, 2, true, 4096, 1024) == MMR_MERGED_BATCH);
    CHECK(mmr_check_store(true, 2, true, 4096, 1024) == MMR_MULTI_GPU && mmr_check_store(false, 1, true, 8, 1) == MMR_MULTI_GPU);
    CHECK(mmr_check_store(true, 2, false, 2056, 1024) == MMR_ROW_TOO_LONG && mmr_check_store(true, 2, false, 2048, 1024) == MMR_OK);
    CHECK(mmr_cap_needed(10, 4, false, 1) == 4 && mmr_cap_needed(10, 40, false, 1) == 10 && mmr_cap_needed(10, 40, true, 3) == 30 && mmr_cap_needed(10, 4, true, 3) == 12);
    const unsigned ns[] = {1, 2, 63, 64, 65, 1023, 1024}, nqs[] = {1, 3, 64, 65};
    for (unsigned a = 0; a < 7; a++)
        for (unsigned b = 0; b < 4; b++) {
            n = ns[a];
            nq = nqs[b];
            // scratch: the pair bytes and the 256 MiB refusal (fetch_k = n)
            const unsigned long long pair = (unsigned long long)nq * n * n * 4;
            CHECK(mmr_pair_bytes(nq, n) == pair);
            CHECK((mmr_check_store(true, nq, false, 768, n) == MMR_PAIRS_TOO_BIG) == (pair > (256ull << 20)));
            CHECK((pair > (256ull << 20)) == (n >= 1023 && nq == 65));  // 64 x 1024^2 x 4 B is exactly the limit; 65 x 1023^2 x 4 B is above it
            for (unsigned k : {1u, n / 2 + 1, n}) {
                const MmrLayout L = mmr_layout(nq, n, k);
                CHECK(L.off_rows == 0 && L.off_rel == (size_t)nq * n * 8 && L.off_n == L.off_rel + (size_t)nq * n * 4 && L.upload_bytes == L.off_n + (size_t)nq * 4);
                CHECK(L.off_picks >= L.upload_bytes && L.off_picks % 256 == 0 && L.off_vals == L.off_picks + (size_t)nq * k * 4 && L.result_bytes == (size_t)nq * k * 8);
                CHECK(L.off_pairs >= L.off_vals + (size_t)nq * k * 4 && L.off_pairs % 256 == 0 && L.total == L.off_pairs + pair);
                CHECK((size_t)nq * n * 12 <= 12288 * (size_t)nq);  // the upload: at most 12 KB of rows and relevances per query
                CHECK(mmr_rounds(k, n) == k && mmr_rounds(k, n / 2) == (k < n / 2 ? k : n / 2));
                CHECK(mmr_needs_pairs(k, n) == (k > 1 && n > 1));
            }
            // the greedy kernel: whole waves, a thread per candidate, at most 1024
            const unsigned t = mmr_greedy_threads(n);
            CHECK(t % 64 == 0 && t >= n && t < n + 64 && t >= 64 && t <= 1024);
            // the pair grid covers every (selected, candidate) pair of every query exactly once; lists shorter than the longest too
            for (unsigned n_q : {n, (n + 1) / 2, 1u}) {
                const MmrGrid g = mmr_pair_grid(nq, n);
                CHECK(g.sel_tiles == (n + 7) / 8 && g.col_tiles == (n + 63) / 64 && g.blocks == (unsigned long long)nq * g.sel_tiles * g.col_tiles && g.blocks < (1ull << 31));
                std::vector<unsigned char> seen((size_t)n_q * n_q);
                unsigned last_q = 0;
                for (unsigned long long blk = 0; blk < g.blocks; blk++) {
                    unsigned q, sel0, col0;
                    mmr_block(g, blk, &q, &sel0, &col0);
                    CHECK(q < nq && sel0 % 8 == 0 && col0 % 64 == 0 && sel0 < g.sel_tiles * 8 && col0 < g.col_tiles * 64);
                    if (q != last_q) {  // query-major: a query's blocks are contiguous
                        CHECK(q == last_q + 1);
                        for (unsigned char v : seen) CHECK(v == 1);
                        memset(seen.data(), 0, seen.size());
                        last_q = q;
                    }
                    if (sel0 >= n_q || col0 >= n_q) continue;  // the kernel's early exit
                    for (unsigned s = sel0; s < sel0 + 8 && s < n_q; s++)
                        for (unsigned c = col0; c < col0 + 64 && c < n_q; c++) seen[(size_t)s * n_q + c]++;
                }
                CHECK(last_q == nq - 1);
                for (unsigned char v : seen) CHECK(v == 1);
            }
        }
    CHECK(mmr_pair_lds_bytes(768) == 8 * 768 * 4 && mmr_pair_lds_bytes(2048) == 65536);
    puts("ok");
    return 0;
}
"""


def test_plan_header_walk_under_asan_ubsan(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = tmp_path / "walk.cpp", tmp_path / "walk"
    src.write_text(WALK)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
