"""CPU: discovery and context search (ott_query_discover, VecStore.discover) without a GPU — a hand-computed case,
the host model's own invariants (tests/discover_ref.py), the planner's refusals, the ABI's device-free argument checks, and a walk
of the HIP-free plan header (ott_discover_plan.h) by a stand-alone C++ program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import discover_ref as D
from otters_amd import Cmp, DiscoverPlan, Metric, OttersError, Path, VecStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")
f32 = np.float32


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


# ---- a hand-computed case ------------------------------------------------------------------------------------------------------------
# dim 3, 6 rows.  Rows 0, 1, 2 are the unit vectors: under dot a row's score against them is its x, y, z.  Pair 0 is (row 0, row 1):
# won where x > y; pair 1 is (row 2, row 1): won where z > y.  Row 1 is the negative of both pairs.
#            x      y      z        pair 0          pair 1           wins  loss     2y
HAND = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1],
                 [0.5, 0.25, 0.125],   # won (+0.25)    lost (-0.125)    1    -0.125   0.5
                 [0.75, 0.5, 0.625],   # won            won              2     0       1.0
                 [0.25, 0.5, 0.125]],  # lost (-0.25)   lost (-0.375)    0    -0.625   1.0
                np.float32)
PAIRS = [(0, 1), (2, 1)]


def test_hand_computed_case(oracle):
    inv = oracle.inv_norms(HAND)
    P = D.pair_scores(oracle, HAND, inv, PAIRS, Metric.DotProduct)
    assert P.shape == (4, 6) and bits(P[0]) == bits(HAND[:, 0]) and bits(P[1]) == bits(HAND[:, 1]) and bits(P[3]) == bits(HAND[:, 1])
    ex = [0, 1, 2]
    # without a target: by the loss, descending
    hits, wins = D.discover(P, 1, 10, examples=ex)
    assert hits["index"].tolist() == [4, 3, 5] and bits(hits["score"]) == bits([0.0, -0.125, -0.625]) and wins.tolist() == [2, 1, 0]
    # a vector target [0, 2, 0] scores 2y: rows 4 and 5 tie at 1.0 and row 3 has 0.5, but the wins come first
    T = D.target_scores(oracle, HAND, inv, [0, 2, 0], Metric.DotProduct)
    assert bits(T) == bits(2 * HAND[:, 1])
    hits, wins = D.discover(P, 1, 10, T=T, examples=ex)
    assert hits["index"].tolist() == [4, 3, 5] and bits(hits["score"]) == bits([1.0, 0.5, 1.0]) and wins.tolist() == [2, 1, 0]
    # k cuts; min_wins drops the rows below it; the filter acts on the target score
    assert D.discover(P, 1, 2, T=T, examples=ex)[0]["index"].tolist() == [4, 3]
    assert D.discover(P, 1, 10, T=T, examples=ex, min_wins=1)[0]["index"].tolist() == [4, 3]
    assert D.discover(P, 1, 10, T=T, examples=ex, min_wins=2)[1].tolist() == [2]
    assert D.discover(P, 1, 10, T=T, examples=ex, cmp=int(Cmp.Gt), thr=0.75)[0]["index"].tolist() == [4, 5]
    # ... and on the loss without a target
    assert D.discover(P, 1, 10, examples=ex, cmp=int(Cmp.Lt), thr=-0.1)[0]["index"].tolist() == [3, 5]
    # a stored row as the target: row 1 scores y and is itself no candidate (it is an example already)
    Trow = P[1]
    hits, wins = D.discover(P, 1, 10, T=Trow, examples=ex + [1])
    assert hits["index"].tolist() == [4, 3, 5] and bits(hits["score"]) == bits([0.5, 0.25, 0.5])
    # a target row that is no example leaves the candidates: row 4
    hits, wins = D.discover(P, 1, 10, T=D.pair_scores(oracle, HAND, inv, [(4, 0)], Metric.DotProduct)[0], examples=ex + [4])
    assert hits["index"].tolist() == [3, 5] and wins.tolist() == [1, 0]
    # take Min: smaller is better — a pair is won where the positive's score is BELOW the negative's, the loss is neg - pos
    hits, wins = D.discover(P, 0, 10, T=T, examples=ex)
    assert hits["index"].tolist() == [5, 3, 4] and bits(hits["score"]) == bits([1.0, 0.5, 1.0]) and wins.tolist() == [2, 1, 0]
    hits, wins = D.discover(P, 0, 10, examples=ex)
    assert hits["index"].tolist() == [5, 3, 4] and bits(hits["score"]) == bits([0.0, -0.25, -0.375]) and wins.tolist() == [2, 1, 0]
    # a mask
    keep = np.array([1, 1, 1, 0, 1, 1], bool)
    assert D.discover(P, 1, 10, T=T, examples=ex, keep=keep)[0]["index"].tolist() == [4, 5]


# ---- the model's own invariants ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric,take", [(Metric.Cosine, 1), (Metric.Euclidean, 0), (Metric.DotProduct, 0), (Metric.Manhattan, 1)])
def test_wins_agree_with_the_loss_terms_and_the_loss_is_never_above_zero(oracle, metric, take):
    rng = np.random.default_rng(21)
    rows = rng.uniform(-1, 1, (300, 13)).astype(np.float32)
    rows[200:204] = rows[7]  # rows that tie with each other
    pairs = [(1, 2), (3, 4), (2, 1), (5, 200), (7, 201)]  # (7, 201): two rows with one vector, never won
    P = D.pair_scores(oracle, rows, oracle.inv_norms(rows), pairs, metric)
    wins, loss, has_nan, terms = D.fold(P, take)
    assert not has_nan.any()
    won = np.stack([D.ordinals(P[2 * i], take) > D.ordinals(P[2 * i + 1], take) for i in range(len(pairs))])
    assert (wins == won.sum(axis=0)).all() and wins.max() <= len(pairs)
    assert (terms[won] == 0).all() and not won[terms < 0].any()  # a won pair adds nothing, a pair with a negative term is lost
    assert not won[4].any() and (terms[4] == 0).all()           # identical examples: never won, +-0 to the loss
    assert (wins + (terms < 0).sum(axis=0) + (P[0::2] == P[1::2]).sum(axis=0) == len(pairs)).all()
    assert (loss <= 0).all() and not np.signbit(loss[loss == 0]).any()  # never above +0; an all-won row keeps +0.0
    assert ((loss == 0) == (terms == 0).all(axis=0)).all()
    # (1, 2) and (2, 1) mirror each other: no row wins both
    assert not (won[0] & won[2]).any()
    # the orders: a hit list is sorted by (wins, ordinal, row) with a target and by (loss ordinal, row) without
    T = P[0]
    hits, w = D.discover(P, take, 300, T=T, examples=[1, 2, 3, 4, 5, 7, 200, 201])
    o = D.ordinals(hits["score"], take).astype(np.int64)
    key = list(zip((-w.astype(np.int64)).tolist(), (-o).tolist(), hits["index"].tolist()))
    assert key == sorted(key) and hits.size == 300 - 8
    hits, w = D.discover(P, take, 300, examples=[1, 2, 3, 4, 5, 7, 200, 201])
    o = D.ordinals(hits["score"], 1).astype(np.int64)
    key = list(zip((-o).tolist(), hits["index"].tolist()))
    assert key == sorted(key)


def test_a_nan_pair_score_removes_the_row_and_inf_minus_inf_counts_zero():
    inf, nan = np.inf, np.nan
    #              row 0   1     2     3
    P = np.array([[inf, 1.0, nan, -inf],   # pair 0's positive
                  [inf, 2.0, 0.0, -inf],   # pair 0's negative
                  [0.0, -0.0, 1.0, 5.0],   # pair 1's positive
                  [-0.0, 0.0, 0.0, inf]], f32)
    wins, loss, has_nan, terms = D.fold(P, 1)
    assert has_nan.tolist() == [False, False, True, False]
    assert wins.tolist()[:2] == [1, 0] and wins[3] == 0        # +0 above -0 under Max; inf against inf is no win
    assert bits(loss[[0, 1, 3]]) == bits([0.0, -1.0, -inf])     # inf - inf = NaN counts 0; 5 - inf = -inf
    hits, w = D.discover(P, 1, 4)
    assert hits["index"].tolist() == [0, 1, 3] and w.tolist() == [1, 0, 0]


# ---- the planner ---------------------------------------------------------------------------------------------------------------------

def fake_store(n=100, devices=None):
    store = VecStore.__new__(VecStore)
    store.dim, store._n, store._n_groups, store.devices = 4, n, 0, devices
    return store


def refused(plan, text):
    with pytest.raises(OttersError) as e:
        plan.validate()
    assert text in str(e.value), str(e.value)


def test_planner_refusals_and_messages():
    s = fake_store()
    q = np.ones(4, f32)
    refused(s.discover([]), "ott_query_discover: between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed")
    refused(s.discover([(i, i + 1) for i in range(33)]), "ott_query_discover: between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed")
    refused(s.discover([(1, 2)], target=np.ones((2, 4), f32)), "ott_query_discover: at most one target vector (d->nq <= 1)")
    refused(s.discover([(1, 2)], target=np.ones(5, f32)), "Query vector length 5 does not match expected dimension 4")
    refused(s.discover([(1, 2)], target=q, target_row=3), "ott_query_discover: a target vector and a target row are both given")
    refused(s.discover([(1, 2)]).min_wins(2), "ott_query_discover: min_wins is above the number of pairs")
    refused(s.discover([(1, 2)]).with_path(Path.Mfma), "ott_query_discover: the MFMA path does not serve discovery queries; use path AUTO or EXACT")
    refused(fake_store(devices=[0, 0]).discover([(1, 2)]), "ott_query_discover: a multi-GPU store is not served")
    refused(s.discover([(1, 100)]), "ott_query_discover: row id 100 is not below the store's length 100")
    refused(s.discover([(100, 1)]), "ott_query_discover: row id 100 is not below the store's length 100")
    refused(s.discover([(1, 2)], target_row=100), "ott_query_discover: row id 100 is not below the store's length 100")
    refused(s.discover([(1, 2), (5, 5)]), "ott_query_discover: row 5 is both the positive and the negative of a pair")
    refused(s.discover([(-1, 2)]), "row id -1 is negative")
    refused(s.discover([(1, 2, 3)]), "the context is a sequence of (positive, negative) row id pairs")
    # two faults at once: the one the library's walk meets first is named (pair by pair, the target row last)
    refused(s.discover([(5, 5), (1, 400)]), "row 5 is both the positive and the negative of a pair")
    refused(s.discover([(1, 400), (5, 5)]), "row id 400 is not below the store's length 100")
    refused(s.discover([(5, 5)], target_row=400), "row 5 is both the positive and the negative of a pair")
    refused(s.discover([(1, 400)]).min_wins(3), "min_wins is above the number of pairs")
    # nothing is deduplicated: one row in many pairs, on either side, is fine — and so are 32 pairs
    s.discover([(1, 2), (2, 1), (1, 3), (1, 2)]).validate()
    s.discover([(i, i + 1) for i in range(32)], target_row=50).min_wins(32).validate()


def test_planner_defaults_and_lowering():
    s = fake_store()
    p = s.discover([(5, 6), (5, 7)])
    assert isinstance(p, DiscoverPlan)
    rd = p.resolve()
    assert rd.metric == int(Metric.Cosine) and rd.take == 1 and rd.k == 100 and rd.min_wins == 0 and rd.path == int(Path.Auto)
    assert rd.positive.dtype == np.uint64 and rd.positive.tolist() == [5, 5] and rd.negative.tolist() == [6, 7]
    assert rd.target is None and rd.target_row == 2 ** 64 - 1
    rd = (s.discover([(5, 6)], target=[1, 2, 3, 4], metric=Metric.Euclidean).take(3).filter(0.5, Cmp.Lt).min_wins(1).with_row_mask([True, False])
          .with_path(Path.Exact).resolve())
    assert (rd.take, rd.k, rd.filter_cmp, rd.filter_thr, rd.min_wins, rd.path) == (0, 3, int(Cmp.Lt), 0.5, 1, int(Path.Exact)) and rd.row_mask.tolist() == [True, False]
    assert rd.target.dtype == np.float32 and rd.target.tolist() == [1, 2, 3, 4] and rd.target_row == 2 ** 64 - 1
    assert s.discover([(5, 6)], target_row=9).resolve().target_row == 9
    assert s.discover([(5, 6)], metric=Metric.Manhattan).take_max(2).resolve().take == 1
    assert s.discover([(5, 6)], metric=Metric.DotProduct).take_min(2).resolve().take == 0


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------

PROTOTYPE = """int ott_query_discover(ott_store* s, const ott_query_desc* d, uint64_t target_row, const uint64_t* positive, const uint64_t* negative,
                       uint64_t n_pairs, uint32_t min_wins, uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out,
                       uint32_t* wins_of_hit , ott_stats* stats);"""
NO_ROW = 2 ** 64 - 1


def test_header_declares_the_call_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert "#define OTT_ABI_VERSION 4" in src and "#define OTT_DISCOVER_MAX_PAIRS 32" in src and "#define OTT_NO_ROW UINT64_MAX" in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ott_discover.hip" in mk  # one source list for the product and the audit build


def test_library_exports_it_and_checks_its_arguments_without_a_device():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    assert hasattr(L, "ott_query_discover")
    out = np.zeros(4, dtype=N.HIT_DTYPE)
    wins = np.full(4, 7, np.uint32)
    n_out = C.c_uint64(9)
    pos, neg = np.array([1, 2], np.uint64), np.array([3, 4], np.uint64)
    q = np.zeros(8, np.float32)

    def desc(**kw):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.k = None, 0, int(Metric.Cosine), 1, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, p=pos, n=neg, n_pairs=2, target_row=NO_ROW, min_wins=0, flags=0):
        return L.ott_query_discover(None, C.byref(d) if d is not None else None, target_row, N.ptr(p) if p is not None else None, N.ptr(n) if n is not None else None,
                                    n_pairs, min_wins, flags, N.ptr(out), 4, C.byref(n_out), N.ptr(wins), None)

    assert call(None) == -1 and b"desc is NULL" in L.ott_last_error()
    assert call(desc(), n_pairs=0) == -1 and b"ott_query_discover: between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed" in L.ott_last_error()
    assert call(desc(), n_pairs=33) == -1 and b"between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed" in L.ott_last_error()
    assert call(desc(), p=None) == -1 and b"ott_query_discover: a pair list is NULL" in L.ott_last_error()
    assert call(desc(), n=None) == -1 and b"ott_query_discover: a pair list is NULL" in L.ott_last_error()
    assert call(desc(), flags=1) == -1 and b"ott_query_discover: flags must be 0" in L.ott_last_error()
    assert call(desc(nq=2, queries=q.ctypes.data)) == -1 and b"ott_query_discover: at most one target vector (d->nq <= 1)" in L.ott_last_error()
    assert call(desc(nq=1)) == -1 and b"d->queries and d->nq disagree" in L.ott_last_error()
    assert call(desc(queries=q.ctypes.data)) == -1 and b"d->queries and d->nq disagree" in L.ott_last_error()
    assert call(desc(nq=1, queries=q.ctypes.data), target_row=5) == -1 and b"ott_query_discover: a target vector and a target row are both given" in L.ott_last_error()
    assert call(desc(), min_wins=3) == -1 and b"ott_query_discover: min_wins is above the number of pairs" in L.ott_last_error()
    assert call(desc(mode=1)) == -4 and b"ott_query_discover: the context makes ONE query; PER_QUERY is not served" in L.ott_last_error()
    assert call(desc(path=2)) == -4 and b"ott_query_discover: the MFMA path does not serve discovery queries" in L.ott_last_error()
    assert call(desc(metric=9)) == -1 and b"unknown metric" in L.ott_last_error()
    assert call(desc(), min_wins=2) == -1 and b"store is NULL" in L.ott_last_error()  # valid arguments: the NULL store is what is left to refuse
    assert call(desc(nq=1, queries=q.ctypes.data)) == -1 and b"store is NULL" in L.ott_last_error()
    assert call(desc(), target_row=5) == -1 and b"store is NULL" in L.ott_last_error()
    assert n_out.value == 9 and not out["index"].any() and (wins == 7).all()  # nothing was touched


def test_audit_build_exports_it():
    import sys
    subprocess.check_call(["make", "-C", CSRC, "-j", "8", "-s", "audit"])
    # (loaded in a child: two builds of one library do not belong in one process)
    code = "import ctypes, sys; A = ctypes.CDLL(sys.argv[1]); [getattr(A, n) for n in sys.argv[2:]]"
    subprocess.check_call([sys.executable, "-c", code, os.path.join(CSRC, "libotters_hip_audit.so"), "ott_query_discover"])


# ---- the plan header: a stand-alone program under ASan + UBSan -----------------------------------------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <vector>
#include "ott_discover_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (n %u)\n", __LINE__, #c, n); return 1; } } while (0)
static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }
// the cut by brute force: the candidates' wins sorted descending, the level of the k-th (0 when there are fewer than k)
static uint32_t brute(const std::vector<uint32_t>& hist, uint64_t k, uint64_t* above) {
    std::vector<uint32_t> w;
    for (uint32_t l = 0; l < hist.size(); l++) w.insert(w.end(), hist[l], l);
    std::sort(w.begin(), w.end(), std::greater<uint32_t>());
    const uint32_t cut = w.size() >= k ? w[k - 1] : 0u;
    *above = 0;
    for (uint32_t x : w) *above += x > cut;
    return cut;
}
int main() {
    unsigned n = 0;
    CHECK(DISC_MAX_PAIRS == 32 && DISC_MAX_SLOTS == 65 && DISC_NO_ROW == ~0ull && DISC_NQ == 4 && DISC_MAX_ROWS == 0xFFFFFFF0ull && DISC_LEVELS == 33);
    // the arguments, in the order the call refuses them: (n_pairs, positive NULL, negative NULL, flags, nq, queries NULL, target row, min_wins, per_query, mfma)
    CHECK(disc_check_args(0, true, true, 1, 2, true, true, 99, true, true) == DISC_BAD_PAIRS && disc_check_args(33, false, false, 0, 0, true, false, 0, false, false) == DISC_BAD_PAIRS);
    CHECK(disc_check_args(1, true, false, 1, 2, true, true, 99, true, true) == DISC_NULL_LIST && disc_check_args(1, false, true, 1, 2, true, true, 99, true, true) == DISC_NULL_LIST);
    CHECK(disc_check_args(1, false, false, 1, 2, true, true, 99, true, true) == DISC_BAD_FLAGS && disc_check_args(1, false, false, 0x80000000u, 0, true, false, 0, false, false) == DISC_BAD_FLAGS);
    CHECK(disc_check_args(1, false, false, 0, 2, true, true, 99, true, true) == DISC_MANY_QUERIES);
    CHECK(disc_check_args(1, false, false, 0, 1, true, true, 99, true, true) == DISC_NULL_QUERY && disc_check_args(1, false, false, 0, 0, false, true, 99, true, true) == DISC_NULL_QUERY);
    CHECK(disc_check_args(1, false, false, 0, 1, false, true, 99, true, true) == DISC_BOTH_TARGETS);
    CHECK(disc_check_args(1, false, false, 0, 1, false, false, 2, true, true) == DISC_BAD_MIN_WINS && disc_check_args(32, false, false, 0, 0, true, true, 33, true, true) == DISC_BAD_MIN_WINS);
    CHECK(disc_check_args(1, false, false, 0, 1, false, false, 1, true, true) == DISC_PER_QUERY && disc_check_args(1, false, false, 0, 0, true, true, 0, false, true) == DISC_MFMA);
    CHECK(disc_check_args(1, false, false, 0, 1, false, false, 1, false, false) == DISC_OK && disc_check_args(32, false, false, 0, 0, true, true, 32, false, false) == DISC_OK &&
          disc_check_args(7, false, false, 0, 0, true, false, 0, false, false) == DISC_OK);
    CHECK(disc_check_store(true, 1ull << 40) == DISC_MULTI_GPU && disc_check_store(false, 0xFFFFFFF1ull) == DISC_TOO_MANY_ROWS && disc_check_store(false, 0xFFFFFFF0ull) == DISC_OK);
    for (int r = DISC_BAD_PAIRS; r <= DISC_NULL_OUT; r++)
        CHECK(disc_refusal_is_invalid((DiscRefusal)r) == !(r == DISC_PER_QUERY || r == DISC_MFMA || r == DISC_MULTI_GPU || r == DISC_TOO_MANY_ROWS));
    CHECK(!disc_refusal_is_invalid(DISC_OK));
    // the slots: pair i at 2i and 2i + 1, nothing deduplicated, the target behind the pairs
    DiscSlots sl;
    uint64_t bad = 0;
    {
        const uint64_t pos[] = {7, 3, 7, 1}, neg[] = {1, 7, 1, 3};
        CHECK(disc_slots(pos, neg, 4, DISC_NO_ROW, false, 10, &sl, &bad) == DISC_OK);
        CHECK(sl.n_pairs == 4 && sl.n_gather == 8 && sl.n_slots == 8 && sl.target == DISC_TARGET_NONE && disc_target_slot(sl) == 0xFFFFFFFFu);
        const uint32_t want[] = {7, 1, 3, 7, 7, 1, 1, 3};
        CHECK(memcmp(sl.rows, want, sizeof(want)) == 0);
        CHECK(disc_slots(pos, neg, 4, 9, false, 10, &sl, &bad) == DISC_OK && sl.n_gather == 9 && sl.n_slots == 9 && sl.rows[8] == 9 && sl.target == DISC_TARGET_ROW && disc_target_slot(sl) == 8);
        CHECK(disc_slots(pos, neg, 4, 7, false, 10, &sl, &bad) == DISC_OK && sl.rows[8] == 7);  // the target row may be an example too
        CHECK(disc_slots(pos, neg, 4, DISC_NO_ROW, true, 10, &sl, &bad) == DISC_OK && sl.n_gather == 8 && sl.n_slots == 9 && sl.target == DISC_TARGET_VECTOR && disc_target_slot(sl) == 8);
        CHECK(disc_slots(pos, neg, 4, 10, false, 10, &sl, &bad) == DISC_BAD_ID && bad == 10);
        CHECK(disc_slots(pos, neg, 4, DISC_NO_ROW, false, 7, &sl, &bad) == DISC_BAD_ID && bad == 7);
        CHECK(disc_slots(pos, neg, 4, DISC_NO_ROW, false, 4, &sl, &bad) == DISC_BAD_ID && bad == 7);
        const uint64_t neg2[] = {1, 3, 1, 3};
        CHECK(disc_slots(pos, neg2, 4, DISC_NO_ROW, false, 10, &sl, &bad) == DISC_SAME_ROW && bad == 3);
        // two faults in one call: the first one the walk meets is reported
        const uint64_t neg3[] = {1, 3, 99, 3}, neg4[] = {99, 3, 1, 3};
        CHECK(disc_slots(pos, neg3, 4, 99, false, 10, &sl, &bad) == DISC_SAME_ROW && bad == 3);
        CHECK(disc_slots(pos, neg4, 4, 99, false, 10, &sl, &bad) == DISC_BAD_ID && bad == 99);
        const uint64_t big[] = {1ull << 32}, zero[] = {0};  // an id that only differs above 32 bits is out of range, not the same row
        CHECK(disc_slots(big, zero, 1, DISC_NO_ROW, false, 100, &sl, &bad) == DISC_BAD_ID && bad == (1ull << 32));
    }
    // passes for 1 .. 32 pairs, with and without a target: four slots per pass; the target rides in an odd count's free slots
    for (n = 1; n <= 32; n++) {
        const unsigned without = disc_passes(n, false), with = disc_passes(n, true);
        CHECK(without == (2 * n + 3) / 4 && with == (2 * n + 1 + 3) / 4);
        CHECK(without == (n + 1) / 2 && with == (n % 2 ? without : without + 1));
        CHECK(with * DISC_NQ >= 2 * n + 1 && (with - 1) * DISC_NQ < 2 * n + 1 && without * DISC_NQ >= 2 * n && (without - 1) * DISC_NQ < 2 * n);
        std::vector<uint64_t> pos(n), neg(n);
        for (unsigned i = 0; i < n; i++) pos[i] = 2 * i, neg[i] = 2 * i + 1;
        CHECK(disc_slots(pos.data(), neg.data(), n, 5, false, 100, &sl, &bad) == DISC_OK && sl.n_slots == 2 * n + 1 && disc_target_slot(sl) % 2 == 0);
        for (unsigned e = 0; e < 2 * n; e++) CHECK(sl.rows[e] == e);
    }
    n = 0;
    CHECK(disc_passes(1, false) == 1 && disc_passes(1, true) == 1 && disc_passes(2, true) == 2 && disc_passes(3, true) == 2 && disc_passes(32, true) == 17 && disc_passes(32, false) == 16);
    CHECK(disc_k_eff(10, 4) == 4 && disc_k_eff(10, 40) == 10 && disc_k_eff(0, 40) == 0 && disc_k_eff(~0ull, 7) == 7);
    CHECK(disc_check_out(5, 4, false) == DISC_SMALL_CAP && disc_check_out(5, 5, true) == DISC_NULL_OUT && disc_check_out(0, 0, true) == DISC_OK && disc_check_out(5, 9, false) == DISC_OK);
    CHECK(disc_state_bytes(0xFFFFFFF0ull) == 0xFFFFFFF0ull * 8 && disc_key_bytes(2000) == 16000);
    CHECK(sizeof(DiscAbove) == 16 && DISC_HDR_CURSOR >= DISC_LEVELS && DISC_HDR_CURSOR < DISC_HDR_WORDS);
    CHECK(disc_scratch_bytes(true, 2000, 10) == 256 + 160 && disc_scratch_bytes(false, 2000, 10) == 256 + 2000 && disc_scratch_bytes(false, 2001, 10) % 16 == 0 &&
          disc_scratch_bytes(false, 2001, 10) >= 256 + 2001);
    // the level cut against a brute-force sort of random histograms
    for (n = 0; n < 4000; n++) {
        const uint32_t levels = 2 + (uint32_t)(rnd() % 32);  // 1 .. 32 pairs
        std::vector<uint32_t> hist(levels);
        const unsigned shape = n % 4;
        for (uint32_t l = 0; l < levels; l++) hist[l] = shape == 0 ? (uint32_t)(rnd() % 40) : shape == 1 ? (rnd() % 4 == 0 ? (uint32_t)(rnd() % 9) : 0u) : 0u;
        if (shape >= 2) hist[rnd() % levels] = 1 + (uint32_t)(rnd() % 50);  // every row on one level
        uint64_t total = 0;
        for (uint32_t h : hist) total += h;
        uint64_t ks[8] = {1, 1 + rnd() % (total + 1), total, total + 1, total + 7, 2, 0, 0};
        // ... a level that fills k exactly: k = the cumulative count down to a level
        uint64_t cum = 0;
        unsigned nk = 6;
        for (uint32_t l = levels; l-- > 0 && nk < 8;) {
            cum += hist[l];
            if (hist[l] != 0 && rnd() % 2) ks[nk++] = cum;
        }
        for (unsigned i = 0; i < nk; i++) {
            const uint64_t k = ks[i];
            if (k == 0) continue;
            uint64_t above = ~0ull, want_above = 0;
            const uint32_t cut = disc_level_cut(hist.data(), levels, k, &above), want = brute(hist, k, &want_above);
            CHECK(cut == want && above == want_above && above < k && cut < levels);
            if (total >= k) CHECK(above + hist[cut] >= k);
            else CHECK(cut == 0 && above == total - hist[0]);
        }
    }
    n = 0;
    {
        const uint32_t h[5] = {100, 0, 7, 0, 3};
        uint64_t a = 0;
        CHECK(disc_level_cut(h, 5, 3, &a) == 4 && a == 0);    // the top level fills k exactly
        CHECK(disc_level_cut(h, 5, 4, &a) == 2 && a == 3);
        CHECK(disc_level_cut(h, 5, 10, &a) == 2 && a == 3);   // 3 + 7 fill k exactly
        CHECK(disc_level_cut(h, 5, 11, &a) == 0 && a == 10);
        CHECK(disc_level_cut(h, 5, 110, &a) == 0 && a == 10);
        CHECK(disc_level_cut(h, 5, 500, &a) == 0 && a == 10); // total below k
    }
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
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
