"""CPU: recommend by example rows (ott_query_recommend, VecStore.recommend) without a GPU — the host model's own
self-checks (tests/recommend_ref.py), a hand-computed case, the planner's refusals, the ABI's device-free argument checks, and a
walk of the HIP-free plan header (ott_recommend_plan.h) by a stand-alone C++ program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import manhattan_ref as M
import recommend_ref as R
from otters_amd import Cmp, Metric, OttersError, Path, RecommendPlan, VecStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")
f32 = np.float32


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


# ---- the host model ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(11)
    return rng.uniform(-1, 1, (300, 13)).astype(np.float32)


@pytest.mark.parametrize("metric,take", [(Metric.DotProduct, 1), (Metric.Euclidean, 0), (Metric.Manhattan, 0), (Metric.DotProduct, 0)])
def test_one_positive_is_the_plain_top_k_of_that_row_with_itself_masked(oracle, corpus, metric, take):
    rows = corpus
    e = 17
    hits, side = R.recommend(oracle, rows, None, [e], [], metric, take, 12)
    mask = np.ones(rows.shape[0], bool)
    mask[e] = False
    if metric == Metric.Manhattan:
        exp = M.select_canonical(M.scores(rows, rows[e][None, :], "l1", 0), take, 12, 0, 0.0, mask)
    else:
        exp = oracle.vec_query(rows, rows[e][None, :], int(metric), take, 12, 0, 0.0, row_mask=mask, ties=oracle.TIES_CANONICAL)
    assert hits["index"].tolist() == exp["index"].tolist() and bits(hits["score"]) == bits(exp["score"])
    assert side.tolist() == [1] * 12


def test_without_negatives_the_fill_flag_changes_nothing(oracle, corpus):
    a = R.recommend(oracle, corpus, oracle.inv_norms(corpus), [3, 9, 3], [], Metric.Cosine, 1, 20, flags=R.FILL)
    b = R.recommend(oracle, corpus, oracle.inv_norms(corpus), [3, 9, 3], [], Metric.Cosine, 1, 20, flags=0)
    R.same(a, b)
    assert a[1].tolist() == [1] * 20 and 3 not in a[0]["index"] and 9 not in a[0]["index"]


def test_ordinals_decode_and_follow_the_total_order():
    v = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-45, 2.5, np.inf], f32)
    for take in (0, 1):
        o = R.ordinals(v, take)
        assert (o != 0).all() and bits(R.decode(o, take)) == bits(v)
        assert (np.diff(o.astype(np.int64)) > 0).all() if take == 1 else (np.diff(o.astype(np.int64)) < 0).all()  # +0.0 above -0.0 under Max
    assert R.ordinals(np.array([np.nan], f32), 1)[0] == 0


# rows 0 and 1 are the examples: the positive [1, 0] scores a row's x under dot, the negative [0, 1] its y
HAND = np.array([[1, 0], [0, 1], [0.5, 0.25], [0.25, 0.5], [0.75, 0.125], [0.625, 0.625]], np.float32)


def test_hand_computed_case(oracle):
    # positives alone: every row on the positive side, by x descending
    hits, side = R.recommend(oracle, HAND, None, [0], [], Metric.DotProduct, 1, 10)
    assert hits["index"].tolist() == [4, 5, 2, 3, 1] and bits(hits["score"]) == bits([0.75, 0.625, 0.5, 0.25, 0.0]) and side.tolist() == [1] * 5
    # row 1 becomes a negative: row 3 (x 0.25 < y 0.5) and row 5 (x == y: as close to the negative as to the positive) leave the
    # positive side — row 5 falls from second place to last — and follow it by y ASCENDING, with y as their score
    hits, side = R.recommend(oracle, HAND, None, [0], [1], Metric.DotProduct, 1, 10)
    assert hits["index"].tolist() == [4, 2, 3, 5] and bits(hits["score"]) == bits([0.75, 0.5, 0.5, 0.625]) and side.tolist() == [1, 1, 0, 0]
    # without the flag the negative side never comes out; k cuts the joined list
    hits, side = R.recommend(oracle, HAND, None, [0], [1], Metric.DotProduct, 1, 10, flags=0)
    assert hits["index"].tolist() == [4, 2] and side.tolist() == [1, 1]
    hits, side = R.recommend(oracle, HAND, None, [0], [1], Metric.DotProduct, 1, 3)
    assert hits["index"].tolist() == [4, 2, 3] and side.tolist() == [1, 1, 0]
    # the filter acts on BP on both sides: x > 0.25 drops row 3 (bp 0.25), keeps row 5 (bp 0.625) on the negative side
    hits, side = R.recommend(oracle, HAND, None, [0], [1], Metric.DotProduct, 1, 10, cmp=int(Cmp.Gt), thr=0.25)
    assert hits["index"].tolist() == [4, 2, 5] and side.tolist() == [1, 1, 0]
    # take Min: smaller is better — the positive side holds the rows whose x is BELOW their y; the negative side starts with the LARGEST y
    hits, side = R.recommend(oracle, HAND, None, [0], [1], Metric.DotProduct, 0, 10)
    assert hits["index"].tolist() == [3, 5, 2, 4] and bits(hits["score"]) == bits([0.25, 0.625, 0.25, 0.125]) and side.tolist() == [1, 0, 0, 0]


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
    refused(s.recommend([], [1]), "ott_query_recommend: at least one positive example is needed")
    refused(s.recommend([100]), "ott_query_recommend: example id 100 is not below the store's length 100")
    refused(s.recommend([1], [2, 400]), "ott_query_recommend: example id 400 is not below the store's length 100")
    refused(s.recommend([1, 2], [3, 2]), "ott_query_recommend: row 2 is listed as both a positive and a negative example")
    refused(s.recommend(list(range(40)), list(range(40, 65))), "ott_query_recommend: more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples")
    refused(s.recommend([-1]), "row id -1 is negative")
    refused(s.recommend([1]).with_path(Path.Mfma), "ott_query_recommend: the MFMA path does not serve recommend queries; use path AUTO or EXACT")
    refused(fake_store(devices=[0, 0]).recommend([1]), "ott_query_recommend: a multi-GPU store is not served")
    # two faults at once: the one the library's walk meets first is named, as by the ABI (positives first, id by id)
    refused(s.recommend(list(range(70)), [400]), "more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples")
    refused(s.recommend(list(range(64)) + [400] + [64], []), "example id 400 is not below the store's length 100")
    refused(s.recommend([1, 2], [2, 400]), "row 2 is listed as both a positive and a negative example")
    refused(s.recommend([1, 2], [400, 2]), "example id 400 is not below the store's length 100")
    # duplicates count once: 64 distinct ids listed three times over are the limit, not above it
    s.recommend(list(range(40)) * 3, list(range(40, 64)) * 2).validate()


def test_planner_defaults_and_lowering():
    s = fake_store()
    p = s.recommend([5, 5, 6], [7])
    assert isinstance(p, RecommendPlan)
    rr = p.resolve()
    assert rr.metric == int(Metric.Cosine) and rr.take == 1 and rr.k == 100 and rr.flags == 1 and rr.path == int(Path.Auto)
    assert rr.positive.dtype == np.uint64 and rr.positive.tolist() == [5, 5, 6] and rr.negative.tolist() == [7]
    rr = s.recommend([5], metric=Metric.Euclidean).take(3).filter(0.5, Cmp.Lt).fill_negative_side(False).with_row_mask([True, False]).with_path(Path.Exact).resolve()
    assert (rr.take, rr.k, rr.filter_cmp, rr.filter_thr, rr.flags, rr.path) == (0, 3, int(Cmp.Lt), 0.5, 0, int(Path.Exact)) and rr.row_mask.tolist() == [True, False]
    assert s.recommend([5], metric=Metric.Manhattan).take_max(2).resolve().take == 1
    assert s.recommend([5], metric=Metric.DotProduct).take_min(2).resolve().take == 0


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------

PROTOTYPE = """int ott_query_recommend(ott_store* s, const ott_query_desc* d, const uint64_t* positive, uint64_t n_positive, const uint64_t* negative,
                        uint64_t n_negative, uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out,
                        uint32_t* side_of_hit , ott_stats* stats);"""


def test_header_declares_the_call_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert "#define OTT_ABI_VERSION 4" in src and "#define OTT_RECOMMEND_MAX_EXAMPLES 64" in src and "#define OTT_RECOMMEND_FILL 1u" in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ott_recommend.hip" in mk  # one source list for the product and the audit build


def test_library_exports_it_and_checks_its_arguments_without_a_device():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    assert hasattr(L, "ott_query_recommend")
    out = np.zeros(4, dtype=N.HIT_DTYPE)
    sides = np.full(4, 7, np.uint32)
    n_out = C.c_uint64(9)
    pos, neg = np.array([1, 2], np.uint64), np.array([3], np.uint64)
    q = np.zeros(4, np.float32)

    def desc(**kw):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.k = None, 0, int(Metric.Cosine), 1, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, p=pos, n_p=2, n=neg, n_n=1, flags=1):
        return L.ott_query_recommend(None, C.byref(d) if d is not None else None, N.ptr(p) if p is not None else None, n_p, N.ptr(n) if n is not None else None, n_n,
                                     flags, N.ptr(out), 4, C.byref(n_out), N.ptr(sides), None)

    assert call(None) == -1 and b"desc is NULL" in L.ott_last_error()
    assert call(desc(), n_p=0) == -1 and b"ott_query_recommend: at least one positive example is needed" in L.ott_last_error()
    assert call(desc(), p=None) == -1 and b"ott_query_recommend: an example list is NULL" in L.ott_last_error()
    assert call(desc(), n=None) == -1 and b"ott_query_recommend: an example list is NULL" in L.ott_last_error()
    assert call(desc(), flags=2) == -1 and b"ott_query_recommend: unknown flag bits" in L.ott_last_error()
    assert call(desc(), flags=0x80000001) == -1 and b"unknown flag bits" in L.ott_last_error()
    assert call(desc(nq=1)) == -1 and b"d->queries must be NULL and d->nq 0" in L.ott_last_error()
    assert call(desc(queries=q.ctypes.data)) == -1 and b"d->queries must be NULL and d->nq 0" in L.ott_last_error()
    assert call(desc(mode=1)) == -4 and b"ott_query_recommend: the examples make ONE query; PER_QUERY is not served" in L.ott_last_error()
    assert call(desc(path=2)) == -4 and b"ott_query_recommend: the MFMA path does not serve recommend queries" in L.ott_last_error()
    assert call(desc(metric=9)) == -1 and b"unknown metric" in L.ott_last_error()
    assert call(desc(), n=None, n_n=0) == -1 and b"store is NULL" in L.ott_last_error()  # valid arguments: the NULL store is what is left to refuse
    assert call(desc()) == -1 and b"store is NULL" in L.ott_last_error()
    assert n_out.value == 9 and not out["index"].any() and (sides == 7).all()  # nothing was touched


def test_audit_build_exports_it():
    import sys
    subprocess.check_call(["make", "-C", CSRC, "-j", "8", "-s", "audit"])
    # (loaded in a child: two builds of one library do not belong in one process)
    code = "import ctypes, sys; A = ctypes.CDLL(sys.argv[1]); [getattr(A, n) for n in sys.argv[2:]]"
    subprocess.check_call([sys.executable, "-c", code, os.path.join(CSRC, "libotters_hip_audit.so"), "ott_query_recommend"])


# ---- the plan header: a stand-alone program under ASan + UBSan -----------------------------------------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ott_recommend_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (n %u)\n", __LINE__, #c, n); return 1; } } while (0)
int main() {
    unsigned n = 0;
    CHECK(REC_MAX_EXAMPLES == 64 && REC_FILL == 1 && REC_NQ == 4 && REC_MAX_ROWS == 0xFFFFFFF0ull);
    // the arguments, in the order the call refuses them
    CHECK(rec_check_args(true, 0, true, 0, 2, true, true, true) == REC_NO_POSITIVE);
    CHECK(rec_check_args(true, 1, false, 0, 2, true, true, true) == REC_NULL_LIST && rec_check_args(false, 1, true, 1, 2, true, true, true) == REC_NULL_LIST);
    CHECK(rec_check_args(false, 1, true, 0, 2, true, true, true) == REC_BAD_FLAGS && rec_check_args(false, 1, true, 0, 0x80000001u, false, false, false) == REC_BAD_FLAGS);
    CHECK(rec_check_args(false, 1, true, 0, 1, true, true, true) == REC_HAS_QUERIES);
    CHECK(rec_check_args(false, 1, true, 0, 1, false, true, true) == REC_PER_QUERY && rec_check_args(false, 1, true, 0, 0, false, false, true) == REC_MFMA);
    CHECK(rec_check_args(false, 1, true, 0, 1, false, false, false) == REC_OK && rec_check_args(false, 9, false, 9, 0, false, false, false) == REC_OK);
    CHECK(rec_check_store(true, 1ull << 40) == REC_MULTI_GPU && rec_check_store(false, 0xFFFFFFF1ull) == REC_TOO_MANY_ROWS && rec_check_store(false, 0xFFFFFFF0ull) == REC_OK);
    for (int r = REC_NO_POSITIVE; r <= REC_NULL_OUT; r++)
        CHECK(rec_refusal_is_invalid((RecRefusal)r) == !(r == REC_PER_QUERY || r == REC_MFMA || r == REC_MULTI_GPU || r == REC_TOO_MANY_ROWS));
    CHECK(!rec_refusal_is_invalid(REC_OK));
    // the examples: distinct positives in first-occurrence order, then the distinct negatives
    RecExamples ex;
    uint64_t bad = 0;
    {
        const uint64_t pos[] = {7, 3, 7, 7, 9, 3}, neg[] = {1, 1, 0};
        CHECK(rec_examples(pos, 6, neg, 3, 10, &ex, &bad) == REC_OK);
        CHECK(ex.n == 5 && ex.first_neg == 3 && ex.rows[0] == 7 && ex.rows[1] == 3 && ex.rows[2] == 9 && ex.rows[3] == 1 && ex.rows[4] == 0);
        CHECK(rec_examples(pos, 6, nullptr, 0, 10, &ex, &bad) == REC_OK && ex.n == 3 && ex.first_neg == 3);
        CHECK(rec_examples(pos, 6, neg, 3, 9, &ex, &bad) == REC_BAD_ID && bad == 9);
        const uint64_t neg2[] = {1, 9};
        CHECK(rec_examples(pos, 6, neg2, 2, 10, &ex, &bad) == REC_BOTH_SIDES && bad == 9);
        // two faults in one call: the first one the walk meets is reported
        const uint64_t neg3[] = {9, 99}, neg4[] = {99, 9};
        CHECK(rec_examples(pos, 6, neg3, 2, 10, &ex, &bad) == REC_BOTH_SIDES && bad == 9);
        CHECK(rec_examples(pos, 6, neg4, 2, 10, &ex, &bad) == REC_BAD_ID && bad == 99);
        const uint64_t big[] = {5, 1ull << 32};  // an id that only differs from a listed one above 32 bits is out of range, not a duplicate
        CHECK(rec_examples(big, 2, nullptr, 0, 100, &ex, &bad) == REC_BAD_ID && bad == (1ull << 32));
    }
    // the limit counts DISTINCT ids over both lists; long lists of duplicates are fine
    for (n = 1; n <= 70; n++) {
        std::vector<uint64_t> pos, neg;
        for (unsigned rep = 0; rep < 3; rep++)
            for (unsigned i = 0; i < n; i++) (i % 3 == 2 ? neg : pos).push_back(1000 + i);
        const RecRefusal r = rec_examples(pos.data(), pos.size(), neg.empty() ? nullptr : neg.data(), neg.size(), 5000, &ex, &bad);
        CHECK((r == REC_OK) == (n <= 64) && (r == REC_OK || r == REC_TOO_MANY));
        if (r != REC_OK) continue;
        CHECK(ex.n == n && ex.first_neg == n - n / 3);
        std::vector<unsigned char> seen(n);
        for (unsigned e = 0; e < ex.n; e++) {
            const unsigned i = ex.rows[e] - 1000;
            CHECK(i < n && !seen[i] && (i % 3 == 2) == (e >= ex.first_neg));
            seen[i] = 1;
        }
        // passes and slots: one example is one single-query pass, more take four per pass; the padded block holds every pass whole
        const unsigned tile = rec_tile(n), passes = rec_passes(n), slots = rec_slots(n);
        CHECK(tile == (n == 1 ? 1u : 4u) && passes == (n == 1 ? 1u : (n + 3) / 4) && passes * tile >= n && (passes - 1) * tile < n);
        CHECK(slots % 8 == 0 && slots >= n && slots < n + 8 && passes * tile <= slots);
        // the second round
        CHECK(rec_fill_possible(1, ex) == (ex.first_neg < ex.n) && !rec_fill_possible(0, ex));
    }
    n = 0;
    CHECK(rec_second_k(true, 10, 4) == 6 && rec_second_k(true, 10, 10) == 0 && rec_second_k(false, 10, 4) == 0 && rec_second_k(true, 10, 0) == 10);
    CHECK(rec_k_eff(10, 4) == 4 && rec_k_eff(10, 40) == 10 && rec_k_eff(0, 40) == 0 && rec_k_eff(~0ull, 7) == 7);
    CHECK(rec_check_out(5, 4, false) == REC_SMALL_CAP && rec_check_out(5, 5, true) == REC_NULL_OUT && rec_check_out(0, 0, true) == REC_OK && rec_check_out(5, 9, false) == REC_OK);
    CHECK(rec_state_bytes(0xFFFFFFF0ull) == 0xFFFFFFF0ull * 8 && rec_key_bytes(2000) == 16000);
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
