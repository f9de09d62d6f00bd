"""CPU: the recommend strategies average_vector and sum_scores (ott_query_recommend_strategy, VecStore.recommend(..., strategy=...);
DESIGN.md 3.1n) without a GPU — the host model's own properties (tests/recommend_strategy_ref.py), the planner's refusals and
lowering, the ABI's device-free argument checks, and a walk of the plan header's added functions (ott_recommend_plan.h) by a
stand-alone C++ program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import manhattan_ref as M
import recommend_ref as R
import recommend_strategy_ref as RS
from otters_amd import Cmp, Metric, OttersError, Path, RecommendStrategy, VecStore
from otters_amd.vec import ResolvedRecommend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")
f32 = np.float32
AVG, SUM = RecommendStrategy.AverageVector, RecommendStrategy.SumScores


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


# ---- the host model ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(21)
    return rng.uniform(-1, 1, (300, 13)).astype(np.float32)


def plain(oracle, rows, q, metric, take, k, mask):
    if metric == Metric.Manhattan:
        return M.select_canonical(M.scores(rows, q[None, :], "l1", 0), take, k, 0, 0.0, mask)
    return oracle.vec_query(rows, q[None, :], int(metric), take, k, 0, 0.0, row_mask=mask, ties=oracle.TIES_CANONICAL)


@pytest.mark.parametrize("metric,take", [(Metric.DotProduct, 1), (Metric.Euclidean, 0), (Metric.Manhattan, 0), (Metric.DotProduct, 0)])
def test_one_positive_ranks_like_that_row_as_a_query_with_itself_masked(oracle, corpus, metric, take):
    rows, e = corpus, 17
    mask = RS.keep_without(rows.shape[0], [e], [])
    exp = plain(oracle, rows, rows[e], metric, take, 12, mask)
    hits, side = RS.sum_scores(oracle, rows, None, [e], [], metric, take, 12)
    assert hits["index"].tolist() == exp["index"].tolist() and bits(hits["score"]) == bits(exp["score"]) and side.tolist() == [1] * 12
    q = RS.average_vector(rows, [e, e])
    assert bits(q) == bits(rows[e])  # one distinct positive: the row itself, divided by 1
    got = plain(oracle, rows, q, metric, take, 12, mask)
    assert got["index"].tolist() == exp["index"].tolist() and bits(got["score"]) == bits(exp["score"])


def test_on_integer_rows_the_sum_of_dot_products_ranks_like_the_scaled_average_vector(oracle):
    rng = np.random.default_rng(22)
    rows = rng.integers(-2, 3, (200, 13)).astype(np.float32)  # every product, sum and difference below is exact in f32
    n = rows.shape[0]
    # four positives: q = (p0 + p1 + p2 + p3) / 4 exactly, so the query's score is S / 4 and the order is S's
    pos = [3, 50, 7, 199]
    S_hits, _ = RS.sum_scores(oracle, rows, None, pos, [], Metric.DotProduct, 1, n)
    q = RS.average_vector(rows, pos)
    A = plain(oracle, rows, q, Metric.DotProduct, 1, n, RS.keep_without(n, pos, []))
    assert S_hits["index"].tolist() == A["index"].tolist() and np.array_equal(S_hits["score"], A["score"] * f32(4))
    assert (np.diff(S_hits["score"]) == 0).any(), "the quantised corpus must produce tied sums"
    # two positives and one negative: (mp + mp) - mn = p0 + p1 - n0 exactly, the query's score is S itself
    pos, neg = [3, 50], [120]
    S_hits, _ = RS.sum_scores(oracle, rows, None, pos, neg, Metric.DotProduct, 1, n)
    q = RS.average_vector(rows, pos, neg)
    assert bits(q) == bits(rows[3] + rows[50] - rows[120])
    A = plain(oracle, rows, q, Metric.DotProduct, 1, n, RS.keep_without(n, pos, neg))
    assert S_hits["index"].tolist() == A["index"].tolist()
    assert np.array_equal(S_hits["score"], A["score"])  # (as values: an exact cancellation is +0.0 in one chain and may be -0.0 in another)
    assert (S_hits["score"] == 0).any(), "the quantised corpus must produce exact cancellations"


def test_a_negative_zero_single_score_survives_and_the_chain_is_in_slot_order():
    P = np.array([[-0.0, 0.0, 1.0, 5.0]], f32)
    assert bits(RS.sum_chain(P, 1)) == bits(P[0])
    hits, side = RS.sum_scores(None, np.zeros((4, 2), f32), None, [3], [], Metric.DotProduct, 1, 4, P=P)
    assert hits["index"].tolist() == [2, 1, 0] and bits(hits["score"]) == [0x3F800000, 0, 0x80000000] and side.tolist() == [1, 1, 1]
    hits, _ = RS.sum_scores(None, np.zeros((4, 2), f32), None, [3], [], Metric.DotProduct, 0, 4, P=P)
    assert hits["index"].tolist() == [0, 1, 2] and bits(hits["score"]) == [0x80000000, 0, 0x3F800000]
    # f32 steps in slot order, positives added and negatives subtracted: (1e8 + 1) - 1e8 is 0, not 1
    P = np.array([[1e8], [1.0], [1e8]], f32)
    assert RS.sum_chain(P, 2)[0] == 0.0 and RS.sum_chain(P[[0, 2, 1]], 1)[0] == -1.0  # ... and (1e8 - 1e8) - 1 is -1
    # NaN pair scores and inf - inf make S NaN: never a candidate
    P = np.array([[np.inf, np.nan, 1.0, 0.0], [np.inf, 1.0, 2.0, 0.0]], f32)
    assert np.isnan(RS.sum_chain(P, 1)[:2]).all() and np.isinf(RS.sum_chain(P, 2)[0])
    hits, _ = RS.sum_scores(None, np.zeros((4, 2), f32), None, [3], [0], Metric.DotProduct, 1, 4, P=P)
    assert hits["index"].tolist() == [2] and bits(hits["score"]) == bits([-1.0])
    # the filter acts on S
    P = np.array([[1.0, 2.0, 3.0, 9.0, 9.0], [0.5, 0.5, 0.5, 9.0, 9.0]], f32)  # S = 0.5, 1.5, 2.5 and the two examples
    for cmp, exp in ((Cmp.Lt, [0]), (Cmp.Gt, [2]), (Cmp.Lte, [1, 0]), (Cmp.Gte, [2, 1]), (Cmp.Eq, [1])):
        hits, _ = RS.sum_scores(None, np.zeros((5, 2), f32), None, [3], [4], Metric.DotProduct, 1, 5, cmp=int(cmp), thr=1.5, P=P)
        assert hits["index"].tolist() == exp, cmp


def test_average_vector_divides_once_and_mirrors_the_negatives(corpus):
    rows = corpus
    q = RS.average_vector(rows, [1, 2, 3, 2, 1])
    s = ((rows[1] + rows[2]).astype(f32) + rows[3]).astype(f32)
    assert bits(q) == bits(s / f32(3))
    assert (q != (s * f32(1.0 / 3.0)).astype(f32)).any(), "the seed must tell a division from a reciprocal multiply"
    qn = RS.average_vector(rows, [1, 2, 3], [9, 8])
    mn = ((rows[9] + rows[8]).astype(f32) / f32(2)).astype(f32)
    assert bits(qn) == bits(((q + q).astype(f32) - mn).astype(f32))


# ---- the planner ---------------------------------------------------------------------------------------------------------------------

def fake_store(n=100, devices=None):
    store = VecStore.__new__(VecStore)
    store.dim, store._n, store._n_groups, store.devices = 4, n, 0, devices
    return store


def refused(plan, text):
    with pytest.raises(OttersError) as e:
        plan.validate()
    assert text in str(e.value), str(e.value)


@pytest.mark.parametrize("strategy", [AVG, SUM])
def test_planner_refusals_messages_and_their_order(strategy):
    s = fake_store()
    who = "ott_query_recommend_strategy: "
    rec = lambda pos, neg=(), **kw: s.recommend(pos, neg, strategy=strategy, **kw)  # noqa: E731
    refused(rec([], [1]), who + "at least one positive example is needed")
    refused(rec([100]), who + "example id 100 is not below the store's length 100")
    refused(rec([1, 2], [3, 2]), who + "row 2 is listed as both a positive and a negative example")
    refused(rec(list(range(40)), list(range(40, 65))), who + "more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples")
    refused(rec([1, 2], [400, 2]), who + "example id 400 is not below the store's length 100")
    refused(fake_store(devices=[0, 0]).recommend([1], strategy=strategy), who + "a multi-GPU store is not served")
    # the examples come before the path, the path before the store
    refused(rec([100]).with_path(Path.Mfma), "example id 100 is not below")
    if strategy == SUM:
        refused(rec([1]).with_path(Path.Mfma), who + "the MFMA path does not serve sum_scores; use path AUTO or EXACT")
        refused(fake_store(devices=[0, 0]).recommend([1], strategy=strategy).with_path(Path.Mfma), "the MFMA path does not serve sum_scores")
    else:
        rec([1]).with_path(Path.Mfma).validate()  # ott_query's path choice
        refused(rec([1], metric=Metric.Manhattan).with_path(Path.Mfma), who + "the MFMA path does not score the Manhattan metric")
    rec(list(range(40)) * 3, list(range(40, 64)) * 2).validate()


def test_planner_lowering():
    s = fake_store()
    # the default strategy resolves to what it always did
    old = s.recommend([5, 5, 6], [7]).resolve()
    new = s.recommend([5, 5, 6], [7], strategy=RecommendStrategy.BestScore).resolve()
    assert isinstance(new, ResolvedRecommend) and old.strategy == new.strategy == 0 and new.flags == 1 and new.path == int(Path.Auto)
    assert new.positive.tolist() == [5, 5, 6] and new.negative.tolist() == [7] and (new.metric, new.take, new.k) == (int(Metric.Cosine), 1, 100)
    assert s.recommend([5], strategy=RecommendStrategy.BestScore).fill_negative_side(False).resolve().flags == 0
    assert ResolvedRecommend(new.positive, new.negative, 0, 1, 3, 0, 0.0, None, 0, 1).strategy == 0  # the fields it had, in their order
    refused(s.recommend([1], strategy=RecommendStrategy.BestScore).with_path(Path.Mfma), "ott_query_recommend: the MFMA path does not serve recommend queries")
    # the other two lower to flags 0, whatever fill_negative_side says
    for strategy in (AVG, SUM):
        for fill in (True, False):
            rr = s.recommend([5, 6], [7], Metric.Euclidean, strategy).take(3).filter(0.5, Cmp.Lt).fill_negative_side(fill).with_path(Path.Exact).resolve()
            assert (rr.strategy, rr.flags, rr.take, rr.k, rr.filter_cmp, rr.filter_thr, rr.path) == (int(strategy), 0, 0, 3, int(Cmp.Lt), 0.5, int(Path.Exact))
    assert s.recommend([5], strategy=AVG).with_path(Path.Mfma).resolve().path == int(Path.Mfma)
    assert [int(x) for x in RecommendStrategy] == [0, 1, 2] and RecommendStrategy(1) is AVG and RecommendStrategy(2) is SUM
    with pytest.raises(ValueError):
        s.recommend([5], strategy=3)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------

PROTOTYPE = """int ott_query_recommend_strategy(ott_store* s, const ott_query_desc* d, uint32_t strategy, const uint64_t* positive,
                                 uint64_t n_positive, const uint64_t* negative, uint64_t n_negative, uint32_t flags, ott_hit* out,
                                 uint64_t cap, uint64_t* n_out, uint32_t* side_of_hit , ott_stats* stats);"""
ENUM = "typedef enum { OTT_RECOMMEND_BEST_SCORE = 0, OTT_RECOMMEND_AVERAGE_VECTOR = 1, OTT_RECOMMEND_SUM_SCORES = 2 } ott_recommend_strategy;"


def test_header_declares_the_call_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat and ENUM in flat
    assert "#define OTT_ABI_VERSION 4" in src
    rust = open(os.path.join(ROOT, "bindings", "rust", "otters-hip-sys", "src", "lib.rs")).read()
    assert "pub fn ott_query_recommend_strategy(s: *mut ott_store, d: *const ott_query_desc, strategy: u32, positive: *const u64, n_positive: u64," in rust


def test_library_exports_it_and_checks_its_arguments_without_a_device():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    assert hasattr(L, "ott_query_recommend_strategy")
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

    def call(d, strategy, p=pos, n_p=2, n=neg, n_n=1, flags=0):
        return L.ott_query_recommend_strategy(None, C.byref(d) if d is not None else None, strategy, N.ptr(p) if p is not None else None, n_p,
                                              N.ptr(n) if n is not None else None, n_n, flags, N.ptr(out), 4, C.byref(n_out), N.ptr(sides), None)

    err = L.ott_last_error
    who = b"ott_query_recommend_strategy: "
    assert call(desc(), 3) == -1 and who + b"unknown strategy" in err()
    assert call(None, 3) == -1 and who + b"unknown strategy" in err()
    assert call(desc(), 0xFFFFFFFF, flags=1) == -1 and who + b"unknown strategy" in err()
    for st in (1, 2):
        assert call(None, st) == -1 and who + b"desc is NULL" in err()
        assert call(desc(), st, n_p=0) == -1 and who + b"at least one positive example is needed" in err()
        assert call(desc(), st, p=None) == -1 and who + b"an example list is NULL" in err()
        assert call(desc(), st, n=None) == -1 and who + b"an example list is NULL" in err()
        assert call(desc(), st, flags=1) == -1 and who + b"flags must be 0 (OTT_RECOMMEND_FILL belongs to best_score)" in err()
        assert call(desc(nq=1, mode=1, path=2), st, flags=2) == -1 and who + b"flags must be 0" in err()  # the flags come first
        assert call(desc(nq=1, mode=1), st) == -1 and who + b"the examples are the queries; d->queries must be NULL and d->nq 0" in err()
        assert call(desc(queries=q.ctypes.data), st) == -1 and b"d->queries must be NULL and d->nq 0" in err()
        assert call(desc(mode=1, path=2), st) == -4 and who + b"the examples make ONE query; PER_QUERY is not served" in err()
        assert call(desc(metric=9), st) == -1 and who + b"unknown metric" in err()
        assert call(desc(), st) == -1 and who + b"store is NULL" in err()  # valid arguments: the NULL store is what is left to refuse
    assert call(desc(path=2), 2) == -4 and who + b"the MFMA path does not serve sum_scores; use path AUTO or EXACT" in err()
    assert call(desc(path=2), 1) == -1 and who + b"store is NULL" in err()  # average_vector: ott_query's path choice
    assert call(desc(path=2, metric=int(Metric.Manhattan)), 1) == -4 and who + b"the MFMA path does not score the Manhattan metric" in err()
    # strategy 0 is ott_query_recommend: its flags rule, its messages
    assert call(desc(), 0, flags=2) == -1 and b"ott_query_recommend: unknown flag bits" in err()
    assert call(desc(path=2), 0, flags=1) == -4 and b"ott_query_recommend: the MFMA path does not serve recommend queries" in err()
    assert call(desc(), 0, flags=1) == -1 and b"ott_query_recommend: store is NULL" in err()
    assert n_out.value == 9 and not out["index"].any() and (sides == 7).all()  # nothing was touched


# ---- the plan header's added functions: a stand-alone program under ASan + UBSan ----------------------------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ott_recommend_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (n %u)\n", __LINE__, #c, n); return 1; } } while (0)
static bool has(RecRefusal r, const char* part) { return strstr(rec_strategy_text(r), part) != nullptr; }
int main() {
    unsigned n = 0;
    CHECK(REC_BEST_SCORE == 0 && REC_AVERAGE_VECTOR == 1 && REC_SUM_SCORES == 2 && REC_SUM_MARK != 0);
    CHECK(rec_strategy_known(0) && rec_strategy_known(1) && rec_strategy_known(2) && !rec_strategy_known(3) && !rec_strategy_known(0xFFFFFFFFu));
    CHECK(rec_strategy_flags(REC_BEST_SCORE) == REC_FILL && rec_strategy_flags(REC_AVERAGE_VECTOR) == 0 && rec_strategy_flags(REC_SUM_SCORES) == 0);
    for (uint32_t st = 1; st <= 2; st++) {
        n = st;
        // the refusals in the order the call makes them: every later fault is present too
        CHECK(rec_strategy_check_args(3, true, 0, true, 1, 1, true, true, true, true) == REC_BAD_STRATEGY);
        CHECK(rec_strategy_check_args(st, true, 0, true, 1, 1, true, true, true, true) == REC_NO_POSITIVE);
        CHECK(rec_strategy_check_args(st, true, 1, false, 0, 1, true, true, true, true) == REC_NULL_LIST);
        CHECK(rec_strategy_check_args(st, false, 1, true, 1, 1, true, true, true, true) == REC_NULL_LIST);
        CHECK(rec_strategy_check_args(st, false, 1, true, 0, 1, true, true, true, true) == REC_BAD_FLAGS);
        CHECK(rec_strategy_check_args(st, false, 1, true, 0, 0x80000000u, false, false, false, false) == REC_BAD_FLAGS);
        CHECK(rec_strategy_check_args(st, false, 1, true, 0, 0, true, true, true, true) == REC_HAS_QUERIES);
        CHECK(rec_strategy_check_args(st, false, 1, true, 0, 0, false, true, true, true) == REC_PER_QUERY);
        CHECK(rec_strategy_check_args(st, false, 1, true, 0, 0, false, false, true, true) == (st == REC_SUM_SCORES ? REC_MFMA : REC_MFMA_L1));
        CHECK(rec_strategy_check_args(st, false, 1, true, 0, 0, false, false, true, false) == (st == REC_SUM_SCORES ? REC_MFMA : REC_OK));
        CHECK(rec_strategy_check_args(st, false, 1, true, 0, 0, false, false, false, true) == REC_OK);
        CHECK(rec_strategy_check_args(st, false, 9, false, 9, 0, false, false, false, false) == REC_OK);
    }
    n = 0;
    CHECK(rec_strategy_mfma(REC_SUM_SCORES, false, true) == REC_OK && rec_strategy_mfma(REC_AVERAGE_VECTOR, false, true) == REC_OK);
    // which refusals are OTT_ERR_INVALID; the old ones keep their class
    CHECK(rec_refusal_is_invalid(REC_BAD_STRATEGY) && !rec_refusal_is_invalid(REC_MFMA_L1) && !rec_refusal_is_invalid(REC_MFMA) && rec_refusal_is_invalid(REC_BAD_FLAGS));
    // every refusal without an id has a text that names the call; the two with an id are the caller's
    for (int r = REC_NO_POSITIVE; r <= REC_MFMA_L1; r++) {
        n = (unsigned)r;
        const bool with_id = r == REC_BAD_ID || r == REC_BOTH_SIDES;
        CHECK(with_id == (rec_strategy_text((RecRefusal)r)[0] == 0));
        if (!with_id) CHECK(strncmp(rec_strategy_text((RecRefusal)r), "ott_query_recommend_strategy: ", 30) == 0);
    }
    n = 0;
    CHECK(rec_strategy_text(REC_OK)[0] == 0);
    CHECK(has(REC_BAD_STRATEGY, "unknown strategy") && has(REC_BAD_FLAGS, "flags must be 0") && has(REC_MFMA, "sum_scores") && has(REC_MFMA_L1, "Manhattan"));
    CHECK(has(REC_MULTI_GPU, "multi-GPU") && has(REC_SMALL_CAP, "output capacity is smaller than min(k, rows)") && has(REC_TOO_MANY_ROWS, "2^32 - 16"));
    // the sign of a slot
    CHECK(rec_slot_positive(0, 1) && !rec_slot_positive(1, 1) && rec_slot_positive(62, 63) && !rec_slot_positive(63, 63) && !rec_slot_positive(0, 0));
    // average_vector's mask: ones everywhere (past the store's end too), the examples' bits cleared; two mask blocks and the vector
    CHECK(rec_mask_words(0) == 0 && rec_mask_words(1) == 1 && rec_mask_words(64) == 1 && rec_mask_words(65) == 2 && rec_mask_words(0xFFFFFFF0ull) == 0x3FFFFFFull + 1);
    CHECK(rec_mask_bytes(65, 100) == 2 * 16 + 400 && rec_mask_bytes(1, 5) == 16 + 20);
    for (n = 1; n <= 64; n++) {
        const uint64_t len = 1000 + 3 * n;
        std::vector<uint64_t> pos, neg;
        for (unsigned i = 0; i < n; i++) (i % 3 == 2 ? neg : pos).push_back(i == n - 1 ? len - 1 : i * 15u);  // distinct; the store's last row among them
        RecExamples ex;
        uint64_t bad = 0;
        CHECK(rec_examples(pos.data(), pos.size(), neg.empty() ? nullptr : neg.data(), neg.size(), len, &ex, &bad) == REC_OK && ex.n == n);
        std::vector<uint64_t> words(rec_mask_words(len), 0x1234);
        rec_mask_fill(ex, len, words.data());
        uint64_t cleared = 0;
        for (uint64_t r = 0; r < rec_mask_words(len) * 64; r++) {
            bool is_ex = false;
            for (unsigned e = 0; e < ex.n; e++) is_ex |= ex.rows[e] == r;
            CHECK((((words[r >> 6] >> (r & 63)) & 1) == 0) == is_ex);
            cleared += is_ex;
        }
        CHECK(cleared == n);
        for (unsigned e = 0; e < ex.n; e++) CHECK(rec_slot_positive(e, ex.first_neg) == (e < pos.size()));
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
