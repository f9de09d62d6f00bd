"""CPU: batch search with a row mask per query (ott_query_masks, the device mask slots, VecQueryPlan.with_row_masks,
MetaQueryPlan.meta_filters) without a GPU — the header's declarations, the ABI's device-free argument checks, the
planners' refusals and lowering, and a walk of the plan header (ott_masks_plan.h) by a stand-alone C++ program under
AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N
from otters_amd.meta import _resolve_filters
from otters_amd.vec import lower_row_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")


# ---- the header --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_calls_and_defines_and_keeps_abi_4():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for fn in ("ott_query_masks", "ott_store_eval_row_mask_slot", "ott_store_write_row_mask_slot", "ott_store_clear_row_mask_slots"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, code), fn
    defs = dict(re.findall(r"#define\s+(OTT_[A-Z0-9_]+)\s+(\d+)", code))
    assert int(defs["OTT_NO_MASK"]) == 0xFFFFFFFF == N.NO_MASK
    assert int(defs["OTT_MASK_SLOT_BASE"]) == 0x80000000 == N.MASK_SLOT_BASE
    assert int(defs["OTT_MASK_SLOTS"]) == 64 == N.MASK_SLOTS
    assert int(defs["OTT_MASKS_MAX_QUERIES"]) == 1024 == N.MASKS_MAX_QUERIES
    assert int(defs["OTT_ABI_VERSION"]) == 4 == N.ABI_VERSION == N.lib().ott_abi_version()
    assert '"masks_sweep"' in src and "OTT_MASKS_SWEEP" in src
    plan = open(os.path.join(CSRC, "ott_masks_plan.h")).read()
    assert plan.count("profiles/masks_batch/README.md") >= 3  # every auto constant cites the measurement
    assert "ott_masks.hip" in open(os.path.join(CSRC, "Makefile")).read()


# ---- the ABI's argument checks: all before any device work ------------------------------------------------------------------------------

def desc(nq=1, mode=1, dim=4, path=0):
    q = np.zeros((max(nq, 1), dim), np.float32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, nq, int(Metric.DotProduct), 1, mode, 3, path
    return d, q


def test_argument_checks_need_no_device():
    L = N.lib()
    out = np.zeros(8, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)

    def call(d, moq, masks=None, n_masks=0, bits=0):
        moq = None if moq is None else np.asarray(moq, np.uint32)
        return L.ott_query_masks(None, C.byref(d[0]), N.ptr(masks), n_masks, bits, N.ptr(moq), N.ptr(out), out.size, C.byref(n_out), None, None)

    def err():
        return L.ott_last_error()

    words = np.zeros(2, dtype=np.uint64)
    assert call(desc(), [N.NO_MASK]) == -1 and b"ott_query_masks: store is NULL" in err()
    assert call(desc(mode=0), [N.NO_MASK]) == -1 and b"needs OTT_MODE_PER_QUERY" in err()
    assert call(desc(), [2], words, 2, 64) == -1 and b"mask 2 is out of range (the call brings 2 masks)" in err()
    assert call(desc(nq=3), [0, 1, 0x7FFFFFFF], words, 2, 64) == -1 and b"query 2: mask 2147483647" in err()
    assert call(desc(), [0], None, 1, 64) == -1 and b"masks is NULL" in err()
    assert call(desc(), None) == -1 and b"mask_of_query is NULL" in err()
    assert call(desc(), [N.MASK_SLOT_BASE + 64]) == -1 and b"slot 64 is not below OTT_MASK_SLOTS" in err()
    assert call(desc(), [N.MASK_SLOT_BASE + 63]) == -1 and b"store is NULL" in err()  # whether a slot is filled is the store's to say
    assert call(desc(nq=0), [N.NO_MASK]) == -1 and b"No queries provided" in err()
    assert call(desc(nq=1025), [N.NO_MASK] * 1025) == -1 and b"1025 queries are above OTT_MASKS_MAX_QUERIES (1024)" in err()
    assert L.ott_query_masks(None, None, None, 0, 0, None, None, 0, None, None, None) == -1 and b"desc is NULL" in err()
    assert n_out.value == 9 and not out["index"].any()  # nothing was touched
    # the slot calls
    assert L.ott_store_eval_row_mask_slot(None, 0, None, 0, 0, None) == -1 and b"ott_store_eval_row_mask_slot: store is NULL" in err()
    assert L.ott_store_write_row_mask_slot(None, 0, N.ptr(words), 64) == -1 and b"ott_store_write_row_mask_slot: store is NULL" in err()
    assert L.ott_store_clear_row_mask_slots(None) == -1 and b"ott_store_clear_row_mask_slots: store is NULL" in err()
    assert L.ott_store_set_option(None, b"masks_sweep", 1) != 0 and b"NULL" in err()


# ---- VecQueryPlan.with_row_masks ------------------------------------------------------------------------------------------------------

def plan_of(nq=3, dim=4):
    store = VecStore(dim)
    return store.query(np.ones((nq, dim), np.float32), Metric.DotProduct).take(5)


def test_with_row_masks_refusals():
    m = [np.ones(7, bool)] * 3

    def refused(p, text):
        with pytest.raises(OttersError) as ei:
            p.validate()
        assert text in str(ei.value), str(ei.value)

    refused(plan_of().with_row_masks(m), "with_row_masks needs per_query()")
    refused(plan_of().per_query().with_row_masks(m[:2]), "with_row_masks: 2 masks for 3 queries")
    refused(plan_of().per_query().with_row_masks(5), "one boolean array or None per query")
    refused(plan_of().per_query().with_row_masks(m).with_row_ids([1]), "with_row_masks cannot be combined with with_row_ids")
    refused(plan_of().per_query().with_row_masks(m).one_per_group(), "with_row_masks cannot be combined with one_per_group")
    refused(plan_of().per_query().with_row_masks(m).per_group(2), "with_row_masks cannot be combined with per_group")
    refused(plan_of().with_row_masks(m).max_sim(), "with_row_masks cannot be combined with max_sim")
    refused(plan_of().per_query().with_row_masks(m).mmr(0.5), "with_row_masks cannot be combined with mmr")
    plan_of().per_query().with_row_masks(m).with_row_mask(np.ones(3, bool)).filter(0.5, Cmp.Gt).with_path(Path.Exact).validate()  # all of these combine


def test_with_row_masks_lowering_dedupes_by_identity_and_by_value():
    a = np.array([1, 0, 1, 1, 0], bool)
    b = np.array([1, 0, 1], bool)
    rq = plan_of(nq=6).per_query().with_row_masks([a, None, b, a, a.copy(), [True, False, True]]).with_row_mask(np.ones(2, bool)).resolve()
    assert rq.mask_of_query.dtype == np.uint32 and rq.mask_of_query.tolist() == [0, N.NO_MASK, 1, 0, 0, 1]
    assert rq.query_masks.shape == (2, 5)
    assert rq.query_masks[0].tolist() == a.tolist() and rq.query_masks[1].tolist() == [True, False, True, True, True]  # padded with keep
    assert rq.row_mask.tolist() == [True, True] and rq.mode == 1  # with_row_mask stays the common mask
    # nothing but None, and nothing but empty masks: no mask at all
    moq, qm = lower_row_masks([None, None])
    assert moq.tolist() == [N.NO_MASK] * 2 and qm.shape == (0, 0)
    moq, qm = lower_row_masks([np.zeros(0, bool), None])
    assert moq.tolist() == [N.NO_MASK] * 2 and qm.shape == (0, 0)
    assert plan_of().resolve().mask_of_query is None  # a plan without with_row_masks is what it was


# ---- MetaQueryPlan.meta_filters -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def meta():
    n = 40
    cols = [Column("age", DataType.Int32).from_(list(range(n))), Column("lang", DataType.String).from_(["en", "de"] * (n // 2))]
    return MetaStore.from_columns(cols).with_vectors(np.ones((n, 3), np.float32).tolist()).with_chunk_size(10).build(_host_only=True)


def test_meta_filters_refusals(meta):
    q = np.ones((2, 3), np.float32)

    def refused(p, text, how="collect_per_query"):
        with pytest.raises(OttersError) as ei:
            getattr(p, how)()
        assert text in str(ei.value), str(ei.value)

    f = [col("age").lt(5), None]
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters(f).meta_filter(col("age").gt(1)), "meta_filters cannot be combined with meta_filter")
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters(f[:1]), "meta_filters: 1 filters for 2 queries")
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters(f).with_row_ids([1]), "meta_filters cannot be combined with with_row_ids")
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters(f).distinct_by("age"), "meta_filters cannot be combined with distinct_by")
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters(f).take(3).mmr(), "meta_filters cannot be combined with mmr")
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters([col("nope").lt(5), None]), "meta_filter compile error: Unknown column 'nope'")
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters(7), "one Expr or None per query")
    refused(meta.query_batch(q, Metric.DotProduct).meta_filters(f), "use collect_per_query()", how="collect")
    refused(meta.query_batch(q, Metric.DotProduct).take(3), "collect_per_query needs meta_filters()")


def test_meta_filters_lowering_dedupes_and_shares_the_or_of_the_chunk_masks(meta):
    q = np.ones((5, 3), np.float32)
    young, old = col("age").lt(5), col("age").gte(35)
    plan = meta.query_batch(q, Metric.DotProduct).meta_filters([young, old, col("age").lt(5), young, old & col("lang").eq("en")]).take(4)
    rq, shared, distinct, chunk_masks, of_query = _resolve_filters(plan)
    assert of_query == [0, 1, 0, 0, 2] and len(distinct) == 3  # the same object and an equal expression share one filter
    assert [cm.tolist() for cm in chunk_masks[:2]] == [[True, False, False, False], [False, False, False, True]]
    assert shared.tolist() == [True, False, False, True]  # the OR
    assert rq.mode == 1 and rq.k == 4 and rq.queries.shape == (5, 3) and rq.row_mask is None
    # a query without a filter needs every chunk
    plan = meta.query_batch(q[:2], Metric.DotProduct).meta_filters([young, None])
    rq, shared, distinct, chunk_masks, of_query = _resolve_filters(plan)
    assert shared is None and of_query == [0, -1] and rq.k == 40
    # a filter the zone statistics decide wholesale still needs its chunk mask as a row mask: the shared chunk mask is wider
    wide = col("age").lt(10)
    cm = meta.build_chunk_mask_for_plan(wide.compile(meta.schema()))
    assert meta.row_mask_is_all_true(wide.compile(meta.schema()), cm) and cm.tolist() == [True, False, False, False]


# ---- the plan header: a stand-alone program under ASan + UBSan ----------------------------------------------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ott_masks_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (n %u)\n", __LINE__, #c, n); return 1; } } while (0)
int main() {
    unsigned n = 0;
    CHECK(MASKS_NO_MASK == 0xFFFFFFFFu && MASKS_SLOT_BASE == 0x80000000u && MASKS_SLOTS == 64 && MASKS_MAX_QUERIES == 1024 && MASKS_NQ == 4);
    // ---- the refusals, in the order the call makes them: every later fault is present too
    uint32_t bad = 99;
    const uint32_t junk[3] = {7, MASKS_SLOT_BASE + 64, 5};
    CHECK(masks_check_args(0, false, nullptr, true, 1, &bad) == MASKS_NO_QUERIES);
    CHECK(masks_check_args(1025, false, nullptr, true, 1, &bad) == MASKS_TOO_MANY);
    CHECK(masks_check_args(3, false, nullptr, true, 1, &bad) == MASKS_MERGED);
    CHECK(masks_check_args(3, true, nullptr, true, 1, &bad) == MASKS_NULL_MAP);
    CHECK(masks_check_args(3, true, junk, true, 1, &bad) == MASKS_NULL_MASKS);
    CHECK(masks_check_args(3, true, junk, false, 1, &bad) == MASKS_BAD_INDEX && bad == 0);
    CHECK(masks_check_args(3, true, junk, false, 8, &bad) == MASKS_BAD_SLOT && bad == 1);
    CHECK(masks_check_args(1, true, junk, false, 8, &bad) == MASKS_OK);
    CHECK(masks_check_args(1, true, junk, true, 0, &bad) == MASKS_BAD_INDEX);  // no masks at all: index 7 names none
    {
        const uint32_t ok[5] = {0, MASKS_NO_MASK, MASKS_SLOT_BASE, MASKS_SLOT_BASE + 63, 2};
        CHECK(masks_check_args(5, true, ok, false, 3, &bad) == MASKS_OK);
        CHECK(masks_check_args(5, true, ok, false, 2, &bad) == MASKS_BAD_INDEX && bad == 4);
        CHECK(masks_check_args(1024, true, std::vector<uint32_t>(1024, MASKS_NO_MASK).data(), true, 0, nullptr) == MASKS_OK);
        uint64_t slot_bits[MASKS_SLOTS] = {};
        CHECK(masks_check_slots(5, ok, slot_bits, &bad) == MASKS_EMPTY_SLOT && bad == 2);
        slot_bits[0] = 100;
        CHECK(masks_check_slots(5, ok, slot_bits, &bad) == MASKS_EMPTY_SLOT && bad == 3);
        slot_bits[63] = 1;
        CHECK(masks_check_slots(5, ok, slot_bits, &bad) == MASKS_OK);
        CHECK(masks_is_slot(MASKS_SLOT_BASE) && masks_is_slot(0xFFFFFFFEu) && !masks_is_slot(MASKS_NO_MASK) && !masks_is_slot(0x7FFFFFFFu));
    }
    // ---- pass order and the permutation's round trip: repeated and absent masks, nq of 1, 3, 4, 5, 9
    const uint32_t S = MASKS_SLOT_BASE, X = MASKS_NO_MASK;
    const uint32_t pool[9] = {2, X, 0, S + 1, 2, 0, X, 2, S + 1};
    for (uint32_t nq : {1u, 3u, 4u, 5u, 9u}) {
        n = nq;
        MasksPlan pl;
        masks_plan_build(pool, nq, pl);
        CHECK(pl.order.size() == nq && pl.place.size() == nq && pl.passes == (nq + 3) / 4 && pl.group_start.size() == pl.n_distinct + 1);
        CHECK(pl.group_start.front() == 0 && pl.group_start.back() == nq);
        std::vector<bool> seen(nq, false);
        for (uint32_t i = 0; i < nq; i++) {
            CHECK(pl.order[i] < nq && !seen[pl.order[i]]);
            seen[pl.order[i]] = true;
            CHECK(pl.place[pl.order[i]] == i);  // the round trip
            if (i) {
                const uint32_t a = pool[pl.order[i - 1]], b = pool[pl.order[i]];
                CHECK(a <= b);                              // host masks by index, then the slots, then the queries without a mask
                if (a == b) CHECK(pl.order[i - 1] < pl.order[i]);  // stable: equal masks keep the caller's order
            }
        }
        uint32_t largest = 0;
        for (uint32_t g = 0; g < pl.n_distinct; g++) {
            const uint32_t lo = pl.group_start[g], hi = pl.group_start[g + 1];
            CHECK(lo < hi);
            for (uint32_t i = lo; i < hi; i++) CHECK(pool[pl.order[i]] == pool[pl.order[lo]]);
            if (g) CHECK(pool[pl.order[lo]] != pool[pl.order[lo - 1]]);
            if (hi - lo > largest) largest = hi - lo;
        }
        CHECK(largest == pl.largest_group);
    }
    n = 0;
    {
        MasksPlan pl;
        masks_plan_build(pool, 9, pl);
        const uint32_t want[9] = {2, 5, 0, 4, 7, 3, 8, 1, 6};
        for (uint32_t i = 0; i < 9; i++) CHECK(pl.order[i] == want[i]);
        CHECK(pl.n_distinct == 4 && pl.largest_group == 3 && pl.passes == 3);
        const uint32_t same[5] = {X, X, X, X, X};
        masks_plan_build(same, 5, pl);
        CHECK(pl.n_distinct == 1 && pl.largest_group == 5 && pl.passes == 2 && pl.order[4] == 4);
    }
    // ---- who may take the sweep
    CHECK(masks_sweep_eligible(0, 0, false, 1000, 10, 4) && masks_sweep_eligible(0, 1, false, 1000, 10, 4));
    CHECK(!masks_sweep_eligible(1, 0, false, 1000, 10, 4) && !masks_sweep_eligible(2, 0, false, 1000, 10, 4));  // tie orders 1 and 2
    CHECK(!masks_sweep_eligible(0, 2, false, 1000, 10, 4));                                                      // Path.Mfma
    CHECK(!masks_sweep_eligible(0, 0, true, 1000, 10, 4));                                                       // a multi-GPU store
    CHECK(!masks_sweep_eligible(0, 0, false, 0, 10, 4));
    CHECK(masks_sweep_eligible(0, 0, false, MASKS_MAX_ROWS - 1, 512, 1024) && !masks_sweep_eligible(0, 0, false, MASKS_MAX_ROWS, 512, 1024));
    CHECK(masks_sweep_eligible(0, 0, false, 1u << 16, 513, 1024) && !masks_sweep_eligible(0, 0, false, (1u << 16) + 1, 513, 1024));  // the pair form's bound
    // ---- the option and the auto rule at its borders
    CHECK(!masks_takes_sweep(0, true, 1000, 8, 16, 16, 1) && masks_takes_sweep(1, true, 1000, 8, 16, 16, 1) && !masks_takes_sweep(1, false, 1000, 8, 16, 16, 1));
    CHECK(!masks_takes_sweep(2, false, 1, 8, 16, 16, 1));
    for (uint32_t nq : {MASKS_AUTO_MIN_NQ, MASKS_AUTO_MAX_NQ}) {
        n = nq;
        for (uint64_t rows : {MASKS_AUTO_MIN_ROWS, MASKS_AUTO_MAX_ROWS})
            for (uint32_t dim : {MASKS_AUTO_MIN_DIM, MASKS_AUTO_MAX_DIM}) {
                CHECK(masks_auto_takes_sweep(rows, dim, nq, nq, 1) && masks_takes_sweep(2, true, rows, dim, nq, nq, 1));  // the measured corners
                CHECK(!masks_takes_sweep(2, false, rows, dim, nq, nq, 1));                                                  // ... only where eligible
                CHECK(!masks_auto_takes_sweep(rows, dim, nq, nq / 2, 2) && !masks_auto_takes_sweep(rows, dim, nq, 1, nq));  // shared masks: the loop
            }
        CHECK(!masks_auto_takes_sweep(MASKS_AUTO_MIN_ROWS - 1, 768, nq, nq, 1) && !masks_auto_takes_sweep(MASKS_AUTO_MAX_ROWS + 1, 768, nq, nq, 1));
        CHECK(!masks_auto_takes_sweep(10000, 768, nq, nq, 1) && !masks_auto_takes_sweep(2000000, 768, nq, nq, 1) && !masks_auto_takes_sweep(10000000, 768, nq, nq, 1));
        CHECK(!masks_auto_takes_sweep(500000, MASKS_AUTO_MIN_DIM - 1, nq, nq, 1) && !masks_auto_takes_sweep(500000, MASKS_AUTO_MAX_DIM + 1, nq, nq, 1));
        CHECK(masks_auto_takes_sweep(500000, 384, nq, nq, 1));  // inside the box
    }
    CHECK(!masks_auto_takes_sweep(500000, 384, MASKS_AUTO_MIN_NQ - 1, MASKS_AUTO_MIN_NQ - 1, 1) && !masks_auto_takes_sweep(500000, 384, MASKS_AUTO_MAX_NQ + 1, MASKS_AUTO_MAX_NQ + 1, 1));
    CHECK(masks_auto_takes_sweep(500000, 384, 32, 32, 1) && !masks_auto_takes_sweep(500000, 384, 1, 1, 1));
    n = 0;
    // ---- the scratch and the word rule
    CHECK(masks_words(0) == 0 && masks_words(1) == 1 && masks_words(64) == 1 && masks_words(65) == 2);
    CHECK(masks_scratch_bytes(65, 3, 130) == (2 * 2 + 3 * 3) * 8 && masks_scratch_bytes(1, 0, 0) == 16);
    {
        const uint64_t w[2] = {0x5ull, 0x3ull};
        CHECK(masks_word_ext(nullptr, 70, 0) == ~0ull && masks_word_ext(w, 0, 0) == ~0ull);
        CHECK(masks_word_ext(w, 70, 0) == 0x5ull && masks_word_ext(w, 70, 1) == (0x3ull | (~0ull << 6)) && masks_word_ext(w, 70, 2) == ~0ull);
        CHECK(masks_word_ext(w, 64, 0) == 0x5ull && masks_word_ext(w, 64, 1) == ~0ull && masks_word_ext(w, 3, 0) == (0x5ull | (~0ull << 3)));
        CHECK(masks_word_ext(w, 128, 1) == 0x3ull);
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
