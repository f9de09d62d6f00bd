"""GPU: sparse rows and the exact sparse dot search (ott_store_set_sparse, ott_query_sparse, VecStore.sparse_query,
MetaStore.sparse_query).  Bar: query b's hits — index, S's f32 bits, order, count, and `query` = b — are exactly the
numpy model's (tests/sparse_ref.py: a serial f32 sum in the row's index order, the overlap rule, masks, NaN drop, filter, canonical
order).  Bit for bit, no tolerances.  Every case that is eligible for both forms of the weight lookup (vocab <= 32768) runs under
store option sparse_table 0 (a table in LDS) and 1 (a device table), which must agree with the model and so with each other.
Values and weights are multiples of 1/4, so exact ties and sums that cancel to +0.0 are frequent — and every sum is exact, whatever
its order: the order and the rounding of the sum are held to the model in tests/test_gpu_sparse_rounding.py."""
import ctypes as C
import threading

import numpy as np
import pytest

import sparse_cases as SC
import sparse_ref as SR
from otters_amd import Cmp, Column, DataType, MetaStore, OttersError, Path, VecStore, col
from otters_amd import _native as N
from otters_amd.expr import CmpOp

pytestmark = pytest.mark.gpu


class Sparse:
    """a store of dim 1 with sparse rows, and the same rows as the model takes them"""

    def __init__(self, rows, vocab, chunk=None, devices=None):
        self.rows, self.vocab, self.n = rows, vocab, len(rows)
        self.ptr, self.idx, self.val = SR.csr(rows)
        self.store = VecStore(1) if devices is None else VecStore(1, devices=devices)
        if chunk:
            self.store.set_chunk_size(chunk)
        if self.n:
            self.store.add_vectors(np.zeros((self.n, 1), np.float32))
        self.set()
        self._scores = {}

    def set(self):
        self.store.set_sparse(self.ptr, self.idx, self.val, self.vocab)

    def forms(self):
        return (0, 1) if self.vocab <= 32768 else (1,)

    def scores(self, queries):
        key = id(queries)
        if key not in self._scores:
            self._scores[key] = (queries, SR.scores(self.ptr, self.idx, self.val, queries, self.vocab))
        return self._scores[key][1]


def run(store, queries, take, k, flt=None, mask=None, chunk_mask=None, use_dev=False, path=None):
    """one ott_query_sparse call: ([hits of query b], stats)"""
    p = store.sparse_query(queries)
    p = p.take_max(k) if take else p.take_min(k)
    if flt is not None:
        p = p.filter(flt[1], flt[0])
    if mask is not None:
        p = p.with_row_mask(mask)
    if path is not None:
        p = p.with_path(path)
    hits, counts, stats = store._run_sparse(p.resolve(), chunk_mask=chunk_mask, use_device_row_mask=use_dev)
    assert sum(counts) == hits.size and len(counts) == len(p.queries)
    out, at = [], 0
    for c in counts:
        out.append(hits[at:at + c])
        at += c
    return out, stats


def same(got, exp, where):
    assert len(got) == len(exp), where
    for b, (g, e) in enumerate(zip(got, exp)):
        w = (where, "query", b)
        assert g.size == e.size, (w, g.size, e.size)
        assert np.array_equal(g["index"].astype(np.int64), e["index"].astype(np.int64)), (w, g["index"][:12], e["index"][:12])
        assert np.array_equal(g["score"].view(np.uint32), e["score"].view(np.uint32)), (w, g["score"][:12], e["score"][:12])
        assert np.array_equal(g["query"].astype(np.int64), e["query"].astype(np.int64)), (w, g["query"][:12], e["query"][:12])


def check(sp, queries, take, k, where, flt=None, keep=None, **kw):
    S, cand = sp.scores(queries)
    exp = SR.expected(S, cand, take, k, int(flt[0]) if flt else 0, flt[1] if flt else 0.0, keep)
    got = None
    for form in sp.forms():
        sp.store.set_option("sparse_table", form)
        got, st = run(sp.store, queries, take, k, flt, **kw)
        same(got, exp, (where, "sparse_table", form))
        assert st["path_used"] == int(Path.Exact) or st["vectors_compared"] == 0  # (no row left: the call returns before any plan)
    sp.store.set_option("sparse_table", -1)
    got_auto, st = run(sp.store, queries, take, k, flt, **kw)
    same(got_auto, exp, (where, "sparse_table", -1))
    return got, st


def queries_for(rng, rows, vocab, lens=(1, 7, 40, 0, 3)):
    """queries of different supports over the indices the rows use; the one before last is empty, the last shares no index with any
    row where the vocab has an unused index"""
    pool = SC.used_indices(rows)
    qs = [SC.random_query(rng, vocab, L, pool=pool if pool.size else None) if L else (SC.u32(), SC.f32()) for L in lens[:-1]]
    unused = np.setdiff1d(np.arange(min(vocab, 4096), dtype=np.uint32), pool)
    if unused.size:
        qs.append((unused[: lens[-1]].astype(np.uint32), np.ones(min(lens[-1], unused.size), np.float32)))
    return qs


# ---- 1. shapes: rows x vocab, five queries (a pass boundary of the table form), both takes -----------------------------------------------

@pytest.mark.parametrize("vocab", [1, 31, 32768, 32769, 1 << 20])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 2000])
def test_shapes_against_the_model(n, vocab):
    rng = np.random.default_rng(n * 7 + vocab % 1000)
    pool = None if vocab <= 31 else rng.integers(0, vocab, 300).astype(np.uint32)  # a hot set: queries and rows overlap
    if pool is not None:
        pool[:2] = [0, vocab - 1]  # the first and the last index of the vocab are in use
    rows = SC.random_rows(rng, n, vocab, 8, pool=pool)
    sp = Sparse(rows, vocab)
    qs = queries_for(rng, rows, vocab)
    got, st = check(sp, qs, 1, 10, ("shapes", n, vocab))
    check(sp, qs, 0, 10, ("shapes take_min", n, vocab))
    assert got[3].size == 0  # the empty query
    if len(qs) == 5:
        assert got[4].size == 0  # shares no index with any row
    info = sp.store.sparse_info()
    lens = np.diff(sp.ptr.astype(np.int64))
    padded = sum(64 * int(lens[t:t + 64].max()) for t in range(0, n, 64))
    slices = (n + 63) // 64
    assert info == {"vocab": vocab, "nnz": int(lens.sum()), "padded_entries": padded, "bytes": padded * 8 + (slices + 1) * 8 + slices * 256}
    assert st["vectors_compared"] == n * len(qs) and st["bytes_scanned"] == st["passes"] * (padded * 8 + slices * 264)


def test_passes_follow_the_form():
    rng = np.random.default_rng(3)
    rows = SC.random_rows(rng, 200, 500, 8)
    sp = Sparse(rows, 500)
    for nq, lds, tab in ((1, 1, 1), (4, 4, 1), (5, 5, 2), (9, 9, 3)):
        qs = [SC.random_query(rng, 500, 12) for _ in range(nq)]
        for form, passes in ((0, lds), (1, tab)):
            sp.store.set_option("sparse_table", form)
            _, st = run(sp.store, qs, 1, 5)
            assert st["passes"] == passes, (nq, form, st["passes"])


# ---- 2. IEEE corners, lane divergence, empty slices, duplicates -----------------------------------------------------------------------------

def test_ieee_corners_overlap_rule_and_every_comparator():
    rows, vocab, qs = SC.ieee_case()
    sp = Sparse(rows, vocab)
    got, _ = check(sp, qs, 1, 100, "ieee take_max")
    idx = got[0]["index"].tolist()
    assert 1 not in idx and 9 not in idx and 10 not in idx  # inf - inf dropped; no shared index; no entries
    assert {4, 5, 6, 7, 8, 13} <= set(idx)  # cancelled sums, a stored 0.0 and a 0.0 weight at a shared index: hits with S = +0.0
    zero = got[0][np.isin(got[0]["index"], [4, 5, 6, 7, 8, 13])]
    assert not zero["score"].view(np.uint32).any()  # +0.0, never -0.0
    assert np.isinf(got[0]["score"]).sum() == 2 and (np.abs(got[0]["score"]) == np.float32(1e-45)).sum() == 1
    check(sp, qs, 0, 100, "ieee take_min")
    for cmp in (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq):
        for thr in (0.0, -0.0, 1e-45, float("inf")):
            check(sp, qs, 1, 100, ("ieee filter", cmp.name, thr), flt=(cmp, thr))


@pytest.fixture(scope="module")
def divergent():
    rng = np.random.default_rng(41)
    rows, vocab = SC.divergent_case(rng)
    pool = np.arange(0, 600, dtype=np.uint32)
    return Sparse(rows, vocab), [SC.random_query(rng, vocab, 60, pool=pool) for _ in range(4)]


def test_a_long_row_among_short_ones_an_empty_slice_and_duplicated_rows(divergent):
    sp, qs = divergent
    got, _ = check(sp, qs, 1, sp.n, "divergent, k above the candidates")
    S, cand = sp.scores(qs)
    for b in range(len(qs)):
        assert got[b].size == int(cand[b].sum()) < sp.n and not np.isin(got[b]["index"], np.arange(128, 192)).any()
        assert 70 in got[b]["index"]  # the row of 300 entries
        dup = [r for r in (3, 5, 66, 199) if cand[b, r]]
        pos = [int(np.flatnonzero(got[b]["index"] == r)[0]) for r in dup]
        assert pos == sorted(pos)  # equal S: the lower row first
    check(sp, qs, 0, 7, "divergent take_min")


# ---- 3. batches, takes, filters, k ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mid():
    """about 2000 rows (31.3 slices), vocab 3000, rows of about 10 entries"""
    rng = np.random.default_rng(77)
    rows = SC.random_rows(rng, 2003, 3000, 10, pool=np.arange(0, 3000, 7, dtype=np.uint32))
    return Sparse(rows, 3000), rng


@pytest.mark.parametrize("nq", [1, 4, 5])
def test_batches_of_one_four_and_five(mid, nq):
    sp, rng = mid
    pool = np.arange(0, 3000, 7, dtype=np.uint32)
    qs = [SC.random_query(rng, 3000, L, pool=pool) for L in (30, 2, 90, 11, 45)[:nq]]
    check(sp, qs, 1, 25, ("batch", nq))  # (nq = 1 goes out as OTT_MODE_MERGED)
    check(sp, qs, 0, 3, ("batch take_min", nq))


def test_filters_k_above_the_candidates_and_the_sort_path(mid):
    sp, rng = mid
    pool = np.arange(0, 3000, 7, dtype=np.uint32)
    qs = [SC.random_query(rng, 3000, L, pool=pool) for L in (120, 60, 200)]
    S, cand = sp.scores(qs)
    thr = float(np.median(S[0][cand[0]]))
    for cmp in (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq):
        for take in (0, 1):
            check(sp, qs, take, 40, ("filter", cmp.name, take), flt=(cmp, thr))
    got, _ = check(sp, qs, 1, sp.n, "k above the candidate count")
    assert [g.size for g in got] == [int(c.sum()) for c in cand] and all(g.size < sp.n for g in got)
    got, _ = check(sp, qs, 1, 600, "k = 600: the top-k's sort path")
    assert got[2].size == 600
    check(sp, qs[:1], 0, 600, "k = 600, one query, take_min")


# ---- 4. masks, deleted rows, chunk masks -----------------------------------------------------------------------------------------------------------

def test_row_mask_device_mask_deleted_and_restored_rows(mid):
    sp, rng = mid
    n = sp.n
    qs = [SC.random_query(rng, 3000, L, pool=np.arange(0, 3000, 7, dtype=np.uint32)) for L in (80, 150)]
    short = rng.random(n - 100) < 0.5  # rows at and beyond the mask's length are kept
    keep = np.ones(n, bool)
    keep[: short.size] = short
    check(sp, qs, 1, 50, "caller's row mask", keep=keep, mask=short)
    none = np.zeros(n, bool)
    got, _ = check(sp, qs, 1, 50, "a mask that keeps nothing", keep=none, mask=none)
    assert all(g.size == 0 for g in got)
    dead = rng.choice(n, 700, replace=False)
    sp.store.delete_rows(dead)
    alive = np.ones(n, bool)
    alive[dead] = False
    check(sp, qs, 1, 50, "deleted rows", keep=alive)
    check(sp, qs, 0, 50, "deleted rows and a mask", keep=alive & keep, mask=short)
    vals = rng.integers(0, 100, n).astype(np.int32)
    leaf = N.Leaf()
    leaf.column, leaf.op, leaf.clause, leaf.lit_i64 = sp.store.add_column(vals, DataType.Int32), int(CmpOp.Lt), 0, 55
    N.check(N.lib().ott_store_eval_row_mask(sp.store._handle(), C.byref(leaf), 1, 1, None))
    check(sp, qs, 1, 50, "evaluated device mask", keep=alive & (vals < 55), use_dev=True)
    sp.store.restore_rows(dead[:400])
    alive[dead[:400]] = True
    check(sp, qs, 1, 50, "restored rows", keep=alive)
    sp.store.restore_rows(dead[400:])


@pytest.mark.parametrize("chunk", [128, 100])
def test_chunk_masks_that_drop_whole_slices_and_cut_through_one(chunk):
    rng = np.random.default_rng(chunk)
    n = 1000
    rows = SC.random_rows(rng, n, 900, 9)
    sp = Sparse(rows, 900, chunk=chunk)
    qs = [SC.random_query(rng, 900, L) for L in (60, 25)]
    n_chunks = (n + chunk - 1) // chunk
    for cm in (rng.random(n_chunks) < 0.5, np.arange(n_chunks) == n_chunks - 1, np.arange(n_chunks) % 2 == 1, np.zeros(n_chunks, bool)):
        keep = np.repeat(cm, chunk)[:n]
        got, st = check(sp, qs, 1, 30, ("chunk mask", chunk, cm.tolist()), keep=keep, chunk_mask=cm)
        assert st["vectors_compared"] == int(keep.sum()) * len(qs)
        # the k of a call is cut at the rows the chunk mask leaves
        check(sp, qs, 0, n, ("chunk mask, every row", chunk), keep=keep, chunk_mask=cm)


# ---- 5. the life cycle: append, set again, clear, compact, read back -------------------------------------------------------------------------------

def test_append_makes_the_query_fail_and_setting_again_makes_it_pass():
    rng = np.random.default_rng(9)
    rows = SC.random_rows(rng, 100, 50, 5)
    sp = Sparse(rows, 50)
    qs = [SC.random_query(rng, 50, 10)]
    check(sp, qs, 1, 10, "before the append")
    sp.store.add_vector([0.0])
    with pytest.raises(OttersError) as ei:
        run(sp.store, qs, 1, 10)
    assert ei.value.status == -1 and "the sparse rows cover 100 rows, the store holds 101" in str(ei.value) and "set them again" in str(ei.value)
    assert sp.store.sparse_info()["nnz"] == int(sp.ptr[-1])  # the rows are left in place
    with pytest.raises(OttersError) as ei:
        sp.set()
    assert "100 sparse rows for a store of 101 rows" in str(ei.value)
    sp2 = Sparse.__new__(Sparse)
    sp2.rows = rows + [(SC.u32(3, 7), SC.f32(1.0, -0.5))]
    sp2.vocab, sp2.n, sp2.store, sp2._scores = 50, 101, sp.store, {}
    sp2.ptr, sp2.idx, sp2.val = SR.csr(sp2.rows)
    sp2.set()
    check(sp2, qs, 1, 101, "set again")
    # a refused call changes nothing: the rows above still answer
    bad = sp2.val.copy()
    bad[5] = np.inf
    for args, text in (((sp2.ptr, sp2.idx, bad, 50), "is not finite"), ((sp2.ptr, sp2.idx, sp2.val, 0), "vocab 0 is not in 1 .. OTT_SPARSE_MAX_VOCAB"),
                       ((sp2.ptr, sp2.idx, sp2.val, (1 << 20) + 1), "is not in 1 .. OTT_SPARSE_MAX_VOCAB"),
                       ((sp2.ptr, sp2.idx, sp2.val, int(sp2.idx.max())), "is not below vocab"),
                       ((sp2.ptr, sp2.idx[::-1].copy(), sp2.val, 50), "not strictly ascending")):
        with pytest.raises(OttersError) as ei:
            sp.store.set_sparse(*args)
        assert ei.value.status == -1 and text in str(ei.value), str(ei.value)
    check(sp2, qs, 1, 101, "after refused calls")
    with pytest.raises(OttersError) as ei:
        sp.store.compact()
    assert ei.value.status == -4 and "rows cannot move while sparse rows are set" in str(ei.value)
    sp.store.clear_sparse()
    assert sp.store.sparse_info() is None
    with pytest.raises(OttersError) as ei:
        run(sp.store, qs, 1, 10)
    assert "no sparse rows are set (ott_store_set_sparse)" in str(ei.value)
    sp.store.compact()  # allowed again


def test_query_refusals_that_need_a_store():
    rng = np.random.default_rng(10)
    sp = Sparse(SC.random_rows(rng, 70, 40, 5), 40)

    def refused(queries, text, status=-1, **kw):
        with pytest.raises(OttersError) as ei:
            run(sp.store, queries, 1, 5, **kw)
        assert ei.value.status == status and text in str(ei.value), str(ei.value)

    refused([(SC.u32(1), SC.f32(1.0)), (SC.u32(3, 40), SC.f32(1.0, 1.0))], "index 40 of query 1 is not below the store's vocab")
    refused([(SC.u32(5, 2, 5), SC.f32(1.0, 1.0, 1.0))], "index 5 appears twice in query 0")
    refused([(SC.u32(5, 2), SC.f32(1.0, np.nan))], "the weight of index 2 of query 0 is not finite")
    refused([(SC.u32(5), SC.f32(1.0))], "the MFMA path does not serve sparse queries", -4, path=Path.Mfma)
    sp.store.set_option("tie_order", 1)
    refused([(SC.u32(5), SC.f32(1.0))], "tie_order 1 and 2 are not served", -4)
    sp.store.set_option("tie_order", 0)
    got, _ = run(sp.store, [(SC.u32(5, 2), SC.f32(1.0, 0.5)), (SC.u32(2, 5), SC.f32(0.5, 1.0))], 1, 70)
    assert got[0].size and np.array_equal(got[0]["index"], got[1]["index"]) and np.array_equal(got[0]["score"], got[1]["score"])  # order is free
    with pytest.raises(OttersError) as ei:
        sp.store.set_option("sparse_table", 2)
    multi = VecStore(1, devices=[0, 0])
    multi.add_vectors(np.zeros((70, 1), np.float32))
    with pytest.raises(OttersError) as ei:
        multi.set_sparse(sp.ptr, sp.idx, sp.val, 40)
    assert ei.value.status == -4 and "a multi-GPU store is not served" in str(ei.value)


def test_an_empty_store_answers_with_no_hits():
    store = VecStore(1)
    store.set_sparse(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 10)
    assert store.sparse_info() == {"vocab": 10, "nnz": 0, "padded_entries": 0, "bytes": 8}
    got, _ = run(store, [(SC.u32(1), SC.f32(1.0))], 1, 5)
    assert got[0].size == 0


def test_read_sparse_round_trip_bit_for_bit(divergent):
    rng = np.random.default_rng(12)
    cases = [divergent[0], Sparse(*SC.ieee_case()[:2]), Sparse(SC.random_rows(rng, 129, 1 << 20, 12), 1 << 20)]
    for sp in cases:
        ptr, idx, val = sp.store.read_sparse()
        assert np.array_equal(ptr, sp.ptr) and np.array_equal(idx, sp.idx) and np.array_equal(val.view(np.uint32), sp.val.view(np.uint32))
        for first, n in ((0, 0), (sp.n, 0), (1, 1), (min(63, sp.n - 1), min(3, sp.n - min(63, sp.n - 1))), (sp.n // 2, sp.n - sp.n // 2)):
            ptr, idx, val = sp.store.read_sparse(first, n)
            lo, hi = int(sp.ptr[first]), int(sp.ptr[first + n])
            assert np.array_equal(ptr, sp.ptr[first:first + n + 1] - sp.ptr[first]), (first, n)
            assert np.array_equal(idx, sp.idx[lo:hi]) and np.array_equal(val.view(np.uint32), sp.val[lo:hi].view(np.uint32)), (first, n)
    sp = cases[0]
    out_ptr, out_idx, out_val = np.zeros(sp.n + 1, np.uint64), np.zeros(4, np.uint32), np.zeros(4, np.float32)
    L = N.lib()
    assert L.ott_store_read_sparse(sp.store._handle(), 0, sp.n, N.ptr(out_ptr), N.ptr(out_idx), N.ptr(out_val), 4) == -1
    assert f"entry_cap is too small: the range holds {int(sp.ptr[-1])} entries".encode() in L.ott_last_error()
    assert L.ott_store_read_sparse(sp.store._handle(), 1, sp.n, N.ptr(out_ptr), N.ptr(out_idx), N.ptr(out_val), 4) == -1
    assert b"are beyond the sparse rows" in L.ott_last_error()


# ---- 6. the table form's scratch: zero whenever a query finds it, one per context -----------------------------------------------------------------

def test_two_calls_in_succession_with_different_supports_find_the_table_zeroed(mid):
    sp, rng = mid
    a = [(np.arange(0, 1400, 7, dtype=np.uint32), np.full(200, 1.5, np.float32))] * 3
    b = [(np.arange(1400, 2800, 7, dtype=np.uint32), np.full(200, -0.75, np.float32))]
    c = [(np.arange(700, 2100, 7, dtype=np.uint32), (np.arange(200) % 5 - 2).astype(np.float32))] * 5
    sp.store.set_option("sparse_table", 1)
    for qs, name in ((a, "a"), (b, "b"), (c, "c"), (a, "a again")):
        S, cand = sp.scores(qs)
        got, _ = run(sp.store, qs, 1, 30)
        same(got, SR.expected(S, cand, 1, 30), ("table form, calls in succession", name))
    sp.store.set_option("sparse_table", -1)


def test_concurrent_callers_on_worker_contexts_get_the_serial_answers(mid):
    sp, rng = mid
    pool = np.arange(0, 3000, 7, dtype=np.uint32)
    sets = [[SC.random_query(rng, 3000, 20 + 15 * t, pool=pool) for _ in range(1 + t % 3)] for t in range(6)]
    for form in (0, 1):
        sp.store.set_option("sparse_table", form)
        serial = [run(sp.store, qs, 1, 20)[0] for qs in sets]
        got, errors = [None] * len(sets), []

        def work(i):
            try:
                for _ in range(3):
                    got[i] = run(sp.store, sets[i], 1, 20)[0]
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(len(sets))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for i in range(len(sets)):
            same(got[i], serial[i], ("concurrent", form, i))
    sp.store.set_option("sparse_table", -1)


# ---- 7. MetaStore -----------------------------------------------------------------------------------------------------------------------------------

def test_meta_sparse_query_with_a_meta_filter_against_the_model():
    rng = np.random.default_rng(15)
    n = 1500
    rows = SC.random_rows(rng, n, 400, 8)
    ptr, idx, val = SR.csr(rows)
    age = rng.integers(0, 100, n).astype(np.int32)
    order = np.sort(rng.integers(0, 1000, n)).astype(np.int64)  # ascending: the zone maps prune chunks
    ms = (MetaStore.from_columns([Column.from_numpy("age", DataType.Int32, age), Column.from_numpy("seq", DataType.Int64, order)])
          .with_vectors(np.zeros((n, 1), np.float32)).with_sparse(ptr, idx, val, 400).with_chunk_size(128).build())
    qs = [SC.random_query(rng, 400, L) for L in (30, 12)]
    S, cand = SR.scores(ptr, idx, val, qs, 400)
    for expr, keep in ((col("age").lt(40), age < 40), (col("seq").gt(700), order > 700), (col("age").gte(10).and_(col("seq").lte(300)), (age >= 10) & (order <= 300)),
                       (col("seq").gt(5000), np.zeros(n, bool))):
        for form in (0, 1):
            ms._store.set_option("sparse_table", form)
            hits, counts = ms.sparse_query(qs).meta_filter(expr).take(25).collect_arrays()
            got, at = [], 0
            for c in counts:
                got.append(hits[at:at + c])
                at += c
            same(got, SR.expected(S, cand, 1, 25, keep=keep), ("meta", str(keep.sum()), form))
    res = ms.sparse_query(qs[0]).meta_filter(col("age").lt(40)).vec_filter(0.0, Cmp.Gt).take(5).collect()
    exp = SR.expected(S[:1], cand[:1], 1, 5, int(Cmp.Gt), 0.0, age < 40)[0]
    assert res.indices == exp["index"].tolist() and res.column("age").values().tolist() == age[exp["index"].astype(np.int64)].tolist()
