"""GPU: hybrid search (ott_query_hybrid, VecStore.hybrid, MetaStore.hybrid) against the numpy model
(tests/hybrid_ref.py) fed with the ORACLE's dense leg lists and the sparse model's (tests/sparse_ref.py) sparse leg lists.  Bar: index,
F's f32 bits, order, counts and `query`, no tolerances.

Stores hold 1000 to 5000 rows of dims 8 and 33 with integer elements in -2..2 and sparse rows whose values are multiples of 1/4, so
exact score ties are frequent inside a leg (the canonical order decides the positions RRF reads) and between rows (equal F goes to the
lower row).  Vocab 100 takes the sparse sweep's LDS form, vocab 40000 its table form."""
import ctypes as C

import numpy as np
import pytest

import fuse_ref as R
import hybrid_cases as HC
import hybrid_ref as H
import sparse_cases as SC
import sparse_ref as SR
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, Path, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
FUSIONS = (R.RRF, R.DBSF, R.MINMAX)


def quantised(rng, shape):
    a = rng.integers(-2, 3, shape).astype(np.float32)
    flat = a.reshape(-1, a.shape[-1])
    flat[np.all(flat == 0, axis=1)] = 1.0
    return a


class World:
    """a store with dense and sparse rows, and the same rows as the models take them"""

    def __init__(self, dim, n, vocab, seed=0, rows=None, sparse=None, mean_len=8):
        self.rng = np.random.default_rng(9000 + 10 * dim + seed)
        self.rows = quantised(self.rng, (n, dim)) if rows is None else rows
        self.n, self.dim, self.vocab = self.rows.shape[0], dim, vocab
        self.pool = np.unique(np.concatenate([np.arange(min(vocab, 30)), self.rng.integers(0, vocab, 50)])).astype(np.uint32)  # rows and queries overlap
        self.sparse = SC.random_rows(self.rng, self.n, vocab, mean_len, pool=self.pool) if sparse is None else sparse
        self.ptr, self.idx, self.val = SR.csr(self.sparse)
        self.store = VecStore(dim)
        self.store.add_vectors(self.rows)
        self.store.set_sparse(self.ptr, self.idx, self.val, vocab)
        self.inv = self.store.inv_norms()

    def dense_sets(self, legs):
        return [quantised(self.rng, (l, self.dim)) if l else None for l in legs]

    def sparse_sets(self, legs, lens=(1, 6, 25)):
        return [[SC.random_query(self.rng, self.vocab, lens[(b + j) % len(lens)], pool=self.pool) for j in range(l)] for b, l in enumerate(legs)]

    def close(self):
        self.store.close()


def plan_of(store, dense, sparse, metric, fusion, k, fetch=None, rrf_k=60.0, weights=None, flt=None, sflt=None, mask=None, path=None, idf=False):
    p = store.hybrid(dense, sparse, metric)
    p = p.take_max(k) if TAKE[metric] == 1 else p.take_min(k)
    p = p.rrf(rrf_k) if fusion == R.RRF else p.dbsf() if fusion == R.DBSF else p.min_max()
    if fetch is not None:
        p = p.fetch(fetch)
    if weights is not None:
        p = p.weights(weights)
    if flt is not None:
        p = p.filter(*flt)
    if sflt is not None:
        p = p.sparse_filter(*sflt)
    if mask is not None:
        p = p.with_row_mask(mask)
    if path is not None:
        p = p.with_path(path)
    if idf:
        p = p.idf()
    return p


def expect(oracle, w, dense, sparse, metric, fusion, k, fetch, rrf_k=60.0, weights=None, flt=None, sflt=None, mask=None, base=0, idf=False, live=None):
    """the model's (hits, counts).  mask: bool[n], what the dense and the sparse legs may return (the caller's mask and the live rows);
    live: the rows the document frequencies count (None: all)"""
    take = TAKE[metric]
    nd, ns = [0 if t is None else len(t) for t in dense], [len(t) for t in sparse]
    dl = []
    if sum(nd):
        cmp, thr = (0, 0.0) if flt is None else (int(flt[1]), flt[0])
        dl = R.leg_lists(oracle, w.rows, np.concatenate([t for t in dense if t is not None]), metric, take, min(fetch, w.n), cmp, thr, mask, inv=w.inv, base=base)
    queries = [q for t in sparse for q in t]
    if idf:
        queries = H.idf_queries(queries, *H.df(w.ptr, w.idx, w.vocab, live))
    scmp, sthr = (0, 0.0) if sflt is None else (int(sflt[1]), sflt[0])
    sl = H.sparse_lists(w.ptr, w.idx, w.val, queries, w.vocab, fetch, scmp, sthr, mask, base)
    flat = None if weights is None else [x for ws in weights for x in ws]
    return H.hybrid(dl, sl, nd, ns, take, fusion, k, rrf_k, flat)


def same(got, exp, where):
    (gh, gc), (eh, ec) = got, exp
    assert list(gc) == list(ec), (where, list(gc), list(ec))
    assert np.array_equal(gh["index"], eh["index"]), (where, gh["index"][:12], eh["index"][:12])
    assert np.array_equal(gh["score"].view(np.uint32), eh["score"].view(np.uint32)), (where, gh["score"][:12], eh["score"][:12])
    assert np.array_equal(gh["query"], eh["query"]), where


LEGS = ((1, 1), (0, 2), (2, 0), (3, 2), (15, 1))  # (dense, sparse) legs of the five requests


# ---- fusions, metrics, dims, both forms of the sparse sweep ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,n,vocab", [(8, 1000, 100), (33, 5000, 40000), (33, 1300, 100), (8, 3000, 40000)])
def test_every_fusion_and_metric(oracle, dim, n, vocab):
    w = World(dim, n, vocab)
    dense, sparse = w.dense_sets([d for d, _ in LEGS]), w.sparse_sets([s for _, s in LEGS])
    for metric in TAKE:
        for fusion in FUSIONS:
            got = plan_of(w.store, dense, sparse, metric, fusion, 9, 30).collect_arrays()
            same(got, expect(oracle, w, dense, sparse, metric, fusion, 9, 30), (dim, n, vocab, metric, fusion))
    w.close()


@pytest.fixture(scope="module")
def wide():
    w = World(8, 3000, 100, seed=1, mean_len=12)
    yield w
    w.close()


@pytest.mark.parametrize("fetch", [1, 63, 64, 65, 512])
def test_entry_counts_straddle_the_network(oracle, wide, fetch):
    """(1 + 1) legs: 2, 126, 128, 130 and 1024 entries; (3 + 2) legs: 5, 315, 320, 325 and 2560; k below, at and above the union"""
    w = wide
    rng = np.random.default_rng(fetch)
    common = [(SC.u32(0, 1, 2, 3), SC.f32(1.0, 0.5, -1.0, 2.0))] * 2  # indices most rows store: lists as long as fetch
    for legs, sq in (((1, 1), [common[:1]]), ((3, 2), [common])):
        dense = [quantised(rng, (legs[0], 8))]
        for fusion in FUSIONS:
            full = expect(oracle, w, dense, sq, Metric.Euclidean, fusion, 10 ** 6, fetch)
            union = full[1][0]
            assert union >= min(fetch, 512)
            for k in sorted({1, union, union + 5, 10}):
                got = plan_of(w.store, dense, sq, Metric.Euclidean, fusion, k, fetch).collect_arrays()
                same(got, (full[0][:k], [min(k, union)]), (legs, fetch, fusion, k))


# ---- short and empty lists ---------------------------------------------------------------------------------------------------------------------

def test_short_and_empty_sparse_lists_and_an_empty_request(oracle):
    rng = np.random.default_rng(4)
    n, vocab = 1200, 100
    sparse = SC.random_rows(rng, n, vocab, 6, pool=np.arange(10, 60, dtype=np.uint32))
    sparse[7] = (SC.u32(0, 20), SC.f32(1.5, 0.25))        # index 0: one row
    for r in (100, 300, 301, 640, 1199):
        sparse[r] = (SC.u32(1), SC.f32(r / 1024.0))       # index 1: five rows; index 2 and 99: none
    w = World(8, n, vocab, seed=4, sparse=sparse)
    one, five, none, many = (SC.u32(0), SC.f32(2.0)), (SC.u32(1, 99), SC.f32(1.0, 1.0)), (SC.u32(2, 99), SC.f32(1.0, 3.0)), (SC.u32(10, 11, 12), SC.f32(1.0, 1.0, 1.0))
    dense = w.dense_sets([1, 1, 1, 1, 0])
    sq = [[one], [five], [none], [many, none], [none, one]]
    for fusion in FUSIONS:
        got = plan_of(w.store, dense, sq, Metric.Manhattan, fusion, 50, 40).collect_arrays()
        same(got, expect(oracle, w, dense, sq, Metric.Manhattan, fusion, 50, 40), ("short lists", fusion))
        # a dense filter no row passes empties every dense leg: request 2 has no list left at all, request 4 one entry
        flt = (-1.0, Cmp.Lt)
        got = plan_of(w.store, dense, sq, Metric.Manhattan, fusion, 50, 40, flt=flt).collect_arrays()
        exp = expect(oracle, w, dense, sq, Metric.Manhattan, fusion, 50, 40, flt=flt)
        assert exp[1][0] == 1 and exp[1][1] == 5 and exp[1][2] == 0 and exp[1][4] == 1
        same(got, exp, ("empty request", fusion))
    w.close()


# ---- the sharp cases of tests/hybrid_cases.py on the device -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_sharp_cases(oracle, name):
    c = HC.CASES[name]()
    w = World(HC.DIM, 0, c["vocab"], rows=c["rows"], sparse=c["sparse"])
    dense, sq = [c["dense"]], [c["sparse_q"]]
    weights = None if c["weights"] is None else [c["weights"]]
    got = plan_of(w.store, dense, sq, c["metric"], c["fusion"], c["k"], c["fetch"], rrf_k=c["rrf_k"], weights=weights, idf=c["idf"]).collect_arrays()
    same(got, expect(oracle, w, dense, sq, c["metric"], c["fusion"], c["k"], c["fetch"], rrf_k=c["rrf_k"], weights=weights, idf=c["idf"]), name)
    assert got[0]["index"].tolist() == [c["first"]] != [c["wrong_first"]]
    w.close()


# ---- weights, rrf_k, the filters -------------------------------------------------------------------------------------------------------------

def test_weights_rrf_k_and_the_two_filters(oracle):
    w = World(8, 1500, 100, seed=5)
    dense, sq = w.dense_sets([2, 1, 0]), w.sparse_sets([1, 2, 2])
    for fusion in FUSIONS:
        absent = plan_of(w.store, dense, sq, Metric.Euclidean, fusion, 40, 30).collect_arrays()
        ones = plan_of(w.store, dense, sq, Metric.Euclidean, fusion, 40, 30, weights=[[1, 1, 1], [1, 1, 1], [1, 1]]).collect_arrays()
        same(ones, absent, ("all 1 = absent", fusion))
        for ws in ([[1.0, -1.0, 0.25], [-3.0, 1e-3, 2.0], [0.5, 4.0]], [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0]]):  # (dense.., sparse..) per request
            got = plan_of(w.store, dense, sq, Metric.Euclidean, fusion, 40, 30, weights=ws).collect_arrays()
            same(got, expect(oracle, w, dense, sq, Metric.Euclidean, fusion, 40, 30, weights=ws), ("weights", fusion, ws))
        # the sparse filter acts on the sparse legs, the dense filter on the dense legs only
        for flt, sflt in ((None, (0.5, Cmp.Gt)), ((9.0, Cmp.Lt), None), ((9.0, Cmp.Lte), (0.0, Cmp.Lte)), ((1.0, Cmp.Lt), (100.0, Cmp.Gt))):
            got = plan_of(w.store, dense, sq, Metric.Euclidean, fusion, 40, 30, flt=flt, sflt=sflt).collect_arrays()
            same(got, expect(oracle, w, dense, sq, Metric.Euclidean, fusion, 40, 30, flt=flt, sflt=sflt), ("filters", fusion, flt, sflt))
    plain, no_sparse = (expect(oracle, w, dense, sq, Metric.Euclidean, R.MINMAX, 40, 30, sflt=f) for f in (None, (100.0, Cmp.Gt)))
    assert plain[1] != no_sparse[1] and no_sparse[1][2] == 0  # a sparse filter nothing passes: request 2 (sparse legs only) is empty
    for rrf_k in (0.0, 60.0, 0.5):
        got = plan_of(w.store, dense, sq, Metric.Cosine, R.RRF, 40, 30, rrf_k=rrf_k).collect_arrays()
        same(got, expect(oracle, w, dense, sq, Metric.Cosine, R.RRF, 40, 30, rrf_k=rrf_k), ("rrf_k", rrf_k))
    for fusion in FUSIONS:  # IDF in the hybrid call
        got = plan_of(w.store, dense, sq, Metric.DotProduct, fusion, 40, 30, idf=True).collect_arrays()
        same(got, expect(oracle, w, dense, sq, Metric.DotProduct, fusion, 40, 30, idf=True), ("idf", fusion))
    w.close()


# ---- store state: the same rows vanish from both kinds of leg ---------------------------------------------------------------------------------

def test_base_offset_deleted_rows_and_a_row_mask(oracle):
    w = World(33, 1200, 40000, seed=6)
    dense, sq = w.dense_sets([2, 0, 1]), w.sparse_sets([1, 2, 1])
    w.store.set_base_offset(5_000_000_000)
    dead = w.rng.choice(1200, 300, replace=False)
    w.store.delete_rows(dead)
    live = np.ones(1200, bool)
    live[dead] = False
    mask = np.ones(1200, bool)
    mask[::3] = False
    for fusion in FUSIONS:
        got = plan_of(w.store, dense, sq, Metric.Cosine, fusion, 25, 40, idf=True).collect_arrays()
        exp = expect(oracle, w, dense, sq, Metric.Cosine, fusion, 25, 40, mask=live, base=5_000_000_000, idf=True, live=live)
        assert exp[0]["index"].min() >= 5_000_000_000 and not np.isin(exp[0]["index"] - 5_000_000_000, dead).any()
        same(got, exp, ("base offset, deleted", fusion))
        got = plan_of(w.store, dense, sq, Metric.Cosine, fusion, 25, 40, mask=mask).collect_arrays()
        same(got, expect(oracle, w, dense, sq, Metric.Cosine, fusion, 25, 40, mask=mask & live, base=5_000_000_000), ("row mask", fusion))
    w.close()


def test_chunk_mask_and_device_row_mask_through_the_meta_plan(oracle):
    rng = np.random.default_rng(13)
    n, dim, vocab = 2048, 8, 100
    w = World(dim, n, vocab, seed=7)
    ms = (MetaStore.from_columns([Column("a", DataType.Int64).from_(list(range(n)))]).with_vectors(w.rows).with_sparse(w.ptr, w.idx, w.val, vocab)
          .with_chunk_size(64).build())
    flt = col("a").gte(300) & col("a").lt(1500)  # prunes whole chunks (a chunk mask) and needs a row mask inside two
    keep = (np.arange(n) >= 300) & (np.arange(n) < 1500)
    dense, sq = [quantised(rng, (2, dim)), None], w.sparse_sets([1, 2])
    w.inv = ms._store.inv_norms()
    for fusion in FUSIONS:
        p = ms.hybrid(dense, sq, Metric.DotProduct).meta_filter(flt).fetch(50).take(20)
        p = p.rrf(2.0) if fusion == R.RRF else p.dbsf() if fusion == R.DBSF else p.min_max()
        got = p.collect_arrays()
        assert ms._store.last_stats["pruned_chunks"] > 0
        same(got, expect(oracle, w, dense, sq, Metric.DotProduct, fusion, 20, 50, rrf_k=2.0, mask=keep), ("meta", fusion))
    res = ms.hybrid(dense, sq, Metric.DotProduct).meta_filter(flt).idf().sparse_filter(0.0, Cmp.Gt).fetch(50).take(4).collect()
    assert [len(r.indices) for r in res] == [4, 4] and all(300 <= i < 1500 for r in res for i in r.indices)
    w.close()


# ---- what the call must agree with ---------------------------------------------------------------------------------------------------------------

def test_without_sparse_legs_it_is_ott_query_fuse_and_one_sparse_leg_is_ott_query_sparse(oracle):
    w = World(33, 2000, 100, seed=8)
    dense = w.dense_sets([3, 1, 16])
    for metric in (Metric.Euclidean, Metric.Cosine):
        for fusion in FUSIONS:
            f = w.store.fuse(dense, metric).fetch(64).take(30)
            f = f.rrf() if fusion == R.RRF else f.dbsf() if fusion == R.DBSF else f.min_max()
            for path in (Path.Auto, Path.Exact):
                same(plan_of(w.store, dense, None, metric, fusion, 30, 64, path=path).collect_arrays(), f.with_path(path).collect_arrays(), ("= fuse", metric, fusion, path))
    # one request, one sparse leg, RRF, weight 1: exactly the rows of ott_query_sparse, in its order
    q = SC.random_query(w.rng, 100, 6, pool=w.pool)
    hits, _ = w.store.sparse_query(q).take_max(64).collect_arrays()
    got, counts = plan_of(w.store, None, [[q]], Metric.DotProduct, R.RRF, 64, 64).collect_arrays()
    assert counts == [hits.size] and hits.size == 64 and np.array_equal(got["index"], hits["index"])
    assert np.array_equal(got["score"], np.float32(1.0) / (np.float32(60.0) + np.arange(1, 65, dtype=np.float32)))
    w.close()


def test_paths_give_the_same_bits_and_many_requests(oracle):
    w = World(8, 1000, 40000, seed=9)
    legs = [(b % 4, (b * 7) % 3 + (1 if b % 4 == 0 else 0)) for b in range(64)]  # 64 requests of 1 to 5 legs, some without a dense, some without a sparse leg
    assert {d for d, _ in legs} == {0, 1, 2, 3} and 0 in {s for _, s in legs} and all(d + s >= 1 for d, s in legs)
    dense, sq = w.dense_sets([d for d, _ in legs]), w.sparse_sets([s for _, s in legs])
    for fusion in FUSIONS:
        exp = expect(oracle, w, dense, sq, Metric.Euclidean, fusion, 7, 20)
        for path in (Path.Auto, Path.Exact):
            same(plan_of(w.store, dense, sq, Metric.Euclidean, fusion, 7, 20, path=path).collect_arrays(), exp, ("64 requests", fusion, path))
    w.close()


# ---- stats, and the refusals that need a store ---------------------------------------------------------------------------------------------------

def raw_call(store, legs, dense_per, sq, sparse_per, k, fetch, cap, out, fusion=0, flags=0):
    legs = np.ascontiguousarray(legs, np.float32)
    dp, sp = np.array(dense_per, np.uint32), np.array(sparse_per, np.uint32)
    ptr, idx, val = SR.csr(sq)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = legs.ctypes.data, legs.shape[0], int(Metric.DotProduct), 1, 1, k, 0
    n_out = C.c_uint64(77)
    per = (C.c_uint64 * len(dense_per))(*([77] * len(dense_per)))
    st = N.Stats()
    rc = N.lib().ott_query_hybrid(store._handle(), C.byref(d), N.ptr(dp), N.ptr(ptr), N.ptr(idx), N.ptr(val), len(sq), N.ptr(sp), 0, 0.0, flags, len(dense_per), fusion, 60.0,
                                  None, fetch, None if out is None else N.ptr(out), cap, C.byref(n_out), per, C.byref(st))
    return rc, N.lib().ott_last_error().decode(), n_out.value, list(per), st.as_dict()


def test_stats_and_the_refusals_that_need_a_store(oracle):
    w = World(8, 300, 100, seed=10)
    legs = quantised(w.rng, (3, 8))
    sq = [(SC.u32(0, 1), SC.f32(1.0, 1.0)), (SC.u32(2), SC.f32(1.0))]
    out = np.zeros(64, N.HIT_DTYPE)
    # cap: the sum over the requests of min(k, legs x min(fetch, rows)) = min(10, 3 x 4) + min(10, 2 x 4) = 18
    rc, err, n_out, per, _ = raw_call(w.store, legs, [2, 1], sq, [1, 1], 10, 4, 17, out)
    assert rc == -1 and "ott_query_hybrid: output capacity is smaller than the sum over the requests" in err and n_out == 77 and per == [77, 77] and not out["index"].any()
    rc, err, n_out, per, _ = raw_call(w.store, legs, [2, 1], sq, [1, 1], 10, 4, 18, None)
    assert rc == -1 and "ott_query_hybrid: out is NULL" in err and n_out == 77
    rc, err, n_out, *_ = raw_call(w.store, legs, [2, 1], [(SC.u32(100), SC.f32(1.0)), sq[1]], [1, 1], 10, 4, 18, out)
    assert rc == -1 and "ott_query_hybrid: index 100 of sparse query 0 is not below the store's vocab" in err and n_out == 77
    rc, err, *_ = raw_call(w.store, legs, [2, 1], [(SC.u32(5, 5), SC.f32(1.0, 1.0)), sq[1]], [1, 1], 10, 4, 18, out)
    assert rc == -1 and "ott_query_hybrid: index 5 appears twice in sparse query 0" in err
    rc, err, *_ = raw_call(w.store, legs, [2, 1], [sq[0], (SC.u32(5), SC.f32(np.inf))], [1, 1], 10, 4, 18, out)
    assert rc == -1 and "ott_query_hybrid: the weight of index 5 of sparse query 1 is not finite" in err
    rc, err, n_out, per, st = raw_call(w.store, legs, [2, 1], sq, [1, 1], 10, 4, 18, out, flags=1)
    exp = expect(oracle, w, [legs[:2], legs[2:]], [[sq[0]], [sq[1]]], Metric.DotProduct, R.RRF, 10, 4, idf=True)
    assert rc == 0 and n_out == sum(per) and per == exp[1] and np.array_equal(out["index"][:n_out], exp[0]["index"])
    assert st["path_used"] in (int(Path.Exact), int(Path.Mfma)) and st["passes"] >= 2 and st["vectors_compared"] == 3 * 300 + 2 * 300  # both stages
    dense_only = raw_call(w.store, legs, [2, 1], [], [0, 0], 10, 4, 18, out)[4]
    assert st["bytes_scanned"] > dense_only["bytes_scanned"] > 0 and st["merge_ns"] > 0 and st["total_ns"] >= st["merge_ns"]
    rc, err, n_out, per, st = raw_call(w.store, np.zeros((0, 8), np.float32), [0, 0], sq, [1, 1], 10, 4, 18, out)  # no dense stage
    assert rc == 0 and st["path_used"] == int(Path.Exact) and st["vectors_compared"] == 2 * 300 and st["passes"] >= 1 and st["merge_ns"] > 0
    # rows appended since set_sparse, no sparse rows: refused only where a sparse leg exists
    w.store.add_vectors(quantised(w.rng, (2, 8)))
    rc, err, *_ = raw_call(w.store, legs, [2, 1], sq, [1, 1], 10, 4, 18, out)
    assert rc == -1 and "ott_query_hybrid: the sparse rows cover 300 rows, the store holds 302" in err
    w.store.clear_sparse()
    rc, err, *_ = raw_call(w.store, legs, [2, 1], sq, [1, 1], 10, 4, 18, out)
    assert rc == -1 and "ott_query_hybrid: no sparse rows are set (ott_store_set_sparse)" in err
    assert raw_call(w.store, legs, [2, 1], [], [0, 0], 10, 4, 18, out)[0] == 0
    # tie orders 1 and 2 are refused for the whole call, whether or not a sparse leg exists
    for tie_order in (1, 2):
        w.store.set_option("tie_order", tie_order)
        for s, sp in ((sq, [1, 1]), ([], [0, 0])):
            rc, err, *_ = raw_call(w.store, legs, [2, 1], s, sp, 10, 4, 18, out)
            assert rc == -4 and "ott_query_hybrid: tie_order 1 and 2 are not served" in err
    w.close()
    multi = VecStore(8, devices=[0, 0])
    multi.add_vectors(w.rows)
    rc, err, *_ = raw_call(multi, legs, [2, 1], sq, [1, 1], 10, 4, 64, out)
    assert rc == -4 and "ott_query_hybrid: a multi-GPU store is not served" in err
