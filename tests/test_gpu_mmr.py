"""GPU: MMR diversity re-ranking (ott_query_mmr, VecQueryPlan.mmr, MetaQueryPlan.mmr).  Bar: every case is
bit-equal to the host model tests/mmr_ref.py — indices, order, relevance bits, value bits, per-query counts.  No tolerances.

The model's candidates come from the oracle (canonical order); where the first stage runs under a mask, a path or a tie order of its
own, the model gets the library's own take(fetch_k) list — the candidates' contract — and only the selection is the model's.  Pair
scores use the STORE's inverse norms (store.inv_norms()).  Stores are a few thousand rows."""
import ctypes as C

import numpy as np
import pytest

import mmr_ref as R
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)
N_ROWS = 2000


@pytest.fixture(scope="module", autouse=True)
def collect_the_models_garbage():
    """The host model makes millions of short-lived Python objects (one oracle call per pair score).  They are collected here, when
    the module is done, so that the interpreter's next full collection does not fall into a test of another module that holds its
    own work to the host clock."""
    yield
    import gc
    gc.collect()


def make(dim, n=N_ROWS, seed=0, reduce_mode=0, rows=None):
    rng = np.random.default_rng(1000 * dim + seed)
    if rows is None:
        rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (9, dim)).astype(np.float32)
    store = VecStore(dim)
    store.set_reduce_order(reduce_mode)  # before the rows: the stored inverse norms are summed in it
    store.add_vectors(rows)
    return store, rows, q, store.inv_norms()


def take_of(plan, take, k):
    return plan.take_max(k) if take == 1 else plan.take_min(k)


def run(store, q, metric, take, k, fetch_k, lam, perq=False, **kw):
    p = take_of(store.query(q, metric), take, k).mmr(lam, fetch_k)
    if kw.get("flt") is not None:
        p = p.filter(*kw["flt"])
    if kw.get("mask") is not None:
        p = p.with_row_mask(kw["mask"])
    if kw.get("ids") is not None:
        p = p.with_row_ids(kw["ids"])
    if kw.get("path") is not None:
        p = p.with_path(kw["path"])
    return (p.per_query() if perq else p).collect_mmr()


def check(got, exp, where):
    (gh, gc, gv), (eh, ec, ev) = got, exp
    assert list(gc) == list(ec), (where, gc, ec)
    try:
        R.same(gh, gv, eh, ev)
    except AssertionError as e:
        raise AssertionError(f"{where}: {e}") from None


# ---- dims, metrics, takes, reduce orders ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [3, 8, 13, 64, 200, 768])  # below 8, no remainder, a remainder, short of the unrolled loop's 12 x 8, two unrolled steps and one single (25 x 8), wide
def test_every_metric_take_and_reduce_order(oracle, dim):
    for reduce_mode in (oracle.REDUCE_AVX, oracle.REDUCE_SEQ4):
        store, rows, q, inv = make(dim, reduce_mode=reduce_mode)
        for metric in ALL_METRICS:
            for take in (0, 1):
                exp = R.mmr(oracle, rows, q[0], metric, take, 7, 65, 0.5, reduce_mode=reduce_mode, inv=inv)
                check(run(store, q[0], metric, take, 7, 65, 0.5), exp, (dim, reduce_mode, metric, take))
        store.close()


# ---- lambda x (fetch_k, k) -----------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (2, 2), (63, 10), (64, 64), (65, 7), (200, 200), (1024, 10), (1024, 1024)]


@pytest.fixture(scope="module")
def shape_store(oracle):
    store, rows, q, inv = make(13, seed=1)
    cache = {}  # (metric, fetch_k) -> (candidates, their rows, their inverse norms, {s: P[s]}): made once, shared by every lambda and k

    def model(metric, take, k, fetch_k, lam):
        if (metric, fetch_k) not in cache:
            cand = R.candidates(oracle, rows, q[0], metric, take, fetch_k, inv=inv)
            idx = cand["index"].astype(np.int64)
            cache[(metric, fetch_k)] = (cand, np.ascontiguousarray(rows[idx]), inv[idx], {})
        cand, crow, cinv, prow = cache[(metric, fetch_k)]

        def pair_of(s):
            if s not in prow:
                prow[s] = R.pair_row(oracle, crow, cinv, s, metric)
            return prow[s]

        picks, vals = R.greedy(cand["score"], pair_of, k, lam, take)
        return cand[picks], [int(picks.size)], vals

    yield store, q, model
    store.close()


@pytest.mark.parametrize("fetch_k,k", SHAPES)
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 1.0])
def test_lambda_and_shapes(shape_store, lam, fetch_k, k):
    store, q, model = shape_store
    for metric in (Metric.Cosine, Metric.Euclidean):
        take = TAKE[metric]
        check(run(store, q[0], metric, take, k, fetch_k, lam), model(metric, take, k, fetch_k, lam), (metric, fetch_k, k, lam))


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_lambda_one_is_take_k_exactly(shape_store, metric):
    store, q, _ = shape_store
    plain, counts = take_of(store.query(q[0], metric), TAKE[metric], 25).collect_arrays()
    hits, c2, vals = run(store, q[0], metric, TAKE[metric], 25, 100, 1.0)
    assert counts == c2 == [25]
    assert hits.tobytes() == plain.tobytes()
    g = plain["score"] if TAKE[metric] == 1 else -plain["score"]
    assert np.array_equal(vals.view(np.uint32), g.view(np.uint32))  # 1 * g(rel) - 0 * red


def test_default_fetch_k_and_collect(shape_store, oracle):
    store, q, model = shape_store
    p = store.query(q[0], Metric.Cosine).take(10).mmr()
    assert p.resolve().mmr == (np.float32(0.5), 50)
    exp = model(Metric.Cosine, 1, 10, 50, 0.5)
    check(p.collect_mmr(), exp, "default")
    hits, counts = p.collect_arrays()
    assert hits.tobytes() == exp[0].tobytes() and counts == [10]
    assert [(r.index, np.float32(r.score)) for r in p.collect()] == [(int(i), s) for i, s in zip(exp[0]["index"], exp[0]["score"])]
    assert store.last_stats["total_ns"] > 0 and store.last_stats["vectors_compared"] == N_ROWS


# ---- short candidate lists -----------------------------------------------------------------------------------------------------------

def test_fewer_candidates_than_fetch_k(oracle):
    # a store of 40 rows
    store, rows, q, inv = make(13, n=40, seed=2)
    for metric in ALL_METRICS:
        exp = R.mmr(oracle, rows, q[0], metric, TAKE[metric], 50, 64, 0.5, inv=inv)
        assert exp[1] == [40]
        check(run(store, q[0], metric, TAKE[metric], 50, 64, 0.5), exp, ("40 rows", metric))
    store.close()
    store, rows, q, inv = make(13, seed=3)
    # a filter that passes 5 rows
    full = R.candidates(oracle, rows, q[0], Metric.Cosine, 1, 6, inv=inv)
    thr = float(full["score"][5])
    assert full["score"][4] > full["score"][5]
    exp = R.mmr(oracle, rows, q[0], Metric.Cosine, 1, 10, 50, 0.3, cmp=int(Cmp.Gt), thr=thr, inv=inv)
    assert exp[1] == [5]
    check(run(store, q[0], Metric.Cosine, 1, 10, 50, 0.3, flt=(thr, Cmp.Gt)), exp, "filter")
    # with_row_ids of 9 ids with duplicates (the gather route), and of 300 ids with fetch_k 200 (the mask route: more than 128 hits)
    rng = np.random.default_rng(5)
    for ids, k, fetch_k in ((np.array([7, 1999, 7, 3, 500, 501, 3, 64, 63, 1000, 8, 1999]), 6, 20), (rng.choice(N_ROWS, 300, replace=False), 15, 200)):
        u = np.unique(ids)
        assert u.size in (9, 300)
        for metric in (Metric.Cosine, Metric.Manhattan):
            cand = R.candidates(oracle, rows[u], q[1], metric, TAKE[metric], fetch_k, inv=inv[u])
            cand["index"] = u[cand["index"].astype(np.int64)]  # ascending ids keep the canonical order
            h, v = R.select(oracle, rows, inv, cand, metric, TAKE[metric], k, 0.5)
            check(run(store, q[1], metric, TAKE[metric], k, fetch_k, 0.5, ids=ids), (h, [h.size], v), ("ids", u.size, metric))
    store.close()


def test_duplicated_corpus_position_decides(oracle):
    rng = np.random.default_rng(17)
    base = rng.uniform(-1, 1, (400, 13)).astype(np.float32)
    store, rows, q, inv = make(13, rows=np.repeat(base, 3, axis=0), seed=4)
    for metric in ALL_METRICS:
        exp = R.mmr(oracle, rows, q[0], metric, TAKE[metric], 60, 60, 0.5, inv=inv)  # every candidate is picked: the copies too
        check(run(store, q[0], metric, TAKE[metric], 60, 60, 0.5), exp, metric)
        idx = exp[0]["index"].astype(np.int64)
        assert len(set((idx // 3).tolist())) < idx.size  # copies of one vector were picked: their order is the positions'
    store.close()


@pytest.mark.parametrize("nq", [2, 3, 9])
def test_per_query(oracle, nq):
    store, rows, q, inv = make(64, seed=5)
    for metric, k, fetch_k in ((Metric.Cosine, 10, 65), (Metric.Euclidean, 3, 200)):
        exp = R.mmr(oracle, rows, q[:nq], metric, TAKE[metric], k, fetch_k, 0.5, inv=inv)
        assert exp[1] == [k] * nq
        check(run(store, q[:nq], metric, TAKE[metric], k, fetch_k, 0.5, perq=True), exp, (nq, metric))
    store.close()


# ---- first-stage masks, paths and orders: the model gets the library's own take(fetch_k) list ------------------------------------------

def via_first_stage(oracle, store, rows, inv, plain_plan, mmr_plan, metric, take, k, lam, where):
    cand, counts = plain_plan.collect_arrays()
    assert cand.size > k, where
    h, v = R.select(oracle, rows, inv, cand, metric, take, k, lam)
    check(mmr_plan.collect_mmr(), (h, [h.size], v), where)
    return cand


def test_first_stage_masks_paths_and_tie_order(oracle):
    rng = np.random.default_rng(23)
    store, rows, q, inv = make(64, n=3000, seed=6)
    full = R.candidates(oracle, rows, q[0], Metric.DotProduct, 1, 40, inv=inv)
    # a row mask that drops every second of the best rows
    mask = np.ones(3000, bool)
    mask[full["index"][::2].astype(np.int64)] = False
    pl = lambda: store.query(q[0], Metric.DotProduct).with_row_mask(mask)  # noqa: E731
    cand = via_first_stage(oracle, store, rows, inv, pl().take(30), pl().take(8).mmr(0.5, 30), Metric.DotProduct, 1, 8, 0.5, "row mask")
    assert not np.isin(cand["index"], full["index"][::2]).any()
    exp = R.mmr(oracle, rows, q[0], Metric.DotProduct, 1, 8, 30, 0.5, row_mask=mask, inv=inv)
    check(pl().take(8).mmr(0.5, 30).collect_mmr(), exp, "row mask against the oracle")
    # Path.MFMA on a dot query
    pl = lambda: store.query(q[0], Metric.DotProduct).with_path(Path.Mfma)  # noqa: E731
    via_first_stage(oracle, store, rows, inv, pl().take(30), pl().take(8).mmr(0.5, 30), Metric.DotProduct, 1, 8, 0.5, "mfma")
    assert store.last_stats["path_used"] == int(Path.Mfma)
    check(pl().take(8).mmr(0.5, 30).collect_mmr(), R.mmr(oracle, rows, q[0], Metric.DotProduct, 1, 8, 30, 0.5, inv=inv), "mfma against the oracle")
    # deleted rows: a pair score reads stored data, the first stage skips the deleted rows
    dead = full["index"][1::3].astype(np.int64)
    store.delete_rows(dead)
    pl = lambda: store.query(q[0], Metric.DotProduct)  # noqa: E731
    cand = via_first_stage(oracle, store, rows, inv, pl().take(30), pl().take(8).mmr(0.5, 30), Metric.DotProduct, 1, 8, 0.5, "deleted")
    assert not np.isin(cand["index"], dead).any()
    live = np.ones(3000, bool)
    live[dead] = False
    check(pl().take(8).mmr(0.5, 30).collect_mmr(), R.mmr(oracle, rows, q[0], Metric.DotProduct, 1, 8, 30, 0.5, row_mask=live, inv=inv), "deleted against the oracle")
    store.close()
    # tie_order 1 on a corpus of duplicates: the reference's collector decides which copies are candidates and in which order
    base = rng.uniform(-1, 1, (500, 8)).astype(np.float32)
    store, rows, q, inv = make(8, rows=np.repeat(base, 4, axis=0), seed=7)
    store.set_tie_order("reference")
    pl = lambda: store.query(q[0], Metric.DotProduct)  # noqa: E731
    via_first_stage(oracle, store, rows, inv, pl().take(30), pl().take(9).mmr(0.5, 30), Metric.DotProduct, 1, 9, 0.5, "tie_order 1")
    store.close()


def test_chunk_mask_through_the_meta_plan(oracle):
    rng = np.random.default_rng(29)
    n, dim = 2048, 24
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    ms = (MetaStore.from_columns([Column("a", DataType.Int64).from_(list(range(n)))]).with_vectors(rows).with_chunk_size(256).build())
    flt = col("a").gte(300) & col("a").lt(1500)  # prunes whole chunks (a chunk mask) and needs a row mask inside two
    plain = ms.query(q, Metric.Cosine).meta_filter(flt).take(40).collect()
    assert ms.last_query_stats().pruned_chunks > 0
    cand = np.zeros(40, N.HIT_DTYPE)
    cand["index"], cand["score"] = plain.indices, np.array(plain.scores, np.float32)
    assert all(300 <= i < 1500 for i in plain.indices)
    h, _ = R.select(oracle, rows, ms._store.inv_norms(), cand, Metric.Cosine, 1, 10, 0.5)
    got = ms.query(q, Metric.Cosine).meta_filter(flt).take(10).mmr(0.5, 40).collect()
    assert got.indices == h["index"].tolist()
    assert np.array_equal(np.array(got.scores, np.float32).view(np.uint32), h["score"].view(np.uint32))
    with pytest.raises(OttersError, match="mmr takes one query"):
        ms.query_batch([q, q], Metric.Cosine).take(3).mmr().collect()
    with pytest.raises(OttersError, match="mmr needs an explicit take"):
        ms.query(q, Metric.Cosine).mmr().collect()


# ---- IEEE edges ----------------------------------------------------------------------------------------------------------------------

def test_pair_scores_overflow_to_inf_and_nan(oracle):
    rng = np.random.default_rng(31)
    rows = rng.uniform(-1, 1, (300, 13)).astype(np.float32)
    big = np.float32(3e38)
    # rows whose pair scores overflow: dot of two such rows is +inf, -inf, or inf - inf = NaN across the chains
    for i, pat in enumerate(([big, big], [big, -big], [-big, big], [-big, -big], [big, 0], [0, -big])):
        rows[10 * i + 3, :2] = pat
        rows[10 * i + 4, 8:10] = pat  # ... and in the second chunk of eight / the remainder
    store, rows, q, inv = make(13, rows=rows, seed=8)
    qq = (q[0] * np.float32(1e-3)).astype(np.float32)  # finite relevances: 3e38 x 1e-3
    seen = {}
    for metric in (Metric.DotProduct, Metric.Euclidean, Metric.Manhattan, Metric.Cosine):
        for lam, k in ((0.5, 300), (0.0, 40)):  # k = every row: the rows whose value stays NaN are picked too, last
            exp = R.mmr(oracle, rows, qq, metric, TAKE[metric], k, 300, lam, inv=inv)
            check(run(store, qq, metric, TAKE[metric], k, 300, lam), exp, (metric, lam))
            seen[(metric, lam)] = exp[2]
    # the case does reach the edges: infinite values under dot, and under Euclidean values that are NaN to the end (one bit pattern)
    assert np.isinf(seen[(Metric.DotProduct, 0.5)]).any() and (seen[(Metric.Euclidean, 0.5)].view(np.uint32) == 0x7FC00000).any()
    store.close()


# ---- refusals: OTT_ERR_UNSUPPORTED, nothing written -----------------------------------------------------------------------------------

def raw_call(store, q, k, fetch_k, mode):
    q = np.ascontiguousarray(q, np.float32).reshape(-1, store.dim)
    cap = 16
    out = np.zeros(cap, N.HIT_DTYPE)
    vals = np.zeros(cap, np.float32)
    n_out = C.c_uint64(77)
    per = (C.c_uint64 * q.shape[0])(*([55] * q.shape[0]))
    st = N.Stats()
    st.total_ns = 99
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k, d.mode = q.ctypes.data, q.shape[0], int(Metric.Cosine), 1, k, mode
    rc = N.lib().ott_query_mmr(store._handle(), C.byref(d), None, 0, fetch_k, 0.5, N.ptr(out), cap, C.byref(n_out), per, N.ptr(vals), C.byref(st))
    untouched = n_out.value == 77 and list(per) == [55] * q.shape[0] and st.total_ns == 99 and not out["index"].any() and not vals.any()
    return rc, N.lib().ott_last_error().decode(), untouched


def test_refusals_leave_nothing_written():
    rng = np.random.default_rng(37)
    multi = VecStore(8, devices=[0, 0])
    multi.add_vectors(rng.uniform(-1, 1, (100, 8)).astype(np.float32))
    rc, msg, untouched = raw_call(multi, np.ones(8), 2, 4, 0)
    assert rc == -4 and "multi-GPU store" in msg and untouched
    with pytest.raises(OttersError, match="multi-GPU store"):
        multi.query(np.ones(8, np.float32), Metric.Cosine).take(2).mmr().collect()
    multi.close()
    wide = VecStore(2049)
    wide.add_vectors(rng.uniform(-1, 1, (20, 2049)).astype(np.float32))
    rc, msg, untouched = raw_call(wide, np.ones(2049), 2, 4, 0)
    assert rc == -4 and "2048 floats" in msg and untouched
    wide.close()
    store = VecStore(8)
    store.add_vectors(rng.uniform(-1, 1, (100, 8)).astype(np.float32))
    rc, msg, untouched = raw_call(store, np.ones((65, 8)), 1, 1024, 1)  # 65 x 1024^2 x 4 B > 256 MiB
    assert rc == -4 and "256 MiB" in msg and untouched
    rc, msg, untouched = raw_call(store, np.ones((2, 8)), 2, 4, 0)
    assert rc == -4 and "OTT_MODE_MERGED takes one query" in msg and untouched
    rc, msg, untouched = raw_call(store, np.ones(8), 100, 200, 0)  # cap 16 < min(k, rows)
    assert rc == -1 and "capacity" in msg and untouched
    rc, msg, untouched = raw_call(store, np.ones((2, 8)), 2, 4, 1)  # ... and a call that is served writes all three
    assert rc == 0 and not untouched
    store.close()


def test_the_store_is_unchanged_by_an_mmr_call(oracle):
    store, rows, q, inv = make(64, seed=9)
    timing = ("prune_ns", "score_ns", "merge_ns", "total_ns")

    def plain():
        hits, counts = store.query(q[:3], Metric.Cosine).take(20).per_query().collect_arrays()
        return hits.tobytes(), counts, {k: v for k, v in store.last_stats.items() if k not in timing}

    before = plain()
    run(store, q[0], Metric.Cosine, 1, 10, 200, 0.5)
    run(store, q[:3], Metric.Euclidean, 0, 10, 64, 0.2, perq=True)
    assert plain() == before
    store.close()
