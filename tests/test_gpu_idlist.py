"""GPU: candidate id lists (ott_query_ids, ott_store_score_rows, VecQueryPlan.with_row_ids).  Bar: a query with
an id list returns exactly the hits — index, score bits, order, per-query counts — of the oracle run on the listed rows only
(ANDed with whatever mask the query carries), with the gather kernel forced on and forced off; raw scores are the oracle's
bits.  Bit for bit, no tolerances.

How the expectation is made: ONE oracle call per (store, metric, nq, take) ranks every (row, query) pair in the canonical
order; a score does not depend on the other rows and ascending ids keep the canonical tie order, so the oracle's answer on
rows[sorted_unique_ids] with the indices mapped back IS that ranking with the unlisted rows taken out (one case checks this
equivalence itself).  The reference tie orders call the oracle's literal collectors with the combined mask.  Manhattan goes
through tests/manhattan_ref.py."""
import numpy as np
import pytest

import ieee_edges as IE
import manhattan_ref as M
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), (where, got["query"][:12], ref["query"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def ranking(oracle, rows, q, metric, take, reduce_mode=0):
    """every (row, query) pair that has a score (NaN pairs are dropped), best first in the canonical order"""
    n, nq = rows.shape[0], q.shape[0]
    if metric == Metric.Manhattan:
        return M.select_canonical(M.scores(rows, q, "l1", reduce_mode), take, n * nq)
    return oracle.vec_query(rows, q, int(metric), take, n * nq, reduce_mode=reduce_mode, ties=oracle.TIES_CANONICAL)


class Rankings:
    def __init__(self, oracle, rows, q_pool, metric):
        self.args, self.have = (oracle, rows, q_pool, metric), {}

    def get(self, nq, take):
        if (nq, int(take)) not in self.have:
            oracle, rows, q_pool, metric = self.args
            self.have[(nq, int(take))] = ranking(oracle, rows, q_pool[:nq], metric, int(take))
        return self.have[(nq, int(take))]


def holds(score, cmp, thr):
    thr = np.float32(thr)
    return {0: np.ones(score.shape, bool), 1: score < thr, 2: score > thr, 3: score <= thr, 4: score >= thr, 5: score == thr}[int(cmp)]


def expected(full, keep, k, nq, perq, cmp=0, thr=0.0):
    """`full` restricted to the rows `keep` keeps and the pairs the filter passes, cut at k (per query: k each, in query order)"""
    f = full[keep[full["index"].astype(np.int64)]]
    f = f[holds(f["score"], cmp, thr)]
    if not perq:
        f = f[:k]
        return f, [int((f["query"] == qi).sum()) for qi in range(nq)]
    parts = [f[f["query"] == qi][:k] for qi in range(nq)]
    return np.concatenate(parts), [p.size for p in parts]


def id_mask(n, ids, caller=None, dead=None):
    keep = np.zeros(n, bool)
    keep[np.asarray(ids, np.int64)] = True
    if caller is not None:  # a caller mask shorter than n keeps the rows it does not reach (src/vec.rs:234)
        keep[:min(caller.size, n)] &= caller[:n]
    if dead is not None:
        keep[dead] = False
    return keep


def build(store, q, metric, k, path, perq, ids=None, mask=None, flt=None):
    p = store.query(q, metric)
    if ids is not None:
        p = p.with_row_ids(ids)
    if mask is not None:
        p = p.with_row_mask(mask)
    if flt is not None:
        p = p.filter(*flt)
    if k is not None:
        p = p.take(k)
    p = p.with_path(path)
    return p.per_query() if perq else p


# ---- 1. small store ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 40, 128])
def test_small_store_every_metric_path_batch_mode_k_and_list(oracle, dim):
    """300 rows: dims cover chain-only (8, 40, 128), tail-only (1, 3, 7) and both (9); lists cover the tile edges"""
    n = 300
    rng = np.random.default_rng(7000 + dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (9, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    for metric in ALL_METRICS:
        ranks = Rankings(oracle, rows, q_pool, metric)
        top = ranks.get(1, TAKE[metric])["index"][:10].astype(np.int64)
        lists = {
            "one id": [137], "63 ids": rng.choice(n, 63, replace=False), "64 ids": rng.choice(n, 64, replace=False),
            "65 ids": rng.choice(n, 65, replace=False), "every row": rng.permutation(n), "the last row": [n - 1],
            "unsorted with duplicates": np.concatenate([rng.choice(n, 90), [5, 5, 299, 0, 299]]), "inside the top-k": top[:7],
        }
        for lname, ids in lists.items():
            keep = id_mask(n, ids)
            for nq in (1, 3, 8, 9):
                q = q_pool[:nq]
                for perq in ((False, True) if nq > 1 else (False,)):
                    for k in (1, 10, 64, 65, None):
                        for path in (Path.Auto, Path.Exact, Path.Mfma):
                            if path == Path.Mfma and (dim < 8 or metric == Metric.Manhattan):
                                continue
                            where = (dim, metric, lname, nq, perq, k, path)
                            plan = build(store, q, metric, k, path, perq, ids=ids)
                            rq = plan.resolve()
                            ref, ref_counts = expected(ranks.get(nq, rq.take), keep, rq.k, nq, perq)
                            by_mask, mask_counts = build(store, q, metric, k, path, perq, mask=keep).collect_arrays()
                            bits_equal(by_mask, ref, where + ("row mask",))
                            for gather in (0, 1):
                                store.set_option("id_gather", gather)
                                got, counts = plan.collect_arrays()
                                bits_equal(got, ref, where + (gather,))
                                if perq:
                                    assert list(counts) == ref_counts == list(mask_counts), where + (gather,)
    store.close()


def test_oracle_on_the_subset_is_the_restricted_ranking(oracle):
    """what the module's expectation rests on, held to the oracle run on rows[sorted_unique_ids] itself"""
    n, dim = 300, 40
    rng = np.random.default_rng(1)
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)  # quantised: many equal scores, so the tie order is exercised
    q = rng.integers(-2, 3, (3, dim)).astype(np.float32)
    ids = np.concatenate([rng.choice(n, 120), [7, 7]])
    u = np.unique(ids)
    store = VecStore(dim)
    store.add_vectors(rows)
    for metric in (Metric.Cosine, Metric.Euclidean, Metric.DotProduct):
        for k in (1, 10, 65):
            sub = oracle.vec_query(rows[u], q, int(metric), TAKE[metric], k, ties=oracle.TIES_CANONICAL)
            sub["index"] = u[sub["index"].astype(np.int64)]
            full = ranking(oracle, rows, q, metric, TAKE[metric])
            bits_equal(expected(full, id_mask(n, ids), k, 3, False)[0], sub, ("model", metric, k))
            for gather in (0, 1):
                store.set_option("id_gather", gather)
                got, _ = build(store, q, metric, k, Path.Exact, False, ids=ids).collect_arrays()
                bits_equal(got, sub, ("subset", metric, k, gather))
    store.close()


# ---- 2. a store larger than the small-store kernel serves ------------------------------------------------------------------

def test_gather_on_a_store_of_more_than_1024_tiles(oracle):
    n, dim, cs = 70_000, 16, 1024
    rng = np.random.default_rng(2)
    store = VecStore(dim)
    store.append_random(n, 41)
    rows = oracle.rand_rows(0, n, dim, 41)
    q = rng.uniform(-1, 1, (1, dim)).astype(np.float32)
    lists = {
        "1": rng.choice(n, 1), "1000": rng.choice(n, 1000, replace=False), "65536": rng.choice(n, 65536, replace=False),
        "65537": rng.choice(n, 65537, replace=False), "block over a chunk boundary": np.arange(3 * cs - 100, 3 * cs + 131),
    }
    store.set_option("id_gather", 1)
    for metric in (Metric.Cosine, Metric.Manhattan):
        full = ranking(oracle, rows, q, metric, TAKE[metric])
        for lname, ids in lists.items():
            keep = id_mask(n, ids)
            for k in (1, 10, 100):
                got, _ = build(store, q, metric, k, Path.Exact, False, ids=ids).collect_arrays()
                bits_equal(got, expected(full, keep, k, 1, False)[0], ("70k", metric, lname, k))
                compared = store.last_stats["vectors_compared"]
                if lname in ("1", "1000", "65536"):  # the sweep did not run: it compares every row of the store
                    assert 0 < compared <= np.unique(ids).size, (lname, compared)
                    assert store.last_stats["path_used"] == int(Path.Exact)
                if lname == "65537":  # more than 1024 tiles: the mask route, which sweeps
                    assert compared == n, (lname, compared)
    store.close()


def test_dim_768_with_500_ids(oracle):
    n, dim = 6000, 768
    rng = np.random.default_rng(3)
    store = VecStore(dim)
    store.append_random(n, 43)
    rows = oracle.rand_rows(0, n, dim, 43)
    q_pool = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    ids = rng.choice(n, 500, replace=False)
    keep = id_mask(n, ids)
    for metric in ALL_METRICS:
        for nq in (1, 3):
            full = ranking(oracle, rows, q_pool[:nq], metric, TAKE[metric])
            for gather in (0, 1):
                store.set_option("id_gather", gather)
                got, _ = build(store, q_pool[:nq], metric, 10, Path.Auto, False, ids=ids).collect_arrays()
                bits_equal(got, expected(full, keep, 10, nq, False)[0], (768, metric, nq, gather))
    store.close()


# ---- 3. composition ----------------------------------------------------------------------------------------------------------

def test_list_and_caller_mask_and_deleted_rows_and_filter(oracle):
    n, dim = 5000, 24
    rng = np.random.default_rng(4)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    ids = rng.choice(n, 700)
    caller = rng.random(n - n // 7) < 0.6  # shorter than the store
    dead = rng.choice(ids, 150, replace=False)
    for metric in ALL_METRICS:
        ranks = Rankings(oracle, rows, q_pool, metric)
        thr = float(np.median(ranks.get(1, TAKE[metric])["score"]))
        for step in ("whole", "deleted", "restored"):
            if step == "deleted":
                store.delete_rows(dead)
            if step == "restored":
                store.restore_rows(dead)
            for mask in (None, caller):
                keep = id_mask(n, ids, mask, dead if step == "deleted" else None)
                for nq, perq in ((1, False), (3, False), (3, True)):
                    for flt in (None,) + tuple((thr, c) for c in (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq)):
                        for k in (10, 100, None):
                            plan = build(store, q_pool[:nq], metric, k, Path.Auto, perq, ids=ids, mask=mask, flt=flt)
                            rq = plan.resolve()
                            ref, ref_counts = expected(ranks.get(nq, rq.take), keep, rq.k, nq, perq, rq.filter_cmp, rq.filter_thr)
                            for gather in (0, 1):
                                store.set_option("id_gather", gather)
                                got, counts = plan.collect_arrays()
                                where = (metric, step, mask is not None, nq, perq, flt, k, gather)
                                bits_equal(got, ref, where)
                                if perq:
                                    assert list(counts) == ref_counts, where
    # Cmp.Eq with a threshold that some listed pair has
    full = ranking(oracle, rows, q_pool[:1], Metric.DotProduct, 1)
    keep = id_mask(n, ids)
    thr = float(expected(full, keep, 5, 1, False)[0]["score"][3])
    for gather in (0, 1):
        store.set_option("id_gather", gather)
        got, _ = build(store, q_pool[:1], Metric.DotProduct, 10, Path.Exact, False, ids=ids, flt=(thr, Cmp.Eq)).collect_arrays()
        assert got.size >= 1
        bits_equal(got, expected(full, keep, 10, 1, False, int(Cmp.Eq), thr)[0], ("eq", gather))
    store.close()


def test_list_and_a_metastore_filter_with_half_the_chunks_pruned(oracle):
    n, dim, cs = 20_000, 32, 1024
    rng = np.random.default_rng(5)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    age = rng.integers(0, 100, n).astype(np.int32)
    shelf = (np.arange(n) // cs).astype(np.int32)  # zone maps prune whole chunks on it
    meta = (MetaStore.from_columns([Column.from_numpy("age", DataType.Int32, age), Column.from_numpy("shelf", DataType.Int32, shelf)])
            .with_vectors(rows).with_chunk_size(cs).build())
    q = rng.uniform(-1, 1, (2, dim)).astype(np.float32)
    ids = rng.choice(n, 900)
    half = (n // cs + 1) // 2
    expr, fmask = col("age").lt(70) & col("shelf").gte(half), (age < 70) & (shelf >= half)
    keep = id_mask(n, ids) & fmask
    for metric in (Metric.Cosine, Metric.Euclidean, Metric.DotProduct):
        full = ranking(oracle, rows, q, metric, TAKE[metric])
        thr = float(np.median(full["score"]))
        for k in (1, 10, 100):
            for flt in (None, (thr, Cmp.Gt)):
                ref = expected(full, keep, k, 2, False, int(flt[1]) if flt else 0, thr)[0]
                for gather in (0, 1):
                    meta._store.set_option("id_gather", gather)
                    p = meta.query_batch(q, metric).meta_filter(expr).with_row_ids(ids).take(k)
                    res = (p.vec_filter(*flt) if flt else p).collect()
                    where = (metric, k, flt, gather)
                    assert res.indices == ref["index"].astype(np.int64).tolist(), where
                    assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), ref["score"].view(np.uint32)), where
                    if gather:  # ids of pruned chunks never reached the library, the rest were gathered
                        assert meta._store.last_stats["vectors_compared"] <= 2 * np.unique(ids).size


# ---- 4. tie orders and IEEE edge values --------------------------------------------------------------------------------------

def same_sets(got, lit, where):
    assert got.size == lit.size, (where, got.size, lit.size)
    assert np.array_equal(got["score"].view(np.uint32), lit["score"].view(np.uint32)), (where, "score sequence")
    a = sorted(zip(got["index"].tolist(), got["query"].tolist()))
    b = sorted(zip(lit["index"].tolist(), lit["query"].tolist()))
    assert a == b, (where, [x for x in a if x not in b][:8], [x for x in b if x not in a][:8])


@pytest.mark.parametrize("seed", range(2))
def test_reference_tie_orders_take_the_mask_route(oracle, seed):
    """quantised and constant rows: nearly every cut runs through equal scores.  With id_gather = 1 the reference tie orders must
    still give the literal collectors' outcome under the combined mask: the fallback engages"""
    rng = np.random.default_rng(950 + seed)
    n, dim, nq, cs = (4099, 5000)[seed], (8, 3)[seed], (1, 3)[seed], (1024, 500)[seed]
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    rows[n // 2:n // 2 + 600] = 1.0  # constant-score rows: flat scores
    q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    q[np.all(q == 0, axis=1)] = 1.0
    store = VecStore(dim)
    store.set_chunk_size(cs)
    store.add_vectors(rows)
    store.set_option("id_gather", 1)
    ids = np.concatenate([rng.choice(n, 800), np.arange(n // 2 + 50, n // 2 + 450)])
    for caller in (None, rng.random(n - 100) < 0.7):
        keep = id_mask(n, ids, caller)
        for metric, take in ((Metric.DotProduct, 1), (Metric.Euclidean, 0), (Metric.Cosine, 1)):
            for k in (1, 10, 100):
                def go():
                    p = store.query(q, metric).with_row_ids(ids)
                    if caller is not None:
                        p = p.with_row_mask(caller)
                    return (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact).collect_arrays()[0]
                where = (seed, metric, k, caller is not None)
                store.set_tie_order("canonical")
                bits_equal(go(), oracle.vec_query(rows, q, int(metric), take, k, row_mask=keep, ties=oracle.TIES_CANONICAL), where + (0,))
                store.set_tie_order("reference")
                same_sets(go(), oracle.vec_query(rows, q, int(metric), take, k, row_mask=keep, ties=oracle.TIES_LITERAL), where + (1,))
                store.set_tie_order("reference_chunked")
                lit, _ = oracle.meta_query(rows, cs, q, int(metric), take, k, row_mask=keep, ties=oracle.TIES_LITERAL)
                got = go()
                assert np.array_equal(got["score"].view(np.uint32), lit["score"].view(np.uint32)), where + (2,)
                assert sorted(got["index"].tolist()) == sorted(lit["index"].tolist()), where + (2,)
    store.close()


def dense_scores(full, nq, ids):
    """[nq, n_ids] from a full ranking: a pair the ranking dropped (a NaN score) is NaN"""
    n = int(max(int(np.max(ids)), int(full["index"].max()) if full.size else 0)) + 1
    S = np.full((nq, n), np.nan, np.float32)
    S[full["query"].astype(np.int64), full["index"].astype(np.int64)] = full["score"]
    return S[:, np.asarray(ids, np.int64)]


def scores_equal(got, ref, where):
    assert got.shape == ref.shape and got.dtype == np.float32, (where, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (where, "NaN pattern")
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok].view(np.uint32), ref[ok].view(np.uint32)), (where, got[ok][:8], ref[ok][:8])


@pytest.mark.parametrize("family, dim", [("a", 8), ("c", 8), ("a", 11), ("c", 11)])
def test_ieee_edge_values(oracle, family, dim):
    """NaN, +-inf and signed zeros: NaN pairs are dropped from ranked results and present as NaN in score_rows"""
    rng = np.random.default_rng(60 + dim)
    rows, q, _ = (IE.signed_zero_cosines if family == "a" else IE.overflow)(rng, n=200, dim=dim)
    rows[17, 0] = np.nan
    rows[18, dim - 1] = np.inf
    rows[19, 0] = -np.inf
    rows[20] = 0.0
    rows[21] = -0.0
    n, nq = rows.shape[0], q.shape[0]
    store = VecStore(dim)
    store.add_vectors(rows)
    ids = np.concatenate([[17, 18, 19, 20, 21, 17], rng.choice(n, 120)])
    keep = id_mask(n, ids)
    for metric in ALL_METRICS:
        full = ranking(oracle, rows, q, metric, TAKE[metric])
        scores_equal(store.score_rows(q, metric, ids), dense_scores(full, nq, ids), (family, dim, metric))
        if metric == Metric.DotProduct:
            assert np.isnan(store.score_rows(q, metric, [17])).all()
        for k in (1, 10, 100, None):
            for perq in (False, True):
                plan = build(store, q, metric, k, Path.Exact, perq, ids=ids)
                rq = plan.resolve()
                ref, ref_counts = expected(ranking(oracle, rows, q, metric, rq.take), keep, rq.k, nq, perq)
                for gather in (0, 1):
                    store.set_option("id_gather", gather)
                    got, counts = plan.collect_arrays()
                    bits_equal(got, ref, (family, dim, metric, k, perq, gather))
                    assert not np.isnan(got["score"]).any()
                    if perq:
                        assert list(counts) == ref_counts
    store.close()


# ---- 5. raw scores -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [3, 9, 128])
def test_score_rows_order_duplicates_deleted_rows_and_both_reduce_orders(oracle, dim):
    n = 2000
    rng = np.random.default_rng(80 + dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (9, dim)).astype(np.float32)
    for reduce_mode in (0, 1):
        store = VecStore(dim)
        store.set_reduce_order(reduce_mode)
        store.add_vectors(rows)
        ids = np.concatenate([[n - 1, 0, 0, 1999, 5], rng.choice(n, 300)])  # unsorted, with duplicates
        store.delete_rows(ids[:40])  # a deleted row is scored like any other: stored data is read
        for metric in ALL_METRICS:
            for nq in (1, 3, 9):
                full = ranking(oracle, rows, q_pool[:nq], metric, TAKE[metric], reduce_mode)
                got = store.score_rows(q_pool[:nq], metric, ids)
                scores_equal(got, dense_scores(full, nq, ids), (dim, reduce_mode, metric, nq))
                assert np.array_equal(got[:, 1].view(np.uint32), got[:, 2].view(np.uint32))  # the duplicate
        # ranked queries in the other reduce order too
        full = ranking(oracle, rows, q_pool[:3], Metric.Cosine, 1, reduce_mode)
        store.restore_rows(ids[:40])
        for gather in (0, 1):
            store.set_option("id_gather", gather)
            got, _ = build(store, q_pool[:3], Metric.Cosine, 10, Path.Exact, False, ids=ids).collect_arrays()
            bits_equal(got, expected(full, id_mask(n, ids), 10, 3, False)[0], (dim, reduce_mode, gather))
        assert store.score_rows(q_pool[:2], Metric.Cosine, []).shape == (2, 0)
        store.close()


def test_score_rows_list_of_70000_entries_takes_more_than_one_launch(oracle):
    n, dim = 30_000, 16
    rng = np.random.default_rng(9)
    store = VecStore(dim)
    store.append_random(n, 47)
    rows = oracle.rand_rows(0, n, dim, 47)
    q = rng.uniform(-1, 1, (2, dim)).astype(np.float32)
    ids = rng.choice(n, 70_000)  # more than 65536 slots: two launches per pass, duplicates throughout
    for metric in (Metric.Cosine, Metric.Euclidean):
        full = ranking(oracle, rows, q, metric, TAKE[metric])
        scores_equal(store.score_rows(q, metric, ids), dense_scores(full, 2, ids), ("70000", metric))
    store.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------

def test_errors_empty_list_and_empty_store():
    dim = 8
    rng = np.random.default_rng(10)
    rows = rng.uniform(-1, 1, (100, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    for gather in (0, 1):
        store.set_option("id_gather", gather)
        for bad in ([100], [0, 5, 100, 6], [2 ** 40]):
            with pytest.raises(OttersError) as e:
                store.query(q, Metric.Cosine).with_row_ids(bad).take(5).collect_arrays()
            assert e.value.status == -1 and "out of range" in str(e.value)
            with pytest.raises(OttersError) as e:
                store.score_rows(q, Metric.Cosine, bad)
            assert e.value.status == -1 and "out of range" in str(e.value)
        for perq in (False, True):
            got, counts = build(store, q, Metric.Cosine, 5, Path.Auto, perq, ids=[]).collect_arrays()
            assert got.size == 0 and list(counts) == [0, 0, 0]
        assert store.query(q, Metric.Cosine).with_row_ids([]).collect() == []
    with pytest.raises(OttersError):
        store.query(q, Metric.Cosine).with_row_ids([-1]).take(5).collect()
    store.close()
    empty = VecStore(dim)
    got, counts = empty.query(q, Metric.Cosine).with_row_ids([]).take(5).collect_arrays()
    assert got.size == 0 and list(counts) == [0, 0, 0]
    with pytest.raises(OttersError) as e:
        empty.query(q, Metric.Cosine).with_row_ids([0]).take(5).collect_arrays()
    assert e.value.status == -1
    empty.close()


# ---- 7. multi-GPU store ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ALL_METRICS)
def test_multi_gpu_store_equals_the_single_store(oracle, metric):
    n, dim = 3000, 24
    rng = np.random.default_rng(11)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    one = VecStore(dim)
    one.add_vectors(rows)
    multi = VecStore(dim, devices=[0] * 4)
    multi.add_vectors(rows)
    ids = np.concatenate([rng.choice(n, 400), [n - 1, 0]])
    caller = rng.random(n - 200) < 0.6
    dead = rng.choice(ids, 60, replace=False)
    for s in (one, multi):
        s.delete_rows(dead)
    full = ranking(oracle, rows, q, metric, TAKE[metric])
    for mask in (None, caller):
        keep = id_mask(n, ids, mask, dead)
        for k in (1, 10, 100):
            for perq in (False, True):
                a, ca = build(one, q, metric, k, Path.Auto, perq, ids=ids, mask=mask).collect_arrays()
                b, cb = build(multi, q, metric, k, Path.Auto, perq, ids=ids, mask=mask).collect_arrays()
                bits_equal(a, expected(full, keep, k, 3, perq)[0], ("single", metric, k, perq, mask is not None))
                bits_equal(b, a, ("multi", metric, k, perq, mask is not None))
                assert list(ca) == list(cb)
    scores_equal(multi.score_rows(q, metric, ids), one.score_rows(q, metric, ids), ("multi scores", metric))
    assert len(multi.shards()) == 4
    one.close()
    multi.close()
