"""GPU: grouped search (ott_query_groups, VecQueryPlan.one_per_group, MetaQueryPlan.distinct_by).  Bar: a grouped
query returns exactly the hits — index, query, score bits, order, per-query counts — of the same query with the default take
after dropping every hit whose group occurred earlier in that list, cut at k.  Bit for bit, no tolerances.

How the expectation is made: ONE oracle call per (store, metric, nq, take) ranks every (row, query) pair in the canonical
order (Manhattan: tests/manhattan_ref.py); it is restricted to the kept rows and the pairs the filter passes; per query the first
occurrence of every group is taken (np.unique(..., return_index=True)); cut at k."""
import numpy as np
import pytest

import manhattan_ref as M
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, Mode, OttersError, Path, VecStore, col

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), (where, got["query"][:12], ref["query"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def take_of(metric, k):
    """the take type of a plan: take(k) infers it from the metric, a plan without take() ranks by Max (src/vec.rs:214)"""
    return TAKE[metric] if k is not None else 1


class Rankings:
    """the full canonical ranking per (metric, nq, take), made once"""

    def __init__(self, oracle, rows, q_pool):
        self.args, self.have = (oracle, rows, q_pool), {}

    def get(self, metric, nq, k):
        key = (metric, nq, take_of(metric, k))
        if key not in self.have:
            oracle, rows, q_pool = self.args
            self.have[key] = ranking(oracle, rows, q_pool[:nq], metric, key[2])
        return self.have[key]


def ranking(oracle, rows, q, metric, take):
    """every (row, query) pair that has a score (NaN pairs are dropped), best first in the canonical order"""
    n, nq = rows.shape[0], q.shape[0]
    if metric == Metric.Manhattan:
        return M.select_canonical(M.scores(rows, q, "l1", 0), take, n * nq)
    return oracle.vec_query(rows, q, int(metric), take, n * nq, ties=oracle.TIES_CANONICAL)


def holds(score, cmp, thr):
    thr = np.float32(thr)
    return {0: np.ones(score.shape, bool), 1: score < thr, 2: score > thr, 3: score <= thr, 4: score >= thr, 5: score == thr}[int(cmp)]


def expected(full, gid, keep, k, nq, cmp=0, thr=0.0):
    """`full` restricted to the kept rows and passing pairs; per query the first hit of every group; cut at k"""
    f = full[keep[full["index"].astype(np.int64)]]
    f = f[holds(f["score"], cmp, thr)]
    parts = []
    for qi in range(nq):
        fq = f[f["query"] == qi]
        _, first = np.unique(gid[fq["index"].astype(np.int64)], return_index=True)
        parts.append(fq[np.sort(first)][:k])
    return np.concatenate(parts), [p.size for p in parts]


def build(store, q, metric, k, path=Path.Auto, perq=False, mask=None, flt=None):
    p = store.query(q, metric).one_per_group()
    if mask is not None:
        p = p.with_row_mask(mask)
    if flt is not None:
        p = p.filter(*flt)
    if k is not None:
        p = p.take(k)
    p = p.with_path(path)
    return p.per_query() if perq else p


def layouts(rng, n):
    return {
        "one group": np.zeros(n, np.int64),
        "two groups": rng.integers(0, 2, n),
        "37 random groups": rng.integers(0, 37, n) * 1000 - 5,  # (labels need not be dense)
        "every row its own": rng.permutation(n),
        "contiguous by row": np.arange(n) // 8,
    }


def check_store(oracle, store, rows, q_pool, metrics, nqs, ks, paths, rng, lay=None):
    n = rows.shape[0]
    keep = np.ones(n, bool)
    ranks = Rankings(oracle, rows, q_pool)
    for lname, labels in (lay or layouts(rng, n)).items():
        store.set_groups(labels)
        gid = np.unique(labels, return_inverse=True)[1].reshape(-1)
        assert store.group_count() == int(gid.max()) + 1
        for metric in metrics:
            for nq in nqs:
                for k in ks:
                    for path in paths:
                        where = (lname, metric, nq, k, path)
                        plan = build(store, q_pool[:nq], metric, k, path, perq=nq > 1)
                        ref, ref_counts = expected(ranks.get(metric, nq, k), gid, keep, plan.resolve().k, nq)
                        got, counts = plan.collect_arrays()
                        bits_equal(got, ref, where)
                        assert list(counts) == ref_counts, where


# ---- 1. small store ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 40, 128])
def test_small_store_every_metric_layout_batch_k_and_path(oracle, dim):
    """300 rows: four full tiles and a partial one; dims cover tail only (1, 3, 7), chains only (8, 40, 128) and both (9); k covers
    the register lists' sizes (64 | 65, 512 | 513 = the sort path; every k above the group count is the group count) and no take"""
    rng = np.random.default_rng(8000 + dim)
    rows = rng.uniform(-1, 1, (300, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (9, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    check_store(oracle, store, rows, q_pool, ALL_METRICS, (1, 3, 8, 9), (1, 10, 64, 65, 512, 513, None), (Path.Auto, Path.Exact), rng)
    store.close()


def test_small_store_quantised_rows_for_the_ties(oracle):
    """integers in -2..2: equal scores inside a group and between groups, so the lower row must win both times"""
    rng = np.random.default_rng(8200)
    rows = rng.integers(-2, 3, (300, 9)).astype(np.float32)
    q_pool = rng.integers(-2, 3, (9, 9)).astype(np.float32)
    store = VecStore(9)
    store.add_vectors(rows)
    check_store(oracle, store, rows, q_pool, ALL_METRICS, (1, 3, 9), (1, 10, 65, None), (Path.Auto,), rng)
    store.close()


def test_more_groups_than_the_register_lists_hold(oracle):
    """3000 rows, 1500 and 3000 groups: k = 512 fills the eight-entry lists from many select workgroups, 513 / 600 / no take sort"""
    rng = np.random.default_rng(8300)
    rows = rng.uniform(-1, 1, (3000, 24)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (5, 24)).astype(np.float32)
    store = VecStore(24)
    store.add_vectors(rows)
    lay = {"pairs": np.arange(3000) // 2, "own": rng.permutation(3000)}
    check_store(oracle, store, rows, q_pool, (Metric.Cosine, Metric.Euclidean), (1, 5), (100, 512, 513, 600, None), (Path.Auto,), rng, lay)
    store.close()


# ---- 2. masks and filters ---------------------------------------------------------------------------------------------------------

def test_row_mask_deleted_rows_restore_and_every_cmp(oracle):
    n, dim = 300, 40
    rng = np.random.default_rng(8400)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    labels = rng.integers(0, 37, n)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(labels)
    gid = labels
    metric = Metric.Cosine
    full1, full3 = ranking(oracle, rows, q[:1], metric, 1), ranking(oracle, rows, q, metric, 1)
    # a caller mask shorter than the store keeps the rows it does not reach (src/vec.rs:234)
    caller = rng.random(200) < 0.5
    keep = np.ones(n, bool)
    keep[:200] = caller
    for k in (1, 10, None):
        ref, _ = expected(full1, gid, keep, k or 37, 1)
        bits_equal(build(store, q[:1], metric, k, mask=caller).collect_arrays()[0], ref, ("caller mask", k))
    # deleted: the current best row of a group (its next best row represents it), and a whole group (it disappears)
    best = int(full1["index"][0])
    whole = np.flatnonzero(gid == gid[int(full1["index"][1])] if gid[int(full1["index"][1])] != gid[best] else gid == (gid[best] + 1) % 37)
    dead = np.unique(np.concatenate([[best], whole, rng.choice(n, 30)]))
    assert store.delete_rows(dead) == dead.size
    alive = np.ones(n, bool)
    alive[dead] = False
    for nq, full in ((1, full1), (3, full3)):
        for k in (1, 10, None):
            ref, ref_counts = expected(full, gid, alive, k or 37, nq)
            got, counts = build(store, q[:nq], metric, k, perq=nq > 1).collect_arrays()
            bits_equal(got, ref, ("deleted", nq, k))
            assert list(counts) == ref_counts
            if nq == 1:
                assert gid[whole[0]] not in gid[got["index"].astype(np.int64)]
                ref, _ = expected(full, gid, alive & keep, k or 37, 1)
                bits_equal(build(store, q[:1], metric, k, mask=caller).collect_arrays()[0], ref, ("deleted & caller mask", k))
    assert store.restore_rows(dead) == dead.size
    ref, _ = expected(full1, gid, np.ones(n, bool), 10, 1)
    bits_equal(build(store, q[:1], metric, 10).collect_arrays()[0], ref, "restored")
    # every Cmp, on both takes' metrics: a filtered row never represents its group
    ranks = Rankings(oracle, rows, q)
    for metric in (Metric.Cosine, Metric.Euclidean):
        thr = float(np.median(ranks.get(metric, 1, 5)["score"]))
        exact = float(ranks.get(metric, 1, 5)["score"][5])  # Eq: a score that occurs
        for cmp in Cmp:
            t = exact if cmp == Cmp.Eq else thr
            for k in (5, None):
                ref, _ = expected(ranks.get(metric, 1, k), gid, np.ones(n, bool), k or 37, 1, int(cmp), t)
                bits_equal(build(store, q[:1], metric, k, flt=(t, cmp)).collect_arrays()[0], ref, (metric, cmp, k))
    store.close()


def test_meta_store_distinct_by_with_a_filter_that_prunes_chunks(oracle):
    n, dim, cs = 1500, 16, 128
    rng = np.random.default_rng(8500)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    doc = rng.integers(0, 60, n).astype(np.int64)
    doc_null = rng.random(n) < 0.05
    shelf = (np.arange(n) // cs).astype(np.int32)
    names = np.array(["n%d" % v for v in rng.integers(0, 25, n)])
    meta = (MetaStore.from_columns([Column.from_numpy("doc", DataType.Int64, doc, doc_null), Column.from_numpy("shelf", DataType.Int32, shelf),
                                    Column.from_numpy("name", DataType.String, names)])
            .with_vectors(rows).with_chunk_size(cs).build())
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    half = (n // cs + 1) // 2
    gid_doc = np.where(doc_null, 1000 + np.arange(n), doc)  # every NULL row is a group of its own
    gid_name = np.unique(names, return_inverse=True)[1].reshape(-1)
    full = ranking(oracle, rows, q[None, :], Metric.Cosine, 1)
    cases = ((None, np.ones(n, bool)), (col("shelf").gte(half), shelf >= half), (col("shelf").gte(half) & col("doc").lt(40), (shelf >= half) & (doc < 40) & ~doc_null))
    for column, gid in (("doc", gid_doc), ("name", gid_name), ("doc", gid_doc)):  # (back to "doc": the ids are uploaded again)
        for expr, fmask in cases:
            for k in (3, 20, None):
                for flt in (None, (0.0, Cmp.Gt)):
                    p = meta.query(q, Metric.Cosine).distinct_by(column)
                    p = p.meta_filter(expr) if expr is not None else p
                    p = p.take(k) if k is not None else p
                    res = (p.vec_filter(*flt) if flt else p).collect()
                    ref, _ = expected(full, gid, fmask, k or n, 1, int(flt[1]) if flt else 0, 0.0)
                    where = (column, str(expr), k, flt)
                    assert res.indices == ref["index"].astype(np.int64).tolist(), where
                    assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), ref["score"].view(np.uint32)), where
    assert meta.last_query_stats().pruned_chunks > 0
    # the vector store's groups changed behind the MetaStore's back: distinct_by uploads its column's ids again
    ref, _ = expected(full, gid_doc, np.ones(n, bool), 20, 1)
    for disturb in (lambda: meta._store.set_groups(np.arange(n) % 3), lambda: meta._store.clear_groups()):
        disturb()
        res = meta.query(q, Metric.Cosine).distinct_by("doc").take(20).collect()
        assert res.indices == ref["index"].astype(np.int64).tolist()


# ---- 3. special scores ---------------------------------------------------------------------------------------------------------

def test_nan_never_represents_a_group_and_signed_zeros_order_canonically(oracle):
    n, dim = 200, 8
    rng = np.random.default_rng(8600)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    rows[10:14] = np.nan                  # NaN scores: dropped
    rows[20:24] = 0.0                     # zero rows: cosine +0.0 (inverse norm 0)
    rows[24:28] = np.float32(-1e30)       # the norm overflows, the inverse norm is 0: cosine (negative dot x 0) = -0.0
    rows[28:30] = np.float32(1e30)        # ... and +0.0
    rows[30] = np.inf
    q = np.abs(rng.uniform(0.1, 1, (1, dim))).astype(np.float32)
    gid = np.arange(n) // 4
    gid[10:12] = 2                        # NaN rows beside the finite rows 8, 9
    gid[12:14] = 49                       # ... and beside rows 196 .. 199; group 3 keeps rows 14, 15
    gid[26:28] = 5                        # -0.0 rows in the group of +0.0 rows
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    zeros = np.zeros(n, bool)
    zeros[20:30] = True
    ranks = Rankings(oracle, rows, q)
    for metric in ALL_METRICS:
        for mask in (None, zeros):
            keep = np.ones(n, bool) if mask is None else mask
            for k in (3, 10, None):
                ref, _ = expected(ranks.get(metric, 1, k), gid, keep, k or n, 1)
                got = build(store, q, metric, k, mask=mask).collect_arrays()[0]
                bits_equal(got, ref, (metric, mask is not None, k))
                assert not np.isnan(got["score"]).any()
                assert not np.isin(got["index"], [10, 11, 12, 13]).any()
    store.close()


# ---- 4. persistent grid ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [8, 40])
def test_persistent_grid_many_tiles_per_wave_and_heavy_contention(oracle, dim):
    """The sweep's grid is capped at 2 workgroups of 4 waves per CU: on the 256 CUs of an MI355X a wave gets a second tile from
    2048 tiles = 131 072 rows on.  200 000 rows: most waves take two tiles.  7 groups: every row of the store contends for seven
    slots; 50 000 groups: k = 600 and the default take go through the sort path with a large table."""
    n = 200_000
    rng = np.random.default_rng(8700 + dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (2, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    full1, full2 = ranking(oracle, rows, q[:1], Metric.Cosine, 1), ranking(oracle, rows, q, Metric.Cosine, 1)
    keep = np.ones(n, bool)
    for n_groups in (7, 50_000):
        gid = rng.integers(0, n_groups, n)
        gid[:n_groups] = np.arange(n_groups)  # (every label occurs: the labels are their own dense ids)
        store.set_groups(gid)
        for k in (10, 600):
            ref, _ = expected(full1, gid, keep, k, 1)
            bits_equal(build(store, q[:1], Metric.Cosine, k).collect_arrays()[0], ref, (n_groups, k))
        ref, ref_counts = expected(full2, gid, keep, 10, 2)
        got, counts = build(store, q, Metric.Cosine, 10, perq=True).collect_arrays()
        bits_equal(got, ref, (n_groups, "per query"))
        assert list(counts) == ref_counts
    store.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------

def test_errors_leave_the_store_usable(oracle):
    n, dim = 300, 8
    rng = np.random.default_rng(8800)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (2, dim)).astype(np.float32)
    gid = rng.integers(0, 20, n)
    store = VecStore(dim)
    store.add_vectors(rows)
    full = ranking(oracle, rows, q[:1], Metric.Cosine, 1)

    def still_works():
        ref, _ = expected(full, gid, np.ones(n, bool), 5, 1)
        bits_equal(build(store, q[:1], Metric.Cosine, 5).collect_arrays()[0], ref, "after an error")

    with pytest.raises(OttersError, match="no group ids are set"):
        build(store, q[:1], Metric.Cosine, 5).collect()
    store.set_groups(gid)
    still_works()
    with pytest.raises(OttersError, match="use PER_QUERY"):
        build(store, q, Metric.Cosine, 5).collect()
    still_works()
    with pytest.raises(OttersError, match="MFMA path does not serve grouped queries"):
        build(store, q[:1], Metric.Cosine, 5, path=Path.Mfma).collect()
    still_works()
    # an id >= n_groups, straight at the C ABI (the Python layer always sends dense ids)
    from otters_amd import _native as N
    bad = np.ascontiguousarray(gid.astype(np.uint32))
    bad[7] = 20
    rc = N.lib().ott_store_set_groups(store._handle(), N.ptr(bad), bad.size, 20)
    assert rc != 0 and "is not below n_groups" in N.lib().ott_last_error().decode()
    assert N.lib().ott_store_group_count(store._handle()) == 20
    still_works()
    rc = N.lib().ott_store_set_groups(store._handle(), N.ptr(bad), bad.size - 1, 21)
    assert rc != 0 and "group ids for a store of" in N.lib().ott_last_error().decode()
    still_works()
    store.delete_rows([3])
    with pytest.raises(OttersError, match="while group ids are set"):
        store.compact()
    store.restore_rows([3])
    still_works()
    # groups stale after an append (which reallocates here: the ids that are there are kept)
    store.add_vectors(rows[:5])
    with pytest.raises(OttersError, match="rows were appended since"):
        build(store, q[:1], Metric.Cosine, 5).collect()
    plain = store.query(q[:1], Metric.Cosine).take(3).collect_arrays()[0]
    assert plain.size == 3
    store.set_groups(np.concatenate([gid, gid[:5]]))
    all_rows = np.concatenate([rows, rows[:5]])
    gid = np.concatenate([gid, gid[:5]])
    ref, _ = expected(ranking(oracle, all_rows, q[:1], Metric.Cosine, 1), gid, np.ones(n + 5, bool), 5, 1)
    bits_equal(build(store, q[:1], Metric.Cosine, 5).collect_arrays()[0], ref, "set again after the append")
    # clear_groups lifts the restriction on compact
    store.clear_groups()
    assert store.group_count() == 0
    store.delete_rows([3])
    assert store.compact().size == n + 5
    store.close()


def test_ids_survive_a_reallocation_on_append(oracle):
    """set_groups on a store that then grows past its capacity and gets its ids for the new rows too: rows [0, n) keep theirs"""
    n, dim = 300, 8
    rng = np.random.default_rng(8900)
    rows = rng.uniform(-1, 1, (4 * n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (1, dim)).astype(np.float32)
    gid = rng.integers(0, 11, 4 * n)
    store = VecStore(dim)
    store.add_vectors(rows[:n])
    store.set_groups(gid[:n])
    store.add_vectors(rows[n:])  # reallocates
    from otters_amd import _native as N
    assert N.lib().ott_store_group_count(store._handle()) == 11
    store.set_groups(gid)
    ref, _ = expected(ranking(oracle, rows, q, Metric.Cosine, 1), gid, np.ones(4 * n, bool), 11, 1)
    bits_equal(build(store, q, Metric.Cosine, None).collect_arrays()[0], ref, "after growth")
    store.close()


# ---- 6. a store without groups is unchanged ---------------------------------------------------------------------------------------

def test_plain_queries_are_the_same_bits_without_groups_and_after_clear(oracle):
    n, dim = 700, 40
    rng = np.random.default_rng(9000)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)

    def plain():
        out = []
        for metric in ALL_METRICS:
            for k in (10, 100, None):
                got = store.query(q, metric).take(k).collect_arrays()[0] if k else store.query(q, metric).collect_arrays()[0]
                ref = ranking(oracle, rows, q, metric, take_of(metric, k))[: (k or n)]  # (merged: the default take is len())
                bits_equal(got, ref, (metric, k))
                out.append(got)
        return out

    before = plain()
    store.set_groups(rng.integers(0, 9, n))
    during = plain()
    build(store, q[:1], Metric.Cosine, 5).collect()
    store.clear_groups()
    after = plain()
    for a, b, c in zip(before, during, after):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    store.close()
