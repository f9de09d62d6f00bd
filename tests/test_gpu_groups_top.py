"""GPU: grouped search with up to m hits per group (ott_query_groups_top, VecQueryPlan.per_group, MetaQueryPlan.distinct_by(keep=);
DESIGN.md 3.1g).  Bar: bit for bit — index, query, score bits, order, per-query counts, group ids — no tolerances.

How the expectation is made: ONE oracle call per (store, metric, nq, take) ranks every (row, query) pair in the canonical order
(Manhattan: tests/manhattan_ref.py), never the library's own default take.  It is restricted to the kept rows and the pairs the
filter passes (L); per query a hit stays iff fewer than m earlier hits have its group; the groups rank by their first hit; the first
k groups are kept and laid out in that order, each group's hits contiguous and in their order in L.

Shapes: 3000 rows (47 tiles: several workgroups, so the slots are contended across CUs), dims 20 (a stage with a remainder) and 64,
rows quantised to small integers so that ties occur inside and between groups."""
import ctypes as C

import numpy as np
import pytest

from grouped_ref import Rankings, bits_equal, dense, expected, holds, ranking  # noqa: F401
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)
N_ROWS = 3000
ALL_M = (1, 2, 3, 8, 16)


def build(store, q, metric, m, k, take=None, perq=False, mask=None, flt=None, path=Path.Auto):
    p = store.query(q, metric).per_group(m)
    if mask is not None:
        p = p.with_row_mask(mask)
    if flt is not None:
        p = p.filter(*flt)
    if k is not None:
        p = p.take(k) if take is None else (p.take_max(k) if take else p.take_min(k))
    p = p.with_path(path)
    return p.per_query() if perq else p


def take_of(metric, k, take=None):
    """take(k) infers it from the metric, a plan without take() ranks by Max (src/vec.rs:214)"""
    return 1 if k is None else (TAKE[metric] if take is None else take)


def check(store, ranks, q_pool, gid, metric, nq, m, k, where, take=None, keep=None, flt=None, mask=None):
    plan = build(store, q_pool[:nq], metric, m, k, take=take, perq=nq > 1, mask=mask, flt=flt)
    keep = np.ones(gid.size, bool) if keep is None else keep
    cmp, thr = (int(flt[1]), flt[0]) if flt else (0, 0.0)
    ref, ref_counts, ref_groups = expected(ranks.get(metric, nq, take_of(metric, k, take)), gid, keep, plan.resolve().k, nq, m, cmp, thr)
    got, counts, groups = plan.collect_arrays()
    bits_equal(got, ref, where)
    assert list(counts) == ref_counts, where
    assert groups.dtype == np.uint32 and np.array_equal(groups, ref_groups), where
    return got, counts, ref


def layouts(rng, n):
    return {
        "one group": np.zeros(n, np.int64),  # all rows cascade into m slots: the worst contention
        "two groups": rng.integers(0, 2, n),
        "37 random groups": rng.integers(0, 37, n) * 1000 - 5,  # (labels need not be dense)
        "contiguous groups of 8": np.arange(n) // 8,  # the lanes of a wave share slots
        "contiguous groups of 2": np.arange(n) // 2,  # groups shorter than m from m = 3 on
        "every row its own": rng.permutation(n),      # 3000 groups > 512: a plan without take() goes through the sort path
    }


class Corpus:
    def __init__(self, oracle, dim, seed):
        rng = np.random.default_rng(seed)
        self.dim, self.rng = dim, rng
        self.rows = rng.integers(-2, 3, (N_ROWS, dim)).astype(np.float32)
        self.q_pool = rng.integers(-2, 3, (5, dim)).astype(np.float32)
        self.ranks = Rankings(oracle, self.rows, self.q_pool)
        self.store = VecStore(dim)
        self.store.add_vectors(self.rows)


@pytest.fixture(scope="module")
def corpora(oracle):
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = Corpus(oracle, dim, 9100 + dim)
        return made[dim]

    yield get
    for c in made.values():
        c.store.close()


# ---- 1. layouts, m, k, nq, metrics ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [20, 64])
def test_every_layout_m_k_batch_and_metric(corpora, dim):
    c = corpora(dim)
    for lname, labels in layouts(c.rng, N_ROWS).items():
        c.store.set_groups(labels)
        gid = dense(labels)
        for metric in ALL_METRICS:
            for nq in (1, 5):  # 5: two passes of the sweep
                for k in (1, 10, None):
                    for m in ALL_M:
                        where = (dim, lname, metric, nq, k, m)
                        got, counts, _ = check(c.store, c.ranks, c.q_pool, gid, metric, nq, m, k, where)
                        if m == 1:  # ... and the same as one_per_group() on every field
                            p = c.store.query(c.q_pool[:nq], metric).one_per_group()
                            p = p.take(k) if k is not None else p
                            one, one_counts = (p.per_query() if nq > 1 else p).collect_arrays()
                            assert got.tobytes() == one.tobytes() and list(counts) == list(one_counts), where


def test_both_takes_on_every_metric(corpora):
    c = corpora(20)
    labels = c.rng.integers(0, 37, N_ROWS)
    c.store.set_groups(labels)
    gid = dense(labels)
    for metric in ALL_METRICS:
        for take in (0, 1):
            for nq in (1, 5):
                for m in (2, 16):
                    check(c.store, c.ranks, c.q_pool, gid, metric, nq, m, 10, (metric, take, nq, m), take=take)


def test_ties_inside_groups_occur_in_these_corpora(corpora):
    """what the module's shapes are for: with quantised rows a group holds equal scores, so the lower row must win a slot"""
    c = corpora(20)
    full = c.ranks.get(Metric.DotProduct, 1, 1)
    gid = np.arange(N_ROWS) // 8
    g, s = gid[full["index"].astype(np.int64)], full["score"]
    assert any(np.unique(s[g == x]).size < (g == x).sum() for x in range(20))


# ---- 2. masks, deleted rows, filters ----------------------------------------------------------------------------------------------

def test_row_mask_deleted_rows_and_every_cmp(corpora):
    c = corpora(64)
    n = N_ROWS
    labels = c.rng.integers(0, 37, n)
    c.store.set_groups(labels)
    gid = dense(labels)
    metric, m = Metric.Cosine, 3
    full1 = c.ranks.get(metric, 1, 1)
    # a row mask that removes the best group's two best rows: its third best row leads it now
    g0 = gid[int(full1["index"][0])]
    best_two = full1["index"][gid[full1["index"].astype(np.int64)] == g0][:2].astype(np.int64)
    mask = np.ones(n, bool)
    mask[best_two] = False
    mask[c.rng.choice(n, 300, replace=False)] = False
    for k in (1, 10, None):
        for nq in (1, 5):
            got, _, _ = check(c.store, c.ranks, c.q_pool, gid, metric, nq, m, k, ("row mask", k, nq), keep=mask, mask=mask)
            assert not np.isin(got["index"].astype(np.int64), best_two).any()
    # deleted rows: the same rows, and a whole group
    whole = np.flatnonzero(gid == (g0 + 1) % 37)
    dead = np.unique(np.concatenate([best_two, whole, c.rng.choice(n, 100, replace=False)]))
    assert c.store.delete_rows(dead) == dead.size
    try:
        alive = np.ones(n, bool)
        alive[dead] = False
        for k in (10, None):
            for nq in (1, 5):
                got, _, _ = check(c.store, c.ranks, c.q_pool, gid, metric, nq, m, k, ("deleted", k, nq), keep=alive)
                assert (g0 + 1) % 37 not in gid[got["index"].astype(np.int64)]
        check(c.store, c.ranks, c.q_pool, gid, metric, 1, m, 10, "deleted & row mask", keep=alive & mask, mask=mask)
    finally:
        assert c.store.restore_rows(dead) == dead.size
    # every Cmp on both takes' metrics; a threshold near the top leaves some groups with fewer than m hits and some with none
    for metric in (Metric.Cosine, Metric.Euclidean):
        take = TAKE[metric]
        sc = c.ranks.get(metric, 1, take)["score"]
        near_top, median, exact = float(sc[60]), float(np.median(sc)), float(sc[5])
        for cmp in Cmp:
            thrs = (exact,) if cmp == Cmp.Eq else (median, near_top)
            for thr in thrs:
                for k in (5, None):
                    check(c.store, c.ranks, c.q_pool, gid, metric, 1, m, k, (metric, cmp, thr, k), flt=(thr, cmp))
        strict = Cmp.Gte if take else Cmp.Lte
        _, _, groups = expected(c.ranks.get(metric, 1, take), gid, np.ones(n, bool), 37, 1, m, int(strict), near_top)
        per_group = np.bincount(groups, minlength=37)
        assert (per_group == 0).any() and ((per_group > 0) & (per_group < m)).any() and (per_group == m).any(), per_group


# ---- 3. the table is zero when the next query finds it ------------------------------------------------------------------------------

def test_table_hygiene_across_grouped_maxsim_and_per_group_queries(corpora, oracle):
    dim = 20
    c = corpora(dim)
    store = VecStore(dim)  # one store, one context: every query below finds what the one before left
    store.add_vectors(c.rows)
    labels = c.rng.integers(0, 37, N_ROWS)
    store.set_groups(labels)
    gid = dense(labels)
    metric = Metric.DotProduct
    # per_group(8) with take(1): the deep slots of the 36 groups that do not win are populated
    check(store, c.ranks, c.q_pool, gid, metric, 1, 8, 1, "per_group(8).take(1)")
    # one_per_group: its table is the front of the same buffer
    full = c.ranks.get(metric, 1, 1)
    ref, _, _ = expected(full, gid, np.ones(N_ROWS, bool), 37, 1, 1)
    bits_equal(store.query(c.q_pool[:1], metric).one_per_group().collect_arrays()[0], ref, "one_per_group after per_group")
    # max_sim over 3 tokens: keys of group sums through the same buffer
    tokens = c.q_pool[:3]
    best = np.stack([np.array([(c.rows[gid == g] @ t).max() for g in range(37)], np.float32) for t in tokens])
    sums = best[0].copy()
    for t in range(1, 3):
        sums = (sums + best[t]).astype(np.float32)  # (small integers: the sums are exact in f32)
    order = np.lexsort((np.arange(37), -sums.astype(np.float64)))[:10]
    got, _ = store.query(tokens, metric).max_sim().take(10).collect_arrays()
    assert np.array_equal(got["index"].astype(np.int64), order) and np.array_equal(got["score"], sums[order])
    # another group count: the table's planes lie elsewhere
    labels2 = np.arange(N_ROWS) // 5
    store.set_groups(labels2)
    for nq in (1, 5):
        check(store, c.ranks, c.q_pool, dense(labels2), metric, nq, 2, 10, ("per_group(2) after set_groups", nq))
    check(store, c.ranks, c.q_pool, dense(labels2), metric, 1, 16, None, "per_group(16), sort path")
    bits_equal(store.query(c.q_pool[:1], metric).one_per_group().take(7).collect_arrays()[0],
               expected(full, dense(labels2), np.ones(N_ROWS, bool), 7, 1, 1)[0], "one_per_group at the end")
    store.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_store_usable(corpora):
    dim = 20
    c = corpora(dim)
    store = VecStore(dim)
    store.add_vectors(c.rows)
    labels = c.rng.integers(0, 37, N_ROWS)
    gid = dense(labels)
    L = N.lib()
    q = np.ascontiguousarray(c.q_pool[:2])
    out = np.empty(37 * 2 * 16, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(0)

    def call(m, nq=1, mode=0, path=0, k=5, cap=None, gids=None):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, nq, int(Metric.DotProduct), 1, mode, k, path
        rc = L.ott_query_groups_top(store._handle(), C.byref(d), m, N.ptr(out), out.size if cap is None else cap, C.byref(n_out), None, gids, None)
        return rc, L.ott_last_error().decode()

    def still_works():
        check(store, c.ranks, c.q_pool, gid, Metric.DotProduct, 1, 3, 5, "after a refusal")

    INVALID, UNSUPPORTED = -1, -4
    rc, msg = call(2)
    assert rc == INVALID and "no group ids are set" in msg
    with pytest.raises(OttersError, match="no group ids are set"):
        build(store, q[:1], Metric.DotProduct, 2, 5).collect()
    store.set_groups(labels)
    still_works()
    for m in (0, 17):
        rc, msg = call(m)
        assert rc == INVALID and "group_size is %d" % m in msg
    still_works()
    rc, msg = call(2, nq=2, mode=0)
    assert rc == UNSUPPORTED and "use PER_QUERY" in msg
    with pytest.raises(OttersError, match="use PER_QUERY"):
        build(store, q, Metric.DotProduct, 2, 5).collect()
    rc, msg = call(2, path=2)
    assert rc == UNSUPPORTED and "MFMA path does not serve grouped queries" in msg
    with pytest.raises(OttersError, match="MFMA path does not serve grouped queries"):
        build(store, q[:1], Metric.DotProduct, 2, 5, path=Path.Mfma).collect()
    rc, msg = call(3, nq=2, mode=1, cap=2 * 5 * 3 - 1)
    assert rc == INVALID and "output capacity is smaller than nq * min(k, n_groups) * group_size" in msg
    still_works()
    # a key table above 2 GiB: 2^25 groups x 16 slots x 8 B (the ids themselves stay below 37)
    dense32 = np.ascontiguousarray(gid.astype(np.uint32))
    assert L.ott_store_set_groups(store._handle(), N.ptr(dense32), dense32.size, 1 << 25) == 0
    rc, msg = call(16)
    assert rc == UNSUPPORTED and "above 2 GiB" in msg
    rc, msg = call(1, k=1)  # (group_size 1 has no such table)
    assert rc == 0 and n_out.value == 1
    store.set_groups(labels)
    still_works()
    # ids that no longer cover the rows
    store.add_vectors(c.rows[:3])
    with pytest.raises(OttersError, match="rows were appended since"):
        build(store, q[:1], Metric.DotProduct, 2, 5).collect()
    store.close()
    # a multi-GPU store
    multi = VecStore(dim, devices=[0, 0])
    multi.add_vectors(c.rows)
    multi.set_groups(labels)
    with pytest.raises(OttersError, match="a multi-GPU store is not served"):
        build(multi, q[:1], Metric.DotProduct, 2, 5).collect()
    ref, _, _ = expected(c.ranks.get(Metric.DotProduct, 1, 1), gid, np.ones(N_ROWS, bool), 5, 1, 1)
    bits_equal(multi.query(q[:1], Metric.DotProduct).one_per_group().take(5).collect_arrays()[0], ref, "the multi-GPU store after the refusal")
    multi.close()


def test_collect_and_collect_groups(corpora):
    c = corpora(20)
    labels = c.rng.integers(0, 37, N_ROWS) * 10 + 3
    c.store.set_groups(labels)
    gid = dense(labels)
    for nq in (1, 5):
        plan = build(c.store, c.q_pool[:nq], Metric.Cosine, 3, 4, perq=nq > 1)
        ref, ref_counts, ref_groups = expected(c.ranks.get(Metric.Cosine, nq, 1), gid, np.ones(N_ROWS, bool), 4, nq, 3)
        flat = plan.collect()
        flat = [flat] if nq == 1 else flat
        grouped = plan.collect_groups()
        grouped = [grouped] if nq == 1 else grouped
        o = 0
        for qi in range(nq):
            want = ref[o:o + ref_counts[qi]]
            assert [r.index for r in flat[qi]] == want["index"].tolist()
            assert [lab for lab, _ in grouped[qi]] == [int(x) for x in np.unique(labels)[ref_groups[o:o + ref_counts[qi]:3]]]
            assert [r.index for _, hits in grouped[qi] for r in hits] == want["index"].tolist()
            assert all(len(hits) == 3 for _, hits in grouped[qi])
            o += ref_counts[qi]


# ---- 5. MetaStore -------------------------------------------------------------------------------------------------------------------

def test_meta_store_distinct_by_keep(oracle):
    n, dim, cs = 1500, 16, 128
    rng = np.random.default_rng(9300)
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    doc = rng.integers(0, 60, n).astype(np.int64)
    doc_null = rng.random(n) < 0.05
    shelf = (np.arange(n) // cs).astype(np.int32)
    meta = (MetaStore.from_columns([Column.from_numpy("doc", DataType.Int64, doc, doc_null), Column.from_numpy("shelf", DataType.Int32, shelf)])
            .with_vectors(rows).with_chunk_size(cs).build())
    q = rng.integers(-2, 3, dim).astype(np.float32)
    half = (n // cs + 1) // 2
    gid = dense(np.where(doc_null, 1000 + np.arange(n), doc))  # every NULL row is a group of its own
    full = ranking(oracle, rows, q[None, :], Metric.Cosine, 1)
    cases = ((None, np.ones(n, bool)), (col("shelf").gte(half) & col("doc").lt(40), (shelf >= half) & (doc < 40) & ~doc_null))
    for expr, fmask in cases:
        for keep in (1, 3):
            for k in (3, 20, None):
                for flt in (None, (0.0, Cmp.Gt)):
                    p = meta.query(q, Metric.Cosine).distinct_by("doc", keep=keep)
                    p = p.meta_filter(expr) if expr is not None else p
                    p = p.take(k) if k is not None else p
                    res = (p.vec_filter(*flt) if flt else p).collect()
                    ref, _, _ = expected(full, gid, fmask, k or n, 1, keep, int(flt[1]) if flt else 0, 0.0)
                    where = (str(expr), keep, k, flt)
                    assert res.indices == ref["index"].astype(np.int64).tolist(), where
                    assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), ref["score"].view(np.uint32)), where
    assert meta.last_query_stats().pruned_chunks > 0
