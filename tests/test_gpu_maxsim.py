"""GPU: late-interaction (MaxSim) search (ott_query_maxsim, VecQueryPlan.max_sim).  Bar: the hits — dense group
id, score bits of the sum, order — are those of tests/maxsim_ref.py, which starts from ONE full canonical ranking of all (row, token)
pairs per (store, metric, nq, take).  Bit for bit, no tolerances.  The shapes are the smallest that reach each mechanism."""
import numpy as np
import pytest

import maxsim_ref as R
import test_gpu_groups as G
from otters_amd import Cmp, Metric, OttersError, Path, VecStore

pytestmark = pytest.mark.gpu

ALL_METRICS = G.ALL_METRICS


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])
    assert not got["query"].any(), where


def build(store, q, metric, k, path=Path.Auto, mask=None, flt=None):
    p = store.query(q, metric).max_sim()
    if mask is not None:
        p = p.with_row_mask(mask)
    if flt is not None:
        p = p.filter(*flt)
    if k is not None:
        p = p.take(k)
    return p.with_path(path)


def dense(labels):
    return np.unique(labels, return_inverse=True)[1].reshape(-1)


def check_store(oracle, store, rows, q_pool, metrics, nqs, ks, paths, rng, lay):
    n = rows.shape[0]
    keep = np.ones(n, bool)
    ranks = G.Rankings(oracle, rows, q_pool)
    for lname, labels in lay.items():
        store.set_groups(labels)
        gid = dense(labels)
        ng = int(gid.max()) + 1
        assert store.group_count() == ng
        for metric in metrics:
            for nq in nqs:
                for k in ks:
                    take = G.take_of(metric, k)
                    ref = R.expected(ranks.get(metric, nq, k), gid, keep, k if k is not None else ng, nq, take, n_groups=ng)
                    for path in paths:
                        got, counts = build(store, q_pool[:nq], metric, k, path).collect_arrays()
                        bits_equal(got, ref, (lname, metric, nq, k, path))
                        assert counts == [ref.size]


# ---- 1. small store ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 40])
def test_small_store_every_metric_layout_token_count_k_and_path(oracle, dim):
    """300 rows: four full tiles and a partial one; dims cover tail only (1, 3, 7), chains only (8, 40) and both (9); nq covers a
    single token, a partial pass, a full pass, full + partial and three passes; k the one-entry lists' size (64 | 65) and no take"""
    rng = np.random.default_rng(9100 + dim)
    rows = rng.uniform(-1, 1, (300, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (9, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    check_store(oracle, store, rows, q_pool, ALL_METRICS, (1, 3, 4, 5, 9), (1, 10, 64, 65, None), (Path.Auto, Path.Exact), rng, G.layouts(rng, 300))
    store.close()


def test_one_token_is_one_per_group_with_rows_mapped_to_groups(oracle):
    rng = np.random.default_rng(9200)
    rows = rng.uniform(-1, 1, (300, 9)).astype(np.float32)
    q = rng.uniform(-1, 1, (1, 9)).astype(np.float32)
    store = VecStore(9)
    store.add_vectors(rows)
    for lname, labels in G.layouts(rng, 300).items():
        store.set_groups(labels)
        gid = dense(labels)
        for metric in ALL_METRICS:
            for k in (1, 10, None):
                grouped = G.build(store, q, metric, k).collect_arrays()[0]
                got = build(store, q, metric, k).collect_arrays()[0]
                where = (lname, metric, k)
                assert got["index"].astype(np.int64).tolist() == gid[grouped["index"].astype(np.int64)].tolist(), where
                assert np.array_equal(got["score"].view(np.uint32), grouped["score"].view(np.uint32)), where
    store.close()


def test_quantised_rows_equal_sums_and_signed_zeros(oracle):
    """integers in -2..2: equal bests inside a group and equal sums between groups (the lower group id wins); rows of zeros and rows
    whose norm overflows make +0.0 and -0.0 cosines, so bests and sums of either sign occur and are compared by their bits"""
    rng = np.random.default_rng(9300)
    rows = rng.integers(-2, 3, (300, 9)).astype(np.float32)
    rows[40:48] = 0.0                      # cosine +0.0 (inverse norm 0)
    rows[48:56] = np.float32(-1e30)        # the norm overflows, the inverse norm is 0: cosine -0.0 against positive tokens
    q_pool = rng.integers(-2, 3, (9, 9)).astype(np.float32)
    q_pool[:2] = np.abs(q_pool[:2]) + 1    # positive tokens: the two first tokens alone make -0.0 sums
    store = VecStore(9)
    store.add_vectors(rows)
    lay = {"37 random groups": rng.integers(0, 37, 300), "contiguous by row": np.arange(300) // 8, "pairs": np.arange(300) // 2}
    check_store(oracle, store, rows, q_pool, ALL_METRICS, (1, 2, 3, 9), (1, 10, 65, None), (Path.Auto,), rng, lay)
    # what the case is there for: a group of -0.0 bests only sums to -0.0, and equal sums occur
    store.set_groups(np.arange(300) // 8)
    got = build(store, q_pool[:2], Metric.Cosine, None).collect_arrays()[0]
    assert got[got["index"] == 6]["score"].view(np.uint32).tolist() == [0x80000000]
    assert got[got["index"] == 5]["score"].view(np.uint32).tolist() == [0]
    got = build(store, q_pool[:3], Metric.DotProduct, None).collect_arrays()[0]
    assert np.unique(got["score"]).size < got.size
    store.close()


def test_more_groups_than_the_register_lists_hold(oracle):
    """3000 rows, 1500 and 3000 groups: k = 512 fills the eight-entry lists from many select workgroups, 513 / 600 / no take sort"""
    rng = np.random.default_rng(9400)
    rows = rng.uniform(-1, 1, (3000, 24)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (5, 24)).astype(np.float32)
    store = VecStore(24)
    store.add_vectors(rows)
    store.set_base_offset(1000)  # a hit's index is the group, not a row: the offset must not show
    lay = {"pairs": np.arange(3000) // 2, "own": rng.permutation(3000)}
    check_store(oracle, store, rows, q_pool, (Metric.Cosine, Metric.Euclidean), (1, 5), (512, 513, 600, None), (Path.Auto,), rng, lay)
    store.close()


# ---- 2. masks ---------------------------------------------------------------------------------------------------------------------

def test_row_mask_deleted_rows_chunk_mask_and_all_three(oracle):
    n, dim, cs = 300, 40, 64
    rng = np.random.default_rng(9500)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    gid = np.arange(n) // 8  # 38 groups
    ng = 38
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_chunk_size(cs)
    store.set_groups(gid)
    full = {m: R.ranking(oracle, rows, q, m, G.TAKE[m]) for m in (Metric.Cosine, Metric.Euclidean)}
    caller = rng.random(n) < 0.5
    caller[16:40] = False      # groups 2, 3, 4 lose every row
    caller[40:47] = False      # group 5 keeps one row
    caller[47] = True
    dead = np.unique(np.concatenate([np.arange(80, 88), rng.choice(n, 30)]))  # group 10 deleted entirely, others thinned
    alive = np.ones(n, bool)
    alive[dead] = False
    chunks = np.array([True, False, True, True, False])  # rows 64 .. 127 and 256 .. 299 are never read
    in_chunk = np.repeat(chunks, cs)[:n]

    def run(metric, k, mask=None, chunk_mask=None):
        rq = build(store, q, metric, k, mask=mask).resolve()
        return store._run(rq, chunk_mask=chunk_mask)[0]

    for metric in (Metric.Cosine, Metric.Euclidean):
        take = G.TAKE[metric]
        for k in (1, 10, ng):
            ref = R.expected(full[metric], gid, caller, k, 5, take, n_groups=ng)
            got = run(metric, k, mask=caller)
            bits_equal(got, ref, ("row mask", metric, k))
            if k == ng:
                assert not np.isin(got["index"], [2, 3, 4]).any() and 5 in got["index"]
            bits_equal(run(metric, k, chunk_mask=chunks), R.expected(full[metric], gid, in_chunk, k, 5, take, n_groups=ng), ("chunk mask", metric, k))
        assert store.delete_rows(dead) == dead.size
        for k in (1, 10, ng):
            got = run(metric, k)
            bits_equal(got, R.expected(full[metric], gid, alive, k, 5, take, n_groups=ng), ("deleted", metric, k))
            assert 10 not in got["index"]
            keep = alive & caller & in_chunk
            bits_equal(run(metric, k, mask=caller, chunk_mask=chunks), R.expected(full[metric], gid, keep, k, 5, take, n_groups=ng), ("all three", metric, k))
        assert store.restore_rows(dead) == dead.size
        bits_equal(run(metric, 10), R.expected(full[metric], gid, np.ones(n, bool), 10, 5, take, n_groups=ng), ("restored", metric))
    store.close()


# ---- 3. special scores ---------------------------------------------------------------------------------------------------------

def test_nan_rows_nan_groups_and_opposite_infinities(oracle):
    n, dim = 200, 8
    rng = np.random.default_rng(9600)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    rows[10:12] = np.nan                   # NaN rows in group 2, beside rows 8, 9
    rows[20:24] = np.nan                   # group 5: only NaN rows
    rows[40:44] = 0.0
    rows[40, 0], rows[41, 0] = np.inf, -np.inf   # group 10: dot = +inf / -inf against a token with a positive / negative first element
    q = rng.uniform(0.1, 1, (3, dim)).astype(np.float32)
    q[1, 0] = -q[1, 0]                     # token 0 prefers row 40 (+inf), token 1 row 41 (+inf as well); under Min both are -inf
    q[2, 0] = 0.0                          # 0 x inf = NaN for both rows: token 2 takes rows 42, 43
    gid = np.arange(n) // 4
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    ranks = G.Rankings(oracle, rows, q)
    for metric in ALL_METRICS:
        for nq in (1, 2, 3):
            for k in (3, None):
                take = G.take_of(metric, k)
                ref = R.expected(ranks.get(metric, nq, k), gid, np.ones(n, bool), k or 50, nq, take, n_groups=50)
                got = build(store, q[:nq], metric, k).collect_arrays()[0]
                bits_equal(got, ref, (metric, nq, k))
                assert not np.isnan(got["score"]).any() and 5 not in got["index"]
                if k is None:
                    assert 2 in got["index"]
    # +inf for token 0 and -inf for token 1 in one group: rows 40 and 41 alone, dot product, Max
    pm = np.zeros(n, bool)
    pm[40:42] = True
    pm[100:104] = True
    q2 = q[:2].copy()
    q2[1, 0] = np.float32(0.0)  # row 40 and 41 score NaN for token 1 ... every row of group 10 does: the group is dropped
    got = build(store, q2, Metric.DotProduct, None, mask=pm).collect_arrays()[0]
    assert got["index"].tolist() == [25]
    rows2 = rows.copy()
    rows2[41] = 0.0
    rows2[41, 1] = -np.inf      # token 0: best +inf (row 40); token 1 (only its second element set): row 40 gives NaN, row 41 -inf
    store2 = VecStore(dim)
    store2.add_vectors(rows2)
    store2.set_groups(gid)
    q3 = np.zeros((2, dim), np.float32)
    q3[0, 0], q3[1, 1] = 1.0, 1.0
    ref = R.expected(R.ranking(oracle, rows2, q3, Metric.DotProduct, 1), gid, pm, 50, 2, 1, n_groups=50)
    got = build(store2, q3, Metric.DotProduct, None, mask=pm).collect_arrays()[0]
    bits_equal(got, ref, "inf - inf")
    assert got["index"].tolist() == [25]  # group 10's bests are +inf and -inf: a NaN sum
    store.close()
    store2.close()


# ---- 4. the filter on the sum ------------------------------------------------------------------------------------------------------

def test_filter_applies_to_the_sum_every_cmp(oracle):
    n, dim = 300, 9
    rng = np.random.default_rng(9700)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    gid = rng.integers(0, 37, n)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    keep = np.ones(n, bool)
    for metric in (Metric.Cosine, Metric.Euclidean):
        for k in (5, None):
            take = G.take_of(metric, k)
            full = R.ranking(oracle, rows, q, metric, take)
            sums = R.expected(full, gid, keep, 37, 5, take, n_groups=37)["score"]
            assert sums.size == 37
            for thr in (float(sums[5]), float(sums[20])):  # sums that occur: Eq hits one, Gte / Lte sit on the boundary
                for cmp in Cmp:
                    ref = R.expected(full, gid, keep, k or 37, 5, take, int(cmp), thr, n_groups=37)
                    got = build(store, q, metric, k, flt=(thr, cmp)).collect_arrays()[0]
                    bits_equal(got, ref, (metric, cmp, k, thr))
                    assert R.holds(got["score"], int(cmp), thr).all()
                    if cmp == Cmp.Eq:
                        assert got.size == 1
    store.close()


# ---- 5. persistent grid, contention, the fold -------------------------------------------------------------------------------------

def test_larger_store_second_tiles_one_group_and_contiguous_groups(oracle):
    """140 000 rows: above 131 072 waves take a second tile.  One group: every row of the store contends for nq slots (the worst case
    of same-slot atomics).  10 000 contiguous groups of 14 rows: runs of equal ids inside every wave, crossing tile boundaries."""
    n, dim = 140_000, 16
    rng = np.random.default_rng(9800)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    keep = np.ones(n, bool)
    full = {m: R.ranking(oracle, rows, q, m, G.TAKE[m]) for m in (Metric.Cosine, Metric.Euclidean)}
    for gid in (np.zeros(n, np.int64), np.arange(n) // 14):
        store.set_groups(gid)
        ng = int(gid.max()) + 1
        for metric in (Metric.Cosine, Metric.Euclidean):
            for k in (10, 600):
                ref = R.expected(full[metric], gid, keep, k, 5, G.TAKE[metric], n_groups=ng)
                bits_equal(build(store, q, metric, k).collect_arrays()[0], ref, (ng, metric, k))
    store.close()


# ---- 6. the tables are left clean ----------------------------------------------------------------------------------------------------

def test_back_to_back_queries_grouped_in_between_and_groups_replaced(oracle):
    n, dim = 300, 8
    rng = np.random.default_rng(9900)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (9, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    keep = np.ones(n, bool)
    ranks = G.Rankings(oracle, rows, q)

    def maxsim(gid, ng, nq, k):
        ref = R.expected(ranks.get(Metric.Cosine, nq, k), gid, keep, k or ng, nq, 1, n_groups=ng)
        bits_equal(build(store, q[:nq], Metric.Cosine, k).collect_arrays()[0], ref, (ng, nq, k))

    gid = rng.integers(0, 37, n)
    gid[:37] = np.arange(37)
    store.set_groups(gid)
    for nq, k in ((9, 5), (2, None), (5, 37), (1, 3), (9, None)):
        maxsim(gid, 37, nq, k)
    ref, ref_counts = G.expected(ranks.get(Metric.Cosine, 3, 10), gid, keep, 10, 3)
    got, counts = G.build(store, q[:3], Metric.Cosine, 10, perq=True).collect_arrays()
    G.bits_equal(got, ref, "grouped in between")
    assert list(counts) == ref_counts
    maxsim(gid, 37, 4, 10)
    maxsim(gid, 37, 9, None)
    gid2 = np.arange(n) // 2  # replaced: more groups than before (both tables grow), then fewer again
    store.set_groups(gid2)
    maxsim(gid2, 150, 9, None)
    maxsim(gid2, 150, 3, 10)
    store.set_groups(gid)
    maxsim(gid, 37, 9, None)
    store.close()


# ---- 7. refusals, labels, stats ----------------------------------------------------------------------------------------------------

def test_refusals_leave_the_store_usable(oracle):
    n, dim = 300, 8
    rng = np.random.default_rng(10000)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    gid = rng.integers(0, 20, n)
    gid[:20] = np.arange(20)
    store = VecStore(dim)
    store.add_vectors(rows)
    full = R.ranking(oracle, rows, q, Metric.Cosine, 1)

    def still_works():
        bits_equal(build(store, q, Metric.Cosine, 5).collect_arrays()[0], R.expected(full, gid, np.ones(n, bool), 5, 3, 1, n_groups=20), "after a refusal")

    with pytest.raises(OttersError, match="ott_query_maxsim: no group ids are set"):
        build(store, q, Metric.Cosine, 5).collect()
    store.set_groups(gid)
    still_works()
    with pytest.raises(OttersError, match="max_sim cannot be combined with per_query"):
        build(store, q, Metric.Cosine, 5).per_query().collect()
    with pytest.raises(OttersError, match="MFMA path does not serve late-interaction") as e:
        build(store, q, Metric.Cosine, 5, path=Path.Mfma).collect()
    assert e.value.status == -4
    still_works()
    # PER_QUERY and a short output buffer straight at the C ABI (the Python layer never sends either)
    import ctypes as C
    from otters_amd import _native as N
    d = N.QueryDesc()
    qq = np.ascontiguousarray(q)
    d.queries, d.nq, d.metric, d.take, d.k, d.mode = qq.ctypes.data, 3, int(Metric.Cosine), 1, 5, 1
    out = np.zeros(8, N.HIT_DTYPE)
    n_out = C.c_uint64(0)
    assert N.lib().ott_query_maxsim(store._handle(), C.byref(d), N.ptr(out), 8, C.byref(n_out), None) == -4
    assert b"tokens of ONE query" in N.lib().ott_last_error()
    d.mode = 0
    assert N.lib().ott_query_maxsim(store._handle(), C.byref(d), N.ptr(out), 4, C.byref(n_out), None) == -1
    assert b"output capacity is smaller than min(k, n_groups)" in N.lib().ott_last_error()
    still_works()
    # the table limit: a group count that is large in arithmetic only (3 tokens x 2^30 groups x 4 B); nothing is allocated
    dense_ids = np.ascontiguousarray(gid.astype(np.uint32))
    store._set_dense_groups(dense_ids, 2 ** 30)
    with pytest.raises(OttersError, match="above 2 GiB") as e:
        build(store, q, Metric.Cosine, 5).collect()
    assert e.value.status == -4
    store.set_groups(gid)
    still_works()
    # rows appended since set_groups
    store.add_vectors(rows[:5])
    with pytest.raises(OttersError, match="rows were appended since"):
        build(store, q, Metric.Cosine, 5).collect()
    store.close()
    multi = VecStore(dim, devices=[0, 0])
    multi.add_vectors(rows)
    multi.set_groups(gid)
    with pytest.raises(OttersError, match="multi-GPU store is not served") as e:
        build(multi, q, Metric.Cosine, 5).collect()
    assert e.value.status == -4
    multi.close()


def test_collect_reports_the_callers_labels_and_last_stats(oracle):
    n, dim = 300, 8
    rng = np.random.default_rng(10100)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (9, dim)).astype(np.float32)
    labels = rng.integers(0, 37, n) * 1000 - 5000  # neither dense nor all positive
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(labels)
    uniq = np.unique(labels)
    assert np.array_equal(store.group_labels(), uniq)
    for nq, passes in ((1, 1), (3, 1), (4, 1), (5, 2), (9, 3)):
        plan = build(store, q[:nq], Metric.Cosine, 10, path=Path.Exact)
        hits = plan.collect_arrays()[0]
        st = store.last_stats
        assert st["path_used"] == int(Path.Exact) and st["passes"] == passes and st["vectors_compared"] == n * nq, (nq, st)
        assert st["bytes_scanned"] == passes * n * (dim * 4 + 4 + 4)
        res = plan.collect()
        assert [r.index for r in res] == uniq[hits["index"].astype(np.int64)].tolist()
        assert np.array_equal(np.array([r.score for r in res], np.float32).view(np.uint32), hits["score"].view(np.uint32))
    assert build(store, q[:5], Metric.Cosine, 10, path=Path.Auto).collect_arrays()[0].size == 10
    assert store.last_stats["path_used"] == int(Path.Exact)
    store.close()
