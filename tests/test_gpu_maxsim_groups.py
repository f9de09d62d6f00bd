"""GPU: MaxSim re-ranking over a listed set of groups (ott_query_maxsim_groups, VecQueryPlan.with_groups).  Bar: the
hits — dense group id, score bits of the sum, order — are those of tests/maxsim_ref.py over the full canonical ranking with `keep`
ANDed with "the row's group is listed".  Both routes (option group_gather = 1: the gather kernel through the group-to-rows index;
0: the list as a row mask in front of ott_query_maxsim's sweep) are held to that reference and therefore to each other.  Bit for
bit, no tolerances.  The shapes are the smallest that reach each mechanism; where a test crosses many values it rotates them so that
every value and every pair of values occurs, not every tuple."""
import ctypes as C

import numpy as np
import pytest

import grouped_ref as GR
import maxsim_ref as R
import test_gpu_groups as G
import test_gpu_groups_top as GT
from otters_amd import Cmp, Metric, OttersError, VecStore
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

ALL_METRICS = G.ALL_METRICS
GATHER, MASK = 1, 0
ROUTES = (GATHER, MASK)


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])
    assert not got["query"].any(), where


def dense(labels):
    return np.unique(labels, return_inverse=True)[1].reshape(-1)


def run(store, q, metric, k, listed_labels, route, mask=None, flt=None, chunk_mask=None):
    """(hits, stats) of a listed plan on one route"""
    store.set_option("group_gather", route)
    p = store.query(q, metric).max_sim().with_groups(listed_labels)
    if mask is not None:
        p = p.with_row_mask(mask)
    if flt is not None:
        p = p.filter(*flt)
    if k is not None:
        p = p.take(k)
    hits, _, st = store._run(p.resolve(), chunk_mask=chunk_mask)
    return hits, st


def reference(full, gid, ng, keep, listed, k, nq, take, cmp=0, thr=0.0):
    listed = np.asarray(listed, np.int64)
    in_list = np.zeros(ng, bool)
    in_list[listed] = True
    return R.expected(full, gid, np.asarray(keep, bool) & in_list[gid], k if k is not None else int(in_list.sum()), nq, take, cmp, thr, n_groups=ng)


def took(st, route, gid, listed, nq, n):
    """the route shows in the stats: the gather compares the listed groups' rows, the sweep the store's"""
    listed_rows = int(np.isin(gid, np.asarray(listed, np.int64)).sum())
    if route == GATHER:
        assert st["vectors_compared"] == listed_rows * nq, (st, listed_rows)
    else:
        assert st["vectors_compared"] == n * nq, st


def lists_of(rng, ng):
    half = rng.choice(ng, max(ng // 2, 1), replace=False)
    some = rng.integers(0, ng, min(ng, 9))
    return {"empty": np.zeros(0, np.int64), "one group": np.array([ng - 1]), "every group": rng.permutation(ng), "unsorted with duplicates": np.concatenate([some, some[::-1], some[:2]]),
            "half": half}


# ---- 1. small store ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 40])
def test_small_store_every_metric_layout_token_count_list_k_and_route(oracle, dim):
    """300 rows; dims cover tail only (1, 3, 7), chains only (8, 40) and both (9); nq a single token, a partial pass, a full 8-wide
    pass, a 16-wide one and 33 = two passes at 32 per pass; every (nq, list) pair with k rotating through 1, 10, 64, 65 and no take"""
    rng = np.random.default_rng(11100 + dim)
    n = 300
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (33, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    ranks = G.Rankings(oracle, rows, q_pool)
    keep = np.ones(n, bool)
    nqs, ks = (1, 3, 8, 9, 33), (1, 10, 64, 65, None)
    turn = 0
    for lname, labels in G.layouts(rng, n).items():
        store.set_groups(labels)
        gid, uniq = dense(labels), np.unique(labels)
        ng = uniq.size
        lists = lists_of(rng, ng)
        for metric in ALL_METRICS:
            turn += 1
            for i, nq in enumerate(nqs):
                for j, (listname, listed) in enumerate(lists.items()):
                    k = ks[(i + j + turn) % len(ks)]
                    take = G.take_of(metric, k)
                    ref = reference(ranks.get(metric, nq, k), gid, ng, keep, listed, k, nq, take)
                    for route in ROUTES:
                        got, st = run(store, q_pool[:nq], metric, k, uniq[listed], route)
                        bits_equal(got, ref, (lname, metric, nq, listname, k, route))
                        if listed.size:
                            took(st, route, gid, listed, nq, n)
                            if route == GATHER:
                                assert st["passes"] == (2 if nq == 33 else 1)
    store.close()


# ---- 2. token-pass width ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim, nq, per_pass", [(520, 17, 16), (1030, 9, 8), (2056, 3, 0)])
def test_token_pass_width_follows_the_dim(oracle, dim, nq, per_pass):
    """64 rows: padded dims of 520 and 1032 floats take 16 and 8 tokens per pass (two passes each); 2056 is past the kernel's LDS and
    must still answer with the option at 1, by the mask route and without an index"""
    rng = np.random.default_rng(11200 + dim)
    n = 64
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    gid = rng.integers(0, 9, n)
    gid[:9] = np.arange(9)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    keep = np.ones(n, bool)
    for metric in ALL_METRICS:
        for k in (4, None):
            take = G.take_of(metric, k)
            full = R.ranking(oracle, rows, q, metric, take)
            for listed in (np.array([7, 1, 3, 8, 1]), np.arange(9)):
                ref = reference(full, gid, 9, keep, listed, k, nq, take)
                for route in ROUTES:
                    got, st = run(store, q, metric, k, listed, route)
                    bits_equal(got, ref, (dim, metric, k, route))
                    if per_pass and route == GATHER:
                        took(st, GATHER, gid, listed, nq, n)
                        assert st["passes"] == -(-nq // per_pass) == 2
                    else:
                        took(st, MASK, gid, listed, nq, n)
    assert st["group_index_builds"] == (1 if per_pass else 0)
    store.close()


# ---- 3. group sizes -----------------------------------------------------------------------------------------------------------------

def test_one_large_group_single_rows_and_pairs(oracle):
    """one group of 300 rows: nine full steps of the workgroup and a partial one; groups of one row: a step with one live row group;
    pairs.  Beside a one-pass query (3 tokens) a two-pass one (33), so both the in-kernel sum and the reduce kernel see each shape"""
    rng = np.random.default_rng(11300)
    n, dim = 300, 9
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (33, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    ranks = G.Rankings(oracle, rows, q_pool)
    keep = np.ones(n, bool)
    for gid in (np.zeros(n, np.int64), np.arange(n), np.arange(n) // 2):
        store.set_groups(gid)
        ng = int(gid.max()) + 1
        for listed in (np.arange(ng), np.arange(0, ng, 3)[::-1]):
            for metric in (Metric.Cosine, Metric.Manhattan):
                for nq, k in ((3, 10), (33, None), (9, 1)):
                    take = G.take_of(metric, k)
                    ref = reference(ranks.get(metric, nq, k), gid, ng, keep, listed, k, nq, take)
                    for route in ROUTES:
                        got, st = run(store, q_pool[:nq], metric, k, listed, route)
                        bits_equal(got, ref, (ng, metric, nq, k, route))
                        took(st, route, gid, listed, nq, n)
    store.close()


# ---- 4. masks ---------------------------------------------------------------------------------------------------------------------

def test_row_mask_deleted_rows_chunk_mask_and_all_three(oracle):
    n, dim, cs = 300, 40, 64
    rng = np.random.default_rng(11400)
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
    chunks = np.array([True, False, True, True, False])  # rows 64 .. 127 and 256 .. 299 are never scored
    in_chunk = np.repeat(chunks, cs)[:n]
    listed = np.array([2, 3, 5, 10, 12, 20, 37, 33, 9, 8, 1, 15, 5])  # masked-out, deleted, chunk-masked and untouched groups

    for metric in (Metric.Cosine, Metric.Euclidean):
        take = G.TAKE[metric]
        for route in ROUTES:
            for k in (1, 10, ng):
                got, _ = run(store, q, metric, k, listed, route, mask=caller)
                bits_equal(got, reference(full[metric], gid, ng, caller, listed, k, 5, take), ("row mask", metric, k, route))
                if k == ng:
                    assert not np.isin(got["index"], [2, 3]).any() and 5 in got["index"]  # every row masked: dropped; one row left: kept
                got, _ = run(store, q, metric, k, listed, route, chunk_mask=chunks)
                bits_equal(got, reference(full[metric], gid, ng, in_chunk, listed, k, 5, take), ("chunk mask", metric, k, route))
            assert store.delete_rows(dead) == dead.size
            for k in (1, 10, ng):
                got, _ = run(store, q, metric, k, listed, route)
                bits_equal(got, reference(full[metric], gid, ng, alive, listed, k, 5, take), ("deleted", metric, k, route))
                assert 10 not in got["index"]
                got, _ = run(store, q, metric, k, listed, route, mask=caller, chunk_mask=chunks)
                bits_equal(got, reference(full[metric], gid, ng, alive & caller & in_chunk, listed, k, 5, take), ("all three", metric, k, route))
            assert store.restore_rows(dead) == dead.size
            got, _ = run(store, q, metric, 10, listed, route)
            bits_equal(got, reference(full[metric], gid, ng, np.ones(n, bool), listed, 10, 5, take), ("restored", metric, route))
    store.close()


# ---- 5. ties and zeros ------------------------------------------------------------------------------------------------------------

def test_quantised_rows_equal_sums_signed_zeros_nan_sums_and_every_cmp(oracle):
    """test_gpu_maxsim.py::test_quantised_rows_equal_sums_and_signed_zeros' construction: integers in -2..2 make equal bests inside a
    group and equal sums between groups (the lower group id wins); rows of zeros and rows whose norm overflows make +0.0 and -0.0
    cosines, so bests and sums of either sign occur and are compared by their bits"""
    rng = np.random.default_rng(9300)
    n = 300
    rows = rng.integers(-2, 3, (n, 9)).astype(np.float32)
    rows[40:48] = 0.0                      # cosine +0.0 (inverse norm 0)
    rows[48:56] = np.float32(-1e30)        # the norm overflows, the inverse norm is 0: cosine -0.0 against positive tokens
    q_pool = rng.integers(-2, 3, (9, 9)).astype(np.float32)
    q_pool[:2] = np.abs(q_pool[:2]) + 1    # positive tokens: the two first tokens alone make -0.0 sums
    store = VecStore(9)
    store.add_vectors(rows)
    ranks = G.Rankings(oracle, rows, q_pool)
    keep = np.ones(n, bool)
    for gid in (rng.integers(0, 37, n), np.arange(n) // 8, np.arange(n) // 2):
        gid = dense(gid)
        store.set_groups(gid)
        ng = int(gid.max()) + 1
        listed = rng.permutation(ng)[: max(ng * 3 // 4, 8)]
        listed = np.union1d(listed, [5, 6])  # (the groups of the zero rows in the contiguous layout)
        for metric in ALL_METRICS:
            for nq, k in ((1, 10), (2, None), (3, 65), (9, 1)):
                take = G.take_of(metric, k)
                ref = reference(ranks.get(metric, nq, k), gid, ng, keep, listed, k, nq, take)
                for route in ROUTES:
                    bits_equal(run(store, q_pool[:nq], metric, k, listed, route)[0], ref, (ng, metric, nq, k, route))
    # what the case is there for: a group of -0.0 bests only sums to -0.0, +0.0 stays +0.0, and equal sums occur
    gid = np.arange(n) // 8
    store.set_groups(gid)
    for route in ROUTES:
        got, _ = run(store, q_pool[:2], Metric.Cosine, None, [6, 5, 30], route)
        assert got[got["index"] == 6]["score"].view(np.uint32).tolist() == [0x80000000]
        assert got[got["index"] == 5]["score"].view(np.uint32).tolist() == [0]
        got, _ = run(store, q_pool[:3], Metric.DotProduct, None, np.arange(38), route)
        assert np.unique(got["score"]).size < got.size
        # every comparator, on the SUM, with thresholds that occur
        full = ranks.get(Metric.DotProduct, 3, None)
        sums = reference(full, gid, 38, keep, np.arange(0, 38, 2), None, 3, 1)["score"]
        for thr in (float(sums[3]), float(sums[10])):
            for cmp in Cmp:
                ref = reference(full, gid, 38, keep, np.arange(0, 38, 2), None, 3, 1, int(cmp), thr)
                got, _ = run(store, q_pool[:3], Metric.DotProduct, None, np.arange(0, 38, 2), route, flt=(thr, cmp))
                bits_equal(got, ref, (cmp, thr, route))
                assert R.holds(got["score"], int(cmp), thr).all()
    store.close()


def test_opposite_infinities_make_a_nan_sum_and_the_group_is_dropped(oracle):
    n, dim = 200, 8
    rng = np.random.default_rng(11500)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    rows[40:44] = 0.0
    rows[40, 0] = np.inf       # token 0 (only its first element set): best +inf
    rows[41, 1] = -np.inf      # token 1 (only its second element set): row 40 gives NaN, row 41 -inf
    rows[20:24] = np.nan       # group 5: only NaN rows
    gid = np.arange(n) // 4
    pm = np.zeros(n, bool)
    pm[40:42] = True
    pm[100:104] = True
    pm[20:24] = True
    q = np.zeros((2, dim), np.float32)
    q[0, 0], q[1, 1] = 1.0, 1.0
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    full = R.ranking(oracle, rows, q, Metric.DotProduct, 1)
    listed = [25, 10, 5, 30]
    ref = reference(full, gid, 50, pm, listed, None, 2, 1)
    for route in ROUTES:
        got, _ = run(store, q, Metric.DotProduct, None, listed, route, mask=pm)
        bits_equal(got, ref, route)
        assert got["index"].tolist() == [25]  # group 10: +inf + -inf; group 5: no score at all; group 30: no row survives the mask
    store.close()


# ---- 6. more listed groups than the register lists hold -------------------------------------------------------------------------------

def test_sort_path_1500_of_3000_groups(oracle):
    rng = np.random.default_rng(11600)
    n = 3000
    rows = rng.uniform(-1, 1, (n, 24)).astype(np.float32)
    q = rng.uniform(-1, 1, (5, 24)).astype(np.float32)
    store = VecStore(24)
    store.add_vectors(rows)
    store.set_base_offset(1000)  # a hit's index is the group, not a row: the offset must not show
    gid = rng.permutation(n)
    store.set_groups(gid)
    listed = rng.choice(n, 1500, replace=False)
    keep = np.ones(n, bool)
    for metric in (Metric.Cosine, Metric.Euclidean):
        for k in (512, 513, None):
            take = G.take_of(metric, k)
            ref = reference(R.ranking(oracle, rows, q, metric, take), gid, n, keep, listed, k, 5, take)
            assert ref.size == (k or 1500)
            for route in ROUTES:
                bits_equal(run(store, q, metric, k, listed, route)[0], ref, (metric, k, route))
    store.close()


# ---- 7. the index's life cycle ---------------------------------------------------------------------------------------------------------

def raw_call(store, q, groups, k):
    """straight at the C ABI (the Python layer refuses some of these itself): (status, message)"""
    d = N.QueryDesc()
    qq = np.ascontiguousarray(q, np.float32)
    g = np.ascontiguousarray(groups, np.uint32)
    d.queries, d.nq, d.metric, d.take, d.k = qq.ctypes.data, qq.shape[0], int(Metric.Cosine), 1, k
    out = np.zeros(max(k, 1), N.HIT_DTYPE)
    n_out = C.c_uint64(0)
    rc = N.lib().ott_query_maxsim_groups(store._handle(), C.byref(d), N.ptr(g) if g.size else None, g.size, N.ptr(out), out.size, C.byref(n_out), None)
    return rc, N.lib().ott_last_error()


def test_index_follows_the_group_ids_and_nothing_else(oracle):
    n, dim = 300, 8
    rng = np.random.default_rng(11700)
    rows = rng.uniform(-1, 1, (4 * n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows[:n])
    full = R.ranking(oracle, rows[:n], q, Metric.Cosine, 1)
    keep = np.ones(n, bool)
    builds = lambda: int(N.lib().ott_store_group_index_builds(store._handle()))  # noqa: E731

    def check(gid, ng, listed, keep_now, where, full_now=full):
        got, st = run(store, q, Metric.Cosine, None, listed, GATHER)
        bits_equal(got, reference(full_now, gid, ng, keep_now, listed, None, 3, 1), where)
        return got

    gid_a, gid_b = np.arange(n) // 8, (np.arange(n) * 7) % 50
    listed = np.array([3, 30, 11, 0, 36])
    store.set_groups(gid_a)
    assert builds() == 0                                   # set_groups alone builds nothing
    G.bits_equal(G.build(store, q[:1], Metric.Cosine, 5).collect_arrays()[0], G.expected(full[full["query"] == 0], gid_a, keep, 5, 1)[0], "grouped")
    run(store, q, Metric.Cosine, 5, listed, MASK)
    assert builds() == 0                                   # ... nor do other query kinds or the mask route
    check(gid_a, 38, listed, keep, "A")
    assert builds() == 1
    check(gid_a, 38, listed[:2], keep, "A again")
    assert builds() == 1                                   # found, not rebuilt
    store.set_groups(gid_b)
    check(gid_b, 50, listed, keep, "B")                    # B's answer, not A's
    assert builds() == 2
    # delete, then restore: the hits change and come back, the index stays
    dead = np.flatnonzero(gid_b == 3)[:4]
    before = check(gid_b, 50, listed, keep, "before delete")
    assert store.delete_rows(dead) == dead.size
    alive = keep.copy()
    alive[dead] = False
    after = check(gid_b, 50, listed, alive, "deleted")
    assert not np.array_equal(before["score"].view(np.uint32), after["score"].view(np.uint32))
    assert store.restore_rows(dead) == dead.size
    check(gid_b, 50, listed, keep, "restored")
    # rewritten rows: the index depends on the ids alone
    store.write_rows(0, rows[n:n + 8])
    rows2 = rows[:n].copy()
    rows2[:8] = rows[n:n + 8]
    check(gid_b, 50, listed, keep, "rewritten", R.ranking(oracle, rows2, q, Metric.Cosine, 1))
    assert builds() == 2
    # cleared: the library refuses, before and after
    store.clear_groups()
    rc, msg = raw_call(store, q, listed, 5)
    assert rc == -1 and b"ott_query_maxsim_groups: no group ids are set" in msg
    store.set_groups(gid_b)
    # appended rows: the ids no longer cover the store
    store.add_vectors(rows[n:])  # reallocates
    rc, msg = raw_call(store, q, listed, 5)
    assert rc == -1 and b"rows were appended since" in msg
    with pytest.raises(OttersError, match="rows were appended since"):
        run(store, q, Metric.Cosine, 5, listed, GATHER)
    rows3 = np.concatenate([rows2, rows[n:]])
    gid_c = rng.integers(0, 60, 4 * n)
    gid_c[:60] = np.arange(60)
    store.set_groups(gid_c)
    b = builds()
    check(gid_c, 60, np.array([59, 3, 30, 11, 0]), np.ones(4 * n, bool), "after growth", R.ranking(oracle, rows3, q, Metric.Cosine, 1))
    assert builds() == b + 1
    # a listed id past the store's groups, and a NULL list with a count
    rc, msg = raw_call(store, q, [1, 60], 5)
    assert rc == -1 and b"group 60 is out of range (the store holds 60 groups)" in msg
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, 3, int(Metric.Cosine), 1, 5
    out = np.zeros(8, N.HIT_DTYPE)
    n_out = C.c_uint64(0)
    assert N.lib().ott_query_maxsim_groups(store._handle(), C.byref(d), None, 2, N.ptr(out), 8, C.byref(n_out), None) == -1
    assert b"groups is NULL" in N.lib().ott_last_error()
    g = np.array([4, 9, 4], np.uint32)
    assert N.lib().ott_query_maxsim_groups(store._handle(), C.byref(d), N.ptr(g), 3, N.ptr(out), 1, C.byref(n_out), None) == -1
    assert b"output capacity is smaller than min(k, distinct listed groups)" in N.lib().ott_last_error()
    assert N.lib().ott_query_maxsim_groups(store._handle(), C.byref(d), N.ptr(g), 3, N.ptr(out), 2, C.byref(n_out), None) == 0 and n_out.value == 2
    store.close()
    multi = VecStore(dim, devices=[0, 0])
    multi.add_vectors(rows[:n])
    multi.set_groups(gid_a)
    with pytest.raises(OttersError, match="ott_query_maxsim_groups: a multi-GPU store is not served") as e:
        run(multi, q, Metric.Cosine, 5, listed, GATHER)
    assert e.value.status == -4
    multi.close()


# ---- 8. the tables are left clean ----------------------------------------------------------------------------------------------------

def test_interleaved_with_the_other_grouped_kinds_on_one_context(oracle):
    """a max_sim query, a listed one, one_per_group and per_group(3) share the context's tables under "zero when found": every
    neighbouring pair in this order and in reverse, each held to its own reference"""
    n, dim = 300, 8
    rng = np.random.default_rng(11800)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (33, dim)).astype(np.float32)
    gid = rng.integers(0, 37, n)
    gid[:37] = np.arange(37)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    keep = np.ones(n, bool)
    ranks = G.Rankings(oracle, rows, q)
    top_ranks = GR.Rankings(oracle, rows, q)
    listed = np.array([36, 2, 9, 9, 17, 30, 31, 4])

    def maxsim(nq, k):
        store.set_option("group_gather", GATHER)
        got = store.query(q[:nq], Metric.Cosine).max_sim().take(k).collect_arrays()[0]
        bits_equal(got, R.expected(ranks.get(Metric.Cosine, nq, k), gid, keep, k, nq, 1, n_groups=37), ("max_sim", nq, k))

    def listed_query(nq, k, route):
        bits_equal(run(store, q[:nq], Metric.Cosine, k, listed, route)[0], reference(ranks.get(Metric.Cosine, nq, k), gid, 37, keep, listed, k, nq, 1), ("listed", nq, k, route))

    def one_per_group(nq, k):
        ref, counts = G.expected(ranks.get(Metric.Cosine, nq, k), gid, keep, k, nq)
        got, got_counts = G.build(store, q[:nq], Metric.Cosine, k, perq=True).collect_arrays()
        G.bits_equal(got, ref, ("one_per_group", nq, k))
        assert list(got_counts) == counts

    def per_group(nq, k):
        GT.check(store, top_ranks, q, gid, Metric.Cosine, nq, 3, k, ("per_group", nq, k))

    for route in ROUTES:
        for nq in (3, 33):  # one token pass (keys straight from the kernel) and two (the table of ordinals and the reduce)
            steps = [lambda: maxsim(nq, 10), lambda: listed_query(nq, 5, route), lambda: one_per_group(3, 10), lambda: per_group(3, 10)]
            for step in steps + steps[::-1]:
                step()
            listed_query(nq, None, route)
            maxsim(9, 37)
            listed_query(nq, 3, route)
            per_group(2, 5)
            listed_query(nq, 8, route)
    store.close()
