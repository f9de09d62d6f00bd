"""GPU: batch search with a row mask per query (ott_query_masks, the device mask slots, VecQueryPlan.with_row_masks,
MetaQueryPlan.meta_filters).  Bar: query b's hits — index, score bits, order, count, and `query` = b — are exactly
the oracle's for that query alone with row_mask = common & mask_b (tests/masks_ref.py: one oracle call per query, canonical ties;
Manhattan through tests/manhattan_ref.py), on BOTH routes: option masks_sweep = 1 (the masks sweep wherever eligible) and 0 (by
mask group), which are also compared with each other.  Bit for bit, no tolerances.  Rows and queries are integers in -2..2, so
exact score ties are frequent (asserted)."""
import ctypes as C

import numpy as np
import pytest

import manhattan_ref as M
import masks_ref as MR
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N
from otters_amd.expr import CmpOp, ColumnFilter, CompiledFilter, NumericLiteral

pytestmark = pytest.mark.gpu

SWEEP, LOOP = 1, 0
TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)


def corpus(n, dim, seed, nq=9):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    rows[np.all(rows == 0, axis=1), 0] = 1.0  # (no zero rows: a cosine against one is NaN, which has a case of its own)
    q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    q[np.all(q == 0, axis=1), 0] = 1.0
    return rng, rows, q


def make_store(rows, chunk=None, **kw):
    store = VecStore(rows.shape[1], **kw)
    if chunk:
        store.set_chunk_size(chunk)
    store.add_vectors(rows)
    return store


def run(store, q, masks, metric, take, k, route, flt=None, common=None, chunk_mask=None, path=Path.Auto, use_dev=False, raw=None):
    """one ott_query_masks call on `route`: ([hits of query b], stats).  raw = (mask_of_query, query_masks) replaces the lowering"""
    p = store.query(q, metric).per_query().with_row_masks(masks).with_path(path)
    p = p.take_max(k) if take else p.take_min(k)
    if flt is not None:
        p = p.filter(flt[1], flt[0])
    if common is not None:
        p = p.with_row_mask(common)
    rq = p.resolve()
    if raw is not None:
        rq.mask_of_query, rq.query_masks = np.asarray(raw[0], np.uint32), raw[1]
    store.set_option("masks_sweep", route)
    hits, counts, stats = store._run(rq, chunk_mask=chunk_mask, use_device_row_mask=use_dev)
    assert sum(counts) == hits.size and len(counts) == q.shape[0]
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


def both_routes(oracle, store, rows, q, masks, metric, take, k, where, flt=None, common=None, chunk_mask=None, chunk=None, **kw):
    """both routes against the oracle and against each other; returns the sweep's and the loop's stats"""
    keep_common = common
    if chunk_mask is not None:  # the chunk mask as rows, ANDed into the expectation's common mask
        cm_rows = np.repeat(chunk_mask, chunk)[: rows.shape[0]]
        keep_common = cm_rows if common is None else MR.keep_of(rows.shape[0], common, cm_rows)
    exp = MR.expected(oracle, rows, q, masks, metric, take, k, int(flt[0]) if flt else 0, flt[1] if flt else 0.0, common=keep_common)
    a, st_a = run(store, q, masks, metric, take, k, SWEEP, flt, common, chunk_mask, **kw)
    b, st_b = run(store, q, masks, metric, take, k, LOOP, flt, common, chunk_mask, **kw)
    same(a, exp, (where, "sweep"))
    same(b, exp, (where, "by mask group"))
    same(a, b, (where, "sweep against by mask group"))
    return st_a, st_b


def random_masks(rng, n, nq):
    """per query: a mask of its own, one shared with an earlier query, a shorter one, or none"""
    pool = [rng.random(n) < 0.5 for _ in range(3)] + [rng.random(n - 70) < 0.3]
    kinds = [0, 1, None, 0, 2, 3, 1, None, 2]
    return [None if kinds[b] is None else pool[kinds[b]] for b in range(nq)]


# ---- 1. the shape and semantics sweep ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ALL_METRICS, ids=lambda m: m.name)
@pytest.mark.parametrize("n", [1000, 4097])
@pytest.mark.parametrize("dim", [8, 43, 128, 1100])
def test_every_metric_take_filter_k_and_batch_size(oracle, dim, n, metric):
    """dims: the lsl4 short row (8), a remainder of dim % 8 (43), several stages (128), rows beyond 1024 floats (1100); n = 4097 is
    no multiple of 64; chunks of 100 rows with two dropped, so tiles straddle mask words and runs"""
    rng, rows, q = corpus(n, dim, 1000 * dim + n)
    store = make_store(rows, chunk=100)
    n_chunks = (n + 99) // 100
    cm = np.ones(n_chunks, bool)
    cm[[1, n_chunks - 2]] = False
    # the corpus really produces ties: fewer distinct scores than rows, for the first query
    if metric == Metric.Manhattan:
        s0 = M.query(rows, q[0], TAKE[metric], n)["score"]
    else:
        s0 = oracle.vec_query(rows, q[:1], int(metric), TAKE[metric], n, ties=oracle.TIES_CANONICAL)["score"]
    assert s0.size == n and np.unique(s0.view(np.uint32)).size < n
    mid, hit = float(np.median(s0)), float(s0[n // 3])  # thresholds inside the score range; `hit` is a score that occurs
    configs = [(1, 10, None), (3, 1, (Cmp.Lt, mid)), (4, 600, (Cmp.Gt, mid)), (5, n, (Cmp.Lte, mid)), (9, 10, (Cmp.Gte, mid)), (4, 10, (Cmp.Eq, hit)),
               (9, 600, None)]
    for take in (0, 1):
        for nq, k, flt in configs:
            masks = random_masks(rng, n, nq)
            both_routes(oracle, store, rows, q[:nq], masks, metric, take, k, (dim, n, metric.name, take, nq, k, flt), flt=flt, chunk_mask=cm, chunk=100)


# ---- 2. named cases ----------------------------------------------------------------------------------------------------------------------

def test_no_hit_leaks_between_the_queries_of_a_pass(oracle):
    n, dim = 1000, 16
    rng, rows, q = corpus(n, dim, 31)
    store = make_store(rows)
    r = np.arange(n)
    masks = [r % 4 == b for b in range(4)] + [np.zeros(n, bool)]  # disjoint masks, and a query that keeps nothing
    for metric in (Metric.DotProduct, Metric.Euclidean):
        st_a, st_b = both_routes(oracle, store, rows, q[:5], masks, metric, TAKE[metric], 20, ("disjoint", metric.name))
        got, _ = run(store, q[:5], masks, metric, TAKE[metric], 20, SWEEP)
        for b in range(4):
            assert got[b].size == 20 and np.all(got[b]["index"] % 4 == b)
        assert got[4].size == 0
        assert st_a["passes"] == 2 and st_b["passes"] >= 5  # the sweep: four queries per pass; by mask group: one run per distinct mask
    # a tile that is alive for only the LAST query of a pass gives the other three nothing
    masks = [r < 64, (r >= 64) & (r < 128), r >= 900, (r >= 128) & (r < 192)]
    both_routes(oracle, store, rows, q[:4], masks, Metric.DotProduct, 1, 200, "one live tile per query")
    got, _ = run(store, q[:4], masks, Metric.DotProduct, 1, 200, SWEEP)
    for b in range(3):
        assert not np.any((got[b]["index"] >= 128) & (got[b]["index"] < 192))
    assert got[3].size == 64 and np.all((got[3]["index"] >= 128) & (got[3]["index"] < 192))


def test_shared_masks_that_are_not_adjacent_no_mask_mixed_in_and_short_masks(oracle):
    n, dim = 1500, 24
    rng, rows, q = corpus(n, dim, 32)
    store = make_store(rows)
    a, b = rng.random(n - 100) < 0.4, rng.random(n - 100) < 0.1  # mask_bits < n: the rows behind are kept
    masks = [a, b, None, a, b.copy(), a, None, b, a]
    for metric in ALL_METRICS:
        both_routes(oracle, store, rows, q, masks, metric, TAKE[metric], 25, ("shared", metric.name))
    got, _ = run(store, q, masks, Metric.DotProduct, 0, n, SWEEP)
    assert all(np.any(g["index"] >= n - 100) for g in got)  # (rows behind the masks' end do come back)
    _, st = run(store, q, [a] * 9, Metric.DotProduct, 1, 10, LOOP)
    assert st["passes"] <= 3  # one shared mask: ONE batch run for the nine queries, not nine runs


def test_common_row_mask_deleted_rows_and_the_device_mask_as_common(oracle):
    n, dim = 2000, 32
    rng, rows, q = corpus(n, dim, 33)
    store = make_store(rows)
    masks = random_masks(rng, n, 6)
    common = rng.random(n - 30) < 0.6
    both_routes(oracle, store, rows, q[:6], masks, Metric.Cosine, 1, 40, "common mask", common=common)
    # deleted rows: the live mask joins the common mask
    dead = rng.choice(n, 300, replace=False)
    store.delete_rows(dead)
    alive = np.ones(n, bool)
    alive[dead] = False
    exp = MR.expected(oracle, rows, q[:6], masks, Metric.Cosine, 1, 40, common=MR.keep_of(n, common, alive))
    for route in (SWEEP, LOOP):
        same(run(store, q[:6], masks, Metric.Cosine, 1, 40, route, common=common)[0], exp, ("deleted + common", route))
    exp = MR.expected(oracle, rows, q[:6], masks, Metric.Euclidean, 0, 700, common=alive)
    for route in (SWEEP, LOOP):
        same(run(store, q[:6], masks, Metric.Euclidean, 0, 700, route)[0], exp, ("deleted", route))
    # use_device_row_mask: what ott_store_eval_row_mask left is the common mask
    vals = rng.integers(0, 100, n).astype(np.int32)
    cid = C.c_uint32(0)
    N.check(N.lib().ott_store_add_column(store._handle(), 0, N.ptr(vals), None, n, C.byref(cid)))
    leaf = N.Leaf()
    leaf.column, leaf.op, leaf.clause, leaf.lit_i64 = cid.value, int(CmpOp.Lt), 0, 55
    N.check(N.lib().ott_store_eval_row_mask(store._handle(), C.byref(leaf), 1, 1, None))
    exp = MR.expected(oracle, rows, q[:6], masks, Metric.DotProduct, 1, 30, common=alive & (vals < 55))
    for route in (SWEEP, LOOP):
        same(run(store, q[:6], masks, Metric.DotProduct, 1, 30, route, use_dev=True)[0], exp, ("device mask as common", route))


def test_a_row_holding_nan_is_dropped(oracle):
    n, dim = 700, 20
    rng, rows, q = corpus(n, dim, 34)
    rows[[5, 130, 699], 3] = np.nan
    store = make_store(rows)
    masks = random_masks(rng, n, 5)
    masks[0] = np.ones(n, bool)
    for metric in ALL_METRICS:
        both_routes(oracle, store, rows, q[:5], masks, metric, TAKE[metric], n, ("nan", metric.name))
    got, _ = run(store, q[:5], masks, Metric.DotProduct, 1, n, SWEEP)
    assert got[0].size == n - 3 and not np.isin([5, 130, 699], got[0]["index"]).any()


def slot_write(store, slot, mask):
    words = N.pack_bits(mask)
    return N.lib().ott_store_write_row_mask_slot(store._handle(), slot, N.ptr(words), int(np.asarray(mask).size))


def test_slot_masks_equal_the_same_bits_sent_as_host_masks(oracle):
    n, dim = 1300, 16
    rng, rows, q = corpus(n, dim, 35)
    store = make_store(rows)
    vals = rng.integers(0, 100, n).astype(np.int64)
    cid = C.c_uint32(0)
    N.check(N.lib().ott_store_add_column(store._handle(), 1, N.ptr(vals), None, n, C.byref(cid)))
    leaf = N.Leaf()
    leaf.column, leaf.op, leaf.clause, leaf.lit_i64 = cid.value, int(CmpOp.Gte), 0, 40
    back = np.zeros((n + 63) // 64, dtype=np.uint64)
    N.check(N.lib().ott_store_eval_row_mask_slot(store._handle(), 7, C.byref(leaf), 1, 1, N.ptr(back)))
    assert np.array_equal(N.unpack_bits(back, n), vals >= 40)  # the evaluator's own bits, copied back
    written = rng.random(n - 41) < 0.3  # a slot shorter than the store keeps the rows behind it
    N.check(slot_write(store, 63, written))
    host = rng.random(n) < 0.5
    masks = [vals >= 40, written, host, None, written, vals >= 40]
    exp = MR.expected(oracle, rows, q[:6], masks, Metric.DotProduct, 1, 50)
    S = N.MASK_SLOT_BASE
    raw = ([S + 7, S + 63, 0, N.NO_MASK, S + 63, S + 7], host[None, :])  # host and slot references in one call
    for route in (SWEEP, LOOP):
        same(run(store, q[:6], masks, Metric.DotProduct, 1, 50, route, raw=raw)[0], exp, ("slots", route))
        same(run(store, q[:6], masks, Metric.DotProduct, 1, 50, route)[0], exp, ("the same bits as host masks", route))
    # the single evaluated mask was not touched by the slot calls
    with pytest.raises(OttersError, match="ott_store_eval_row_mask was not called"):
        run(store, q[:1], [None], Metric.DotProduct, 1, 5, LOOP, use_dev=True)
    # a slot that was never filled, a cleared one
    with pytest.raises(OttersError, match="slot 8 was never filled") as ei:
        run(store, q[:2], [None, None], Metric.DotProduct, 1, 5, SWEEP, raw=([N.NO_MASK, S + 8], np.ones((0, 0), bool)))
    assert ei.value.status == -1
    N.check(N.lib().ott_store_clear_row_mask_slots(store._handle()))
    with pytest.raises(OttersError, match="slot 7 was never filled"):
        run(store, q[:1], [None], Metric.DotProduct, 1, 5, LOOP, raw=([S + 7], np.ones((0, 0), bool)))
    assert slot_write(store, 64, host) == -1 and b"slot 64 is not below OTT_MASK_SLOTS" in N.lib().ott_last_error()


def test_slots_are_dropped_when_the_rows_move():
    n, dim = 600, 8
    rng, rows, q = corpus(n, dim, 36)
    store = make_store(rows)
    S, none = N.MASK_SLOT_BASE, np.ones((0, 0), bool)
    N.check(slot_write(store, 2, rng.random(n) < 0.5))
    assert run(store, q[:1], [None], Metric.DotProduct, 1, 5, SWEEP, raw=([S + 2], none))[0][0].size == 5
    store.add_vectors(np.tile(rows, (8, 1)))  # nine times the rows: the append reallocates
    for route in (SWEEP, LOOP):
        with pytest.raises(OttersError, match="slot 2 was never filled, or was dropped") as ei:
            run(store, q[:1], [None], Metric.DotProduct, 1, 5, route, raw=([S + 2], none))
        assert ei.value.status == -1
    N.check(slot_write(store, 2, rng.random(store.len()) < 0.5))
    assert run(store, q[:1], [None], Metric.DotProduct, 1, 5, LOOP, raw=([S + 2], none))[0][0].size == 5
    store.delete_rows([1, 2, 3])
    store.compact()
    with pytest.raises(OttersError, match="slot 2 was never filled, or was dropped") as ei:
        run(store, q[:1], [None], Metric.DotProduct, 1, 5, SWEEP, raw=([S + 2], none))
    assert ei.value.status == -1


def test_the_key_table_is_left_clean_for_the_other_query_kinds(oracle):
    n, dim = 1200, 16
    rng, rows, q = corpus(n, dim, 37)
    labels = rng.integers(0, 40, n)
    masks = random_masks(rng, n, 7)

    def others(store):
        g = store.query(q[:2], Metric.DotProduct).per_query().one_per_group().take(15).collect_arrays()
        r = store.recommend([3, 77], [500], Metric.DotProduct).take(15).collect_arrays()
        return g, r

    used, fresh = make_store(rows), make_store(rows)
    used.set_groups(labels)
    fresh.set_groups(labels)
    first, _ = run(used, q[:7], masks, Metric.DotProduct, 1, 30, SWEEP)
    second, _ = run(used, q[:7], masks, Metric.DotProduct, 1, 30, SWEEP)  # the same call twice
    same(second, first, "twice")
    same(first, MR.expected(oracle, rows, q[:7], masks, Metric.DotProduct, 1, 30), "against the oracle")
    third, _ = run(used, q[:7], masks, Metric.Euclidean, 0, 600, SWEEP)   # ... and through the pair form of the top-k
    same(third, MR.expected(oracle, rows, q[:7], masks, Metric.Euclidean, 0, 600), "pair form")
    (g_u, r_u), (g_f, r_f) = others(used), others(fresh)
    for u, f in ((g_u, g_f), (r_u, r_f)):
        assert np.array_equal(u[0]["index"], f[0]["index"]) and np.array_equal(u[0]["score"].view(np.uint32), f[0]["score"].view(np.uint32))
        assert list(u[1]) == list(f[1])


@pytest.mark.parametrize("how", ["reference", "reference_chunked", "mfma"])
def test_tie_orders_and_the_mfma_path_equal_the_query_alone(how):
    """what the sweep does not serve is answered by mask group even with masks_sweep = 1: the hits of ott_query for the query alone"""
    n, dim = 3000, 32
    rng, rows, q = corpus(n, dim, 38)
    store = make_store(rows, chunk=256)
    path = Path.Auto
    if how == "mfma":
        path = Path.Mfma
    else:
        store.set_tie_order(how)
    masks = random_masks(rng, n, 6)
    common = rng.random(n) < 0.8
    for metric in (Metric.Cosine, Metric.DotProduct):
        a, _ = run(store, q[:6], masks, metric, 1, 12, SWEEP, common=common, path=path)
        b, _ = run(store, q[:6], masks, metric, 1, 12, LOOP, common=common, path=path)
        same(a, b, (how, metric.name, "routes"))
        for i in range(6):
            alone = store.query(q[i:i + 1], metric).with_row_mask(MR.keep_of(n, common, masks[i])).take_max(12).with_path(path).per_query().collect_arrays()[0]
            alone = alone.copy()
            alone["query"] = i
            same([a[i]], [alone], (how, metric.name, i))


def test_a_multi_gpu_store_answers_with_host_masks(oracle):
    n, dim = 2500, 24
    rng, rows, q = corpus(n, dim, 39)
    multi = VecStore(dim, devices=[0, 0])
    multi.set_option("multi_min_shard_rows", 0)
    multi.set_chunk_size(128)
    multi.reserve(n)  # (plans the even split: both shards hold rows)
    multi.add_vectors(rows)
    single = make_store(rows, chunk=128)
    masks = random_masks(rng, n, 7)
    common = rng.random(n - 11) < 0.7
    for metric in (Metric.Cosine, Metric.Manhattan):
        exp = MR.expected(oracle, rows, q[:7], masks, metric, TAKE[metric], 33, common=common)
        for route in (SWEEP, LOOP):
            same(run(multi, q[:7], masks, metric, TAKE[metric], 33, route, common=common)[0], exp, ("multi", metric.name, route))
        same(run(single, q[:7], masks, metric, TAKE[metric], 33, SWEEP, common=common)[0], exp, ("single", metric.name))
    assert len(multi.shards()) == 2 and all(cnt > 0 for _, _, cnt in multi.shards())
    L, h = N.lib(), multi._handle()
    words = N.pack_bits(np.ones(n, bool))
    assert L.ott_store_write_row_mask_slot(h, 0, N.ptr(words), n) == -4
    assert L.ott_store_eval_row_mask_slot(h, 0, None, 0, 0, None) == -4
    assert L.ott_store_clear_row_mask_slots(h) == -4 and b"multi-GPU" in L.ott_last_error()


def test_meta_filters_equal_one_filtered_query_each():
    n, dim, cs = 3000, 16, 200
    rng, rows, q = corpus(n, dim, 40, nq=8)
    chunk = np.arange(n) // cs
    price = Column.from_numpy("price", DataType.Float64, (chunk % 5) * 20.0 + rng.uniform(0, 25, n), rng.random(n) < 0.05)
    ver = Column.from_numpy("version", DataType.Int32, (chunk % 3) + rng.integers(0, 2, n), rng.random(n) < 0.05)
    ts = Column.from_numpy("ts", DataType.DateTime, 1_700_000_000_000 + chunk.astype(np.int64) * 86_400_000 + rng.integers(0, 86_400_000, n))
    grade = Column.from_numpy("grade", DataType.String, np.array(["A", "B", "C", "D"])[(chunk + rng.integers(0, 2, n)) % 4], rng.random(n) < 0.03)
    tenant = Column.from_numpy("tenant", DataType.Int32, (chunk // 4).astype(np.int32))
    meta = MetaStore.from_columns([price, ver, ts, grade, tenant]).with_vectors(rows).with_chunk_size(cs).build()
    host_only = CompiledFilter([[ColumnFilter("Numeric", "grade", CmpOp.Gt, NumericLiteral("I64", 1)), ColumnFilter("Numeric", "version", CmpOp.Eq, NumericLiteral("I64", 2))]])
    assert not meta._device_mask_ok(host_only)  # a Numeric leaf on a String column: the host builds this mask
    whole_chunks = col("tenant").eq(1)          # the zone statistics decide every row: its chunk mask is its row mask
    compiled = whole_chunks.compile(meta.schema())
    assert meta.row_mask_is_all_true(compiled, meta.build_chunk_mask_for_plan(compiled))
    shared = col("price").lt(50.0) & col("version").gte(2)
    filters = [shared, col("ts").gte("2023-11-20") & col("grade").eq("A"), host_only, None, whole_chunks, shared,
               col("grade").neq("C") & col("price").gt(10), col("version").eq(77)]  # (the last one prunes every chunk: no hits)
    for metric in (Metric.Cosine, Metric.Euclidean):
        for route in (SWEEP, LOOP):
            meta._store.set_option("masks_sweep", route)
            got = meta.query_batch(q, metric).meta_filters(filters).take(9).collect_per_query()
            assert len(got) == 8
            for b, f in enumerate(filters):
                plan = meta.query(q[b], metric).take(9)
                if isinstance(f, CompiledFilter):
                    plan._meta_filter = f
                elif f is not None:
                    plan = plan.meta_filter(f)
                alone = plan.collect()
                assert got[b].indices == alone.indices, (metric.name, route, b, got[b].indices, alone.indices)
                assert np.array_equal(np.array(got[b].scores, np.float32).view(np.uint32), np.array(alone.scores, np.float32).view(np.uint32)), (metric.name, route, b)
            assert len(got[7]) == 0 and len(got[3]) == 9
    # without a filter for some query the batch needs every chunk; with one for every query it shares the OR of their chunk masks
    meta.query_batch(q[:2], Metric.Cosine).meta_filters([whole_chunks, col("tenant").eq(2)]).take(3).collect_per_query()
    st = meta.last_query_stats()
    assert st.evaluated_chunks == 8 and st.total_chunks == 15
