"""GPU: the Manhattan (L1) metric on every exact query path, bit for bit against tests/manhattan_ref.py — indices, query ids and
f32 score bits.  rows8 (small stores) and the persistent grid; one to 17 queries; k from 1 to every pair (the fused lists, the
block lists, the sort path); merged and per query; the five filters; host and device row masks and MetaStore chunk pruning;
both reduce orders; the three tie orders; ott_query_device; IEEE edge rows; AUTO against EXACT with the stats; the MFMA refusal;
and the 10M x 768 store."""
import ctypes as C

import numpy as np
import pytest

import ieee_edges as E
import manhattan_ref as M
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

MAN = Metric.Manhattan
DIMS = [1, 3, 7, 8, 9, 31, 32, 33, 100, 128, 768, 1000]
NQS = [1, 2, 3, 4, 5, 8, 17]
KS = [1, 10, 16, 17, 64, 65, 100, 512, 513]


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), (where, got["query"][:12], ref["query"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def run(store, queries, take, k, path=Path.Exact, filt=None, mask=None, perq=False):
    """take: 0 / 1, or None for the default take (.take(k): Min for Manhattan)"""
    p = store.query(queries, MAN)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    p = p.take(k) if take is None else (p.take_max(k) if take else p.take_min(k))
    p = p.with_path(path)
    if perq:
        p = p.per_query()
    return p.collect_arrays()[0]


def corpus(n, dim, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, dim)).astype(np.float32), rng


@pytest.mark.parametrize("dim", DIMS)
def test_small_store_every_dim_nq_k_and_mode(dim):
    """2500 rows (rows8 up to k = 128 and 16 queries; the streaming kernel beyond; the sort path past 512)"""
    n = 2500
    rows, rng = corpus(n, dim, dim)
    pool = rng.uniform(-1, 1, (17, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    S_all = M.scores(rows, pool)
    for nq in NQS:
        q, S = pool[:nq], S_all[:nq]
        for k in KS + [n * nq]:
            for perq in (False, True):
                ref = M.select_canonical(S, M.TAKE_MIN, k, perq=perq)
                bits_equal(run(store, q, None, k, perq=perq), ref, (dim, nq, k, perq, "default take"))
        for k in (10, 600):
            bits_equal(run(store, q, 1, k), M.select_canonical(S, M.TAKE_MAX, k), (dim, nq, k, "take_max"))
    store.close()


@pytest.mark.parametrize("dim", [33, 128])
def test_persistent_grid_store(dim):
    n = 200_000
    rows, rng = corpus(n, dim, 50 + dim)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    S_all = M.scores(rows, q)
    for nq in (1, 4, 5):
        for k in (10, 65, 300, 513):
            for perq in ((False, True) if nq > 1 else (False,)):
                for path in (Path.Exact, Path.Auto):
                    got = run(store, q[:nq], None, k, path=path, perq=perq)
                    bits_equal(got, M.select_canonical(S_all[:nq], M.TAKE_MIN, k, perq=perq), (dim, nq, k, perq, path))
                    assert store.last_stats["path_used"] == int(Path.Exact)
    store.close()


def test_filters_masks_and_reduce_orders():
    """the five filters (thresholds taken from the scores themselves, so that they are hit exactly), host row masks, both
    reduce orders, on rows8 and on the streaming kernel"""
    for n, dim in ((3000, 33), (70_000, 20)):
        rows, rng = corpus(n, dim, n + dim)
        q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
        mask = rng.random(n) < 0.7
        for reduce_mode in (M.REDUCE_AVX, M.REDUCE_SEQ4):
            store = VecStore(dim)
            store.set_reduce_order(reduce_mode)
            store.add_vectors(rows)
            S = M.scores(rows, q, "l1", reduce_mode)
            srt = np.sort(S.ravel())
            for cmp in (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq):
                for thr in (srt[len(srt) // 3], srt[5], srt[-5]):
                    for k in (10, 100, 700):
                        for m in (None, mask):
                            for perq in (False, True):
                                ref = M.select_canonical(S, M.TAKE_MIN, k, int(cmp), float(thr), row_mask=m, perq=perq)
                                got = run(store, q, None, k, filt=(float(thr), cmp), mask=m, perq=perq)
                                bits_equal(got, ref, (n, dim, reduce_mode, cmp, float(thr), k, m is not None, perq))
            store.close()


def test_tie_orders_on_integer_rows():
    """tie_order canonical / reference / reference_chunked on integer-valued rows, where nearly every cut runs through ties"""
    rng = np.random.default_rng(17)
    for n, dim, nq in ((203, 3, 2), (4099, 8, 3), (20011, 12, 1)):
        rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
        q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
        S = M.scores(rows, q)
        store = VecStore(dim)
        store.add_vectors(rows)
        for order in ("canonical", "reference"):
            store.set_tie_order(order)
            for k in (1, 3, 10, 64, 65, 130, 600):
                for filt in (None, (float(dim), Cmp.Lte)):
                    fc, ft = (int(filt[1]), filt[0]) if filt else (0, 0.0)
                    got = run(store, q, None, k, filt=filt)
                    if order == "canonical":
                        bits_equal(got, M.select_canonical(S, M.TAKE_MIN, k, fc, ft), (n, order, k, filt))
                    else:
                        ref = M.select_reference(S, M.TAKE_MIN, k, fc, ft)
                        bits_equal(np.sort(got, order=["index", "query"]), np.sort(ref, order=["index", "query"]), (n, order, k, filt))
                        assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (n, order, k, filt)
        store.close()
    # MetaStore, one collector per chunk (tie_order reference on a MetaStore = the reference's per-chunk collect)
    for cs, n in ((64, 1000), (5, 803)):
        rows = rng.integers(-1, 2, (n, 4)).astype(np.float32)
        q = rng.integers(-2, 3, (2, 4)).astype(np.float32)
        S = M.scores(rows, q)
        bucket = ((np.arange(n) // cs) % 3).astype(np.int32)
        meta = MetaStore.from_columns([Column.from_numpy("bucket", DataType.Int32, bucket)]).with_vectors(rows).with_chunk_size(cs).build()
        meta.set_tie_order("reference")
        n_chunks = (n + cs - 1) // cs
        for k in (1, 4, 10, 33, 100):
            for with_filter in (False, True):
                plan = meta.query_batch(q, MAN)
                cmask = None
                if with_filter:
                    plan = plan.meta_filter(col("bucket").neq(1))
                    cmask = (np.arange(n_chunks) % 3) != 1
                res = plan.take(k).collect()
                ref = M.select_reference_chunked(S, M.TAKE_MIN, k, cs, chunk_mask=cmask)
                assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), ref["score"].view(np.uint32)), (cs, k, with_filter)
                assert sorted(res.indices) == sorted(ref["index"].tolist()), (cs, k, with_filter)


def test_metastore_chunk_pruning_device_row_mask_and_materialised_columns():
    n, dim, cs = 50_000, 24, 1024
    rows, rng = corpus(n, dim, 99)
    bucket = ((np.arange(n) // cs) % 4).astype(np.int32)
    val = rng.integers(0, 100, n).astype(np.int64)
    meta = (MetaStore.from_columns([Column.from_numpy("bucket", DataType.Int32, bucket), Column.from_numpy("val", DataType.Int64, val)])
            .with_vectors(rows).with_chunk_size(cs).build())
    q = rng.uniform(-1, 1, (2, dim)).astype(np.float32)
    S = M.scores(rows, q)
    thr = float(np.sort(S.ravel())[20_000])
    for expr, keep in ((col("bucket").eq(2), bucket == 2), (col("bucket").lt(3) & col("val").gt(40), (bucket < 3) & (val > 40))):
        for k in (5, 100, 600):
            for vf in (None, (thr, Cmp.Lt)):
                plan = meta.query_batch(q, MAN).meta_filter(expr)
                if vf:
                    plan = plan.vec_filter(*vf)
                res = plan.take(k).collect()
                ref = M.select_canonical(S, M.TAKE_MIN, k, int(vf[1]) if vf else 0, vf[0] if vf else 0.0, row_mask=keep)
                assert res.indices == ref["index"].tolist(), (k, vf)
                assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), ref["score"].view(np.uint32))
                assert np.asarray(res.column("val").values()).tolist() == val[ref["index"].astype(np.int64)].tolist()
                assert meta.last_query_stats().pruned_chunks > 0


def test_query_device():
    import torch
    n, dim = 40_000, 40
    rows, rng = corpus(n, dim, 5)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    S = M.scores(rows, q)
    for k, perq in ((10, False), (100, False), (10, True)):
        cap = k * (3 if perq else 1)
        buf = torch.empty(cap * 16, dtype=torch.uint8, device="cuda:0")
        nout = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, 3, int(MAN), 0, k
        d.mode, d.path = (1 if perq else 0), int(Path.Exact)
        N.check(N.lib().ott_query_device(store._handle(), C.byref(d), C.c_void_p(buf.data_ptr()), cap, C.c_void_p(nout.data_ptr()), None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(N.HIT_DTYPE)
        assert int(nout.cpu()[0]) == cap
        bits_equal(got[:cap], M.select_canonical(S, M.TAKE_MIN, k, perq=perq), (k, perq))
    store.close()


@pytest.mark.parametrize("dim", [1, 7, 8, 33])
def test_ieee_edge_rows(dim):
    """+-inf (inf - inf: NaN, dropped; an infinite difference: +inf, kept), NaN, +-0, subnormal differences, sums that overflow"""
    rng = np.random.default_rng(300 + dim)
    parts = [E.signed_zero_cosines(rng, 40, dim), E.subnormal_sums(rng, 64, dim), E.overflow(rng, 48, dim)]
    rows = np.concatenate([p[0] for p in parts] + [rng.uniform(-1, 1, (57, dim))]).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38], np.float32)
    extra = special[rng.integers(0, special.size, (64, dim))]
    rows = np.concatenate([rows, extra, rows[:8] * np.float32(1e-40)]).astype(np.float32)
    queries = np.concatenate([p[1] for p in parts] + [extra[:3], np.zeros((1, dim), np.float32), -np.zeros((1, dim), np.float32)]).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    n = rows.shape[0]
    for reduce_mode in (M.REDUCE_AVX, M.REDUCE_SEQ4):
        store.set_reduce_order(reduce_mode)
        for sel in ([0], [len(queries) - 1], list(range(min(4, len(queries)))), list(range(len(queries) - 5, len(queries)))):
            q = queries[sel]
            S = M.scores(rows, q, "l1", reduce_mode)
            for k in (1, 10, 100, 600, n * len(sel)):
                for take in (None, 1):
                    for perq in (False, True):
                        ref = M.select_canonical(S, M.TAKE_MAX if take else M.TAKE_MIN, k, perq=perq)
                        bits_equal(run(store, q, take, k, perq=perq), ref, (dim, reduce_mode, sel, k, take, perq))
            bits_equal(run(store, q, None, 50, filt=(np.inf, Cmp.Eq)), M.select_canonical(S, M.TAKE_MIN, 50, M.CMP_EQ, np.inf), (dim, "inf"))
    store.close()


def test_auto_routes_to_exact_and_builds_no_plane():
    n, dim = 100_000, 64
    store = VecStore(dim)
    store.set_option("hi_prebuild", 0)  # no background build after the append: whatever plane exists, a query built it
    store.append_random(n, 11)
    rng = np.random.default_rng(1)
    for nq in (1, 4, 64):
        q = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
        a = run(store, q, None, 10, path=Path.Auto)
        st = dict(store.last_stats)
        e = run(store, q, None, 10, path=Path.Exact)
        bits_equal(a, e, ("auto vs exact", nq))
        assert st["path_used"] == int(Path.Exact) and st["rescored"] == 0 and st["retries"] == 0, st
        passes = (nq + 3) // 4
        assert st["bytes_scanned"] == passes * n * dim * 4, (nq, st["bytes_scanned"])
        assert not store.batch_ready(), nq
    # the contrast: a dot batch on the matrix cores does build its plane
    q = rng.uniform(-1, 1, (64, dim)).astype(np.float32)
    store.query(q, Metric.DotProduct).take(10).with_path(Path.Mfma).collect_arrays()
    assert store.last_stats["path_used"] == int(Path.Mfma) and store.batch_ready()
    # and Manhattan on that store still streams the f32 rows, same bits
    bits_equal(run(store, q, None, 10, path=Path.Auto), run(store, q, None, 10, path=Path.Exact), "with a plane resident")
    assert store.last_stats["path_used"] == int(Path.Exact) and store.last_stats["rescored"] == 0
    store.close()
    # a store that forbids the batch copies
    s2 = VecStore(dim)
    s2.set_batch_image(False)
    s2.append_random(50_000, 12)
    before = s2.batch_ready()
    run(s2, rng.uniform(-1, 1, (32, dim)).astype(np.float32), None, 10, path=Path.Auto)
    assert s2.batch_ready() == before
    s2.close()


def test_mfma_is_refused_and_unknown_metrics_still_fail():
    store = VecStore(16)
    store.append_random(5000, 2)
    q = np.ones((4, 16), np.float32)
    with pytest.raises(OttersError) as ei:
        run(store, q, None, 10, path=Path.Mfma)
    assert "Manhattan" in str(ei.value) and "AUTO or EXACT" in str(ei.value), str(ei.value)
    for bad in (4, 9):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, 1, bad, 0, 10
        buf = np.zeros(10, dtype=N.HIT_DTYPE)
        n_out = C.c_uint64(0)
        assert N.lib().ott_query(store._handle(), C.byref(d), N.ptr(buf), 10, C.byref(n_out), None, None) != 0
        assert b"unknown metric" in N.lib().ott_last_error()
    store.close()


# ---- full size --------------------------------------------------------------------------------------------------------------

SEED = 0x4D41


def test_10Mx768_top10_properties(oracle):
    n, dim = 10_000_000, 768
    store = VecStore(dim)
    store.set_option("hi_prebuild", 0)
    store.append_random(n, SEED)
    q = oracle.rand_rows(0, 1, dim, SEED + 1)[0]
    got = run(store, q, None, 10)
    assert got.size == 10 and store.last_stats["path_used"] == int(Path.Exact)
    sc = got["score"]
    assert np.all(np.diff(sc) >= 0)
    # every returned score re-derived on the host from the regenerated row
    for i, s in zip(got["index"].tolist(), sc):
        row = oracle.rand_rows(int(i), 1, dim, SEED)
        assert np.array_equal(store.rows(int(i), 1), row)
        assert M.scores(row, q)[0, 0].view(np.uint32) == np.float32(s).view(np.uint32), i
    # no row of a 200k-row random sample (20 slices of 10k rows) scores strictly better than the 10th
    rng = np.random.default_rng(3)
    for first in rng.integers(0, n - 10_000, 20).tolist():
        S = M.scores(oracle.rand_rows(int(first), 10_000, dim, SEED), q)[0]
        assert not np.any(S < sc[-1]), first
    store.close()


def test_1M_store_top10_equals_the_reference(oracle):
    n, dim = 1_000_000, 128
    store = VecStore(dim)
    store.append_random(n, SEED)
    rows = oracle.rand_rows(0, n, dim, SEED)
    q = oracle.rand_rows(0, 2, dim, SEED + 7)
    S = M.scores(rows, q)
    for nq in (1, 2):
        bits_equal(run(store, q[:nq], None, 10), M.select_canonical(S[:nq], M.TAKE_MIN, 10), ("1M", nq))
    assert store.last_stats["bytes_scanned"] == n * dim * 4
    store.close()
