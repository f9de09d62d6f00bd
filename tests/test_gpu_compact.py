"""GPU: ott_store_compact — the deleted rows are physically removed, order preserved.  Afterwards the store is bit-equal to a
FRESH store built from the surviving rows: rows, inverse norms, query results (mapped through the returned index map) on the
exact-order kernel, on the cascade once its plane is rebuilt, and on the pruned sweep with the sketch; appends work; with nothing
deleted it is a no-op; with metadata columns resident it is refused."""
import numpy as np
import pytest

from otters_amd import Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col

pytestmark = pytest.mark.gpu


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), (where, got["query"][:12], ref["query"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def dead_sets(rng, n):
    return {
        "random 1 %": rng.choice(n, max(n // 100, 1), replace=False),
        "random half": rng.choice(n, n // 2, replace=False),
        "block": np.arange(1024, min(n, 1024 + 2048 + 64)),
        "head": np.arange(0, n // 3),
        "tail": np.arange(n - n // 3, n),
        "all but a few": rng.permutation(n)[5:],
        "every row": np.arange(n),
    }


@pytest.mark.parametrize("n,dim", [(3000, 3), (3000, 128), (70_001, 768), ((1 << 18) + 77, 128)])
def test_compacted_store_equals_a_fresh_store_of_the_survivors(n, dim):
    rng = np.random.default_rng(n + dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    for sname, dead in dead_sets(rng, n).items():
        if n > 100_000 and sname in ("head", "tail", "all but a few"):
            continue
        store = VecStore(dim)
        store.set_option("exact_sketch", 1)
        store.add_vectors(rows)
        if dim >= 8:
            store.prepare_batch()  # a plane exists: compaction must drop it, the next batch rebuilds it
        store.delete_rows(dead)
        keep = np.ones(n, bool)
        keep[dead] = False
        masked, _ = store.query(qs[:4], Metric.Cosine).take(100).with_path(Path.Exact).collect_arrays()
        new_index = store.compact()
        n_live = int(keep.sum())
        # the index map: survivors in order, -1 for the removed
        want_map = np.full(n, -1, np.int64)
        want_map[keep] = np.arange(n_live)
        assert new_index.dtype == np.int64 and np.array_equal(new_index, want_map), sname
        assert store.len() == store.live_len() == n_live
        assert store.live_mask().all()
        fresh = VecStore(dim)
        fresh.set_option("exact_sketch", 1)
        if n_live:
            fresh.add_vectors(rows[keep])
        assert np.array_equal(store.rows().view(np.uint32), rows[keep].view(np.uint32)), sname
        if n_live:
            assert np.array_equal(store.inv_norms().view(np.uint32), fresh.inv_norms().view(np.uint32)), sname
        # what the store answered with the rows deleted is what it answers compacted, through the map
        after, _ = store.query(qs[:4], Metric.Cosine).take(100).with_path(Path.Exact).collect_arrays()
        mapped = masked.copy()
        mapped["index"] = new_index[masked["index"].astype(np.int64)].astype(np.uint64)
        bits_equal(after, mapped, (sname, "mapped"))
        for metric in (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan):
            for q in (qs[:1], qs[:4]):
                for k in (1, 10, 100, 600):
                    a, _ = store.query(q, metric).take(k).with_path(Path.Exact).collect_arrays()
                    b, _ = fresh.query(q, metric).take(k).with_path(Path.Exact).collect_arrays()
                    bits_equal(a, b, (sname, metric, q.shape[0], k, "exact"))
        if dim >= 8 and n_live:
            for path in (Path.Mfma, Path.Auto):
                for k in (10, 100):
                    a, _ = store.query(qs, Metric.Cosine).take(k).with_path(path).collect_arrays()
                    b, _ = fresh.query(qs, Metric.Cosine).take(k).with_path(Path.Exact).collect_arrays()
                    bits_equal(a, b, (sname, path, k, "cascade"))
                    if path == Path.Mfma:  # (AUTO may answer a store this small on the exact-order kernel)
                        assert store.last_stats["path_used"] == 2
        # the pruned sweep with the sketch: lines were made again by the ingest kernel
        if dim >= 64 and n_live:
            for s in (store, fresh):
                s.set_option("exact_prune", 1)
            for metric in (Metric.Cosine, Metric.DotProduct):
                for k in (1, 10, 100):
                    a, _ = store.query(qs[0], metric).take(k).with_path(Path.Exact).collect_arrays()
                    b, _ = fresh.query(qs[0], metric).take(k).with_path(Path.Exact).collect_arrays()
                    bits_equal(a, b, (sname, metric, k, "pruned sweep"))
                    assert store.last_stats["rescored"] == fresh.last_stats["rescored"], (sname, metric, k)
        # appends after compaction work (and the rows appended are live, the store one piece again)
        extra = rng.uniform(-1, 1, (700, dim)).astype(np.float32)
        for s in (store, fresh):
            s.add_vector(extra[0])
            s.add_vectors(extra[1:])
        assert store.len() == n_live + 700 == store.live_len()
        assert np.array_equal(store.inv_norms().view(np.uint32), fresh.inv_norms().view(np.uint32)), sname
        for k in (10, 600):
            a, _ = store.query(qs[:4], Metric.DotProduct).take(k).collect_arrays()
            b, _ = fresh.query(qs[:4], Metric.DotProduct).take(k).collect_arrays()
            bits_equal(a, b, (sname, k, "after append"))
        # a second round on the compacted store
        d2 = rng.choice(store.len(), 100, replace=False)
        store.delete_rows(d2)
        m2 = store.compact()
        assert store.len() == n_live + 600 and int((m2 >= 0).sum()) == n_live + 600
        store.close()
        fresh.close()


def test_compaction_with_nothing_deleted_is_a_no_op():
    n, dim = 5000, 48
    rng = np.random.default_rng(2)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    a, _ = store.query(q, Metric.Cosine).take(20).collect_arrays()
    assert np.array_equal(store.compact(), np.arange(n))
    assert store.len() == n
    # deleted and restored again: still nothing to remove
    store.delete_rows([5, 6, 7])
    store.restore_rows([5, 6, 7])
    assert np.array_equal(store.compact(), np.arange(n)) and store.len() == n == store.live_len()
    b, _ = store.query(q, Metric.Cosine).take(20).collect_arrays()
    bits_equal(b, a, "no-op")
    assert np.array_equal(store.rows().view(np.uint32), rows.view(np.uint32))
    store.close()


def test_compaction_is_refused_while_columns_are_resident():
    n, dim = 4000, 16
    rng = np.random.default_rng(4)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    meta = MetaStore.from_columns([Column.from_numpy("age", DataType.Int32, rng.integers(0, 90, n).astype(np.int32))]).with_vectors(rows).build()
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    assert len(meta.query(q, Metric.Cosine).meta_filter(col("age").gt(30)).take(5).collect().indices) == 5  # (the column goes to HBM)
    assert meta.delete_rows([1, 2, 3]) == 3
    with pytest.raises(OttersError) as e:
        meta._store.compact()
    assert e.value.status == -4 and "columns" in str(e.value)
    assert meta._store.len() == n and meta.live_len() == n - 3
