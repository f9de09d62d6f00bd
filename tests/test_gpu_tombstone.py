"""GPU: deleted rows (ott_store_delete_rows / restore_rows / live_len / read_live_mask).  Bar: a query on a
store with deleted set D returns exactly the hits — index, score bits, order, per-query counts — of the oracle run with the row
mask `caller_mask & ~D`, on every path, metric, k, mode and tie order; bit for bit, no tolerances.

How the expectation is made: ONE oracle call per (store, metric) ranks every (row, query) pair in the canonical order (k = every
pair); the expected answer of any (mask, k, mode) is that ranking with the masked rows taken out, cut at k (per query: cut per
query).  The reference tie orders, where the outcome at a cut through equal scores depends on the visit order, call the oracle's
literal collectors outright with the combined mask.  Manhattan (EXACT only) is held to tests/manhattan_ref.py the same way."""
import numpy as np
import pytest

import manhattan_ref as M
from otters_amd import Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), (where, got["query"][:12], ref["query"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def ranking(oracle, rows, q, metric, take=None):
    """every (row, query) pair, best first in the canonical order (take: 0 Min / 1 Max; default: the metric's own)"""
    n, nq = rows.shape[0], q.shape[0]
    take = TAKE[metric] if take is None else int(take)
    if metric == Metric.Manhattan:
        return M.select_canonical(M.scores(rows, q), take, n * nq)
    return oracle.vec_query(rows, q, int(metric), take, n * nq, ties=oracle.TIES_CANONICAL)


class Rankings:
    """the rankings of one (store, metric), made on first need: a plan without .take() may rank the other way round"""

    def __init__(self, oracle, rows, q_pool, metric):
        self.args, self.have = (oracle, rows, q_pool, metric), {}

    def get(self, nq, take):
        if (nq, int(take)) not in self.have:
            oracle, rows, q_pool, metric = self.args
            self.have[(nq, int(take))] = ranking(oracle, rows, q_pool[:nq], metric, take)
        return self.have[(nq, int(take))]


def expected(full, keep, k, nq, perq):
    """`full` without the rows `keep` clears, cut at k (per query: k each, in query order) -> (hits, per-query counts)"""
    f = full[keep[full["index"].astype(np.int64)]]
    if not perq:
        f = f[:k]
        return f, [int((f["query"] == qi).sum()) for qi in range(nq)]
    parts = [f[f["query"] == qi][:k] for qi in range(nq)]
    return np.concatenate(parts), [p.size for p in parts]


def combined(n, dead, caller):
    """caller_mask & ~deleted over n rows; a caller mask shorter than n keeps the rows it does not reach (src/vec.rs:234)"""
    keep = np.ones(n, bool)
    if caller is not None:
        keep[:min(caller.size, n)] = caller[:n]
    keep[dead] = False
    return keep


def run(store, q, metric, k, path, perq, caller):
    p = store.query(q, metric)
    if caller is not None:
        p = p.with_row_mask(caller)
    if k is not None:
        p = p.take(k)
    p = p.with_path(path)
    if perq:
        p = p.per_query()
    return p, p.collect_arrays()


def deleted_sets(rng, n, top_rows, k_few):
    block = np.arange(1024, min(n, 1024 + 2048 + 64))  # whole tiles and whole chunks, and a piece of the next
    return {
        "random 1 %": rng.choice(n, max(n // 100, 1), replace=False),
        "block": block,
        "top-k of the query": np.unique(top_rows),
        "all but a few": rng.permutation(n)[k_few:],
        "every row": np.arange(n),
    }


def check_store(oracle, store, rows, q_pool, rng, metrics, paths, ks, nqs, what):
    n, dim = rows.shape
    caller_short = rng.random(n - n // 7) < 0.6
    for metric in metrics:
        ranks = Rankings(oracle, rows, q_pool, metric)
        sets = deleted_sets(rng, n, ranks.get(nqs[0], TAKE[metric])["index"][:100].astype(np.int64), 5)
        for sname, dead in sets.items():
            changed = store.delete_rows(dead)
            assert changed == np.unique(dead).size, (what, sname)
            model = np.ones(n, bool)
            model[dead] = False
            assert store.live_len() == int(model.sum()) and store.len() == n
            assert np.array_equal(store.live_mask(), model), (what, sname)
            for nq in nqs:
                q = q_pool[:nq]
                for caller in (None, caller_short):
                    keep = combined(n, dead, caller)
                    for path in paths:
                        if metric == Metric.Manhattan and path != Path.Exact:
                            continue
                        for k in ks:
                            if path == Path.Mfma and (dim < 8 or (k is None or k > 484)):
                                continue
                            for perq in ((False, True) if nq > 1 else (False,)):
                                plan, (got, counts) = run(store, q, metric, k, path, perq, caller)
                                rq = plan.resolve()
                                ref, ref_counts = expected(ranks.get(nq, rq.take), keep, rq.k, nq, perq)
                                where = (what, metric, sname, nq, "caller" if caller is not None else "no caller", path, k, perq)
                                bits_equal(got, ref, where)
                                if perq:  # (a merged query reports one count: its length)
                                    assert list(counts) == ref_counts, where
            assert store.restore_rows(dead) == np.unique(dead).size
            assert store.live_len() == n


@pytest.mark.parametrize("dim", [3, 128, 768])
def test_small_store_every_metric_path_k_mode_and_batch(oracle, dim):
    n = 3000
    rng = np.random.default_rng(100 + dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q_pool = rng.uniform(-1, 1, (64, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    check_store(oracle, store, rows, q_pool, rng, (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan),
                (Path.Exact, Path.Mfma, Path.Auto), (1, 10, 100, 600, None), (1, 4, 64), ("small", dim))
    store.close()


@pytest.mark.parametrize("dim", [3, 128, 768])
def test_large_store_streaming_kernel_cascade_and_sort_path(oracle, dim):
    """2^18 + 77 rows: the persistent grid, the cascade's planes (AUTO takes them for the batches), the sort path for k = 600"""
    n = (1 << 18) + 77
    rng = np.random.default_rng(200 + dim)
    store = VecStore(dim)
    store.append_random(n, 31 + dim)
    rows = oracle.rand_rows(0, n, dim, 31 + dim)
    q_pool = rng.uniform(-1, 1, (4, dim)).astype(np.float32)
    metrics = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct) + ((Metric.Manhattan,) if dim == 128 else ())
    check_store(oracle, store, rows, q_pool, rng, metrics, (Path.Exact, Path.Mfma, Path.Auto), (1, 10, 100, 600), (1, 4), ("large", dim))
    store.close()


def test_batch_of_64_on_the_large_store(oracle):
    n, dim = 1 << 18, 128
    rng = np.random.default_rng(5)
    store = VecStore(dim)
    store.append_random(n, 77)
    rows = oracle.rand_rows(0, n, dim, 77)
    q = rng.uniform(-1, 1, (64, dim)).astype(np.float32)
    dead = rng.choice(n, n // 100, replace=False)
    store.delete_rows(dead)
    keep = combined(n, dead, None)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for k in (10, 100):
            ref = oracle.vec_query(rows, q, int(metric), 1, k, row_mask=keep, ties=oracle.TIES_CANONICAL)
            for path in (Path.Exact, Path.Mfma, Path.Auto):
                got, _ = store.query(q, metric).take(k).with_path(path).collect_arrays()
                bits_equal(got, ref, ("batch 64", metric, k, path))
            # per query: the oracle one query at a time
            got, counts = store.query(q, metric).take(k).per_query().collect_arrays()
            parts = []
            for qi in range(64):
                r = oracle.vec_query(rows, q[qi], int(metric), 1, k, row_mask=keep, ties=oracle.TIES_CANONICAL)
                r["query"] = qi
                parts.append(r)
            bits_equal(got, np.concatenate(parts), ("batch 64 per query", metric, k))
            assert list(counts) == [k] * 64
    store.close()


@pytest.mark.parametrize("dim", [128, 768])
def test_pruned_sweep_and_sketch_forced_on(oracle, dim):
    n = 1 << 18
    rng = np.random.default_rng(9 + dim)
    store = VecStore(dim)
    store.set_option("exact_sketch", 1)
    store.set_option("exact_prune", 1)
    store.append_random(n, 5)
    rows = oracle.rand_rows(0, n, dim, 5)
    q = rng.uniform(-1, 1, (1, dim)).astype(np.float32)
    for metric in (Metric.Cosine, Metric.DotProduct):
        full = ranking(oracle, rows, q, metric)
        for sname, dead in deleted_sets(rng, n, full["index"][:100].astype(np.int64), 5).items():
            store.delete_rows(dead)
            for caller in (None, rng.random(n - 999) < 0.5):
                keep = combined(n, dead, caller)
                for k in (1, 10, 100):
                    _, (got, _) = run(store, q, metric, k, Path.Exact, False, caller)
                    bits_equal(got, expected(full, keep, k, 1, False)[0], ("prune", dim, metric, sname, k, caller is not None))
            store.restore_rows(dead)
    store.close()


def quantised(rng, n, dim, levels):
    return rng.integers(-levels, levels + 1, (n, dim)).astype(np.float32)


def same_sets(got, lit, where):
    assert got.size == lit.size, (where, got.size, lit.size)
    assert np.array_equal(got["score"].view(np.uint32), lit["score"].view(np.uint32)), (where, "score sequence")
    a = sorted(zip(got["index"].tolist(), got["query"].tolist()))
    b = sorted(zip(lit["index"].tolist(), lit["query"].tolist()))
    assert a == b, (where, [x for x in a if x not in b][:8], [x for x in b if x not in a][:8])


@pytest.mark.parametrize("seed", range(4))
def test_tie_orders_with_deleted_rows(oracle, seed):
    """quantised rows: nearly every cut runs through a group of equal scores.  tie_order 0 against the canonical collector (bit
    for bit), 1 against the literal collector over the store, 2 against one literal collector per chunk — all with the combined mask"""
    rng = np.random.default_rng(900 + seed)
    n, dim, nq, cs = (4099, 5000, 20011, 2500)[seed], (8, 3, 12, 33)[seed], (1, 3, 2, 4)[seed], (1024, 500, 1024, 64)[seed]
    rows = quantised(rng, n, dim, 2)
    q = quantised(rng, nq, dim, 2)
    q[np.all(q == 0, axis=1)] = 1.0
    store = VecStore(dim)
    store.set_chunk_size(cs)
    store.add_vectors(rows)
    dead = rng.choice(n, n // 5, replace=False)
    store.delete_rows(dead)
    for caller in (None, rng.random(n - 100) < 0.7):
        keep = combined(n, dead, caller)
        for metric, take in ((Metric.DotProduct, 1), (Metric.Euclidean, 0), (Metric.Cosine, 1)):
            for k in (1, 10, 100, 600):
                for path in (Path.Exact, Path.Auto):
                    def go():
                        p = store.query(q, metric)
                        if caller is not None:
                            p = p.with_row_mask(caller)
                        return (p.take_max(k) if take else p.take_min(k)).with_path(path).collect_arrays()[0]
                    where = (seed, metric, k, path, caller is not None)
                    store.set_tie_order("canonical")
                    bits_equal(go(), oracle.vec_query(rows, q, int(metric), take, k, row_mask=keep, ties=oracle.TIES_CANONICAL), where + (0,))
                    store.set_tie_order("reference")
                    same_sets(go(), oracle.vec_query(rows, q, int(metric), take, k, row_mask=keep, ties=oracle.TIES_LITERAL), where + (1,))
                    store.set_tie_order("reference_chunked")
                    lit, _ = oracle.meta_query(rows, cs, q, int(metric), take, k, row_mask=keep, ties=oracle.TIES_LITERAL)
                    got = go()
                    assert np.array_equal(got["score"].view(np.uint32), lit["score"].view(np.uint32)), where + (2,)
                    assert sorted(got["index"].tolist()) == sorted(lit["index"].tolist()), where + (2,)  # (the reference drops the query id there)
    store.close()


def test_device_eval_mask_and_chunk_mask_from_a_metastore_filter(oracle):
    """the evaluated device mask joins the live mask per query and is not modified: a later restore shows through"""
    n, dim, cs = 20_000, 96, 1024
    rng = np.random.default_rng(3)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    age = rng.integers(0, 100, n).astype(np.int32)
    shelf = (np.arange(n) // cs).astype(np.int32)  # zone maps prune whole chunks on it
    meta = (MetaStore.from_columns([Column.from_numpy("age", DataType.Int32, age), Column.from_numpy("shelf", DataType.Int32, shelf)])
            .with_vectors(rows).with_chunk_size(cs).build())
    q = rng.uniform(-1, 1, (4, dim)).astype(np.float32)
    dead = np.concatenate([rng.choice(n, 500, replace=False), np.arange(3 * cs, 5 * cs)])
    for expr, fmask in ((col("age").gt(40), age > 40), (col("age").lt(70) & col("shelf").gte(4), (age < 70) & (shelf >= 4))):
        for step in ("deleted", "restored"):
            if step == "deleted":
                assert meta.delete_rows(dead) == np.unique(dead).size and meta.live_len() == n - np.unique(dead).size
            else:
                assert meta.restore_rows(dead) == np.unique(dead).size and meta.live_len() == n
            keep = fmask.copy()
            if step == "deleted":
                keep[dead] = False
            for metric in (Metric.Cosine, Metric.Euclidean, Metric.DotProduct):
                for k in (1, 10, 100, 600):
                    for path in (Path.Exact, Path.Auto):
                        res = meta.query_batch(q, metric).meta_filter(expr).take(k).with_path(path).collect()
                        ref = oracle.vec_query(rows, q, int(metric), TAKE[metric], k, row_mask=keep, ties=oracle.TIES_CANONICAL)
                        where = (step, metric, k, path)
                        assert res.indices == ref["index"].astype(np.int64).tolist(), where
                        assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), ref["score"].view(np.uint32)), where


def test_append_restore_write_rows_counts_and_bad_indices(oracle):
    dim = 40
    rng = np.random.default_rng(11)
    rows = rng.uniform(-1, 1, (5000, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows[:3000])
    never, _ = store.query(q, Metric.Cosine).take(50).collect_arrays()
    assert store.restore_rows([1, 2, 3]) == 0 and store.live_len() == 3000  # nothing was ever deleted
    # n_changed: duplicates within a call count once, repeats not at all
    assert store.delete_rows([7, 7, 9, 7, 2999]) == 3
    assert store.delete_rows([7, 10]) == 1
    assert store.live_len() == 2996
    assert store.restore_rows([7, 7, 11]) == 1 and store.live_len() == 2997
    # an out-of-range index fails and changes nothing (not even the rows listed before it)
    before = store.live_mask()
    for bad in ([5, 3000], [2 ** 40], [0, 1, 2, 3000, 4]):
        with pytest.raises(OttersError) as e:
            store.delete_rows(bad)
        assert e.value.status == -1 and "out of range" in str(e.value)
        with pytest.raises(OttersError):
            store.restore_rows(bad)
    assert np.array_equal(store.live_mask(), before) and store.live_len() == 2997
    # delete, then append (one staged row, then a block that reallocates): the new rows are live
    dead = np.array([9, 10, 2999])
    store.add_vector(rows[3000])
    assert store.live_len() == 2998 and store.len() == 3001
    store.add_vectors(rows[3001:])
    model = np.ones(5000, bool)
    model[dead] = False
    assert np.array_equal(store.live_mask(), model) and store.live_len() == 4997
    for k in (10, 600, None):
        p = store.query(q, Metric.Cosine)
        p = p.take(k) if k is not None else p
        got, _ = p.collect_arrays()
        full = ranking(oracle, rows, q, Metric.Cosine, p.resolve().take)
        bits_equal(got, expected(full, model, p.resolve().k, 3, False)[0], ("after append", k))
    # a deleted row that is listed for deletion right after the append of staged rows: indices of staged rows are valid
    store.add_vector(rows[0])
    assert store.delete_rows([5000]) == 1 and store.live_len() == 4997 and store.len() == 5001
    assert store.restore_rows([5000]) == 1
    # write_rows on a deleted row: stays deleted, shows its new data after restore
    planted = (q[0] * 3).astype(np.float32)
    store.write_rows(9, planted)
    got, _ = store.query(q[0], Metric.Cosine).take(5).collect_arrays()
    assert 9 not in got["index"].tolist()
    assert store.restore_rows([9]) == 1
    got, _ = store.query(q[0], Metric.Cosine).take(5).collect_arrays()
    assert int(got["index"][0]) == 9
    store.close()
    # delete, then restore, equals never deleted
    s2 = VecStore(dim)
    s2.add_vectors(rows[:3000])
    d = rng.choice(3000, 700, replace=False)
    s2.delete_rows(d)
    s2.restore_rows(d)
    again, _ = s2.query(q, Metric.Cosine).take(50).collect_arrays()
    bits_equal(again, never, "restore")
    s2.close()


def test_chunk_mask_with_deleted_rows(oracle):
    n, dim, cs = 30_000, 64, 1024
    rng = np.random.default_rng(21)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (4, dim)).astype(np.float32)
    store = VecStore(dim)
    store.set_chunk_size(cs)
    store.add_vectors(rows)
    dead = np.concatenate([rng.choice(n, 300, replace=False), np.arange(2 * cs, 4 * cs + 17)])
    store.delete_rows(dead)
    n_chunks = (n + cs - 1) // cs
    cmask = rng.random(n_chunks) < 0.6
    cmask[2] = cmask[4] = True
    keep = np.repeat(cmask, cs)[:n]
    keep[dead] = False
    for metric in (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan):
        full = ranking(oracle, rows, q, metric)
        for k in (1, 10, 100, 600):
            for perq in (False, True):
                p = store.query(q, metric).take(k)
                p = p.per_query() if perq else p
                hits, _, _ = store._run(p.resolve(), chunk_mask=cmask)
                bits_equal(hits, expected(full, keep, k, 4, perq)[0], ("chunk mask", metric, k, perq))
    store.close()
