"""GPU: document frequencies on the device and IDF query weights (ott_store_sparse_df, ott_store_sparse_df_builds,
ott_query_sparse_idf, VecStore.sparse_df, SparseQueryPlan.idf).  Bar: df and n_docs are exactly the numpy model's
(tests/hybrid_ref.py: a bincount over the live rows' indices), under both forms of the kernel (store option sparse_df_lds 0: global
atomic adds, 1: a histogram in LDS) wherever the LDS form fits; an IDF query's hits — index, score bits, order — are exactly
ott_query_sparse's model (tests/sparse_ref.py) fed with the model's scaled weights."""
import threading

import numpy as np
import pytest

import fuse_ref as R
import hybrid_ref as H
import sparse_cases as SC
import sparse_ref as SR
from otters_amd import Metric, OttersError, VecStore

pytestmark = pytest.mark.gpu


def store_of(rows, vocab, dim=1):
    store = VecStore(dim)
    store.add_vectors(np.ones((len(rows), dim), np.float32))
    ptr, idx, val = SR.csr(rows)
    store.set_sparse(ptr, idx, val, vocab)
    return store, ptr, idx, val


def forms(vocab):
    return (0, 1, -1) if vocab <= 32768 else (0, -1)


def check_df(store, ptr, idx, vocab, live, where):
    """the store's df and n_docs against the model over the `live` rows (None: all)"""
    counts, n_docs = store.sparse_df()
    exp, exp_docs = H.df(ptr, idx, vocab, live)
    assert n_docs == exp_docs, (where, n_docs, exp_docs)
    assert counts.dtype == np.uint32 and np.array_equal(counts, exp), (where, np.flatnonzero(counts != exp)[:8])
    return counts, n_docs


def both_forms(rows, vocab, where):
    """df under every form of the kernel: the option is read by the build, so every form gets a store whose counts are not built yet"""
    got = None
    for form in forms(vocab):
        store, ptr, idx, _ = store_of(rows, vocab)
        store.set_option("sparse_df_lds", form)
        got = check_df(store, ptr, idx, vocab, None, (where, "sparse_df_lds", form))
        assert store.sparse_df_builds() == 1
        store.close()
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 5000])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    pool = rng.integers(0, 3000, 200).astype(np.uint32)  # a hot set: bins well above 1
    rows = SC.random_rows(rng, n, 3000, 8, empty_frac=0.2, pool=pool)  # rows without entries among them; stored values of 0.0 too
    assert n < 60 or (any(len(i) == 0 for i, _ in rows) and any((v == 0).any() for _, v in rows))
    counts, n_docs = both_forms(rows, 3000, ("rows", n))
    assert n_docs == n and int(counts.sum()) == sum(len(i) for i, _ in rows)


def test_vocab_1_and_one_index_in_every_row():
    rng = np.random.default_rng(1)
    rows = [(SC.u32(0), SC.f32(0.0)) if i % 3 else (SC.u32(), SC.f32()) for i in range(200)]  # vocab 1: stored zeros and empty rows
    counts, n_docs = both_forms(rows, 1, "vocab 1")
    assert counts.tolist() == [133] and n_docs == 200
    rows = SC.random_rows(rng, 5000, 500, 4, empty_frac=0.0, pool=np.arange(1, 500, dtype=np.uint32))
    rows = [(np.concatenate([SC.u32(0), i]), np.concatenate([SC.f32(1.0), v])) for i, v in rows]  # index 0 in every row: 5000 adds to one bin
    counts, _ = both_forms(rows, 500, "contention")
    assert counts[0] == 5000


@pytest.mark.parametrize("vocab", [32768, 32769, 1 << 20])
def test_vocab_at_the_lds_boundary_and_at_the_most(vocab):
    rng = np.random.default_rng(vocab % 977)
    pool = rng.integers(0, vocab, 400).astype(np.uint32)
    pool[:2] = [0, vocab - 1]  # the first and the last bin are in use
    rows = SC.random_rows(rng, 700, vocab, 6, pool=pool)
    rows[0] = (SC.u32(0, vocab - 1), SC.f32(1.0, 1.0))
    counts, _ = both_forms(rows, vocab, ("vocab", vocab))
    assert counts[0] >= 1 and counts[vocab - 1] >= 1 and 2000 < int(counts.sum()) < 6000


def test_counts_follow_deletes_and_restores_and_the_cache_holds_between():
    rng = np.random.default_rng(3)
    n, vocab = 1000, 64
    rows = SC.random_rows(rng, n, vocab, 5)
    store, ptr, idx, val = store_of(rows, vocab)
    live = np.ones(n, bool)
    assert store.sparse_df_builds() == 0
    check_df(store, ptr, idx, vocab, live, "fresh")
    check_df(store, ptr, idx, vocab, live, "fresh again")
    q = [([1, 2, 3], [1.0, 0.5, -1.0])]
    store.sparse_query(q).idf().take(5).collect_per_query()
    store.hybrid(None, [q], Metric.DotProduct).idf().take(5).collect()
    assert store.sparse_df_builds() == 1  # two reads and two queries: one build
    dead = rng.choice(n, 300, replace=False)
    store.delete_rows(dead)
    live[dead] = False
    store.sparse_query(q).idf().take(5).collect_per_query()  # a query is the first to need them
    assert store.sparse_df_builds() == 2
    counts, n_docs = check_df(store, ptr, idx, vocab, live, "deleted")
    assert n_docs == 700 and store.sparse_df_builds() == 2
    store.restore_rows(dead[:100])
    live[dead[:100]] = True
    check_df(store, ptr, idx, vocab, live, "restored")
    assert store.sparse_df_builds() == 3
    store.restore_rows(dead[:100])  # nothing changes: no build
    check_df(store, ptr, idx, vocab, live, "restored twice")
    assert store.sparse_df_builds() == 3
    store.delete_rows(np.arange(n))  # every row deleted: every slice is skipped
    counts, n_docs = check_df(store, ptr, idx, vocab, np.zeros(n, bool), "all deleted")
    assert n_docs == 0 and not counts.any() and store.sparse_df_builds() == 4
    store.restore_rows(np.arange(n))
    store.set_sparse(ptr, idx, val, vocab)  # set again: one more build, the same counts
    check_df(store, ptr, idx, vocab, None, "set again")
    assert store.sparse_df_builds() == 5
    store.clear_sparse()
    with pytest.raises(OttersError, match="no sparse rows are set"):
        store.sparse_df()
    store.set_sparse(ptr, idx, val, vocab)
    store.add_vectors(np.ones((3, 1), np.float32))
    with pytest.raises(OttersError, match="rows were appended since ott_store_set_sparse"):
        store.sparse_df()
    store.close()
    multi = VecStore(1, devices=[0, 0])
    multi.add_vectors(np.ones((10, 1), np.float32))
    with pytest.raises(OttersError):
        multi.sparse_df()


def same_lists(got, exp, where):
    assert len(got) == len(exp), where
    for b, (g, e) in enumerate(zip(got, exp)):
        assert np.array_equal(g["index"].astype(np.int64), e["index"].astype(np.int64)), (where, b, g["index"][:10], e["index"][:10])
        assert np.array_equal(g["score"].view(np.uint32), e["score"].view(np.uint32)), (where, b, g["score"][:10], e["score"][:10])
        assert (g["query"] == b).all(), (where, b)


def split(hits, counts):
    out, at = [], 0
    for c in counts:
        out.append(hits[at:at + c])
        at += c
    return out


@pytest.mark.parametrize("vocab", [100, 40000])
def test_idf_query_equals_the_plain_query_with_the_models_weights(vocab):
    rng = np.random.default_rng(vocab)
    n = 1500
    pool = np.unique(np.concatenate([np.arange(40), rng.integers(0, vocab, 60)])).astype(np.uint32)
    zipf = pool[np.minimum((rng.zipf(1.3, 4000) - 1), pool.size - 1)]  # a few indices in most rows
    rows = SC.random_rows(rng, n, vocab, 10, pool=zipf)
    store, ptr, idx, val = store_of(rows, vocab)
    dead = rng.choice(n, 200, replace=False)
    store.delete_rows(dead)
    live = np.ones(n, bool)
    live[dead] = False
    counts, n_docs = H.df(ptr, idx, vocab, live)
    unused = int(np.setdiff1d(np.arange(vocab), SC.used_indices(rows))[0])  # a query index with df = 0: idf = log(1 + (n + 0.5) / 0.5), no hit from it
    assert counts[unused] == 0
    queries = [SC.random_query(rng, vocab, L, pool=pool) for L in (1, 6, 30)] + [(SC.u32(unused, int(pool[0])), SC.f32(1.0, 1.0)), (SC.u32(), SC.f32())]
    scaled = H.idf_queries(queries, counts, n_docs)
    assert scaled[3][1][0] == np.float32(np.log(1.0 + (n_docs + 0.5) / 0.5))
    for take in (1, 0):
        exp = SR.query(ptr, idx, val, scaled, vocab, take, 20, keep=live)
        p = store.sparse_query(queries).idf()
        p = p.take_max(20) if take else p.take_min(20)
        same_lists(split(*p.collect_arrays()), exp, ("idf", vocab, take))
        p = store.sparse_query(scaled)  # ... which is the plain query with the scaled weights
        p = p.take_max(20) if take else p.take_min(20)
        same_lists(split(*p.collect_arrays()), exp, ("scaled", vocab, take))
    plain = SR.query(ptr, idx, val, queries, vocab, 1, 20, keep=live)
    with_idf = SR.query(ptr, idx, val, scaled, vocab, 1, 20, keep=live)
    assert any(not np.array_equal(a["index"], b["index"]) for a, b in zip(plain, with_idf)), "idf must show in a ranking"
    store.close()


def test_worker_threads_answer_as_the_serial_run(oracle):
    """eight threads beside one another on one store whose document frequencies are NOT built yet: hybrid and IDF queries, every call
    returns what it returns alone, and the counts were built once"""
    rng = np.random.default_rng(8)
    n, dim, vocab = 2000, 8, 300
    dense_rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    dense_rows[np.all(dense_rows == 0, axis=1)] = 1.0
    rows = SC.random_rows(rng, n, vocab, 8)
    store = VecStore(dim)
    store.add_vectors(dense_rows)
    ptr, idx, val = SR.csr(rows)
    store.set_sparse(ptr, idx, val, vocab)
    counts, n_docs = H.df(ptr, idx, vocab)
    jobs = []
    for t in range(8):
        qs = [SC.random_query(rng, vocab, 5 + t) for _ in range(1 + t % 3)]
        scaled = H.idf_queries(qs, counts, n_docs)
        if t % 2:
            exp = SR.query(ptr, idx, val, scaled, vocab, 1, 15)
            jobs.append(("idf", store.sparse_query(qs).idf().take_max(15).resolve(), exp))
        else:
            legs = rng.integers(-2, 3, (2, dim)).astype(np.float32) + np.float32(0.5)
            fusion = (R.RRF, R.DBSF, R.MINMAX)[t % 3]
            dl = R.leg_lists(oracle, dense_rows, legs, Metric.Euclidean, 0, 40, inv=store.inv_norms())
            sl = H.sparse_lists(ptr, idx, val, scaled, vocab, 40)
            exp = H.hybrid(dl, sl, [2], [len(qs)], 0, fusion, 12)
            p = store.hybrid([legs], [qs], Metric.Euclidean).idf().fetch(40).take(12)
            p = p.rrf() if fusion == R.RRF else p.dbsf() if fusion == R.DBSF else p.min_max()
            jobs.append(("hybrid", p.resolve(), exp))
    errors = []
    start = threading.Barrier(len(jobs))

    def check(kind, resolved, exp, where):
        if kind == "idf":
            hits, cnt, _ = store._run_sparse(resolved)
            same_lists(split(hits, cnt), exp, where)
        else:
            hits, cnt, _ = store._run_hybrid(resolved)
            assert list(cnt) == list(exp[1]) and np.array_equal(hits["index"], exp[0]["index"]), where
            assert np.array_equal(hits["score"].view(np.uint32), exp[0]["score"].view(np.uint32)), where

    def work(t):
        try:
            start.wait()
            for _ in range(4):
                check(*jobs[t], ("thread", t))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(len(jobs))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert store.sparse_df_builds() == 1  # concurrent callers saw one build
    for t, job in enumerate(jobs):
        check(*job, ("serial", t))
    store.close()
