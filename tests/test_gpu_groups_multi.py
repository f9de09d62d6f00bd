"""GPU: grouped search on a multi-GPU store (four shards of this process on GPU 0).  Group ids are global and
routed by row range; every shard answers for its rows, the host merges the shards' lists by the canonical order and keeps each
group's first hit.  Same bar and same expectation as tests/test_gpu_groups.py: the oracle's canonical ranking, restricted, the
first hit of every group per query, cut at k — index, query, score bits, counts, no tolerances."""
import numpy as np
import pytest

from otters_amd import Cmp, Metric, OttersError, VecStore
from test_gpu_groups import ALL_METRICS, Rankings, bits_equal, build, expected, ranking

pytestmark = pytest.mark.gpu


def multi_store(dim, rows):
    store = VecStore(dim, devices=[0] * 4)
    store.set_option("multi_min_shard_rows", 0)  # (a store this small would stay on one shard: the tests want all four)
    store.reserve(rows.shape[0])
    store.add_vectors(rows)
    return store


def test_groups_that_straddle_the_shards(oracle):
    """5000 rows over four shards; 'striped' puts every group into every shard, 'halves' lets groups straddle one boundary, 'own'
    is the plain query; k below and above 512, a per-query batch, every metric"""
    n, dim = 5000, 24
    rng = np.random.default_rng(9100)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    store = multi_store(dim, rows)
    sh = store.shards()
    assert len(sh) == 4 and all(cnt > 0 for _, _, cnt in sh), sh
    keep = np.ones(n, bool)
    ranks = Rankings(oracle, rows, q)
    lay = {"striped": np.arange(n) % 1200, "halves": (np.arange(n) + 600) // 1250, "own": rng.permutation(n), "one": np.zeros(n, np.int64)}
    for lname, labels in lay.items():
        store.set_groups(labels)
        gid = np.unique(labels, return_inverse=True)[1].reshape(-1)
        assert store.group_count() == int(gid.max()) + 1
        for metric in ALL_METRICS:
            for nq in (1, 5):
                for k in (1, 10, 300, 512, 513, 700, None):
                    plan = build(store, q[:nq], metric, k, perq=nq > 1)
                    ref, ref_counts = expected(ranks.get(metric, nq, k), gid, keep, plan.resolve().k, nq)
                    got, counts = plan.collect_arrays()
                    bits_equal(got, ref, (lname, metric, nq, k))
                    assert list(counts) == ref_counts
    store.close()


def test_deleted_rows_masks_and_filters_on_the_shards(oracle):
    n, dim = 5000, 16
    rng = np.random.default_rng(9200)
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)  # quantised: ties across the shards
    q = rng.integers(-2, 3, (3, dim)).astype(np.float32)
    store = multi_store(dim, rows)
    gid = np.arange(n) % 900
    store.set_groups(gid)
    full1, full3 = ranking(oracle, rows, q[:1], Metric.DotProduct, 1), ranking(oracle, rows, q, Metric.DotProduct, 1)
    best = int(full1["index"][0])
    dead = np.unique(np.concatenate([[best], np.flatnonzero(gid == gid[int(full1["index"][40])]), rng.choice(n, 500)]))
    store.delete_rows(dead)
    alive = np.ones(n, bool)
    alive[dead] = False
    caller = rng.random(3000) < 0.6
    both = alive.copy()
    both[:3000] &= caller
    for nq, full in ((1, full1), (3, full3)):
        for k in (10, 600, None):
            ref, ref_counts = expected(full, gid, alive, k or 900, nq)
            got, counts = build(store, q[:nq], Metric.DotProduct, k, perq=nq > 1).collect_arrays()
            bits_equal(got, ref, ("deleted", nq, k))
            assert list(counts) == ref_counts
            ref, _ = expected(full, gid, both, k or 900, nq, int(Cmp.Gt), 1.0)
            got, _ = build(store, q[:nq], Metric.DotProduct, k, perq=nq > 1, mask=caller, flt=(1.0, Cmp.Gt)).collect_arrays()
            bits_equal(got, ref, ("deleted, mask, filter", nq, k))
    store.restore_rows(dead)
    ref, _ = expected(full1, gid, np.ones(n, bool), 10, 1)
    bits_equal(build(store, q[:1], Metric.DotProduct, 10).collect_arrays()[0], ref, "restored")
    # errors on the front
    with pytest.raises(OttersError, match="use PER_QUERY"):
        build(store, q, Metric.DotProduct, 5).collect()
    store.add_vectors(rows[:3])
    with pytest.raises(OttersError, match="rows were appended since"):
        build(store, q[:1], Metric.DotProduct, 5).collect()
    store.clear_groups()
    with pytest.raises(OttersError, match="no group ids are set"):
        build(store, q[:1], Metric.DotProduct, 5).collect()
    assert store.query(q[:1], Metric.DotProduct).take(3).collect_arrays()[0].size == 3
    store.close()
