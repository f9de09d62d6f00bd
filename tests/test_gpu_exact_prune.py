"""GPU: the pruned exact sweep (store option exact_prune) returns what scoring every row returns — exact_prune = 1
(forced, on stores far below the automatic size) against exact_prune = 0 bit for bit, and both against the oracle.  The rows8 small-
store kernel is switched off (exact_small = 0) so that these stores take the streaming kernel the pruned sweep lives in."""
import numpy as np
import pytest

import ieee_edges as E
from otters_amd import Cmp, Metric, Path, VecStore

pytestmark = pytest.mark.gpu


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"], ref["query"]), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def make_store(rows, prune, devices=None, tie_order=None):
    store = VecStore(rows.shape[1], devices=devices) if devices else VecStore(rows.shape[1])
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", prune)
    if devices:
        store.set_option("multi_min_shard_rows", 0)
    if tie_order:
        store.set_tie_order(tie_order)
    store.add_vectors(rows)
    return store


def run(store, q, metric, take, k, filt=None, mask=None):
    p = store.query(q, metric)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    return (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact).collect_arrays()[0]


def corpus(n, dim, seed):
    """uniform rows, a few rows near the query (scores well above the uniform ones), and copies of one of them on both sides of
    the seed boundary (a tenth of the rows) so that equal scores sit at the k-th place"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    near = rng.integers(0, n, 40)
    rows[near] = (q + rng.normal(0, 0.8, (40, dim))).astype(np.float32)
    dup = rows[near[0]].copy()
    for r in (5, n // 10 - 1, n // 10 + 3, n // 2, n - 1):
        rows[r] = dup
    return rows, q


def oracle_ref(oracle, rows, q, metric, take, k, filt=None, mask=None):
    fc, ft = (int(filt[1]), filt[0]) if filt else (0, 0.0)
    return oracle.vec_query(rows, q, int(metric), take, k, fc, ft, row_mask=mask, ties=oracle.TIES_CANONICAL)


@pytest.mark.parametrize("dim", [768, 769, 200])
def test_prune_equals_full_sweep_and_oracle(oracle, dim):
    rows, q = corpus(40_000, dim, dim)
    on, off = make_store(rows, 1), make_store(rows, 0)
    rng = np.random.default_rng(3)
    mask = rng.random(rows.shape[0]) < 0.7
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 100, 512):
                for filt, m in ((None, None), ((0.0, Cmp.Gt), None), (None, mask)):
                    if take == 0 and filt is not None:
                        filt = (0.0, Cmp.Lt)
                    got = run(on, q, metric, take, k, filt, m)
                    bits_equal(got, run(off, q, metric, take, k, filt, m), ("on/off", dim, metric, take, k, filt is not None, m is not None))
                    if k in (10, 512):
                        bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k, filt, m), ("oracle", dim, metric, take, k))
    on.close()
    off.close()


def test_prune_filter_passing_fewer_than_k(oracle):
    """the seed lists fewer than k rows: the gate stays open, nothing is dropped"""
    rows, q = corpus(30_000, 768, 5)
    on = make_store(rows, 1)
    for metric in (Metric.Cosine, Metric.DotProduct):
        ref = oracle_ref(oracle, rows, q, metric, 1, 100, (0.3 if metric == Metric.Cosine else 60.0, Cmp.Gt))
        assert ref.size < 100
        bits_equal(run(on, q, metric, 1, 100, (0.3 if metric == Metric.Cosine else 60.0, Cmp.Gt)), ref, metric)
    on.close()


@pytest.mark.parametrize("tie_order", ["canonical", "reference"])
def test_prune_ties_across_the_seed_boundary(tie_order):
    """many rows tied at the k-th score, in the seed and behind it: every tie order picks the same rows with and without pruning"""
    rng = np.random.default_rng(9)
    rows = rng.uniform(-1, 1, (20_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    top = (q * 0.9).astype(np.float32)
    rows[rng.choice(20_000, 30, replace=False)] = top
    on, off = make_store(rows, 1, tie_order=tie_order), make_store(rows, 0, tie_order=tie_order)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for k in (10, 25, 100):
            bits_equal(run(on, q, metric, 1, k), run(off, q, metric, 1, k), (tie_order, metric, k))
    on.close()
    off.close()


def test_prune_ieee_edge_rows(oracle):
    """signed-zero, subnormal and overflowing rows among uniform ones (tests/ieee_edges.py): such rows are never dropped on a
    bound they break"""
    rng = np.random.default_rng(21)
    dim = 768
    parts = [E.signed_zero_cosines(rng, 40, dim), E.subnormal_sums(rng, 64, dim), E.overflow(rng, 48, dim)]
    edge = np.concatenate([p[0] for p in parts]).astype(np.float32)
    rows = rng.uniform(-1, 1, (20_000, dim)).astype(np.float32)
    at = rng.choice(20_000, edge.shape[0], replace=False)
    rows[at] = edge
    queries = np.concatenate([rng.uniform(-1, 1, (3, dim)).astype(np.float32)] + [p[1][:2] for p in parts])
    on, off = make_store(rows, 1), make_store(rows, 0)
    for qi, q in enumerate(queries):
        for metric in (Metric.Cosine, Metric.DotProduct):
            for take in (1, 0):
                got = run(on, q, metric, take, 10)
                bits_equal(got, run(off, q, metric, take, 10), ("on/off", qi, metric, take))
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, 10), ("oracle", qi, metric, take))
    on.close()
    off.close()


def test_prune_on_a_multi_shard_store(oracle):
    rows, q = corpus(30_000, 768, 13)
    on = make_store(rows, 1, devices=[0, 0])
    for metric in (Metric.Cosine, Metric.DotProduct):
        bits_equal(run(on, q, metric, 1, 10), oracle_ref(oracle, rows, q, metric, 1, 10), metric)
    on.close()


def test_prune_reads_fewer_rows_than_it_scores_and_reports_the_full_scan():
    """the option is live: the same bytes_scanned (algorithmic) with and without it"""
    rows, q = corpus(20_000, 768, 17)
    on, off = make_store(rows, 1), make_store(rows, 0)
    run(on, q, Metric.Cosine, 1, 10)
    run(off, q, Metric.Cosine, 1, 10)
    assert on.last_stats["bytes_scanned"] == off.last_stats["bytes_scanned"] > 0
    on.close()
    off.close()
