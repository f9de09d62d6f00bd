"""GPU: the sketch form of the pruned exact sweep (store options exact_prune = 1, exact_sketch).  A store that keeps
the tail sign sketch (exact_sketch = 1), one that does not (0: the 7/8 checkpoint) and the full sweep (exact_prune = 0) return the
same rows in the same order with the same score bits, and all match the oracle.  The rows8 small-store kernel is switched off so
that these stores take the streaming kernel the pruned sweep lives in.  The CPU half is tests/test_exact_prune_sketch_bound.py."""
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


def make_store(rows, prune, sketch, devices=None, pieces=None):
    """pieces: the rows go in with several appends of these sizes (no reserve: the store reallocates as it grows)"""
    store = VecStore(rows.shape[1], devices=devices) if devices else VecStore(rows.shape[1])
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", prune)
    store.set_option("exact_sketch", sketch)
    if devices:
        store.set_option("multi_min_shard_rows", 0)
    at = 0
    for n in (pieces or [rows.shape[0]]):
        store.add_vectors(rows[at:at + n])
        at += n
    assert at == rows.shape[0]
    return store


def trio(rows, **kw):
    """with the sketch, without it (7/8 checkpoint), and the full sweep"""
    return make_store(rows, 1, 1, **kw), make_store(rows, 1, 0, **kw), make_store(rows, 0, 0, **kw)


def run(store, q, metric, take, k, filt=None, mask=None):
    p = store.query(q, metric)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    return (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact).collect_arrays()[0]


def corpus(n, dim, seed):
    """uniform rows, a few rows near the query (scores well above the uniform ones: the gate closes early), and copies of one of
    them on both sides of the seed boundary (a tenth of the rows) so that equal scores sit at the k-th place"""
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


def close(*stores):
    for s in stores:
        s.close()


@pytest.mark.parametrize("dim", [256, 768, 1000])
def test_sketch_equals_no_sketch_equals_full_sweep_and_oracle(oracle, dim):
    """cosine and dot, Max and Min, k in 1, 10 and 64, a ragged last tile (40 003 rows), a row mask"""
    rows, q = corpus(40_003, dim, dim)
    sk, no, full = trio(rows)
    rng = np.random.default_rng(3)
    mask = rng.random(rows.shape[0]) < 0.7
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 64):
                for filt, m in ((None, None), ((0.0, Cmp.Gt if take else Cmp.Lt), None), (None, mask)):
                    where = (dim, metric, take, k, filt is not None, m is not None)
                    got = run(sk, q, metric, take, k, filt, m)
                    bits_equal(got, run(no, q, metric, take, k, filt, m), ("sketch/7-8",) + where)
                    bits_equal(got, run(full, q, metric, take, k, filt, m), ("sketch/full",) + where)
                    bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k, filt, m), ("oracle",) + where)
    close(sk, no, full)


def test_sketch_with_a_chunk_mask(oracle):
    """a chunk mask that leaves two runs of chunks (the single-query launch carries up to two)"""
    rows, q = corpus(40_000, 768, 8)
    sk, no, full = trio(rows)
    n_chunks = (rows.shape[0] + 1023) // 1024
    keep = np.ones(n_chunks, bool)
    keep[7:19] = False
    rmask = np.repeat(keep, 1024)[:rows.shape[0]]
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            got = []
            for s in (sk, no, full):
                plan = s.query(q, metric)
                plan = (plan.take_max(10) if take else plan.take_min(10)).with_path(Path.Exact)
                got.append(s._run(plan.resolve(), chunk_mask=keep)[0])  # (the call MetaStore makes with its zone-map mask)
            bits_equal(got[0], got[1], ("sketch/7-8", metric, take))
            bits_equal(got[0], got[2], ("sketch/full", metric, take))
            bits_equal(got[0], oracle_ref(oracle, rows, q, metric, take, 10, None, rmask), ("oracle", metric, take))
    close(sk, no, full)


def test_sketch_filter_passing_fewer_than_k(oracle):
    """the seed lists fewer than k rows: the gate stays open, nothing is dropped"""
    rows, q = corpus(30_000, 768, 5)
    sk = make_store(rows, 1, 1)
    for metric in (Metric.Cosine, Metric.DotProduct):
        filt = (0.3 if metric == Metric.Cosine else 60.0, Cmp.Gt)
        ref = oracle_ref(oracle, rows, q, metric, 1, 64, filt)
        assert ref.size < 64
        bits_equal(run(sk, q, metric, 1, 64, filt), ref, metric)
    sk.close()


@pytest.mark.parametrize("dim", [768, 1000])
def test_sketch_follows_appends_and_reallocations(oracle, dim):
    """rows appended in several calls without a reserve: every growth step reallocates, the sketch is copied like the inverse norms"""
    rows, q = corpus(30_011, dim, 31)
    pieces = [1, 700, 63, 5000, 1300, 9000, 13_947]
    sk = make_store(rows, 1, 1, pieces=pieces)
    no = make_store(rows, 1, 0, pieces=pieces)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 64):
                got = run(sk, q, metric, take, k)
                bits_equal(got, run(no, q, metric, take, k), ("sketch/7-8", metric, take, k))
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), ("oracle", metric, take, k))
    run(sk, q, Metric.Cosine, 1, 10)
    if dim <= 896:  # (the pruned sweep takes queries of up to 896 dims, the ones a launch carries in its arguments; see the stats test)
        assert 0 < sk.last_stats["rescored"] < rows.shape[0]
    else:
        assert sk.last_stats["rescored"] == 0
    close(sk, no)


def test_sketch_on_a_multi_shard_store(oracle):
    """two shards; appended in pieces, so that rows — and their sketch lines — move between the shards"""
    rows, q = corpus(30_000, 768, 13)
    sk = make_store(rows, 1, 1, devices=[0, 0], pieces=[20_000, 10_000])
    one = make_store(rows, 1, 1, devices=[0, 0])
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            ref = oracle_ref(oracle, rows, q, metric, take, 10)
            bits_equal(run(sk, q, metric, take, 10), ref, ("pieces", metric, take))
            bits_equal(run(one, q, metric, take, 10), ref, ("one append", metric, take))
    close(sk, one)


def test_sketch_ieee_edge_rows(oracle):
    """signed-zero, subnormal and overflowing rows among uniform ones (tests/ieee_edges.py, as in test_gpu_exact_prune.py): such rows
    are never dropped on a bound they break"""
    rng = np.random.default_rng(21)
    dim = 768
    parts = [E.signed_zero_cosines(rng, 40, dim), E.subnormal_sums(rng, 64, dim), E.overflow(rng, 48, dim)]
    edge = np.concatenate([p[0] for p in parts]).astype(np.float32)
    rows = rng.uniform(-1, 1, (20_000, dim)).astype(np.float32)
    at = rng.choice(20_000, edge.shape[0], replace=False)
    rows[at] = edge
    rows[rng.choice(20_000, 6, replace=False), -5] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 3e38]  # ... and tails the sketch cannot hold
    queries = np.concatenate([rng.uniform(-1, 1, (3, dim)).astype(np.float32)] + [p[1][:2] for p in parts])
    sk, no, full = trio(rows)
    for qi, q in enumerate(queries):
        for metric in (Metric.Cosine, Metric.DotProduct):
            for take in (1, 0):
                got = run(sk, q, metric, take, 10)
                bits_equal(got, run(no, q, metric, take, 10), ("sketch/7-8", qi, metric, take))
                bits_equal(got, run(full, q, metric, take, 10), ("sketch/full", qi, metric, take))
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, 10), ("oracle", qi, metric, take))
    close(sk, no, full)


@pytest.mark.parametrize("dim", [96, 256])
def test_sketch_on_a_store_reserved_to_exactly_its_rows(oracle, dim):
    """the sketch buffer holds exactly n lines and ends on a 2 MiB boundary (2^17 rows, a 16-B line at both dims: one and two sign
    words): the kernel reads a row's line and not a byte more, the store's last row included.  Dim 96 keeps a sketch by option
    only, dim 256 (eight stages) by the automatic rule too"""
    n = 1 << 17
    rng = np.random.default_rng(dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows[n - 1] = q * 0.5   # the last row is a top hit: it is read in full, and its sketch line first
    stores = []
    for sketch in (1, -1, 0):
        store = VecStore(dim)
        store.set_option("exact_small", 0)
        store.set_option("exact_prune", 1)
        store.set_option("exact_sketch", sketch)
        store.reserve(n)
        store.add_vectors(rows[:n // 2])
        store.add_vectors(rows[n // 2:])
        stores.append(store)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            ref = oracle_ref(oracle, rows, q, metric, take, 10)
            for store, name in zip(stores, ("on", "automatic", "off")):
                bits_equal(run(store, q, metric, take, 10), ref, (name, dim, metric, take))
                assert 0 < store.last_stats["rescored"] < n, (name, dim, store.last_stats)
    close(*stores)


def test_sketch_form_is_the_one_that_runs():
    """uniform rows and nothing planted, so the gate is the uniform rows' own and the two bounds stop different rows: the count of
    finished tails of a store with a sketch differs from that of a store without one, which is the same on every run (tiles go to
    waves in a fixed order).  A sweep that fell back to the 7/8 checkpoint while the store keeps a sketch would count as the
    store without one does"""
    rng = np.random.default_rng(99)
    rows = rng.uniform(-1, 1, (40_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    sk, no, full = trio(rows)
    ref = run(full, q, Metric.Cosine, 1, 10)
    counts = {}
    for name, s in (("sketch", sk), ("7/8", no)):
        counts[name] = []
        for _ in range(2):
            bits_equal(run(s, q, Metric.Cosine, 1, 10), ref, name)
            counts[name].append(s.last_stats["rescored"])
    print("finished tails of", rows.shape[0] - 4032, "gated rows:", counts)
    for name in counts:
        assert counts[name][0] == counts[name][1], counts
        assert 0 < counts[name][0] < rows.shape[0] - 4032, counts  # (the seed's 4032 rows have no checkpoint)
    assert counts["sketch"][0] != counts["7/8"][0], counts
    close(sk, no, full)


def test_sketch_stats_finished_tails_and_bytes_scanned():
    """the kernel's count of finished tails (stats field `rescored` on the pruned sweep) is below the rows scored, with the sketch
    at a checkpoint two stages earlier too; bytes_scanned stays algorithmic: the same with the sketch, without it, and unpruned"""
    rows, q = corpus(40_000, 768, 17)
    sk, no, full = trio(rows)
    for s in (sk, no, full):
        run(s, q, Metric.Cosine, 1, 10)
    scored = sk.last_stats["vectors_compared"]
    assert scored == rows.shape[0]
    print("finished tails: sketch", sk.last_stats["rescored"], "7/8", no.last_stats["rescored"], "of", scored)
    assert 0 < sk.last_stats["rescored"] < scored
    assert 0 < no.last_stats["rescored"] < scored
    assert full.last_stats["rescored"] == 0
    assert sk.last_stats["bytes_scanned"] == no.last_stats["bytes_scanned"] == full.last_stats["bytes_scanned"] > 0
    assert sk.last_stats["path_used"] == no.last_stats["path_used"] == int(Path.Exact)
    close(sk, no, full)
