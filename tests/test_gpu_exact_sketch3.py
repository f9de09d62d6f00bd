"""GPU: the three-bit sketch form of the pruned exact sweep (store options exact_prune = 1, exact_sketch, exact_sketch_bits;
DESIGN.md 3.1b).  Four stores of the same rows — the three-bit sketch (the default), the sign sketch (exact_sketch_bits = 1), no
sketch (the 7/8 checkpoint) and the full sweep (exact_prune = 0) — return the same rows in the same order with the same score
bits, and all match the oracle.  The rows8 small-store kernel is switched off so that these stores take the streaming kernel the
pruned sweep lives in.  The CPU half is tests/test_exact_prune_sketch3_bound.py."""
import numpy as np
import pytest

import ieee_edges as E
from otters_amd import Cmp, Metric, Path, VecStore

pytestmark = pytest.mark.gpu

FORMS = (("3 bits", 1, 1, 3), ("1 bit", 1, 1, 1), ("7/8", 1, 0, 3), ("full", 0, 0, 3))  # name, exact_prune, exact_sketch, exact_sketch_bits


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"], ref["query"]), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def make_store(rows, prune, sketch, bits, devices=None, pieces=None, reserve=False):
    """pieces: the rows go in with several appends of these sizes (no reserve: the store reallocates as it grows)"""
    store = VecStore(rows.shape[1], devices=devices) if devices else VecStore(rows.shape[1])
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", prune)
    store.set_option("exact_sketch", sketch)
    store.set_option("exact_sketch_bits", bits)
    if devices:
        store.set_option("multi_min_shard_rows", 0)
    if reserve:
        store.reserve(rows.shape[0])
    at = 0
    for n in (pieces or [rows.shape[0]]):
        store.add_vectors(rows[at:at + n])
        at += n
    assert at == rows.shape[0]
    return store


def four(rows, **kw):
    return [make_store(rows, p, s, b, **kw) for _, p, s, b in FORMS]


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


def hold(oracle, stores, rows, q, metric, take, k, filt=None, mask=None, where=()):
    """every form against the first, and the first against the oracle"""
    got = run(stores[0], q, metric, take, k, filt, mask)
    for (name, *_), s in zip(FORMS[1:], stores[1:]):
        bits_equal(got, run(s, q, metric, take, k, filt, mask), ("3 bits/" + name,) + tuple(where))
    bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k, filt, mask), ("oracle",) + tuple(where))


@pytest.mark.parametrize("dim", [256, 768, 773, 896, 1000])
def test_four_forms_hold_each_other_and_the_oracle(oracle, dim):
    """cosine and dot, Max and Min, k in 1, 10 and 64 (at dim 768 also 200 and 512: the wide lists), a ragged last tile (40 003
    rows), a filter, a row mask.  256: 8 stages, the checkpoint at stage 3; 773: 25 stages and a remainder term; 896: the widest
    query a launch carries; 1000: not pruned"""
    rows, q = corpus(40_003, dim, dim)
    stores = four(rows)
    rng = np.random.default_rng(3)
    mask = rng.random(rows.shape[0]) < 0.7
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 64) + ((200, 512) if dim == 768 else ()):
                for filt, m in ((None, None), ((0.0, Cmp.Gt if take else Cmp.Lt), None), (None, mask)):
                    hold(oracle, stores, rows, q, metric, take, k, filt, m, (dim, metric, take, k, filt is not None, m is not None))
    run(stores[0], q, Metric.Cosine, 1, 10)
    if dim <= 896:
        assert 0 < stores[0].last_stats["rescored"] < rows.shape[0]
    else:  # (the pruned sweep takes queries of up to 896 dims, the ones a launch carries in its arguments)
        assert stores[0].last_stats["rescored"] == 0
    close(*stores)


def test_with_a_chunk_mask_of_two_runs(oracle):
    """a chunk mask that leaves two runs of chunks (the single-query launch carries up to two)"""
    rows, q = corpus(40_000, 768, 8)
    stores = four(rows)
    n_chunks = (rows.shape[0] + 1023) // 1024
    keep = np.ones(n_chunks, bool)
    keep[7:19] = False
    rmask = np.repeat(keep, 1024)[:rows.shape[0]]
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            got = []
            for s in stores:
                plan = s.query(q, metric)
                plan = (plan.take_max(10) if take else plan.take_min(10)).with_path(Path.Exact)
                got.append(s._run(plan.resolve(), chunk_mask=keep)[0])  # (the call MetaStore makes with its zone-map mask)
            for (name, *_), g in zip(FORMS[1:], got[1:]):
                bits_equal(got[0], g, ("3 bits/" + name, metric, take))
            bits_equal(got[0], oracle_ref(oracle, rows, q, metric, take, 10, None, rmask), ("oracle", metric, take))
    close(*stores)


def test_filter_passing_fewer_than_k(oracle):
    """the seed lists fewer than k rows: the gate stays open, no line is fetched, nothing is dropped — every gated row is finished"""
    rows, q = corpus(30_000, 768, 5)
    stores = four(rows)
    for metric in (Metric.Cosine, Metric.DotProduct):
        filt = (0.3 if metric == Metric.Cosine else 60.0, Cmp.Gt)
        assert oracle_ref(oracle, rows, q, metric, 1, 64, filt).size < 64
        hold(oracle, stores, rows, q, metric, 1, 64, filt, where=(metric,))
        for s in stores[:3]:
            run(s, q, metric, 1, 64, filt)
            assert s.last_stats["rescored"] == rows.shape[0] - 3008, s.last_stats  # (the seed: a tenth of the rows, whole tiles)
    close(*stores)


@pytest.mark.parametrize("dim", [768, 773])
def test_lines_follow_appends_and_reallocations(oracle, dim):
    """rows appended in several calls without a reserve: every growth step reallocates, the wide lines are copied like the inverse norms"""
    rows, q = corpus(30_011, dim, 31)
    pieces = [1, 700, 63, 5000, 1300, 9000, 13_947]
    sk = make_store(rows, 1, 1, 3, pieces=pieces)
    no = make_store(rows, 1, 0, 3, pieces=pieces)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 64):
                got = run(sk, q, metric, take, k)
                bits_equal(got, run(no, q, metric, take, k), ("3 bits/7-8", metric, take, k))
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), ("oracle", metric, take, k))
    run(sk, q, Metric.Cosine, 1, 10)
    assert 0 < sk.last_stats["rescored"] < rows.shape[0]
    close(sk, no)


def test_lines_move_between_the_shards_of_a_store(oracle):
    """two shards; appended in two pieces, so that rows — and their sketch lines — move between the shards.  (A shard answers into
    device memory, where the count of finished tails is not read back: `rescored` is 0 on such a store in every form, so the
    results are what this case can hold)"""
    rows, q = corpus(30_000, 768, 13)
    sk = make_store(rows, 1, 1, 3, devices=[0, 0], pieces=[20_000, 10_000])
    one = make_store(rows, 1, 1, 3, devices=[0, 0])
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            ref = oracle_ref(oracle, rows, q, metric, take, 10)
            bits_equal(run(sk, q, metric, take, 10), ref, ("pieces", metric, take))
            bits_equal(run(one, q, metric, take, 10), ref, ("one append", metric, take))
    close(sk, one)


def test_lines_are_made_again_after_a_compaction(oracle):
    """1 % of the rows deleted, then compacted: the store answers as a fresh store of the survivors, and still prunes"""
    rows, q = corpus(40_000, 768, 19)
    rng = np.random.default_rng(4)
    dead = rng.choice(rows.shape[0], rows.shape[0] // 100, replace=False)
    keep = np.ones(rows.shape[0], bool)
    keep[dead] = False
    store = make_store(rows, 1, 1, 3)
    store.delete_rows(dead)
    for metric in (Metric.Cosine, Metric.DotProduct):  # deleted rows keep their lines; the live mask hides them
        bits_equal(run(store, q, metric, 1, 10), oracle_ref(oracle, rows, q, metric, 1, 10, None, keep), ("deleted", metric))
    store.compact()
    fresh = make_store(rows[keep], 1, 1, 3)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 64):
                got = run(store, q, metric, take, k)
                bits_equal(got, run(fresh, q, metric, take, k), ("compacted/fresh", metric, take, k))
                bits_equal(got, oracle_ref(oracle, rows[keep], q, metric, take, k), ("oracle", metric, take, k))
    run(store, q, Metric.Cosine, 1, 10)
    run(fresh, q, Metric.Cosine, 1, 10)
    assert 0 < store.last_stats["rescored"] == fresh.last_stats["rescored"] < int(keep.sum())
    close(store, fresh)


@pytest.mark.parametrize("dim", [96, 256])
def test_the_line_ends_with_a_store_reserved_to_exactly_its_rows(oracle, dim):
    """the sketch buffer holds exactly n lines and ends on a 2 MiB boundary (2^17 rows; a 32-B line at dim 96: two stages of three
    words, a 64-B line at dim 256: five): the kernel reads the pieces a line has and not a byte more, the store's last row
    included.  Dim 96 keeps a sketch by option only, dim 256 (eight stages) by the automatic rule too"""
    n = 1 << 17
    rng = np.random.default_rng(dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows[n - 1] = q * 0.5   # the last row is a top hit: its line is read, and then its tail
    stores = []
    for sketch in (1, -1) if dim >= 256 else (1,):
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
            for store in stores:
                got = run(store, q, metric, take, 10)
                bits_equal(got, ref, (dim, metric, take))
                assert 0 < store.last_stats["rescored"] < n, (dim, store.last_stats)
            if take and metric == Metric.Cosine:
                assert int(ref["index"][0]) == n - 1
    close(*stores)


def test_ieee_edge_rows(oracle):
    """signed-zero, subnormal and overflowing rows among uniform ones (tests/ieee_edges.py), and six rows with NaN, +-inf, +-0 or
    3e38 in the tail: such rows are never dropped on a bound they break"""
    rng = np.random.default_rng(21)
    dim = 768
    parts = [E.signed_zero_cosines(rng, 40, dim), E.subnormal_sums(rng, 64, dim), E.overflow(rng, 48, dim)]
    edge = np.concatenate([p[0] for p in parts]).astype(np.float32)
    rows = rng.uniform(-1, 1, (20_000, dim)).astype(np.float32)
    at = rng.choice(20_000, edge.shape[0], replace=False)
    rows[at] = edge
    rows[rng.choice(20_000, 6, replace=False), -5] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 3e38]  # ... and tails the sketch cannot hold
    queries = np.concatenate([rng.uniform(-1, 1, (3, dim)).astype(np.float32)] + [p[1][:2] for p in parts])
    stores = four(rows)
    for qi, q in enumerate(queries):
        for metric in (Metric.Cosine, Metric.DotProduct):
            for take in (1, 0):
                hold(oracle, stores, rows, q, metric, take, 10, where=(qi, metric, take))
    close(*stores)


def test_the_wide_form_is_the_one_that_runs():
    """40 000 uniform rows and nothing planted, so the gate is the uniform rows' own and the three bounds stop different rows: the
    count of finished tails is the same on every run of a store (tiles go to waves in a fixed order), differs between the three-bit
    sketch, the sign sketch and the 7/8 form, and is lowest with three bits (a float64 model of the 4032-row seed's low gate gives
    about a quarter of the rows against about three quarters).  bytes_scanned stays algorithmic: the same in every form"""
    rng = np.random.default_rng(99)
    rows = rng.uniform(-1, 1, (40_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    stores = four(rows)
    ref = run(stores[3], q, Metric.Cosine, 1, 10)
    full_bytes = stores[3].last_stats["bytes_scanned"]
    assert stores[3].last_stats["rescored"] == 0
    counts = {}
    for (name, *_), s in zip(FORMS[:3], stores[:3]):
        counts[name] = []
        for _ in range(2):
            bits_equal(run(s, q, Metric.Cosine, 1, 10), ref, name)
            counts[name].append(s.last_stats["rescored"])
            assert s.last_stats["bytes_scanned"] == full_bytes > 0
            assert s.last_stats["path_used"] == int(Path.Exact)
    print("finished tails of", rows.shape[0] - 4032, "gated rows:", counts)
    for name in counts:
        assert counts[name][0] == counts[name][1], counts
        assert 0 < counts[name][0] < rows.shape[0] - 4032, counts  # (the seed's 4032 rows have no checkpoint)
    assert len({c[0] for c in counts.values()}) == 3, counts
    assert counts["3 bits"][0] < counts["1 bit"][0], counts
    close(*stores)
