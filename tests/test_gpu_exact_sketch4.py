"""GPU: the four-bit sketch form of the pruned exact sweep (store options exact_prune = 1, exact_sketch, exact_sketch_bits = 4, the
default; DESIGN.md 3.1b, "four bits per dim").  Stores of the same rows in four forms — the four-bit sketch, the three-bit sketch,
no sketch (the 7/8 checkpoint) and the full sweep (exact_prune = 0) — return the same rows in the same order with the same score
bits, and all match the oracle.  The rows8 small-store kernel is switched off so that these stores take the streaming kernel the
pruned sweep lives in.  The shapes are the smallest at which the four-bit kernel can go wrong: a line of 3 (dim 96: header and
two stages), 8 (dim 256), 24 (dim 768), 25 (dim 773) and 28 pieces (dim 896: every ping-pong round of the streamed line), a short
last tile, an open gate, and a store whose line buffer ends exactly behind its last row.  The CPU half is
tests/test_exact_prune_sketch4_bound.py."""
import numpy as np
import pytest

import ieee_edges as E
from otters_amd import Cmp, Metric, Path, VecStore

pytestmark = pytest.mark.gpu

FORMS = (("4 bits", 1, 1, 4), ("3 bits", 1, 1, 3), ("7/8", 1, 0, 3), ("full", 0, 0, 3))  # name, exact_prune, exact_sketch, exact_sketch_bits


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
    if bits is not None:  # (None: the default form, which is the four-bit one)
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
        bits_equal(got, run(s, q, metric, take, k, filt, mask), ("4 bits/" + name,) + tuple(where))
    bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k, filt, mask), ("oracle",) + tuple(where))


def planted(rows, q, rng):
    """a few rows near the query (the gate closes early) and copies of one of them on both sides of the seed boundary (a tenth of
    the rows), so that equal scores sit at the k-th place"""
    n, dim = rows.shape
    near = rng.integers(0, n, 40)
    rows[near] = (q + rng.normal(0, 0.8, (40, dim))).astype(np.float32)
    dup = rows[near[0]].copy()
    for r in (5, n // 10 - 1, n // 10 + 3, n // 2, n - 1):
        rows[r] = dup


@pytest.fixture(scope="module")
def uniform_768():
    """40 000 x 768 uniform rows and nothing planted: the gate is the uniform rows' own"""
    rng = np.random.default_rng(99)
    rows = rng.uniform(-1, 1, (40_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    stores = four(rows)
    yield rows, q, stores
    close(*stores)


@pytest.mark.parametrize("k", [1, 10, 64, 100, 512])
def test_uniform_rows_at_every_list_width(oracle, uniform_768, k):
    """k = 1, 10 | 64 (the block code) | 100 | 512: the list widths of the pruned kernel; cosine and dot, Max and Min"""
    rows, q, stores = uniform_768
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            hold(oracle, stores, rows, q, metric, take, k, where=(metric, take, k))


def test_the_four_bit_form_is_the_one_that_runs(uniform_768):
    """the count of finished tails is the same on every run of a store (tiles go to waves in a fixed order), differs between the
    four-bit and the three-bit sketch, and is lower with four bits although its checkpoint is at stage 1 instead of 9 (the float64
    model of tests/test_exact_prune_sketch4_bound.py at the low gate of a 4032-row seed).  The default form is the four-bit one:
    a store that sets no exact_sketch_bits counts the same tails.  bytes_scanned stays algorithmic: the same in every form"""
    rows, q, stores = uniform_768
    ref = run(stores[3], q, Metric.Cosine, 1, 10)
    full_bytes = stores[3].last_stats["bytes_scanned"]
    assert stores[3].last_stats["rescored"] == 0
    default = make_store(rows, 1, 1, None)
    counts = {}
    for name, s in (("4 bits", stores[0]), ("3 bits", stores[1]), ("default", default)):
        counts[name] = []
        for _ in range(2):
            bits_equal(run(s, q, Metric.Cosine, 1, 10), ref, name)
            counts[name].append(s.last_stats["rescored"])
            assert s.last_stats["bytes_scanned"] == full_bytes > 0
            assert s.last_stats["path_used"] == int(Path.Exact)
    default.close()
    print("finished tails of", rows.shape[0] - 4032, "gated rows:", counts)
    for name in counts:
        assert counts[name][0] == counts[name][1], counts
        assert 0 < counts[name][0] < rows.shape[0] - 4032, counts  # (the seed's 4032 rows have no checkpoint)
    assert counts["4 bits"][0] != counts["3 bits"][0], counts
    assert counts["4 bits"][0] < counts["3 bits"][0], counts
    assert counts["default"][0] == counts["4 bits"][0], counts


@pytest.mark.parametrize("dim", [96, 256, 773, 896])
def test_line_lengths_and_a_short_last_tile(oracle, dim):
    """20 000 rows (312 tiles and one of 32 rows): 96 = 3 stages, a sketch by option only; 256 = 8 stages; 773 = 25 stages and a
    remainder term; 896 = 28 stages, the widest query a launch carries and the longest line.  A filter and a row mask as well"""
    rng = np.random.default_rng(dim)
    rows = rng.uniform(-1, 1, (20_000, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    planted(rows, q, rng)
    stores = four(rows)
    mask = rng.random(rows.shape[0]) < 0.7
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 64):
                hold(oracle, stores, rows, q, metric, take, k, where=(dim, metric, take, k))
            hold(oracle, stores, rows, q, metric, take, 10, (0.0, Cmp.Gt if take else Cmp.Lt), None, (dim, metric, take, "filter"))
            hold(oracle, stores, rows, q, metric, take, 10, None, mask, (dim, metric, take, "mask"))
    run(stores[0], q, Metric.Cosine, 1, 10)
    assert 0 < stores[0].last_stats["rescored"] < rows.shape[0]
    close(*stores)


def test_filter_passing_fewer_than_k(oracle):
    """the seed lists fewer than k rows: the gate stays open, no line is fetched, nothing is dropped — every gated row is finished"""
    rng = np.random.default_rng(5)
    rows = rng.uniform(-1, 1, (30_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    planted(rows, q, rng)
    stores = four(rows)
    for metric in (Metric.Cosine, Metric.DotProduct):
        filt = (0.3 if metric == Metric.Cosine else 60.0, Cmp.Gt)
        assert oracle_ref(oracle, rows, q, metric, 1, 64, filt).size < 64
        hold(oracle, stores, rows, q, metric, 1, 64, filt, where=(metric,))
        for s in stores[:3]:
            run(s, q, metric, 1, 64, filt)
            assert s.last_stats["rescored"] == rows.shape[0] - 3008, s.last_stats  # (the seed: a tenth of the rows, whole tiles)
    close(*stores)


def test_lines_follow_appends_and_reallocations(oracle):
    """30 011 x 768 rows appended in several calls without a reserve: every growth step reallocates, the lines are copied like the
    inverse norms"""
    rng = np.random.default_rng(31)
    rows = rng.uniform(-1, 1, (30_011, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    planted(rows, q, rng)
    pieces = [1, 700, 63, 5000, 1300, 9000, 13_947]
    sk = make_store(rows, 1, 1, 4, pieces=pieces)
    no = make_store(rows, 1, 0, 4, pieces=pieces)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 64):
                got = run(sk, q, metric, take, k)
                bits_equal(got, run(no, q, metric, take, k), ("4 bits/7-8", metric, take, k))
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), ("oracle", metric, take, k))
    run(sk, q, Metric.Cosine, 1, 10)
    assert 0 < sk.last_stats["rescored"] < rows.shape[0]
    close(sk, no)


def test_lines_move_between_the_shards_of_a_store(oracle):
    """two shards on one device; appended in two pieces, so that rows — and their lines — move between the shards"""
    rng = np.random.default_rng(13)
    rows = rng.uniform(-1, 1, (30_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    planted(rows, q, rng)
    sk = make_store(rows, 1, 1, 4, devices=[0, 0], pieces=[20_000, 10_000])
    one = make_store(rows, 1, 1, 4, devices=[0, 0])
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            ref = oracle_ref(oracle, rows, q, metric, take, 10)
            bits_equal(run(sk, q, metric, take, 10), ref, ("pieces", metric, take))
            bits_equal(run(one, q, metric, take, 10), ref, ("one append", metric, take))
    close(sk, one)


def test_lines_are_made_again_after_a_compaction(oracle):
    """1 % of the rows deleted, then compacted: the store answers as a fresh store of the survivors, and finishes the same tails"""
    rng = np.random.default_rng(19)
    rows = rng.uniform(-1, 1, (40_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    planted(rows, q, rng)
    dead = np.random.default_rng(4).choice(rows.shape[0], rows.shape[0] // 100, replace=False)
    keep = np.ones(rows.shape[0], bool)
    keep[dead] = False
    store = make_store(rows, 1, 1, 4)
    store.delete_rows(dead)
    for metric in (Metric.Cosine, Metric.DotProduct):  # deleted rows keep their lines; the live mask hides them
        bits_equal(run(store, q, metric, 1, 10), oracle_ref(oracle, rows, q, metric, 1, 10, None, keep), ("deleted", metric))
    store.compact()
    fresh = make_store(rows[keep], 1, 1, 4)
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
    """the line buffer holds exactly n lines and ends on a 2 MiB boundary (2^17 rows; a 48-B line at dim 96: the header and two
    stages, a 128-B line at dim 256: the header and seven): the kernel asks for eight pieces and more of every line, clamped to
    the pieces the line has, and reads not a byte more, the store's last row included"""
    n = 1 << 17
    rng = np.random.default_rng(dim)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows[n - 1] = q * 0.5   # the last row is a top hit: its line is read, and then its tail
    store = VecStore(dim)
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", 1)
    store.set_option("exact_sketch", 1)
    store.set_option("exact_sketch_bits", 4)
    store.reserve(n)
    store.add_vectors(rows[:n // 2])
    store.add_vectors(rows[n // 2:])
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            ref = oracle_ref(oracle, rows, q, metric, take, 10)
            bits_equal(run(store, q, metric, take, 10), ref, (dim, metric, take))
            assert 0 < store.last_stats["rescored"] < n, (dim, store.last_stats)
            if take and metric == Metric.Cosine:
                assert int(ref["index"][0]) == n - 1
    store.close()


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


def test_seed_rule_on_a_large_store():
    """1.4M x 256 rows, a tenth of which is more than 131072.  A filter that nothing passes leaves the gate open, so `rescored` is
    the rows behind the seed: 131072 rows up to k = 64 (1.4M / 32 is below that floor), the tenth in whole tiles from k = 65: the
    four-bit store takes the small seed as the three-bit one does.  And a query that does prune returns the full sweep's bits"""
    n = 1_400_000
    store = VecStore(256)
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", 1)
    store.set_option("exact_sketch", 1)
    store.set_option("exact_sketch_bits", 4)
    store.append_random(n, 14)
    q = np.random.default_rng(14).uniform(-1, 1, 256).astype(np.float32)
    for k, seed in ((10, 131072), (64, 131072), (65, 140032), (512, 140032)):
        for _ in range(2):
            got = store.query(q, Metric.Cosine).filter(2.0, Cmp.Gt).take_max(k).with_path(Path.Exact).collect_arrays()[0]
            assert got.size == 0
            assert store.last_stats["rescored"] == n - seed, (k, store.last_stats)
    for k in (10, 65):
        for metric in (Metric.Cosine, Metric.DotProduct):
            store.set_option("exact_prune", 0)
            ref = run(store, q, metric, 1, k)
            assert store.last_stats["rescored"] == 0
            store.set_option("exact_prune", 1)
            counts = []
            for _ in range(2):
                bits_equal(run(store, q, metric, 1, k), ref, ("1.4M", metric, k))
                counts.append(store.last_stats["rescored"])
            assert counts[0] == counts[1] and 0 < counts[0] <= n - (131072 if k <= 64 else 140032), (k, counts)
    store.close()
