"""GPU: the pruned exact sweep on stores where every wave takes several tiles, where the tile a wave takes next is
not the next of its stride, and where its queue of survivors fills every tile or two; and the seed rule of run_exact on both
sides of each of its boundaries.  The stores are sized from the device.  The reference of every case is the SAME store queried
with exact_prune = 0 (the full sweep): indices, order and score bits are equal.  Every pruned query runs twice: same hits, same
count of finished tails."""
import numpy as np
import pytest

from otters_amd import Cmp, Metric, Path, VecStore

pytestmark = pytest.mark.gpu


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"], ref["query"]), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def new_store(dim, prune=1):
    store = VecStore(dim)
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", prune)
    store.set_option("exact_sketch", 1)
    store.set_option("exact_sketch_bits", 3)
    return store


def run(store, q, metric, take, k, mask=None, chunk_mask=None):
    p = store.query(q, metric)
    if mask is not None:
        p = p.with_row_mask(mask)
    p = (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact)
    if chunk_mask is not None:
        hits, _, stats = store._run(p.resolve(), chunk_mask=chunk_mask)  # (the call MetaStore makes with its zone-map mask)
        return hits, stats["rescored"]
    hits = p.collect_arrays()[0]
    return hits, store.last_stats["rescored"]


def pruned_twice_against_full(store, q, metric, take, k, where, prune=1, **kw):
    """-> the count of finished tails of the pruned query (the same on both runs)"""
    store.set_option("exact_prune", 0)
    ref, finished = run(store, q, metric, take, k, **kw)
    assert finished == 0, where
    store.set_option("exact_prune", prune)
    counts = []
    for _ in range(2):
        got, finished = run(store, q, metric, take, k, **kw)
        bits_equal(got, ref, where)
        counts.append(finished)
    assert counts[0] == counts[1], (where, counts)
    return counts[0]


def ceil64(n):
    return (n + 63) // 64 * 64


def seed_rows(n, k=10):
    """the seed rule of run_exact for a store with the three-bit sketch: a tenth of the rows; up to k = 64, once that is more
    than 131072 rows, a thirty-second of them but never fewer than 131072; whole tiles"""
    s = n // 10
    if k <= 64 and s > 131072:
        s = max(n // 32, 131072)
    return ceil64(s)


def waves():
    """the waves of a persistent grid of three workgroups per CU: more than the two per CU that run, so that with three tiles for
    each of these every wave of the real grid takes at least four"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 3 * 4


@pytest.fixture(scope="module")
def main_store():
    """three tiles for each of waves() and a ragged last tile; dim 256: 8 stages, the checkpoint at stage 3"""
    n = waves() * 64 * 3 + 37
    store = new_store(256)
    store.append_random(n, 0x5EED)
    yield store, n
    store.close()


@pytest.mark.parametrize("k", [1, 10, 17, 64, 100, 512])
def test_main_store(main_store, k):
    """k = 1, 10 | 17, 64 (the block code) | 100 | 512: the four list widths of the pruned kernel"""
    store, n = main_store
    rng = np.random.default_rng(k)
    q = rng.uniform(-1, 1, 256).astype(np.float32)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            got = pruned_twice_against_full(store, q, metric, take, k, (n, metric, take, k))
            print("main", n, metric, take, k, "finished tails", got)
            assert 0 < got <= n - seed_rows(n, k), (got, n, seed_rows(n, k))


@pytest.mark.parametrize("n,dim", [(300_000, 768), (200_000, 773)])
def test_real_line_length_and_a_remainder_dim(n, dim):
    store = new_store(dim)
    store.append_random(n, dim)
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (10, 100):
                got = pruned_twice_against_full(store, q, metric, take, k, (n, dim, metric, take, k))
                assert 0 < got <= n - seed_rows(n, k), (got, n)
    store.close()


def test_one_tile_per_wave_and_the_oracle(oracle):
    """40 000 x 768: 625 tiles, at most one per wave — no wave has a next tile.  The top-10 is held to the CPU oracle too"""
    rng = np.random.default_rng(40)
    rows = rng.uniform(-1, 1, (40_000, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    store = new_store(768)
    store.add_vectors(rows)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            got = pruned_twice_against_full(store, q, metric, take, 10, (metric, take))
            assert 0 < got < rows.shape[0]
            ref = oracle.vec_query(rows, q, int(metric), take, 10, 0, 0.0, ties=oracle.TIES_CANONICAL)
            bits_equal(run(store, q, metric, take, 10)[0], ref, ("oracle", metric, take))
    store.close()


def test_seed_rule_keeps_the_tenth_on_small_stores():
    """30 000 rows: the seed is a tenth, 3008 rows in whole tiles; a filter that nothing passes leaves the gate open, so every
    other row's tail is finished"""
    store = new_store(768)
    store.append_random(30_000, 3)
    q = np.random.default_rng(3).uniform(-1, 1, 768).astype(np.float32)
    for _ in range(2):
        got = store.query(q, Metric.Cosine).filter(2.0, Cmp.Gt).take_max(64).with_path(Path.Exact).collect_arrays()[0]
        assert got.size == 0
        assert store.last_stats["rescored"] == 30_000 - 3008, store.last_stats
    store.close()


def finished_with_an_open_gate(store, q, k):
    """a filter that nothing passes: the seed lists nothing, the gate stays open and every row behind the seed is finished; twice"""
    out = []
    for _ in range(2):
        got = store.query(q, Metric.Cosine).filter(2.0, Cmp.Gt).take_max(k).with_path(Path.Exact).collect_arrays()[0]
        assert got.size == 0
        out.append(store.last_stats["rescored"])
    assert out[0] == out[1], out
    return out[0]


def test_seed_rule_on_a_large_store():
    """1.4M x 256 rows, a tenth of which is more than 131072.  Open gate, so `rescored` is the rows behind the seed: the floor of
    131072 rows up to k = 64 (1.4M / 32 is below it), the tenth in whole tiles from k = 65.  Grown to 4 200 037 rows the
    thirty-second rules (131 251 -> 131 264 rows in whole tiles).  Without the three-bit sketch the tenth stays at every k.  And
    a query that does prune returns the full sweep's bits at k = 64 and 65"""
    n = 1_400_000
    store = new_store(256)
    store.append_random(n, 14)
    q = np.random.default_rng(14).uniform(-1, 1, 256).astype(np.float32)
    assert seed_rows(n, 64) == 131072 and seed_rows(n, 65) == ceil64(n // 10) == 140032
    for k in (1, 10, 64):
        assert finished_with_an_open_gate(store, q, k) == n - 131072, k
    for k in (65, 100, 512):
        assert finished_with_an_open_gate(store, q, k) == n - 140032, k
    for k in (10, 64, 65):
        for metric in (Metric.Cosine, Metric.DotProduct):
            got = pruned_twice_against_full(store, q, metric, 1, k, ("1.4M", metric, k))
            assert 0 < got <= n - seed_rows(n, k), (got, k)
    store.set_option("exact_sketch", 0)  # (the lines are ignored: the form without a sketch, checkpoint at 7/8, keeps the tenth)
    assert finished_with_an_open_gate(store, q, 10) == n - 140032
    store.close()
    # the last store whose tenth is not above 131072 rows, the first whose tenth is, and one where the thirty-second rules
    for n, seed in ((1_310_719, ceil64(131071)), (1_310_730, 131072), (4_200_037, 131264)):
        store = new_store(256)
        store.append_random(n, n)
        assert seed_rows(n, 10) == seed
        assert finished_with_an_open_gate(store, q, 10) == n - seed, (n, seed)
        assert finished_with_an_open_gate(store, q, 100) == n - ceil64(n // 10), n
        store.close()


def test_queues_fill_every_tile_or_two():
    """the gate stays open or low, so a wave's queue reaches 64 rows every tile or two and survivors are finished between the
    tiles all through the sweep.  (i) a row mask leaves the seed 50 rows, fewer than k = 64: the seed's gate is open and a
    wave's own gate, from its first 64 rows, is low; (ii) one tight cluster queried with one of its rows: most rows survive"""
    n = waves() * 64 * 3 + 37
    store = new_store(256)
    store.append_random(n, 5)
    q = np.random.default_rng(5).uniform(-1, 1, 256).astype(np.float32)
    mask = np.ones(n, bool)
    mask[50:seed_rows(n)] = False
    for metric in (Metric.Cosine, Metric.DotProduct):
        got = pruned_twice_against_full(store, q, metric, 1, 64, ("short seed", metric), mask=mask)
        print("short seed", metric, "finished tails", got, "of", n)
        assert got > 64 * waves(), (got, waves())
    store.close()
    store = new_store(256)
    store.append_clustered(n, 7, 1, 0.05)
    q = store.rows(12345, 1).reshape(-1).astype(np.float32)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for k in (10, 100):
            got = pruned_twice_against_full(store, q, metric, 1, k, ("clustered", metric, k))
            print("clustered", metric, k, "finished tails", got, "of", n)
            assert got > 64 * waves(), (got, waves())
    store.close()


def test_next_tile_is_not_the_next_of_the_stride():
    """a chunk mask that leaves two runs; a row mask that blanks whole tiles in the middle of a wave's stride; deleted rows
    covering whole tiles"""
    n = waves() * 64 * 3 + 37
    nw = waves()
    store = new_store(256)
    store.append_random(n, 11)
    q = np.random.default_rng(11).uniform(-1, 1, 256).astype(np.float32)
    n_chunks = (n + 1023) // 1024
    keep = np.ones(n_chunks, bool)
    keep[n_chunks // 3: n_chunks // 3 + 40] = False
    rmask = np.ones(n, bool)
    seed = seed_rows(n)
    # whole tiles blanked behind the seed: every tile of one wave's second visit and a band of consecutive tiles
    for t in range(seed // 64 + nw, seed // 64 + nw + 300):
        rmask[t * 64:(t + 1) * 64] = False
    rmask[seed + 64 * 7: seed + 64 * 8] = False
    rmask[::5] = False
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (10, 100):
                assert pruned_twice_against_full(store, q, metric, take, k, ("chunks", metric, take, k), chunk_mask=keep) > 0
                assert pruned_twice_against_full(store, q, metric, take, k, ("rows", metric, take, k), mask=rmask) > 0
    dead = np.concatenate([np.arange(seed + 64 * 40, seed + 64 * 43), np.arange(seed + 64 * (nw + 40), seed + 64 * (nw + 41) + 5)])
    store.delete_rows(dead)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for k in (10, 100):
            assert pruned_twice_against_full(store, q, metric, 1, k, ("deleted", metric, k)) > 0
    store.close()
