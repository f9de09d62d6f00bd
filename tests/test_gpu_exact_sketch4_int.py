"""GPU: the integer decode of the four-bit sketch form of the pruned exact sweep ("the integer decode"): the
workgroup quantises the query, the lane's line meets its digit planes in 4-bit dot products, and prune_score_bound_sketchq decides.
Pruning only decides which rows are finished, so every answer is the oracle's, bit for bit, and the full sweep's.  The queries are
the ones that stress the quantiser (tests/sketchq_queries.py), at the line lengths of tests/test_gpu_exact_sketch4.py: 3 (dim 96),
8 (256), 25 (773) and 28 pieces (896).  Stores hold 20 000 to 40 000 rows; the rows8 small-store kernel is switched off so that they
take the streaming kernel the pruned sweep lives in.  The CPU half is tests/test_exact_prune_sketchq_bound.py."""
import numpy as np
import pytest

from otters_amd import Metric, Path, VecStore
from sketchq_queries import QUERY_KINDS, REFUSED, stress_query

pytestmark = pytest.mark.gpu

N = 20_000
SEED_ROWS = 2048  # a tenth of the rows in whole tiles: these have no checkpoint


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"], ref["query"]), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def make_store(rows, prune):
    store = VecStore(rows.shape[1])
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", prune)
    store.set_option("exact_sketch", 1)
    store.set_option("exact_sketch_bits", 4)
    store.add_vectors(rows)
    return store


def run(store, q, metric, take, k):
    p = store.query(q, metric)
    return (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact).collect_arrays()[0]


def oracle_ref(oracle, rows, q, metric, take, k):
    return oracle.vec_query(rows, q, int(metric), take, k, 0, 0.0, ties=oracle.TIES_CANONICAL)


def corpus(q, n, seed):
    """uniform rows; 40 rows along the query at unit scale (the gate closes early whatever the query's scale); and 200 rows no
    bound can miss — the prefix against the query, the tail zero, so a = rho = 0 and the bound is the prefix's score"""
    rng = np.random.default_rng(seed)
    dim = q.size
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    unit = (q / np.abs(q).max()).astype(np.float32)
    near = rng.choice(n, 40, replace=False)
    rows[near] = (unit * (1 + rng.normal(0, 0.3, (40, dim)))).astype(np.float32)
    anti = rng.choice(np.setdiff1d(np.arange(SEED_ROWS, n), near), 200, replace=False)
    rows[anti] = 0.0
    rows[anti, :32] = -unit[:32] * rng.uniform(0.5, 1.0, (200, 1)).astype(np.float32)
    return rows


@pytest.mark.parametrize("kind", QUERY_KINDS)
@pytest.mark.parametrize("dim", [96, 256, 773, 896])
def test_stress_queries_return_the_oracles_bits(oracle, dim, kind):
    """cosine and dot, Max and Min, k = 1, 10, 100: the four-bit store against the oracle and against the full sweep; and the sweep
    did prune: 0 < rescored < the gated rows (dot, Take Max: at 2^-100 the reference's cosine is NaN throughout and the gate
    stays open).  The refused kind takes the 7/8 form, and its scores underflow: only the bits are held"""
    q = stress_query(kind, dim)
    rows = corpus(q, N, dim)
    sk, full = make_store(rows, 1), make_store(rows, 0)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 100):
                got = run(sk, q, metric, take, k)
                bits_equal(got, run(full, q, metric, take, k), ("4 bits/full", dim, kind, metric, take, k))
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), ("oracle", dim, kind, metric, take, k))
    run(full, q, Metric.DotProduct, 1, 10)
    assert full.last_stats["rescored"] == 0
    run(sk, q, Metric.DotProduct, 1, 10)
    r = sk.last_stats["rescored"]
    print(dim, kind, "finished tails:", r, "of", N - SEED_ROWS, "gated rows")
    if kind in REFUSED:
        assert 0 < r <= N - SEED_ROWS, r  # the pruned sweep ran, in the form the plan fell back to
    else:
        assert 0 < r < N - SEED_ROWS, r
    sk.close()
    full.close()


def planted(rows, q, rng):
    """a few rows near the query (the gate closes early) and copies of one of them on both sides of the seed boundary (a tenth of
    the rows), so that equal scores sit at the k-th place"""
    n, dim = rows.shape
    near = rng.integers(0, n, 40)
    rows[near] = (q + rng.normal(0, 0.8, (40, dim))).astype(np.float32)
    dup = rows[near[0]].copy()
    for r in (5, n // 10 - 1, n // 10 + 3, n // 2, n - 1):
        rows[r] = dup


@pytest.mark.parametrize("dim", [768, 773])
def test_equal_scores_at_the_kth_place_and_an_early_gate(oracle, dim):
    rng = np.random.default_rng(dim + 3)
    rows = rng.uniform(-1, 1, (40_000, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    planted(rows, q, rng)
    sk, full = make_store(rows, 1), make_store(rows, 0)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 3, 5, 10, 64, 100):
                got = run(sk, q, metric, take, k)
                bits_equal(got, run(full, q, metric, take, k), ("4 bits/full", metric, take, k))
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), ("oracle", metric, take, k))
    run(sk, q, Metric.Cosine, 1, 10)
    assert 0 < sk.last_stats["rescored"] < rows.shape[0] - 4032, sk.last_stats
    sk.close()
    full.close()


@pytest.mark.parametrize("dim", [256, 768])
def test_a_query_the_quantiser_refuses_takes_another_form(oracle, dim):
    """max |q| = 2^-126: 2^e would be subnormal.  Uniform rows, so the dot products are distinct subnormals and small normals; the
    answers are the oracle's through the 7/8 form (its tails are counted: the pruned sweep ran), and a query the quantiser accepts
    on the same store takes the four-bit form again"""
    q = stress_query("max_2^-126", dim)
    rng = np.random.default_rng(dim + 8)
    rows = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    sk, no = make_store(rows, 1), make_store(rows, 1)
    no.set_option("exact_sketch", 0)
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (1, 10, 100):
                got = run(sk, q, metric, take, k)
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), ("oracle", dim, metric, take, k))
                refused = sk.last_stats["rescored"]
                bits_equal(got, run(no, q, metric, take, k), ("refused/7-8", dim, metric, take, k))
                assert refused == no.last_stats["rescored"] > 0, (metric, take, k, refused, no.last_stats)  # the same form: the same tails
    q2 = np.random.default_rng(dim).uniform(-1, 1, dim).astype(np.float32)
    bits_equal(run(sk, q2, Metric.DotProduct, 1, 10), oracle_ref(oracle, rows, q2, Metric.DotProduct, 1, 10), ("accepted", dim))
    four = sk.last_stats["rescored"]
    run(no, q2, Metric.DotProduct, 1, 10)
    assert 0 < four < N - SEED_ROWS and four != no.last_stats["rescored"], (four, no.last_stats)
    sk.close()
    no.close()
