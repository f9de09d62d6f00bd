"""GPU: the seed of the pruned exact sweep as an estimate pass ("the seed by estimate"; ott_exact_plan.h:
prune_plan_seed_est).  From 1 310 720 scored rows, in the head form, for k <= 64 and a query without a filter, the seed launch
streams the lines, heads and inverse norms of the first rows, ranks them by the decode's estimate, and every wave scores its best
min(k, 16) exactly; their merged k-th best gates a launch over ALL rows, whose lists alone make the result.  Whatever the estimate
picks, the gate is a k-th best of real scores, so every case is held bit for bit — indices, order, score bits — to the CPU oracle
over the same rows and to the same store with exact_prune = 0, on two runs each with the same `rescored`.

The rule starts at 1 310 720 rows and 8 stages, so the stores are 1 310 784 x 232 and 1 400 000 x 256: a crafted first block of
131 072 rows (the seed of both) by add_vectors, append_random behind it, and 64 crafted rows in the middle of the rest.  The rows
are read back from the store for the oracle; one reference per (metric, take) at k = 65 serves every k (the canonical order of a
shorter list is a prefix of a longer one's).  The CPU half is tests/test_exact_seed_est_cpu.py."""
import threading

import numpy as np
import pytest

from otters_amd import Cmp, Metric, Path, VecStore

pytestmark = pytest.mark.gpu

SEED = 131_072
MID = 600_000
KS = (1, 10, 16, 17, 64, 65)  # one list entry per lane without and (from 17) with the block code; 65: two entries, the full seed
METRICS = (Metric.Cosine, Metric.DotProduct)
OUT = 40  # the decoys' outlier dim (in the tail: it sets the line's cell width); the queries are zero there


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"], ref["query"]), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def plan_of(store, q, metric, take, k, filt=None, mask=None):
    p = store.query(q, metric)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    return (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact)


def run(store, q, metric, take, k, filt=None, mask=None):
    hits = plan_of(store, q, metric, take, k, filt, mask).collect_arrays()[0]
    return hits, store.last_stats["rescored"]


def oracle_ref(oracle, rows, q, metric, take, k, mask=None):
    return oracle.vec_query(rows, q, int(metric), take, k, 0, 0.0, row_mask=mask, ties=oracle.TIES_CANONICAL)


def held(store, ref, q, metric, take, k, mask=None, filt=None, where=()):
    """the pruned sweep twice and the full sweep of the same store twice: every answer is the reference's, the two counts are equal.
    Returns the count"""
    counts = []
    for i in range(2):
        got, n = run(store, q, metric, take, k, filt, mask)
        bits_equal(got, ref, ("pruned", i) + tuple(where))
        counts.append(n)
    store.set_option("exact_prune", 0)
    try:
        for i in range(2):
            full, n = run(store, q, metric, take, k, filt, mask)
            assert n == 0
            bits_equal(full, ref, ("exact_prune = 0", i) + tuple(where))
    finally:
        store.set_option("exact_prune", 1)
    assert counts[0] == counts[1], (where, counts)
    return counts[0]


def decoys(block, q, rng, every):
    """Rows whose estimate is far beyond their score.  One outlier dim (where the query is zero) makes the line coarse — a cell is
    an eighth of it — and every other dim is tiny with the sign of the query's (odd decoys: against it), so each decodes to plus
    or minus half a cell: the estimate is a cosine of +-0.8, the score +-0.001.  With `every` = 2 there are 16 of either sign in
    every tile: they crowd every wave's best rows by estimate for Take Max and for Take Min"""
    at = np.arange(1, block.shape[0], every)
    sgn = np.where(np.signbit(q), np.float32(-1), np.float32(1))
    pol = np.where((at // every) % 2 == 0, np.float32(1), np.float32(-1))
    block[at] = (pol[:, None] * sgn[None, :] * rng.uniform(0.5e-2, 1.5e-2, (at.size, q.size)).astype(np.float32))
    block[at, OUT] = 100.0
    return at


def special_rows(block):
    """NaN / inf / all-zero rows, on even rows (no bound and no estimate: never offered by the estimate pass, finished by the gated launch)"""
    block[1000, 3] = np.nan
    block[1002, 0] = np.inf
    block[1004, OUT + 7] = -np.inf
    block[1006, :] = 0.0
    block[1008, 32:] = 0.0
    block[64 * 900 + 10, block.shape[1] - 1] = np.nan


class Box:
    pass


def build(dim, n, craft):
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    q[OUT] = 0.0
    block = rng.uniform(-1, 1, (SEED, dim)).astype(np.float32)
    mid = rng.uniform(-1, 1, (64, dim)).astype(np.float32)
    b = Box()
    craft(b, block, mid, q, rng)
    store = VecStore(dim)
    for name, v in (("exact_small", 0), ("exact_prune", 1), ("exact_sketch", 1), ("exact_sketch_bits", 4)):
        store.set_option(name, v)
    store.reserve(n)
    store.add_vectors(block)
    store.append_random(MID, dim + 1)
    store.add_vectors(mid)
    store.append_random(n - SEED - MID - 64, dim + 2)
    assert len(store) == n
    b.store, b.q, b.n, b.dim = store, q, n, dim
    b.rows = store.rows()  # (what the oracle scores: the crafted rows and the generator's, as the store holds them)
    assert b.rows.shape == (n, dim) and np.array_equal(b.rows[:SEED].view(np.uint32), block.view(np.uint32))
    b.refs = {}
    return b


def ref65(oracle, b, metric, take, mask=None, tag=None):
    """one oracle run per (metric, take, mask), at the longest list: every shorter list is its prefix"""
    key = (int(metric), take, tag)
    if key not in b.refs:
        b.refs[key] = oracle_ref(oracle, b.rows, b.q, metric, take, 65, mask)
    return b.refs[key]


def craft_ties(b, block, mid, q, rng):
    """decoys in every tile; 70 identical best rows, half in the seed (in as many tiles) and half in the rest: ties at the gate at
    every k; 69 distinct rows against the query for Take Min, on both sides too; the special rows"""
    dim = q.size
    decoys(block, q, rng, 2)
    special_rows(block)
    best = (q + rng.normal(0, 1.0, dim)).astype(np.float32)
    best[OUT] = 0.0
    b.dup_seed = 64 * np.linspace(3, 2040, 35).astype(np.int64) + 2
    block[b.dup_seed] = best
    mid[:35] = best
    anti_at = 64 * np.linspace(7, 2000, 40).astype(np.int64) + 4
    block[anti_at] = (-q + rng.normal(0, 1.0, (40, dim))).astype(np.float32)
    mid[35:] = (-q + rng.normal(0, 1.0, (29, dim))).astype(np.float32)


def craft_one_tile(b, block, mid, q, rng):
    """the 64 best rows of the whole store in ONE seed tile (tile 5), the 64 lowest in another (tile 9): one wave meets them all
    and keeps min(k, 16); three copies of the best of them in the rest; a few decoys; the special rows"""
    dim = q.size
    decoys(block, q, rng, 16)
    special_rows(block)
    block[320:384] = (q + rng.normal(0, 0.8, (64, dim))).astype(np.float32)
    block[576:640] = (-q + rng.normal(0, 0.8, (64, dim))).astype(np.float32)
    b.best_tile = np.arange(320, 384)
    mid[:3] = block[321]


@pytest.fixture(scope="module")
def ties_store():
    b = build(232, 1_310_784, craft_ties)
    yield b
    b.store.close()


@pytest.fixture(scope="module")
def tile_store():
    b = build(256, 1_400_000, craft_one_tile)
    yield b
    b.store.close()


def sweep(oracle, b, metric, take):
    ref = ref65(oracle, b, metric, take)
    assert ref.size == 65
    out = {}
    for k in KS:
        out[k] = held(b.store, ref[:k], b.q, metric, take, k, where=(b.n, metric, take, k))
        # behind an estimate pass the gated launch covers every row, so it finishes the k hits at least; behind the full seed
        # (k = 65) it may finish none: the 65 best may all be seed rows
        assert (k if k <= 64 else 0) <= out[k] < b.n, (k, out)
    print(b.n, "x", b.dim, metric, "take max" if take else "take min", "rows the gated launch finished, by k:", out)
    return ref


@pytest.mark.parametrize("take", [1, 0])
@pytest.mark.parametrize("metric", METRICS)
def test_decoys_in_every_tile_and_ties_at_the_gate(oracle, ties_store, metric, take):
    """1 310 784 x 232, 64 rows past the rule's start.  Every wave's best rows by estimate are decoys, so the gate is a decoy's
    score and the gated launch finishes far more rows than it would — the answer is the oracle's all the same.  Take Max: the 65
    best are 65 of 70 identical rows, 35 of them seed rows: the gate ties with rows on both sides, and a seed row must come out
    once, not twice"""
    b = ties_store
    ref = sweep(oracle, b, metric, take)
    if take and metric == Metric.Cosine:  # (a dot product with an infinite row is a score: such a row leads one of the two lists)
        assert len(set(ref["score"].view(np.uint32).tolist())) == 1 and np.count_nonzero(ref["index"] < SEED) == 35
        assert np.array_equal(ref["index"][:35], b.dup_seed)
    else:
        assert len(set(ref["index"].tolist())) == 65


@pytest.mark.parametrize("take", [1, 0])
@pytest.mark.parametrize("metric", METRICS)
def test_the_best_rows_of_the_store_in_one_seed_tile(oracle, tile_store, metric, take):
    """1 400 000 x 256: the estimate pass's one wave that meets tile 5 keeps min(k, 16) of its 64 rows, every other wave offers
    what it has; at k = 17 and 64 the gate then lies below the final k-th best"""
    b = tile_store
    ref = sweep(oracle, b, metric, take)
    if take and metric == Metric.Cosine:
        assert set(ref["index"][:64].tolist()) - set(b.best_tile.tolist()) <= {SEED + MID, SEED + MID + 1, SEED + MID + 2}


def test_the_seeds_best_rows_deleted(oracle, tile_store):
    """tombstones: tile 5's rows are deleted.  Were a deleted row to feed the gate, the gate would lie above every live row's
    score and hits would go missing"""
    b = tile_store
    live = np.ones(b.n, bool)
    live[b.best_tile] = False
    assert b.store.delete_rows(b.best_tile) == 64
    try:
        for metric in METRICS:
            ref = ref65(oracle, b, metric, 1, live, "deleted")
            assert ref.size == 65 and not set(ref["index"].tolist()) & set(b.best_tile.tolist())
            for k in (10, 64):
                held(b.store, ref[:k], b.q, metric, 1, k, where=("deleted", metric, k))
    finally:
        b.store.restore_rows(b.best_tile)
    got, _ = run(b.store, b.q, Metric.Cosine, 1, 10)
    bits_equal(got, ref65(oracle, b, Metric.Cosine, 1)[:10], "restored")


def sparse_mask(b):
    """five eligible rows in the seed and one in each of a thousand consecutive tiles of the rest (behind either seed, 131 072 rows
    or a tenth): no wave meets ten eligible rows, so no wave's own k-th best ever closes its gate"""
    mask = np.zeros(b.n, bool)
    mask[[70, 9000, 64 * 700 + 1, 64 * 1500 + 33, SEED - 1]] = True
    mask[64 * (3000 + np.arange(1000)) + (7 * np.arange(1000)) % 64] = True
    return mask


@pytest.mark.parametrize("which", ["ties", "tile"])
def test_which_seed_ran(oracle, ties_store, tile_store, which):
    """Read from `rescored`, which counts what the gated launch finished.  A row mask leaves five eligible rows in the seed, with
    k = 10: the gate stays open.  Behind an estimate pass the gated launch covers every row and finishes all 1005 eligible ones;
    behind the full seed it covers the rest: 1000.  The same query with a filter that everything passes, and k = 65, take the
    full seed"""
    b = ties_store if which == "ties" else tile_store
    mask = sparse_mask(b)
    eligible = int(np.count_nonzero(mask))
    assert eligible == 1005
    for metric in METRICS:
        ref = ref65(oracle, b, metric, 1, mask, "sparse")
        assert held(b.store, ref[:10], b.q, metric, 1, 10, mask, where=("estimate", metric)) == eligible
        passes_all = (-2.0, Cmp.Gt) if metric == Metric.Cosine else (-1e30, Cmp.Gt)
        assert held(b.store, ref[:10], b.q, metric, 1, 10, mask, passes_all, where=("filter", metric)) == eligible - 5
        assert held(b.store, ref, b.q, metric, 1, 65, mask, where=("k = 65", metric)) == eligible - 5
        assert held(b.store, ref[:64], b.q, metric, 1, 64, mask, where=("k = 64", metric)) == eligible
    ref = ref65(oracle, b, Metric.Cosine, 0, mask, "sparse")
    assert held(b.store, ref[:10], b.q, Metric.Cosine, 0, 10, mask, where=("estimate, take min",)) == eligible


def test_a_chunk_mask_whose_first_run_ends_inside_the_seed(oracle, tile_store):
    """chunks of 1024 rows; chunks 50 .. 59 are out, so the first run ends at row 51 200: the seed's 131 072 scored rows are two
    runs, and so is the gated launch's whole plan (1 389 760 scored rows: the rule holds)"""
    b = tile_store
    n_chunks = (b.n + 1023) // 1024
    keep = np.ones(n_chunks, bool)
    keep[50:60] = False
    rmask = np.repeat(keep, 1024)[:b.n]
    for metric in METRICS:
        for take in (1, 0):
            ref = ref65(oracle, b, metric, take, rmask, "chunks")
            for k in (10, 64):
                counts = []
                for _ in range(2):
                    hits, _, stats = b.store._run(plan_of(b.store, b.q, metric, take, k).resolve(), chunk_mask=keep)  # (the call MetaStore makes)
                    bits_equal(hits, ref[:k], ("chunks", metric, take, k))
                    counts.append(stats["rescored"])
                assert counts[0] == counts[1] and 0 < counts[0] < b.n, counts


def test_worker_contexts(oracle, tile_store):
    """four threads query the store at once: overlapping calls run on worker contexts.  Every answer and every count is the serial one"""
    b = tile_store
    cases = [(metric, take, k) for metric in METRICS for take in (1, 0) for k in (10, 64)]
    want = {}
    for c in cases:
        want[c] = run(b.store, b.q, *c)
        bits_equal(want[c][0], ref65(oracle, b, c[0], c[1])[:c[2]], ("serial", c))
    resolved = {c: plan_of(b.store, b.q, *c).resolve() for c in cases}
    barrier = threading.Barrier(4)
    got, errors = [[] for _ in range(4)], []

    def body(t):
        try:
            barrier.wait()
            for _ in range(2):
                for c in cases[t % 2::2] + cases[(t + 1) % 2::2]:
                    hits, _, stats = b.store._run(resolved[c])
                    got[t].append((c, hits, stats["rescored"]))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=body, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(4):
        assert len(got[t]) == 2 * len(cases)
        for c, hits, rescored in got[t]:
            bits_equal(hits, want[c][0], ("thread", t, c))
            assert rescored == want[c][1] > 0, (t, c, rescored, want[c][1])
