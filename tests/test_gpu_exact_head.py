"""GPU: the head form of the pruned exact sweep's four-bit sketch (store option exact_sketch_head, the default wherever a store keeps
four-bit lines; DESIGN.md 3.1b, "no f32 stage in front"): a gated row reads its line, 16 B of stage 0's codes and rho_all, and no
f32 stage; survivors run all of their stages behind the checkpoint.  Pruning only decides which rows are finished, so stores of the
same rows in four forms — the head, exact_sketch_head = 0 (the c = 1 form of a store without a head), no sketch (the 7/8 checkpoint)
and the full sweep — return the same rows in the same order with the same score bits, and all match the oracle.  The rows8
small-store kernel is switched off so that these stores take the streaming kernel the pruned sweep lives in.  Shapes: 20 000 rows
(312 tiles and one of 32) at the line lengths 3 (dim 96), 8 (256), 25 (773) and 28 pieces (896), and 40 320 x 768 (630 whole
tiles: with 2048 waves most waves meet one gated tile or none, some none at all).  The CPU half is tests/test_exact_prune_head_bound.py."""
import threading

import numpy as np
import pytest

from otters_amd import Cmp, Metric, Path, VecStore
from sketchq_queries import QUERY_KINDS, REFUSED, stress_query

pytestmark = pytest.mark.gpu

FORMS = (("head", 1, 1, -1), ("no head", 1, 1, 0), ("7/8", 1, 0, -1), ("full", 0, 0, -1))  # name, exact_prune, exact_sketch, exact_sketch_head

# `rescored` of the store with exact_sketch_head = 0 on the inputs of test_the_head_form_is_the_one_that_runs (40 320 x 768, seed
# 99, cosine and dot product, Take Max, k = 10), as counted by the build BEFORE the head existed (the parent commit's library on the
# same rows and query; profiles/exact_head/README.md): the option gives that build's sweep back, tile for tile.
PARENT_RESCORED = {"cosine": 4108, "dot": 4292}


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"], ref["query"]), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def make_store(rows, prune, sketch, head, pieces=None, reserve=False, devices=None):
    store = VecStore(rows.shape[1], devices=devices) if devices else VecStore(rows.shape[1])
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", prune)
    store.set_option("exact_sketch", sketch)
    store.set_option("exact_sketch_bits", 4)
    store.set_option("exact_sketch_head", head)
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
    return [make_store(rows, p, s, h, **kw) for _, p, s, h in FORMS]


def plan_of(store, q, metric, take, k, filt=None, mask=None):
    p = store.query(q, metric)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    return (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact)


def run(store, q, metric, take, k, filt=None, mask=None):
    return plan_of(store, q, metric, take, k, filt, mask).collect_arrays()[0]


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
        bits_equal(got, run(s, q, metric, take, k, filt, mask), ("head/" + name,) + tuple(where))
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


def stage0_rows(rows, q, rng):
    """what only the head form meets, behind the seed (a tenth of the rows): NaN / inf / -0 in stage 0 (no bound is claimed, or the
    code of a zero), a stage 0 that holds nearly the whole norm — along the query and against it, so that such rows are top hits of
    Take Max and Take Min although every code of their head clamps — and rows that are zero outside stage 0"""
    n, dim = rows.shape
    at = rng.choice(np.arange(n // 10 + 64, n), 24, replace=False)
    rows[at[0], 3] = np.nan
    rows[at[1], 0] = np.inf
    rows[at[2], 31] = -np.inf
    rows[at[3], :32] = -0.0
    rows[at[4], :32:2] = -0.0
    rows[at[5], 1:32:2] = 0.0
    unit = (q[:32] / np.abs(q[:32]).max()).astype(np.float32)
    for j, sgn in enumerate((1, -1, 1, -1, 1, -1)):
        rows[at[6 + j], :32] = np.float32(sgn) * unit * np.float32(10.0 ** (1 + j))
    for j in range(6):
        rows[at[12 + j], 32:] = 0.0 if j % 2 else -0.0
        rows[at[12 + j], :32] = np.float32(1 if j < 3 else -1) * unit * rng.uniform(0.5, 1.0, 32).astype(np.float32)
    rows[at[18], :] = 0.0
    return at


@pytest.fixture(scope="module")
def uniform_768():
    """40 320 x 768 uniform rows and nothing planted: the gate is the uniform rows' own"""
    rng = np.random.default_rng(99)
    rows = rng.uniform(-1, 1, (40_320, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    stores = four(rows)
    yield rows, q, stores
    close(*stores)


@pytest.mark.parametrize("k", [1, 10, 64, 100, 256, 512])
def test_uniform_rows_at_every_list_width(oracle, uniform_768, k):
    """k = 1, 10 | 64 (the block code) | 100 | 256 | 512: the list widths of the pruned kernel (one, one with the block code, two,
    four and eight entries per lane); cosine and dot, Max and Min.  Which form ran is read from `rescored`: up to k = 256 the head
    form runs, and finishes other rows than the c = 1 form of the store without a head; at k = 512 the plan keeps the c = 1 form on
    purpose (ott_exact_plan.h: prune_plan_head — the head kernel with eight list entries per lane runs one wave per SIMD and
    measured slower), so there the two stores count the same"""
    rows, q, stores = uniform_768
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            hold(oracle, stores, rows, q, metric, take, k, where=(metric, take, k))
            run(stores[0], q, metric, take, k)
            head = stores[0].last_stats["rescored"]
            run(stores[1], q, metric, take, k)
            off = stores[1].last_stats["rescored"]
            print(k, metric, take, "finished rows: head", head, "head off", off)
            assert 0 < head < rows.shape[0] and 0 < off < rows.shape[0], (k, metric, take, head, off)
            if k <= 256:
                assert head != off, (k, metric, take, head, off)
            else:
                assert head == off, (k, metric, take, head, off)


def test_the_head_form_is_the_one_that_runs(uniform_768):
    """`rescored` — the rows the gated launch finished — is the same on two runs of a store (tiles go to waves in a fixed order),
    differs between the head form and the c = 1 form (the head form's bound is the wider one: it finishes more rows), and with
    exact_sketch_head = 0 is what the build before the head counted on these inputs.  A store that sets no exact_sketch_head takes
    the head form.  bytes_scanned stays algorithmic: the same in every form"""
    rows, q, stores = uniform_768
    default = VecStore(rows.shape[1])
    for name, v in (("exact_small", 0), ("exact_prune", 1), ("exact_sketch", 1)):
        default.set_option(name, v)
    default.add_vectors(rows)
    for mname, metric in (("cosine", Metric.Cosine), ("dot", Metric.DotProduct)):
        ref = run(stores[3], q, metric, 1, 10)
        full_bytes = stores[3].last_stats["bytes_scanned"]
        assert stores[3].last_stats["rescored"] == 0
        counts = {}
        for name, s in (("head", stores[0]), ("no head", stores[1]), ("default", default)):
            counts[name] = []
            for _ in range(2):
                bits_equal(run(s, q, metric, 1, 10), ref, name)
                counts[name].append(s.last_stats["rescored"])
                assert s.last_stats["bytes_scanned"] == full_bytes > 0
                assert s.last_stats["path_used"] == int(Path.Exact)
        print(mname, "finished rows of", rows.shape[0] - 4032, "gated rows:", counts, "the build before the head:", PARENT_RESCORED[mname])
        for name in counts:
            assert counts[name][0] == counts[name][1], counts
            assert 0 < counts[name][0] < rows.shape[0] - 4032, counts  # (the seed's 4032 rows have no checkpoint)
        assert counts["head"][0] != counts["no head"][0], counts
        assert counts["head"][0] > counts["no head"][0], counts
        assert counts["default"][0] == counts["head"][0], counts
        assert counts["no head"][0] == PARENT_RESCORED[mname], (counts, PARENT_RESCORED)
    default.close()


@pytest.mark.parametrize("dim", [96, 256, 773, 896])
def test_line_lengths_a_short_last_tile_and_stage_0_rows(oracle, dim):
    """20 000 rows (312 tiles and one of 32 rows) with the stage-0 rows planted among uniform ones: 96 = 3 stages, a sketch by option
    only; 256 = 8 stages; 773 = 25 stages and a remainder term; 896 = 28 stages, the widest query a launch carries and the longest
    line.  A filter and a row mask as well"""
    rng = np.random.default_rng(dim)
    rows = rng.uniform(-1, 1, (20_000, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    planted(rows, q, rng)
    stage0_rows(rows, q, rng)
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


def test_stage_0_rows_at_768_with_sparse_masks_and_a_chunk_mask(oracle):
    """40 320 x 768 with the stage-0 rows; a row mask that empties whole tiles (such a tile is skipped, also as the NEXT tile of the
    pipelined loop) and one that keeps one row in a hundred; a chunk mask that leaves two runs of chunks"""
    rng = np.random.default_rng(7)
    rows = rng.uniform(-1, 1, (40_320, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    planted(rows, q, rng)
    at = stage0_rows(rows, q, rng)
    stores = four(rows)
    holes = np.ones(rows.shape[0], bool)
    for t in (70, 71, 72, 200, 629):
        holes[64 * t:64 * t + 64] = False
    holes[64 * 300:64 * 420] = False
    sparse = rng.random(rows.shape[0]) < 0.01
    sparse[at] = True
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in (10, 100):
                hold(oracle, stores, rows, q, metric, take, k, where=("stage 0", metric, take, k))
            hold(oracle, stores, rows, q, metric, take, 10, None, holes, ("holes", metric, take))
            hold(oracle, stores, rows, q, metric, take, 10, None, sparse, ("sparse", metric, take))
    n_chunks = (rows.shape[0] + 1023) // 1024
    keep = np.ones(n_chunks, bool)
    keep[7:19] = False
    rmask = np.repeat(keep, 1024)[:rows.shape[0]]
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            got = [s._run(plan_of(s, q, metric, take, 10).resolve(), chunk_mask=keep)[0] for s in stores]  # (the call MetaStore makes with its zone-map mask)
            for (name, *_), g in zip(FORMS[1:], got[1:]):
                bits_equal(got[0], g, ("chunks head/" + name, metric, take))
            bits_equal(got[0], oracle_ref(oracle, rows, q, metric, take, 10, None, rmask), ("chunks oracle", metric, take))
    close(*stores)


def test_an_open_gate_finishes_every_row(oracle):
    """the seed lists fewer than k rows: the gate stays open, no line and no head is fetched, every gated row is finished"""
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


@pytest.mark.parametrize("kind", QUERY_KINDS)
def test_queries_that_stress_the_quantiser(oracle, kind):
    """dim 256 and 773, 20 000 rows: the head form quantises the WHOLE query (m = 0).  The refused kind takes the 7/8 form"""
    for dim in (256, 773):
        q = stress_query(kind, dim)
        rng = np.random.default_rng(dim + 17)
        rows = rng.uniform(-1, 1, (20_000, dim)).astype(np.float32)
        unit = (q / np.abs(q).max()).astype(np.float32)
        near = rng.choice(20_000, 40, replace=False)
        rows[near] = (unit * (1 + rng.normal(0, 0.3, (40, dim)))).astype(np.float32)
        head, full = make_store(rows, 1, 1, -1), make_store(rows, 0, 0, -1)
        for metric in (Metric.Cosine, Metric.DotProduct):
            for take in (1, 0):
                for k in (1, 10, 100):
                    got = run(head, q, metric, take, k)
                    bits_equal(got, run(full, q, metric, take, k), ("head/full", dim, kind, metric, take, k))
                    bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), ("oracle", dim, kind, metric, take, k))
        run(head, q, Metric.DotProduct, 1, 10)
        r = head.last_stats["rescored"]
        assert (0 < r <= 20_000 - 2048) if kind in REFUSED else (0 < r < 20_000 - 2048), (dim, kind, r)
        close(head, full)


# ---- the life cycle: each against a fresh store of the same rows, hits and `rescored` ---------------------------------------------------
def same_as_fresh(oracle, store, fresh, rows, q, where, ks=(1, 10, 64)):
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            for k in ks:
                got = run(store, q, metric, take, k)
                a = store.last_stats["rescored"]
                bits_equal(got, run(fresh, q, metric, take, k), (where, "fresh", metric, take, k))
                assert a == fresh.last_stats["rescored"] > 0, (where, metric, take, k, a, fresh.last_stats)
                bits_equal(got, oracle_ref(oracle, rows, q, metric, take, k), (where, "oracle", metric, take, k))


@pytest.fixture(scope="module")
def life():
    rng = np.random.default_rng(31)
    rows = rng.uniform(-1, 1, (30_011, 768)).astype(np.float32)
    q = rng.uniform(-1, 1, 768).astype(np.float32)
    planted(rows, q, rng)
    stage0_rows(rows, q, rng)
    fresh = make_store(rows, 1, 1, -1, reserve=True)
    nohead = make_store(rows, 1, 1, 0, reserve=True)
    yield rows, q, fresh, nohead
    close(fresh, nohead)


def test_appends_in_pieces_and_growth_without_reserve(oracle, life):
    """several appends without a reserve: every growth step reallocates, the head is copied like the lines (two arrays in one
    allocation: the second one moves with the capacity)"""
    rows, q, fresh, _ = life
    store = make_store(rows, 1, 1, -1, pieces=[1, 700, 63, 5000, 1300, 9000, 13_947])
    same_as_fresh(oracle, store, fresh, rows, q, "pieces")
    store.close()


def test_the_option_switched_off_and_on_again(oracle, life):
    """exact_sketch_head = 0 on a store that has a head: the next append drops it and the store counts what a store without one
    counts; back to -1: the next append makes the head for every row"""
    rows, q, fresh, nohead = life
    store = make_store(rows[:20_000], 1, 1, -1)
    store.set_option("exact_sketch_head", 0)
    store.add_vectors(rows[20_000:25_000])
    store.add_vectors(rows[25_000:])
    same_as_fresh(oracle, store, nohead, rows, q, "switched off", ks=(10,))
    tail = rows[:4096]
    store.set_option("exact_sketch_head", -1)
    store.add_vectors(tail)
    both = np.concatenate([rows, tail])
    fresh2 = make_store(both, 1, 1, -1)
    same_as_fresh(oracle, store, fresh2, both, q, "switched on", ks=(10,))
    close(store, fresh2)


def test_a_delete_and_a_compaction(oracle, life):
    rows, q, _, _ = life
    dead = np.random.default_rng(4).choice(rows.shape[0], rows.shape[0] // 100, replace=False)
    keep = np.ones(rows.shape[0], bool)
    keep[dead] = False
    store = make_store(rows, 1, 1, -1)
    store.delete_rows(dead)
    for metric in (Metric.Cosine, Metric.DotProduct):  # deleted rows keep their lines and heads; the live mask hides them
        bits_equal(run(store, q, metric, 1, 10), oracle_ref(oracle, rows, q, metric, 1, 10, None, keep), ("deleted", metric))
    store.compact()
    fresh = make_store(rows[keep], 1, 1, -1)
    same_as_fresh(oracle, store, fresh, rows[keep], q, "compacted")
    close(store, fresh)


def test_heads_move_between_the_shards_of_a_store(oracle, life):
    """two shards on one device; appended in two pieces, so that rows — with their lines and heads — move between the shards (a
    sharded query leaves its hits on the device and reports no `rescored`: the hits are what is held)"""
    rows, q, _, _ = life
    sk = make_store(rows, 1, 1, -1, devices=[0, 0], pieces=[20_000, 10_011])
    one = make_store(rows, 1, 1, -1, devices=[0, 0])
    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            ref = oracle_ref(oracle, rows, q, metric, take, 10)
            bits_equal(run(sk, q, metric, take, 10), ref, ("pieces", metric, take))
            bits_equal(run(one, q, metric, take, 10), ref, ("one append", metric, take))
    close(sk, one)


def test_worker_contexts(oracle, life):
    """four threads query one store at once: overlapping calls run on worker contexts, which alias the lines and the head.  Every
    answer and every count is the serial one"""
    rows, q, fresh, _ = life
    store = make_store(rows, 1, 1, -1, reserve=True)
    cases = [(metric, take, k) for metric in (Metric.Cosine, Metric.DotProduct) for take in (1, 0) for k in (10, 64)]
    want = {}
    for c in cases:
        want[c] = (run(fresh, q, *c), fresh.last_stats["rescored"])
    resolved = {c: plan_of(store, q, *c).resolve() for c in cases}
    barrier = threading.Barrier(4)
    got, errors = [[] for _ in range(4)], []

    def body(t):
        try:
            barrier.wait()
            for _ in range(3):
                for c in cases[t % 2::2] + cases[(t + 1) % 2::2]:
                    hits, _, stats = store._run(resolved[c])
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
        assert len(got[t]) == 3 * len(cases)
        for c, hits, rescored in got[t]:
            bits_equal(hits, want[c][0], ("thread", t, c))
            assert rescored == want[c][1] > 0, (t, c, rescored, want[c][1])
    store.close()
