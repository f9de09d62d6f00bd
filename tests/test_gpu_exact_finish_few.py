"""GPU: the narrow finish of the pruned exact sweep (otters_amd/csrc/ott_exact.hip: pq_finish_few; ott_finish_few.h; DESIGN.md 3.1b,
"a few queued rows").  In the head form with one list entry per lane (k <= 64) a finish of at most sixteen queued rows asks for
several stages of those rows per round trip instead of one stage of a dense tile of 64.  Nothing else changes: the same rows are
finished at the same tile, by the same loads and the same additions in the same order.  So every hit is held bit for bit to the CPU
oracle (TIES_CANONICAL) and to the same store with exact_prune = 0, and `rescored` and exact_finished() to the runs they are
defined to equal.

Stores (exact_small = 0, exact_prune = 1, the four-bit sketch, prepare_batch() for the int8 plane): 1 310 784 x 232 and
1 400 000 x 256, the smallest that take the estimate seed; 1 310 784 x 96, three stages, fewer than a round holds; 1 310 784 x 237,
a remainder (dim % 8 = 5) and a ragged last stage.

Known n.  A row mask leaves eligible: eight whole tiles of the seed (the even tiles 0 .. 14 — eight waves of the estimate pass list
16 rows each, 128 >= k, so the gate is closed at every k <= 64) and n planted rows in ONE tile behind the seed (tile 9001, odd), the
rest of that tile and every other tile masked.  A wave owns the tiles congruent to its number modulo the number of waves, which is
even on every device: the wave that owns tile 9001 owns none of the even seed tiles, and every other tile it owns is masked and
never read.  Its queue therefore holds the n planted rows and nothing else when the sweep ends, and ONE finish holds exactly n
rows: n = 1 .. 16 the narrow one (one row group up to 8, two from 9), n = 17 the wide one.
The planted rows are copies of the best eligible seed row with one element moved by a few ulps in the direction that does not
lower the score (checked with the oracle): real hits at or above the gate, which the int8 check cannot drop.
Behind an estimate pass the gated launch covers the seed's rows as well, and the k best of them pass the line gate always: so
`rescored` of such a query cannot be n itself.  What is held instead is no weaker: against the same query with the planted rows
masked out, `rescored` grows by exactly n and exact_finished() by exactly n.  With NO seed row eligible (the gate open, the check
not asked) the two counters are n themselves, and that case is held too."""
import threading

import numpy as np
import pytest

from otters_amd import Cmp, Metric, Path, VecStore

pytestmark = pytest.mark.gpu

KS = (1, 10, 16, 17, 64)
SHAPES = ((1_310_784, 232), (1_400_000, 256), (1_310_784, 96), (1_310_784, 237))
SEED = 131_072            # the first block, crafted by add_vectors (the seed of every shape is at least this)
SEED_TILES = np.arange(0, 16, 2)
PLANT_TILE = 9001
PLANT = PLANT_TILE * 64 + (np.arange(17) * 11 + 5) % 64 + 0  # 17 distinct rows of the tile, not in order
OUT = 40                  # the decoys' outlier dim; the query is zero there
CASES = [(Metric.Cosine, 1), (Metric.Cosine, 0), (Metric.DotProduct, 1), (Metric.DotProduct, 0)]
CASE_IDS = ["cosine-max", "cosine-min", "dot-max", "dot-min"]


@pytest.fixture(scope="module")
def oracle():
    import oracle as O
    O.build()
    return O


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:20], ref["index"][:20])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def plan_of(store, q, metric, take, k, filt=None, mask=None):
    p = store.query(q, metric)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    return (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact)


def run(store, q, metric, take, k, filt=None, mask=None):
    """hits, rescored, rows finished in f32 by this query"""
    before = store.exact_finished()
    hits = plan_of(store, q, metric, take, k, filt, mask).collect_arrays()[0]
    return hits, int(store.last_stats["rescored"]), store.exact_finished() - before


def oracle_on(O, rows, idx, q, metric, take, k, filt=None):
    """the oracle over the eligible rows `idx` (ascending) alone: the canonical order ranks ties by row, and idx keeps the rows' order"""
    fc, ft = (int(filt[1]), filt[0]) if filt else (0, 0.0)
    ref = O.vec_query(np.ascontiguousarray(rows[idx]), q, int(metric), take, k, fc, ft, ties=O.TIES_CANONICAL)
    ref["index"] = idx[ref["index"].astype(np.int64)]
    return ref


def score_of(O, row, q, metric):
    return O.vec_query(np.ascontiguousarray(row[None, :]), q, int(metric), 1, 1, ties=O.TIES_CANONICAL)["score"][0]


class Box:
    pass


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def big(request, oracle):
    n, dim = request.param
    rng = np.random.default_rng(dim)
    b = Box()
    b.n, b.dim = n, dim
    b.q = rng.uniform(-1, 1, dim).astype(np.float32)
    b.q[OUT] = 0.0
    b.block = rng.uniform(-1, 1, (SEED, dim)).astype(np.float32)
    s = VecStore(dim)
    for name, v in (("exact_small", 0), ("exact_prune", 1), ("exact_sketch", 1), ("exact_sketch_bits", 4)):
        s.set_option(name, v)
    s.reserve(n)
    s.add_vectors(b.block)
    s.append_random(n - SEED, dim + 1)
    s.prepare_batch()
    assert len(s) == n and s.batch_ready()
    b.store = s
    b.rows = s.rows()
    b.seed_idx = (SEED_TILES[:, None] * 64 + np.arange(64)[None, :]).ravel()
    yield b
    s.close()


def held(b, O, rows, idx, metric, take, k, filt=None, where=()):
    """The query over the eligible rows idx: the check on (twice), off, and exact_prune = 0 — every answer the oracle's; the two
    runs' counters equal; `rescored` the same with the check off, where every row that passed the line gate is finished.  Returns
    (rescored, finished with the check)"""
    mask = np.zeros(b.n, bool)
    mask[idx] = True
    ref = oracle_on(O, rows, idx, b.q, metric, take, k, filt)
    s = b.store
    got, resc, fin = run(s, b.q, metric, take, k, filt, mask)
    bits_equal(got, ref, ("check on",) + tuple(where))
    again, resc2, fin2 = run(s, b.q, metric, take, k, filt, mask)
    bits_equal(again, ref, ("second run",) + tuple(where))
    assert (resc, fin) == (resc2, fin2), (where, resc, fin, resc2, fin2)
    s.set_option("exact_i8_check", 0)
    try:
        got0, resc0, fin0 = run(s, b.q, metric, take, k, filt, mask)
        s.set_option("exact_prune", 0)
        gotp, rescp, finp = run(s, b.q, metric, take, k, filt, mask)
    finally:
        s.set_option("exact_prune", 1)
        s.set_option("exact_i8_check", -1)
    bits_equal(got0, ref, ("exact_i8_check = 0",) + tuple(where))
    bits_equal(gotp, ref, ("exact_prune = 0",) + tuple(where))
    assert resc0 == resc and fin0 == resc0 and fin <= resc and (rescp, finp) == (0, 0), (where, resc, fin, resc0, fin0, rescp, finp)
    return resc, fin


def planted_rows(O, b, metric, take, count=17):
    """copies of the best eligible seed row, one element each moved by a few ulps so that the score does not get worse"""
    best = int(oracle_on(O, b.rows, b.seed_idx, b.q, metric, take, 1)["index"][0])
    A = b.rows[best]
    sA = score_of(O, A, b.q, metric)
    out = np.repeat(A[None, :], count, axis=0)
    for i in range(count):
        j = (7 * i + 3) % b.dim
        if j == OUT:
            j += 1
        for towards in (np.float32(np.inf), np.float32(-np.inf)):
            r = A.copy()
            for _ in range(2 + i % 5):
                r[j] = np.nextafter(r[j], towards)
            sc = score_of(O, r, b.q, metric)
            if (sc >= sA) if take else (sc <= sA):
                out[i] = r
                break
        # (neither direction keeps the score: the row stays a plain copy, a tie with A)
    return best, out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_known_n_one_finish_holds_exactly_n_rows(big, oracle, case):
    b, O = big, oracle
    metric, take = case
    best, planted = planted_rows(O, b, metric, take)
    rows = b.rows.copy()
    rows[PLANT] = planted
    keep = b.rows[PLANT_TILE * 64:PLANT_TILE * 64 + 64].copy()
    tile = keep.copy()
    tile[PLANT - PLANT_TILE * 64] = planted
    b.store.write_rows(PLANT_TILE * 64, tile)
    try:
        base = {}
        for n in range(1, 18):
            idx = np.sort(np.concatenate([b.seed_idx, PLANT[:n]]))
            for k in (n, 64):
                if k not in base:  # the same query without the planted rows
                    base[k] = held(b, O, rows, b.seed_idx, metric, take, k, where=("baseline", k))
                resc, fin = held(b, O, rows, idx, metric, take, k, where=("planted", n, k))
                assert (resc - base[k][0], fin - base[k][1]) == (n, n), (n, k, resc, fin, base[k])
            # no seed row eligible: the gate is open, the n rows are queued and finished, and nothing else is
            only = np.sort(PLANT[:n])
            resc, fin = held(b, O, rows, only, metric, take, max(n, 10), where=("planted alone", n))
            assert (resc, fin) == (n, n), (n, resc, fin)
        print(f"{b.n} x {b.dim} metric {int(metric)} take {take}: baselines (rescored, finished) by k: {base}")
    finally:
        b.store.write_rows(PLANT_TILE * 64, keep)


def decoys(block, q, rng, every):
    """tests/test_gpu_exact_seed_est.py's decoys: rows whose estimate is far beyond their score — one outlier dim (where the query is
    zero) makes the line coarse, every other dim is tiny with the sign of the query's (odd decoys: against it)"""
    at = np.arange(1, block.shape[0], every)
    sgn = np.where(np.signbit(q), np.float32(-1), np.float32(1))
    pol = np.where((at // every) % 2 == 0, np.float32(1), np.float32(-1))
    block[at] = (pol[:, None] * sgn[None, :] * rng.uniform(0.5e-2, 1.5e-2, (at.size, q.size)).astype(np.float32))
    block[at, OUT] = 100.0


def test_estimate_pass_tail_and_the_uniform_query(big, oracle):
    """the estimate pass ends every wave with one narrow finish of min(k, 16) rows: k = 1, 10, 16, 17, 64 is seed_keep 1, 10 and 16.
    The unmasked uniform query first, the counters printed; then with decoys in every seed tile, whose estimates crowd every wave's
    best rows"""
    b, O = big, oracle
    for metric, take in ((Metric.Cosine, 1), (Metric.DotProduct, 0)):
        ref = O.vec_query(b.rows, b.q, int(metric), take, 64, ties=O.TIES_CANONICAL)
        for k in KS:
            got, resc, fin = run(b.store, b.q, metric, take, k)
            bits_equal(got, ref[:k], ("uniform", int(metric), take, k))
            again, resc2, fin2 = run(b.store, b.q, metric, take, k)
            bits_equal(again, ref[:k], ("uniform, second run", int(metric), take, k))
            b.store.set_option("exact_i8_check", 0)
            try:
                got0, resc0, fin0 = run(b.store, b.q, metric, take, k)
                b.store.set_option("exact_prune", 0)
                gotp, rescp, finp = run(b.store, b.q, metric, take, k)
            finally:
                b.store.set_option("exact_prune", 1)
                b.store.set_option("exact_i8_check", -1)
            bits_equal(got0, ref[:k], ("uniform, exact_i8_check = 0", k))
            bits_equal(gotp, ref[:k], ("uniform, exact_prune = 0", k))
            print(f"{b.n} x {b.dim} metric {int(metric)} take {take} k {k}: rescored {resc}, finished {fin} with the check, {fin0} without")
            assert (resc, fin) == (resc2, fin2) and resc == resc0 == fin0 and (rescp, finp) == (0, 0) and k <= fin <= resc < b.n, (k, resc, fin, resc0, fin0)
    block = b.block.copy()
    decoys(block, b.q, np.random.default_rng(5), 2)
    rows = b.rows.copy()
    rows[:SEED] = block
    b.store.write_rows(0, block)
    try:
        for metric, take in ((Metric.Cosine, 1), (Metric.DotProduct, 0)):
            ref = O.vec_query(rows, b.q, int(metric), take, 64, ties=O.TIES_CANONICAL)
            for k in KS:
                got, resc, fin = run(b.store, b.q, metric, take, k)
                bits_equal(got, ref[:k], ("decoys", int(metric), take, k))
                again, resc2, fin2 = run(b.store, b.q, metric, take, k)
                bits_equal(again, ref[:k], ("decoys, second run", int(metric), take, k))
                assert (resc, fin) == (resc2, fin2) and k <= fin <= resc, (k, resc, fin, resc2, fin2)
                print(f"decoys {b.n} x {b.dim} metric {int(metric)} take {take} k {k}: rescored {resc}, finished {fin}")
    finally:
        b.store.write_rows(0, b.block)


def test_ties_a_filter_a_deleted_row_and_worker_contexts(big, oracle):
    b, O = big, oracle
    metric, take = Metric.Cosine, 1
    order = oracle_on(O, b.rows, b.seed_idx, b.q, metric, take, 64)
    best = int(order["index"][0])
    A = b.rows[best]
    keep_plant = b.rows[PLANT_TILE * 64:PLANT_TILE * 64 + 64].copy()
    seed_tile = int(SEED_TILES[3]) * 64
    keep_seed = b.rows[seed_tile:seed_tile + 64].copy()
    rows = b.rows.copy()
    # a tie at the gate on both sides of the seed: plain copies of the best row, three in an eligible seed tile, five planted
    dup_seed = seed_tile + np.array([9, 30, 51]) + (1 if best in (seed_tile + 9, seed_tile + 30, seed_tile + 51) else 0)
    rows[dup_seed] = A
    rows[PLANT[:5]] = A
    # a planted row that fails a filter the others pass: a copy of the 30th best eligible seed row, the threshold the 20th best's score
    rows[PLANT[5]] = b.rows[int(order["index"][29])]
    filt = (float(order["score"][19]), Cmp.Gt)
    b.store.write_rows(PLANT_TILE * 64, rows[PLANT_TILE * 64:PLANT_TILE * 64 + 64])
    b.store.write_rows(seed_tile, rows[seed_tile:seed_tile + 64])
    try:
        idx = np.sort(np.concatenate([b.seed_idx, PLANT[:6]]))
        base_idx = b.seed_idx
        for k in (1, 3, 4, 8, 9, 10, 64):  # the gate ties with the planted copies up to k = 9 (A and its eight copies)
            base = held(b, O, rows, base_idx, metric, take, k, where=("ties, baseline", k))
            resc, fin = held(b, O, rows, idx, metric, take, k, where=("ties", k))
            # the five copies score the gate's value or above and pass the line gate at every k; the 30th best's copy does for certain
            # only where the gate is at most its score: at k = 64 (the gate is a 64th best of eligible seed rows)
            assert resc - base[0] in ((6,) if k == 64 else (5, 6)) and fin - base[1] >= 5, (k, resc, fin, base)
        # the filter: the full seed, no estimate pass — the gated launch covers the rows behind the seed alone, so the counters are the
        # planted rows' own: all six pass the line gate while the gate is the 64th best passing seed row's or open
        ref = oracle_on(O, rows, idx, b.q, metric, take, 64, filt)
        assert int(PLANT[5]) not in ref["index"].tolist() and set(PLANT[:5].tolist()) <= set(ref["index"].tolist())
        resc, fin = held(b, O, rows, idx, metric, take, 64, filt, where=("filter",))
        assert (resc, fin) == (6, 6), (resc, fin)
        # a deleted planted row: not a hit, not queued, not finished
        assert b.store.delete_rows(PLANT[1:2]) == 1
        try:
            live = np.sort(np.concatenate([b.seed_idx, PLANT[:1], PLANT[2:6]]))
            base = held(b, O, rows, base_idx, metric, take, 64, where=("deleted, baseline",))
            mask = np.zeros(b.n, bool)
            mask[idx] = True  # (the mask still names the deleted row: the tombstone removes it)
            ref = oracle_on(O, rows, live, b.q, metric, take, 64)
            got, resc, fin = run(b.store, b.q, metric, take, 64, None, mask)
            bits_equal(got, ref, "deleted")
            assert (resc - base[0], fin - base[1]) == (5, 5), (resc, fin, base)
        finally:
            assert b.store.restore_rows(PLANT[1:2]) == 1
        # worker contexts: four threads at once; every answer the serial one, the finished rows the serial call's per call
        mask = np.zeros(b.n, bool)
        mask[idx] = True
        want, _, fin1 = run(b.store, b.q, metric, take, 10, None, mask)
        bits_equal(want, oracle_on(O, rows, idx, b.q, metric, take, 10), "serial")
        before = b.store.exact_finished()
        barrier = threading.Barrier(4)
        out, errors = [None] * 4, []

        def body(t):
            try:
                barrier.wait()
                out[t] = [plan_of(b.store, b.q, metric, take, 10, None, mask).collect_arrays()[0] for _ in range(3)]
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=body, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for t in range(4):
            for hits in out[t]:
                bits_equal(hits, want, ("thread", t))
        assert b.store.exact_finished() - before == 12 * fin1, (b.store.exact_finished() - before, fin1)
    finally:
        b.store.write_rows(PLANT_TILE * 64, keep_plant)
        b.store.write_rows(seed_tile, keep_seed)
