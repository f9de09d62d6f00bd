"""GPU: the int8 check of the pruned exact sweep's survivors (store option exact_i8_check; otters_amd/csrc/ott_exact.hip: pq_refine,
ott_i8_check.h, DESIGN.md 3.1b "survivors on the int8 plane").  In the head form with k <= 64 a row that passes the four-bit bound
is scored on the store's int8 plane first and finished in f32 only unless that score plus the int8 level's certified error ranks
strictly below the gate.  Hits must be the oracle's bit for bit, `rescored` (rows that passed the line gate) must not move, and
ott_store_exact_finished must show that the check ran.

The plane's presence is made deterministic: prepare_batch() builds it before the first query; a second store with the planes
switched off (set_batch_image(False)) gives the off case, and so do exact_i8_check = 0 and exact_prune = 0 on the first.
Stores: the smallest that take the estimate seed (1 310 720 rows): 1 310 784 x 232 (plane pitch 256, a 24-byte tail), 1 400 000 x
256, and 1 310 784 x 96 (a single plane stage; exact_prune = 1, such a store is below the automatic rule's eight stages).  The sharp
rows (tests/prune_sharp.py's manner) sit in small stores with the full seed (exact_prune = 1)."""
import threading

import numpy as np
import pytest

from otters_amd import Cmp, Metric, Path, VecStore

pytestmark = pytest.mark.gpu

KS = (1, 10, 16, 17, 64)
SHAPES = ((1_310_784, 232), (1_400_000, 256), (1_310_784, 96))


@pytest.fixture(scope="module")
def oracle():
    import oracle as O
    O.build()
    return O


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def new_store(dim, planes=True, prune=1):
    s = VecStore(dim)
    s.set_option("exact_small", 0)
    s.set_option("exact_prune", prune)
    s.set_option("exact_sketch", 1)
    s.set_option("exact_sketch_bits", 4)
    if not planes:
        s.set_batch_image(False)
    return s


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


def oracle_ref(O, rows, q, metric, take, k, filt=None, mask=None):
    fc, ft = (int(filt[1]), filt[0]) if filt else (0, 0.0)
    return O.vec_query(rows, q, int(metric), take, k, fc, ft, row_mask=mask, ties=O.TIES_CANONICAL)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def big(request, oracle):
    """(rows, store with the plane, store without planes, the oracle's top-64 per metric and take)"""
    n, dim = request.param
    rows = oracle.rand_rows(0, n, dim, 7)
    on, off = new_store(dim), new_store(dim, planes=False)
    for s in (on, off):
        s.append_random(n, 7)
    on.prepare_batch()
    assert on.batch_ready() and not off.batch_ready()
    q = np.random.default_rng(dim).uniform(-1, 1, dim).astype(np.float32)
    refs = {(m, t): oracle_ref(oracle, rows, q, m, t, 64) for m in (Metric.Cosine, Metric.DotProduct) for t in (1, 0)}
    yield rows, on, off, q, refs
    on.close()
    off.close()


@pytest.mark.parametrize("metric", [Metric.Cosine, Metric.DotProduct], ids=["cosine", "dot"])
@pytest.mark.parametrize("take", [1, 0], ids=["max", "min"])
def test_hits_and_counters_with_the_check_on_and_off(big, metric, take):
    rows, on, off, q, refs = big
    for k in KS:
        ref = refs[(metric, take)][:k]  # (canonical ties: the top-k is a prefix of the top-64)
        got, resc, fin = run(on, q, metric, take, k)
        bits_equal(got, ref, ("check on", k))
        again, resc2, fin2 = run(on, q, metric, take, k)
        bits_equal(again, ref, ("second run", k))
        assert (resc, fin) == (resc2, fin2), ("two runs agree", k)
        on.set_option("exact_i8_check", 0)
        got0, resc0, fin0 = run(on, q, metric, take, k)
        on.set_option("exact_prune", 0)
        gotp, rescp, finp = run(on, q, metric, take, k)
        on.set_option("exact_prune", 1)
        on.set_option("exact_i8_check", -1)
        gotb, rescb, finb = run(off, q, metric, take, k)
        bits_equal(got0, ref, ("exact_i8_check = 0", k))
        bits_equal(gotp, ref, ("exact_prune = 0", k))
        bits_equal(gotb, ref, ("no planes", k))
        print(f"{rows.shape} metric {int(metric)} take {take} k {k}: rescored {resc}, finished {fin} with the check, {fin0} without")
        assert resc == resc0 == rescb and rescp == 0 and finp == 0, (k, resc, resc0, rescb, rescp)
        assert 0 < resc < rows.shape[0]
        assert fin < resc and fin0 == resc0 and finb == rescb, (k, fin, resc, fin0, finb)


def test_masks_deletes_rewrites_and_a_refused_query(big, oracle):
    rows, on, off, q, refs = big
    n, dim = rows.shape
    rng = np.random.default_rng(1)
    # a row mask that keeps two rows in three
    mask = rng.random(n) < 0.66
    ref = oracle_ref(oracle, rows, q, Metric.Cosine, 1, 10, None, mask)
    got, resc, fin = run(on, q, Metric.Cosine, 1, 10, None, mask)
    bits_equal(got, ref, "row mask")
    gotb, rescb, _ = run(off, q, Metric.Cosine, 1, 10, None, mask)
    bits_equal(gotb, ref, "row mask, no planes")
    assert resc == rescb and fin < resc
    # a score filter (the full seed instead of the estimate pass)
    filt = (float(refs[(Metric.Cosine, 1)]["score"][40]), Cmp.Gt)
    ref = oracle_ref(oracle, rows, q, Metric.Cosine, 1, 64, filt)
    got, resc, fin = run(on, q, Metric.Cosine, 1, 64, filt)
    bits_equal(got, ref, "filter")
    assert run(off, q, Metric.Cosine, 1, 64, filt)[1] == resc
    # a query the int8 level's error model refuses: one element of 1 among elements of 0.004, which sit at a rounding midpoint of the
    # operand's scale (1 / 127) — the measured loss, 0.0039 sqrt(dim - 1), is above the 0.0158 the bound assumes from dim 18 on.  The
    # sweep runs without the check and finishes every row that passes the line gate
    qr = np.full(dim, 4e-3, np.float32)
    qr[3] = 1.0
    ref = oracle_ref(oracle, rows, qr, Metric.DotProduct, 1, 10)
    got, resc, fin = run(on, qr, Metric.DotProduct, 1, 10)
    bits_equal(got, ref, "refused query")
    assert fin == resc
    # rewritten rows (the plane is kept in step) and deleted rows, the best hits among them
    best = refs[(Metric.Cosine, 1)]["index"][:6].astype(np.int64)
    new = (q[None, :] * np.array([[2.0], [0.5], [-1.0]], np.float32) + rng.normal(0, 0.05, (3, dim))).astype(np.float32)
    at = int(n // 2 + 5)
    rows2 = rows.copy()
    rows2[at:at + 3] = new
    dead = np.ones(n, bool)
    dead[best[:3]] = False
    for s in (on, off):
        s.write_rows(at, new)
        s.delete_rows(best[:3])
    try:
        assert on.batch_ready()
        for metric, take in ((Metric.Cosine, 1), (Metric.DotProduct, 0)):
            ref = oracle_ref(oracle, rows2, q, metric, take, 16, None, dead)
            got, resc, fin = run(on, q, metric, take, 16)
            bits_equal(got, ref, ("rewritten and deleted", int(metric), take))
            gotb, rescb, _ = run(off, q, metric, take, 16)
            bits_equal(gotb, ref, ("rewritten and deleted, no planes", int(metric), take))
            assert resc == rescb and fin < resc
    finally:
        for s in (on, off):
            s.restore_rows(best[:3])
            s.write_rows(at, rows[at:at + 3])


def test_a_chunk_mask_whose_first_run_ends_inside_the_seed(big, oracle):
    """chunks of 1024 rows; chunks 50 .. 59 are out, so the first run ends at row 51 200, inside the seed's 131 072 rows: the seed and
    the gated launch's whole plan are two runs each, the gated launch meets the tile tails of both runs, and the plane's rows are
    addressed by store row across the gap"""
    rows, on, off, q, refs = big
    n = rows.shape[0]
    keep = np.ones((n + 1023) // 1024, bool)
    keep[50:60] = False
    rmask = np.repeat(keep, 1024)[:n]

    def chunked(store, metric, take, k):
        before = store.exact_finished()
        hits, _, stats = store._run(plan_of(store, q, metric, take, k).resolve(), chunk_mask=keep)  # (the call MetaStore makes)
        return hits, int(stats["rescored"]), store.exact_finished() - before

    for metric in (Metric.Cosine, Metric.DotProduct):
        for take in (1, 0):
            ref = oracle_ref(oracle, rows, q, metric, take, 64, None, rmask)
            for k in (10, 64):
                got, resc, fin = chunked(on, metric, take, k)
                bits_equal(got, ref[:k], ("chunks, check on", int(metric), take, k))
                again, resc2, fin2 = chunked(on, metric, take, k)
                bits_equal(again, ref[:k], ("chunks, second run", int(metric), take, k))
                on.set_option("exact_i8_check", 0)
                try:
                    got0, resc0, fin0 = chunked(on, metric, take, k)
                finally:
                    on.set_option("exact_i8_check", -1)
                bits_equal(got0, ref[:k], ("chunks, exact_i8_check = 0", int(metric), take, k))
                gotb, rescb, finb = chunked(off, metric, take, k)
                bits_equal(gotb, ref[:k], ("chunks, no planes", int(metric), take, k))
                print(f"chunks {rows.shape} metric {int(metric)} take {take} k {k}: rescored {resc}, finished {fin} with the check, {fin0} without")
                assert (resc, fin) == (resc2, fin2) and resc == resc0 == rescb and 0 < resc < n, (resc, resc2, resc0, rescb)
                assert fin < resc and fin0 == resc0 and finb == rescb, (fin, resc, fin0, finb)


def test_worker_contexts(big):
    """four threads query one store at once: overlapping calls run on worker contexts, which alias the plane's owner.  Every answer is
    the serial one, and the store's count of finished rows grows by the serial call's for every call: each of them took the check"""
    rows, on, off, q, refs = big
    ref = refs[(Metric.Cosine, 1)][:10]
    _, resc1, fin1 = run(on, q, Metric.Cosine, 1, 10)
    assert fin1 < resc1
    before = on.exact_finished()
    barrier = threading.Barrier(4)
    out = [None] * 4

    def body(t):
        barrier.wait()
        out[t] = [plan_of(on, q, Metric.Cosine, 1, 10).collect_arrays()[0] for _ in range(3)]

    threads = [threading.Thread(target=body, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(4):
        for hits in out[t]:
            bits_equal(hits, ref, ("thread", t))
    assert on.exact_finished() - before == 12 * fin1, (on.exact_finished() - before, fin1)


# ---- sharp rows ---------------------------------------------------------------------------------------------------------------------

def sharp_store_rows(oracle, dim, n, metric, rng):
    """Copies of a row A in the seed (the first tenth), so that the gate is A's score.  A lies along the query with every element
    just below an int8 rounding midpoint of the row's own scale, so its int8 image rounds every element down and the approximate
    score sits nearly a whole quantisation loss (0.7 %) below the exact one.  Behind the seed: challengers, copies of A moved by the
    smallest step of a doubling search that changes the oracle's score — scaled for dot, turned towards the query for cosine — so
    that they score a few ulps above the gate (required hits, whose image rounds against them like A's), exactly at it (ties: plain
    copies) and a few ulps below.  Near rows: 120 rows whose score lies 0.2 % to 8 % (cosine) or 10 % (dot) below the gate, a ladder
    across the int8 bound (about 1 %) and the four-bit bound's slack (several %): those in between pass the line gate and are dropped
    by the check, which is what shows in the counters that the check ran.  Filler scores far below."""
    q = rng.uniform(0.2, 1.0, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (n, dim)) * 0.05).astype(np.float32)
    # A: along the query, on a midpoint grid of its own scale
    k = np.clip(np.rint(q / q.max() * 120.0), 1, 126)
    s = np.float32(0.003)
    A = (s * (k + 0.5 - 2.0 ** -10)).astype(np.float32)
    A[int(np.argmax(k))] = s * np.float32(127.0)
    seed = n // 10
    rows[8:8 + 256] = A
    score = lambda r: oracle_ref(oracle, np.ascontiguousarray(r[None, :]), q, metric, 1, 1)["score"][0]
    gate = score(A)
    slots = rng.choice(np.arange(seed + 64, n), 96, replace=False)
    above, ties, below = [], [], []
    a64, q64 = A.astype(np.float64), q.astype(np.float64)
    along = q64 * (np.linalg.norm(a64) / np.linalg.norm(q64)) - a64  # towards the query's direction, at A's length
    for i, slot in enumerate(slots):
        r = A.copy()
        want = ("above", "tie", "below")[i % 3]
        found = want == "tie"
        for e in range(-30 + i // 3 % 2, -5):  # (two interleaved ladders of steps: the challengers are not all one row)
            if found:
                break
            t = 2.0 ** e if want == "above" else -(2.0 ** e)
            r = (a64 * (1.0 + t) if metric == Metric.DotProduct else a64 + t * along).astype(np.float32)
            sc = score(r)
            found = sc > gate if want == "above" else sc < gate
        assert found
        rows[slot] = r
        (above if want == "above" else ties if want == "tie" else below).append(int(slot))
    near = [int(x) for x in np.setdiff1d(np.arange(seed + 64, n), slots)[:: (n - seed - 64) // 130][:120]]
    for i, slot in enumerate(near):
        if metric == Metric.DotProduct:
            r = a64 * (1.0 - (0.002 + 0.098 * i / 119.0))
        else:
            noise = rng.standard_normal(dim)
            r = a64 + np.sqrt(2.0 * (0.002 + 0.078 * i / 119.0)) * np.linalg.norm(a64) * noise / np.linalg.norm(noise)
        rows[slot] = r.astype(np.float32)
    return rows, q, float(gate), above, ties, below, near


@pytest.mark.parametrize("metric", [Metric.Cosine, Metric.DotProduct], ids=["cosine", "dot"])
def test_sharp_rows_at_the_gate(oracle, metric):
    rng = np.random.default_rng(17)
    n, dim = 40_320, 768
    rows, q, gate, above, ties, below, near = sharp_store_rows(oracle, dim, n, metric, rng)
    # rows outside the plane's error model (flag bits 0 / 2) skip the check; here they are required hits.  Dot: copies of A with one
    # element of 5 where the query is smallest — the int8 image loses 4 % of the row (bit 2; above 2^-5) and the score is above the
    # gate.  Cosine: A turned halfway towards the query (1e-5 above the gate) and scaled to a norm of 7e-19, below 1e-18 (bit 0)
    taken = set(above + ties + below + near)
    flagged = [int(x) for x in np.arange(n - 2000, n) if int(x) not in taken][:4]
    A = rows[8].astype(np.float64)
    q64 = q.astype(np.float64)
    for f in flagged:
        if metric == Metric.DotProduct:
            rows[f] = A.astype(np.float32)
            rows[f, int(np.argmin(q))] = 5.0
        else:
            rows[f] = ((A + 0.5 * (q64 * (np.linalg.norm(A) / np.linalg.norm(q64)) - A)) * 2.0 ** -63).astype(np.float32)
        assert oracle_ref(oracle, np.ascontiguousarray(rows[f][None, :]), q, metric, 1, 1)["score"][0] > gate
    on, off, shrunk = new_store(dim), new_store(dim, planes=False), new_store(dim)
    shrunk.set_option("eps_scale_ppm", 1)
    for s in (on, off, shrunk):
        s.add_vectors(rows)
    try:
        for s in (on, shrunk):
            s.prepare_batch()
            assert s.batch_ready()
        lost = 0
        for k in (10, 64):
            ref = oracle_ref(oracle, rows, q, metric, 1, k)
            need = set(above) & set(ref["index"].tolist())
            assert need, "the challengers above the gate are among the hits"
            assert set(flagged) <= set(ref["index"].tolist()), "the rows outside the error model are required hits"
            got, resc, fin = run(on, q, metric, 1, k)
            bits_equal(got, ref, ("sharp, check on", k))
            gotb, rescb, finb = run(off, q, metric, 1, k)
            bits_equal(gotb, ref, ("sharp, no planes", k))
            print(f"sharp metric {int(metric)} k {k}: rescored {resc}, finished {fin} with the check, {finb} without")
            assert resc == rescb and finb == rescb
            assert fin < resc, "near rows pass the line gate and are dropped on the int8 plane: the check ran"
            bad = run(shrunk, q, metric, 1, k)[0]
            lost += len(need - set(bad["index"].tolist()))
        # with the bound shrunk a million times the midpoint rows' int8 image puts required hits below the gate: the file can fail
        assert lost > 0
    finally:
        for s in (on, off, shrunk):
            s.close()
