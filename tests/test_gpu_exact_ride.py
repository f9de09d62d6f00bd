"""GPU: the pruned exact sweep's counters riding in the result block (otters_amd/csrc/ott_exact.hip: merge_rank_totals_kernel;
ott_exact_plan.h: prune_plan_ride; DESIGN.md 3.1b, "the counters ride").  Behind an estimate pass, on host output, the final merge
launch writes the sweep's two counter totals behind the hits it writes into the pinned block: no copy is queued behind the merge and
no timing marker stands between the gated launch and its merge.  The merge's text is one device function for both kernels.
Nothing about the result changes, so every case is held three ways: bit for bit to the CPU oracle (TIES_CANONICAL), to the same
store with force_fallback = 2 (round 2's merge for k <= 64: the counters do not ride, the copy and the marker are back) and to the
same store with exact_prune = 0; `rescored` and exact_finished() are equal riding and not, and equal to each other with
exact_i8_check = 0, where every row that passes the line gate is finished.  A riding call reports merge_ns == 0 (its score_ns
spans the chain), the others a merge_ns of their own: no case passes without the path it names having run.

Stores (exact_small = 0, exact_prune = 1, the four-bit sketch, prepare_batch()): 1 310 784 x 96, three stages, and 1 310 784 x 232,
the headline's stage structure; the smallest that take the estimate pass.

The plateau.  The merge's survivor buffer holds MS_CAP = 2048 candidates; a block list holds at most 64 copies of one score at
k = 64, and a run of consecutive tiles goes to consecutive waves, four to a workgroup.  So copies of the best row in
(2048 / 64 + 2) x 4 = 136 whole tiles leave 34 lists of 64 survivors at the bound, 2176 > 2048: the merge takes merge_walk, in the
launch that also writes the totals; 72 tiles, 1152 survivors, stay inside the buffer."""
import ctypes as C
import threading

import numpy as np
import pytest

from otters_amd import Cmp, Metric, Path, VecStore
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

KS = (1, 10, 16, 17, 64)
SHAPES = ((1_310_784, 96), (1_310_784, 232))
CASES = [(Metric.Cosine, 1), (Metric.Cosine, 0), (Metric.DotProduct, 1), (Metric.DotProduct, 0)]
CASE_IDS = ["cosine-max", "cosine-min", "dot-max", "dot-min"]
HALF_CAP, MS_CAP = 1024, 2048
PLATEAU_TILE = 5000  # behind the estimate pass's rows


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
    """hits, rescored, rows finished in f32 by this query, the call's stats"""
    before = store.exact_finished()
    hits = plan_of(store, q, metric, take, k, filt, mask).collect_arrays()[0]
    return hits, int(store.last_stats["rescored"]), store.exact_finished() - before, dict(store.last_stats)


def riding(st):
    return st["merge_ns"] == 0 and st["score_ns"] > 0


class Box:
    pass


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def big(request, oracle):
    n, dim = request.param
    rng = np.random.default_rng(1000 + dim)
    b = Box()
    b.n, b.dim = n, dim
    b.qs = rng.uniform(-1, 1, (4, dim)).astype(np.float32)
    b.q = b.qs[0]
    s = VecStore(dim)
    for name, v in (("exact_small", 0), ("exact_prune", 1), ("exact_sketch", 1), ("exact_sketch_bits", 4)):
        s.set_option(name, v)
    s.reserve(n)
    s.append_random(n, dim + 1)
    s.prepare_batch()
    assert len(s) == n and s.batch_ready()
    b.store = s
    b.rows = s.rows()
    b.refs = {}
    yield b
    s.close()


def ref_of(b, O, qi, metric, take):
    """the oracle's 64 best of query qi over the store's own rows: computed once, shared, never changed"""
    key = (qi, int(metric), take)
    if key not in b.refs:
        r = O.vec_query(b.rows, b.qs[qi], int(metric), take, 64, ties=O.TIES_CANONICAL)
        r.setflags(write=False)
        b.refs[key] = r
    return b.refs[key]


def held(b, ref, q, metric, take, k, filt=None, mask=None, where=(), expect_ride=True):
    """one query: riding, force_fallback = 2 (not riding), exact_i8_check = 0, exact_prune = 0; every answer `ref`, the counters of the
    first two equal, those without the check equal to each other"""
    s = b.store
    got, resc, fin, st = run(s, q, metric, take, k, filt, mask)
    bits_equal(got, ref, ("riding",) + tuple(where))
    assert st["path_used"] == int(Path.Exact), (where, st)
    assert riding(st) == expect_ride, (where, st)
    s.set_option("force_fallback", 2)
    try:
        got0, resc0, fin0, st0 = run(s, q, metric, take, k, filt, mask)
    finally:
        s.set_option("force_fallback", 0)
    s.set_option("exact_i8_check", 0)
    try:
        gotc, rescc, finc, _ = run(s, q, metric, take, k, filt, mask)
        s.set_option("exact_prune", 0)
        gotp, rescp, finp, stp = run(s, q, metric, take, k, filt, mask)
    finally:
        s.set_option("exact_prune", 1)
        s.set_option("exact_i8_check", -1)
    bits_equal(got0, ref, ("force_fallback = 2",) + tuple(where))
    bits_equal(gotc, ref, ("exact_i8_check = 0",) + tuple(where))
    bits_equal(gotp, ref, ("exact_prune = 0",) + tuple(where))
    assert not riding(st0) and not riding(stp), (where, st0, stp)
    assert (resc, fin) == (resc0, fin0) and rescc == finc == resc and (rescp, finp) == (0, 0), (where, resc, fin, resc0, fin0, rescc, finc, rescp, finp)
    return resc, fin


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_basic_sweep(big, oracle, case):
    metric, take = case
    ref = ref_of(big, oracle, 0, metric, take)
    for k in KS:
        resc, fin = held(big, ref[:k], big.q, metric, take, k, where=(int(metric), take, k))
        print(f"{big.n} x {big.dim} metric {int(metric)} take {take} k {k}: rescored {resc}, finished {fin}")
        assert k <= fin <= resc < big.n


def test_timing_of_a_riding_call(big):
    _, _, _, st = run(big.store, big.q, Metric.Cosine, 1, 10)
    assert st["score_ns"] > 0 and st["merge_ns"] == 0 and st["path_used"] == int(Path.Exact), st


def query_device(store, q, metric, take, k, mask):
    """ott_query_device, merged, into a buffer of k + 8 slots prefilled with 0x5A: (the k slots, the count, the slots behind them)"""
    import torch
    cap = k
    buf = torch.full(((cap + 8) * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
    nout = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d = N.QueryDesc()
    keep = [np.ascontiguousarray(q)]
    d.queries, d.nq, d.metric, d.take, d.k = keep[0].ctypes.data, 1, int(metric), take, k
    d.mode, d.path = 0, int(Path.Exact)
    if mask is not None:
        rm = N.pack_bits(mask)
        keep.append(rm)
        d.row_mask, d.row_mask_bits = rm.ctypes.data, int(mask.size)
    N.check(N.lib().ott_query_device(store._handle(), C.byref(d), C.c_void_p(buf.data_ptr()), cap, C.c_void_p(nout.data_ptr()), None))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    return raw[:cap * 16].view(N.HIT_DTYPE), int(nout.cpu()[0]), raw[cap * 16:]


def test_fewer_than_k_and_no_eligible_rows(big, oracle):
    b, O = big, oracle
    ref = ref_of(b, O, 0, Metric.Cosine, 1)
    # five eligible rows in five different tiles: the 3rd, 9th, 20th, 41st and 64th best of the store
    idx = np.sort(ref["index"][[2, 8, 19, 40, 63]].astype(np.int64))
    mask = np.zeros(b.n, bool)
    mask[idx] = True
    want = ref[np.isin(ref["index"], idx)]
    assert want.size == 5
    for k in (10, 64, 5, 4):
        held(b, want[:k], b.q, Metric.Cosine, 1, k, mask=mask, where=("five rows", k))
    # device output (never riding: nobody reads the counters there): the count, and sentinels behind the hits; nothing written behind the k slots
    for fb in (0, 2):
        b.store.set_option("force_fallback", fb)
        try:
            hits, count, tail = query_device(b.store, b.q, Metric.Cosine, 1, 10, mask)
        finally:
            b.store.set_option("force_fallback", 0)
        assert count == 5, (fb, count)
        bits_equal(hits[:5], want, ("device output", fb))
        assert np.all(hits["index"][5:] == np.uint64(0xFFFFFFFFFFFFFFFF)), (fb, hits[5:])
        assert np.all(tail == 0x5A), fb
    # no eligible row at all
    none = np.zeros(b.n, bool)
    for k in (1, 10, 64):
        held(b, want[:0], b.q, Metric.Cosine, 1, k, mask=none, where=("no rows", k))
    hits, count, _ = query_device(b.store, b.q, Metric.Cosine, 1, 10, none)
    assert count == 0 and np.all(hits["index"] == np.uint64(0xFFFFFFFFFFFFFFFF))


def test_ties_across_lists_and_a_deleted_hit(big, oracle):
    b, O = big, oracle
    metric, take = Metric.Cosine, 1
    ref = ref_of(b, O, 0, metric, take)
    best = int(ref["index"][0])
    A = b.rows[best].copy()
    # copies of the best row in tiles that different workgroups own (a tile goes to wave tile mod waves, four waves to a workgroup)
    at = np.array([100 * 64 + 7, 4500 * 64 + 63, 9001 * 64, 13007 * 64 + 31, 20000 * 64 + 5])
    at = at[at != best]
    keep = [b.rows[r].copy() for r in at]
    rows = b.rows.copy()
    rows[at] = A
    for r in at:
        b.store.write_rows(int(r), A[None, :])
    try:
        want = O.vec_query(rows, b.q, int(metric), take, 64, ties=O.TIES_CANONICAL)
        assert set(at.tolist()) <= set(want["index"][:at.size + 1].astype(np.int64).tolist())
        for k in (1, 3, at.size + 1, 10, 64):
            held(b, want[:k], b.q, metric, take, k, where=("ties", k))
        # a deleted row among the hits: the lowest of the tied rows, the first hit
        gone = int(want["index"][0])
        assert b.store.delete_rows(np.array([gone])) == 1
        try:
            left = want[want["index"] != np.uint64(gone)]
            for k in (1, 10, 63):
                held(b, left[:k], b.q, metric, take, k, where=("deleted", k))
        finally:
            assert b.store.restore_rows(np.array([gone])) == 1
    finally:
        for r, v in zip(at, keep):
            b.store.write_rows(int(r), v[None, :])


@pytest.mark.parametrize("cap", [HALF_CAP, MS_CAP], ids=["inside-the-buffer", "overflow"])
def test_plateau_overflows_the_survivor_buffer(big, oracle, cap):
    b, O = big, oracle
    metric, take = Metric.Cosine, 1
    ref = ref_of(b, O, 0, metric, take)
    A = b.rows[int(ref["index"][0])].copy()
    tiles = (cap // 64 + 2) * 4
    lo, cnt = PLATEAU_TILE * 64, tiles * 64
    keep = b.rows[lo:lo + cnt].copy()
    rows = b.rows.copy()
    rows[lo:lo + cnt] = A
    b.store.write_rows(lo, rows[lo:lo + cnt])
    try:
        want = O.vec_query(rows, b.q, int(metric), take, 64, ties=O.TIES_CANONICAL)
        assert np.unique(want["score"].view(np.uint32)).size == 1  # 64 hits of one score: the lowest rows win
        for k in (64, 10):
            held(b, want[:k], b.q, metric, take, k, where=("plateau", cap, k))
    finally:
        b.store.write_rows(lo, keep)


def test_filtered_query_takes_the_copy_and_the_marker(big, oracle):
    b, O = big, oracle
    ref = ref_of(b, O, 0, Metric.Cosine, 1)
    thr = float(ref["score"][19])
    want = O.vec_query(b.rows, b.q, int(Metric.Cosine), 1, 64, int(Cmp.Gt), thr, ties=O.TIES_CANONICAL)
    assert want.size == int(np.sum(ref["score"] > np.float32(thr)))
    for k in (10, 64):
        held(b, want[:k], b.q, Metric.Cosine, 1, k, filt=(thr, Cmp.Gt), where=("filter", k), expect_ride=False)


def test_a_run_of_queries_and_the_toggle(big, oracle):
    """200 queries in a row, k alternating 10 / 64 / 1, four queries in turn: the totals are running sums, and every call reports its own
    share of them.  Then the same with the riding switched off and on between the queries (force_fallback = 2: the copy reads the
    same totals)"""
    b, O = big, oracle
    refs = [ref_of(b, O, qi, Metric.Cosine, 1) for qi in range(4)]
    ks = (10, 64, 1)
    counters = {}
    for i in range(200):
        qi, k = i % 4, ks[i % 3]
        got, resc, fin, st = run(b.store, b.qs[qi], Metric.Cosine, 1, k)
        bits_equal(got, refs[qi][:k], ("run", i))
        assert riding(st), (i, st)
        assert counters.setdefault((qi, k), (resc, fin)) == (resc, fin), (i, resc, fin)
    try:
        for i in range(200):
            qi, k = i % 4, ks[i % 3]
            on = i % 2 == 0 or i % 7 == 0
            b.store.set_option("force_fallback", 0 if on else 2)
            got, resc, fin, st = run(b.store, b.qs[qi], Metric.Cosine, 1, k)
            bits_equal(got, refs[qi][:k], ("toggle", i))
            assert riding(st) == on, (i, st)
            assert counters[(qi, k)] == (resc, fin), (i, resc, fin)
    finally:
        b.store.set_option("force_fallback", 0)


def test_four_worker_contexts(big, oracle):
    b, O = big, oracle
    refs = [ref_of(b, O, qi, Metric.Cosine, 1) for qi in range(4)]
    serial = []
    for t in range(4):
        _, _, fin, _ = run(b.store, b.qs[t], Metric.Cosine, 1, (10, 64, 1, 17)[t])
        serial.append(fin)
    before = b.store.exact_finished()
    barrier = threading.Barrier(4)
    out, errors = [None] * 4, []

    def body(t):
        try:
            barrier.wait()
            out[t] = [plan_of(b.store, b.qs[t], Metric.Cosine, 1, (10, 64, 1, 17)[t]).collect_arrays()[0] for _ in range(6)]
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
            bits_equal(hits, refs[t][:(10, 64, 1, 17)[t]], ("thread", t))
    assert b.store.exact_finished() - before == 6 * sum(serial), (b.store.exact_finished() - before, serial)
