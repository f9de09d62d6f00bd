"""GPU: bit rows and ott_query_binary against the numpy model (tests/binary_ref.py), bit for bit: index, the score's f32 bits, order,
count and `query`, on the table route (binary_gate 0), the gated route (1) and automatic (-1)."""
import ctypes as C

import numpy as np
import pytest

import binary_ref as BR
import manhattan_ref as M
from otters_amd import _native as N
from otters_amd import Cmp, Column, DataType, Metric, MetaStore, Mode, OttersError, Path, VecStore, col
from otters_amd.vec import ResolvedBinary

pytestmark = pytest.mark.gpu

GATES = (0, 1, -1)
MIN, MAX = M.TAKE_MIN, M.TAKE_MAX


def make_store(n, words, n_bits, chunk=None, dim=1):
    store = VecStore(dim)
    if chunk:
        store.set_chunk_size(chunk)
    if n:
        store.add_vectors(np.zeros((n, dim), np.float32))
    else:
        store._handle()
    store.set_binary(words, n_bits)
    return store


def run(store, q_words, n_bits, take, k, flt=None, mask=None, chunk_mask=None, path=None):
    """the hits of every query as a list of record arrays, and the stats"""
    p = store.binary_query(q_words, n_bits)
    if flt is not None:
        p.filter(flt[1], Cmp(flt[0]))
    if mask is not None:
        p.with_row_mask(mask)
    if path is not None:
        p.with_path(path)
    (p.take_max if take == MAX else p.take_min)(k)
    hits, counts, stats = store._run_binary(p.resolve(), chunk_mask=chunk_mask)
    out, at = [], 0
    for c in counts:
        out.append(hits[at:at + c])
        at += c
    assert at == hits.size
    return out, stats


def same(got, exp, what):
    assert len(got) == len(exp), what
    for b, (g, e) in enumerate(zip(got, exp)):
        assert g.size == e.size, (what, b, g.size, e.size)
        assert np.array_equal(g["index"], e["index"]), (what, b, g["index"][:12], e["index"][:12])
        assert np.array_equal(g["score"].view(np.uint32), e["score"].view(np.uint32)), (what, b)
        assert np.array_equal(g["query"], e["query"]), (what, b)


def gated(store, gate, fn, n_bits, k):
    """fn() under binary_gate = gate; the counters' deltas per call.  gate 1 on a call the plan calls eligible MUST take the gated
    route (one gated call, no table call), gate 0 and automatic the table route; on the gated route hits <= pairs emitted <=
    rows x nq, and nothing overflows.  Returns fn's value."""
    store.set_option("binary_gate", gate)
    before = store.binary_counters()
    got, stats = fn()
    after = store.binary_counters()
    delta = {c: after[c] - before[c] for c in after}
    n_hits, nq, rows = sum(g.size for g in got), len(got), len(store)
    assert delta["overflows"] == 0, delta
    k_eff = min(k, stats["vectors_compared"] // nq)  # the rows the chunk mask leaves
    if k_eff == 0:
        assert delta["gated_calls"] == 0 and delta["table_calls"] == 0, delta
    elif gate == 1 and BR.gate_eligible(n_bits, nq, k_eff, rows):
        assert delta["gated_calls"] == 1 and delta["table_calls"] == 0, (delta, n_bits, nq, k_eff)
        assert n_hits <= delta["pairs_emitted"] <= rows * nq, (delta, n_hits)
    else:  # gate 0, automatic (the table route: BINARY_AUTO_GATE), or not eligible
        assert delta["gated_calls"] == 0 and delta["table_calls"] == 1 and delta["pairs_emitted"] == 0, (delta, gate)
    return got, stats


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [1, 64, 65, 127, 128, 129, 1024, 16384])
def test_shapes_against_the_model(n_bits):
    rng = np.random.default_rng(n_bits)
    queries = {}
    for nq in (1, 4, 5, 9):
        qb = rng.integers(0, 2, (nq, n_bits)).astype(bool)
        if nq > 1:
            qb[nq - 1] = qb[0]  # two equal queries
        queries[nq] = BR.pack(qb)
    for n in (0, 1, 63, 64, 65, 4097):
        words = BR.pack(rng.integers(0, 2, (n, n_bits)).astype(bool))  # i.i.d.: ties are dense at small n_bits
        store = make_store(n, words, n_bits)
        assert store.binary_info() == ({"n_bits": n_bits, "bytes": BR.layout_bytes(n, n_bits)})
        for nq in (1, 4, 5, 9):
            S = BR.scores(words, queries[nq])
            for k in (1, 10, 512, 513, n + 3):
                for tk in (MIN, MAX):
                    exp = BR.expected(S, tk, k)
                    for gate in GATES:
                        got, stats = gated(store, gate, lambda: run(store, queries[nq], n_bits, tk, k), n_bits, k)
                        same(got, exp, (n_bits, n, nq, k, tk, gate))
                        if n:
                            assert stats["path_used"] == int(Path.Exact) and stats["vectors_compared"] == n * nq
                            assert stats["bytes_scanned"] == stats["passes"] * BR.layout_bytes(n, n_bits)
        store.close()


def test_the_largest_histogram_that_fits():
    """n_bits = 16382: one query per pass, 64 KiB of histogram and gate word — the opt-in above 48 KiB of dynamic LDS and the gate
    scan's 256 steps; 16383 is not eligible and takes the table route under binary_gate = 1"""
    rng = np.random.default_rng(16382)
    n = 4097
    for n_bits in (16382, 16383):
        assert BR.gate_eligible(n_bits, 1, 10, n) == (n_bits == 16382) and BR.gate_tile(16382, 5) == 1
        words = BR.pack(rng.integers(0, 2, (n, n_bits)).astype(bool))
        q = BR.pack(rng.integers(0, 2, (5, n_bits)).astype(bool))
        store = make_store(n, words, n_bits)
        S = BR.scores(words, q)
        for nq, k, tk in ((1, 10, MIN), (5, 512, MAX), (1, 1, MAX)):
            exp = BR.expected(S[:nq], tk, k)
            for gate in GATES:
                got, stats = gated(store, gate, lambda: run(store, q[:nq], n_bits, tk, k), n_bits, k)
                same(got, exp, (n_bits, nq, k, tk, gate))
                assert stats["passes"] == (nq if gate == 1 and n_bits == 16382 else (nq + 3) // 4)
        store.close()


# ---- 2. one store of 200 000 x 128 bits: every wave of the persistent grid owns rows ----------------------------------------------------------------
BIG_N, BIG_BITS, BIG_CHUNK = 200000, 128, 1024


def rows_at_distance(q_bits, dist, rng):
    """rows whose Hamming distance from q_bits is dist[r]: q with the first dist[r] bits of one random order of the bits flipped"""
    rank = rng.permutation(q_bits.size)
    return (rank[None, :] < np.asarray(dist)[:, None]) ^ q_bits[None, :]


class Big:
    def __init__(self):
        self.rng = np.random.default_rng(2024)
        self.q_bits = self.rng.integers(0, 2, (2, BIG_BITS)).astype(bool)
        self.q = BR.pack(self.q_bits)
        self.store = VecStore(1)
        self.store.set_chunk_size(BIG_CHUNK)
        self.store.add_vectors(np.zeros((BIG_N, 1), np.float32))

    def set(self, bits):
        self.words = BR.pack(bits)
        self.store.set_binary(self.words, BIG_BITS)
        self.S = BR.scores(self.words, self.q)

    def check(self, what, take, k, nq=1, flt=None, keep=None, mask=None, chunk_mask=None, gates=GATES):
        exp = BR.expected(self.S[:nq], take, k, 0 if flt is None else flt[0], 0.0 if flt is None else flt[1], keep)
        for gate in gates:
            got, stats = gated(self.store, gate, lambda: run(self.store, self.q[:nq], BIG_BITS, take, k, flt, mask, chunk_mask), BIG_BITS, k)
            same(got, exp, (what, gate))
        return exp


@pytest.fixture(scope="module")
def big():
    b = Big()
    yield b
    b.store.close()


def test_big_all_rows_equal_the_hits_are_the_lowest_rows(big):
    big.set(np.broadcast_to(big.rng.integers(0, 2, BIG_BITS).astype(bool), (BIG_N, BIG_BITS)))
    for k in (1, 10, 512):
        exp = big.check(("all equal", k), MIN, k, nq=2)
        assert exp[0]["index"].tolist() == list(range(k))
    big.check("all equal, max", MAX, 10)


def test_big_the_best_rows_are_the_last_rows_or_lie_in_one_slice(big):
    k = 10
    dist = big.rng.integers(50, 80, BIG_N)
    dist[-k:] = np.arange(k)[::-1]  # the k best rows are the LAST k rows
    big.set(rows_at_distance(big.q_bits[0], dist, big.rng))
    exp = big.check("best last", MIN, k)
    assert sorted(exp[0]["index"].tolist()) == list(range(BIG_N - k, BIG_N))
    big.check("best last, two queries", MIN, k, nq=2)
    dist = big.rng.integers(50, 80, BIG_N)
    dist[64 * 1000 + 7: 64 * 1000 + 7 + k] = 3  # the k best rows all lie in one slice, tied
    big.set(rows_at_distance(big.q_bits[0], dist, big.rng))
    exp = big.check("best in one slice", MIN, k)
    assert exp[0]["index"].tolist() == list(range(64007, 64007 + k))
    big.check("best in one slice, k = 512", MIN, 512, nq=2)


def test_big_filters_masks_deleted_rows_and_chunk_runs(big):
    bits = big.rng.integers(0, 2, (BIG_N, BIG_BITS)).astype(bool)
    big.set(bits)
    d0 = big.S[0]
    order = np.argsort(d0, kind="stable")
    best100 = order[:100]
    thr = float(d0[order[99]])
    # a filter that removes the best 100 rows (and what ties with the 100th): the gate counts only rows that pass it
    exp = big.check("filter", MIN, 10, flt=(int(Cmp.Gt), thr))
    assert not np.isin(exp[0]["index"], best100).any() and (exp[0]["score"] > thr).all()
    big.check("filter, two queries, k = 512", MIN, 512, nq=2, flt=(int(Cmp.Gte), thr + 1))
    keep = np.ones(BIG_N, bool)
    keep[best100] = False
    exp = big.check("row mask", MIN, 10, keep=keep, mask=keep)
    assert not np.isin(exp[0]["index"], best100).any()
    big.store.delete_rows(best100)
    big.check("deleted rows", MIN, 10, nq=2, keep=keep)
    big.store.restore_rows(best100)
    big.check("restored rows", MIN, 10)
    n_chunks = (BIG_N + BIG_CHUNK - 1) // BIG_CHUNK
    cm = np.zeros(n_chunks, bool)
    cm[3:50] = True
    cm[120:190] = True  # two separate runs
    keep = np.repeat(cm, BIG_CHUNK)[:BIG_N]
    big.check("chunk mask, two runs", MIN, 10, nq=2, keep=keep, chunk_mask=cm)
    _, stats = run(big.store, big.q[:1], BIG_BITS, MIN, 10, chunk_mask=cm)
    assert stats["vectors_compared"] == int(keep.sum()) and stats["bytes_scanned"] == stats["passes"] * (47 + 70) * BIG_CHUNK * 16
    # take Max, with a filter on the other side
    hi = float(np.sort(d0)[-100])
    exp = big.check("take max, filter", MAX, 10, flt=(int(Cmp.Lt), hi))
    assert (exp[0]["score"] < hi).all()
    big.check("take max", MAX, 512, nq=2)


def test_big_overflow_falls_back_to_the_table_route(big):
    # sorted so that every row is at most as far as all rows before it; the last 3000 rows share the best distance, and rows tied at
    # the k-th best level pass every gate: more than 1024 pairs come out however the tiles arrive
    d = np.sort(big.rng.binomial(BIG_BITS, 0.5, BIG_N))[::-1].copy()
    d = np.maximum(d, d[-3000])
    assert (np.diff(d) <= 0).all()
    big.set(rows_at_distance(big.q_bits[0], d, big.rng))
    assert np.array_equal(big.S[0], d.astype(np.float32))
    exp = BR.expected(big.S[:1], MIN, 10)
    big.store.set_option("binary_gate", 1)
    big.store.set_option("binary_gate_cap", 1024)
    before = big.store.binary_counters()
    got, stats = run(big.store, big.q[:1], BIG_BITS, MIN, 10)
    after = big.store.binary_counters()
    big.store.set_option("binary_gate_cap", 0)
    same(got, exp, "overflow")
    assert after["overflows"] == before["overflows"] + 1 and after["table_calls"] == before["table_calls"] + 1
    assert after["gated_calls"] == before["gated_calls"] + 1 and after["pairs_emitted"] == before["pairs_emitted"] + 1024
    assert stats["passes"] == 2  # both sweeps are counted
    # with the plan's own capacity the same call stays on the gated route
    got, _ = gated(big.store, 1, lambda: run(big.store, big.q[:1], BIG_BITS, MIN, 10), BIG_BITS, 10)
    same(got, exp, "no overflow at the plan's capacity")
    assert big.store.binary_counters()["overflows"] == after["overflows"]


# ---- 3. set_binary_sign, read_binary ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 127, 128, 129, 768])
def test_set_binary_sign_and_read_binary(dim):
    rng = np.random.default_rng(dim)
    n = 200
    rows = rng.normal(size=(n, dim)).astype(np.float32)
    special = np.array([np.nan, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf], np.float32)
    at = rng.random((n, dim)) < 0.3
    rows[at] = special[rng.integers(0, special.size, int(at.sum()))]
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_binary_sign()
    want = BR.pack(BR.sign_bits(rows))
    assert store.binary_info() == {"n_bits": dim, "bytes": BR.layout_bytes(n, dim)}
    assert np.array_equal(store.read_binary(), want)
    for first, cnt in ((0, 0), (n, 0), (1, 1), (63, 3), (n // 2, n - n // 2)):
        assert np.array_equal(store.read_binary(first, cnt), want[first:first + cnt]), (first, cnt)
    # a sign query ranks by the Hamming distance of the sign bits
    q = rng.normal(size=(2, dim)).astype(np.float32)
    hits, counts = store.binary_query_sign(q).take(7).collect_arrays()
    exp = BR.query(want, BR.pack(BR.sign_bits(q)), MIN, 7)
    same([hits[:counts[0]], hits[counts[0]:]], exp, ("sign query", dim))
    # set_binary followed by read_binary is the identity
    bits = rng.integers(0, 2, (n, dim)).astype(bool)
    store.set_binary(bits)
    assert np.array_equal(store.read_binary(), BR.pack(bits))
    store.clear_binary()
    assert store.binary_info() is None
    with pytest.raises(OttersError, match="ott_store_read_binary: no bit rows are set"):
        store.read_binary()
    store.close()


# ---- 4. rescore, MetaStore ----------------------------------------------------------------------------------------------------------------------------
def test_rescore_equals_the_id_list_call_on_the_first_stages_ids():
    rng = np.random.default_rng(77)
    n, dim = 3000, 128
    rows = rng.normal(size=(n, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_binary_sign()
    q = rng.normal(size=(3, dim)).astype(np.float32)
    for gate in GATES:
        store.set_option("binary_gate", gate)
        first, counts = store.binary_query_sign(q).take(50).collect_arrays()
        assert counts == [50, 50, 50]
        got = store.binary_query_sign(q).take(50).rescore(q, Metric.Cosine, 10)
        for b in range(3):
            ids = first["index"][50 * b:50 * (b + 1)]
            want = store.query(q[b:b + 1], Metric.Cosine).with_row_ids(ids).take(10).collect()
            assert got[b] == want and len(want) == 10, (gate, b)
    store.close()


def test_meta_binary_query_with_a_meta_filter_against_the_model():
    rng = np.random.default_rng(15)
    n, nb = 1500, 200
    bits = rng.integers(0, 2, (n, nb)).astype(bool)
    words = BR.pack(bits)
    age = rng.integers(0, 100, n).astype(np.int32)
    order = np.sort(rng.integers(0, 1000, n)).astype(np.int64)  # ascending: the zone maps prune chunks
    ms = (MetaStore.from_columns([Column.from_numpy("age", DataType.Int32, age), Column.from_numpy("seq", DataType.Int64, order)])
          .with_vectors(np.zeros((n, 1), np.float32)).with_binary(bits).with_chunk_size(128).build())
    qb = rng.integers(0, 2, (2, nb)).astype(bool)
    S = BR.scores(words, BR.pack(qb))
    for expr, keep in ((col("age").lt(40), age < 40), (col("seq").gt(700), order > 700), (col("age").gte(10).and_(col("seq").lte(300)), (age >= 10) & (order <= 300)),
                       (col("seq").gt(5000), np.zeros(n, bool))):
        for gate in GATES:
            ms._store.set_option("binary_gate", gate)
            hits, counts = ms.binary_query(qb).meta_filter(expr).take(25).collect_arrays()
            got, at = [], 0
            for c in counts:
                got.append(hits[at:at + c])
                at += c
            same(got, BR.expected(S, MIN, 25, keep=keep), ("meta", int(keep.sum()), gate))
    res = ms.binary_query(qb[0]).meta_filter(col("age").lt(40)).vec_filter(95.0, Cmp.Gt).take(5).collect()
    exp = BR.expected(S[:1], MIN, 5, int(Cmp.Gt), 95.0, age < 40)[0]
    assert res.indices == exp["index"].tolist() and res.column("age").values().tolist() == age[exp["index"].astype(np.int64)].tolist()
    sign = (MetaStore.from_columns([Column.from_numpy("age", DataType.Int32, age)]).with_vectors(rng.normal(size=(n, 16)).astype(np.float32))
            .with_binary_sign().with_chunk_size(128).build())
    assert sign._store.binary_info()["n_bits"] == 16


# ---- 5. refusals, each with its message ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    rng = np.random.default_rng(10)
    n, nb = 100, 70
    bits = rng.integers(0, 2, (n, nb)).astype(bool)
    words = BR.pack(bits)
    store = make_store(n, words, nb)
    q = BR.pack(rng.integers(0, 2, (1, nb)).astype(bool))
    exp = BR.query(words, q, MIN, 5)

    def refused(fn, text, status=-1):
        with pytest.raises(OttersError) as ei:
            fn()
        assert ei.value.status == status and text in str(ei.value), str(ei.value)

    bad = words.copy()
    bad[7, -1] |= np.uint64(1) << np.uint64(nb % 64)
    refused(lambda: store.set_binary(bad, nb), "ott_store_set_binary: row 7 has a bit set at or above n_bits (70) in its last word")
    refused(lambda: store.set_binary(words[:-1], nb), "ott_store_set_binary: 99 bit rows for a store of 100 rows")
    refused(lambda: N.check(N.lib().ott_store_set_binary(store._handle(), N.ptr(words), n, 0)), "ott_store_set_binary: n_bits 0 is not in 1 .. OTT_BINARY_MAX_BITS (16384)")
    refused(lambda: N.check(N.lib().ott_store_set_binary(store._handle(), N.ptr(words), n, 16385)), "ott_store_set_binary: n_bits 16385 is not in 1 ..")
    same(run(store, q, nb, MIN, 5)[0], exp, "a refused call changes nothing")
    qbad = q.copy()
    qbad[0, -1] |= np.uint64(1) << np.uint64(63)
    refused(lambda: run(store, qbad, nb, MIN, 5), "ott_query_binary: query 0 has a bit set at or above n_bits (70) in its last word")
    refused(lambda: run(store, q, nb, MIN, 5, path=Path.Mfma), "ott_query_binary: the MFMA path does not serve binary queries", -4)
    store.set_option("tie_order", 1)
    refused(lambda: run(store, q, nb, MIN, 5), "ott_query_binary: tie_order 1 and 2 are not served", -4)
    store.set_option("tie_order", 0)
    rb = store.binary_query(q, nb).take(5).resolve()
    for metric in (Metric.Cosine, Metric.Euclidean, Metric.DotProduct):
        other = ResolvedBinary(words=rb.words, n_bits=nb, take=rb.take, k=5, filter_cmp=0, filter_thr=0.0, row_mask=None, path=0, metric=int(metric))
        refused(lambda: store._run_binary(other), "ott_query_binary: the metric must be OTT_METRIC_MANHATTAN")
    # cap too small: straight at the ABI
    d = N.QueryDesc()
    d.nq, d.metric, d.take, d.mode, d.k = 1, int(Metric.Manhattan), MIN, int(Mode.Merged), 5
    out, n_out = np.empty(4, dtype=N.HIT_DTYPE), C.c_uint64(0)
    assert N.lib().ott_query_binary(store._handle(), C.byref(d), N.ptr(q), N.ptr(out), 4, C.byref(n_out), None, None) == -1
    assert b"ott_query_binary: output capacity is smaller than nq * min(k, rows)" in N.lib().ott_last_error()
    d.mode, d.nq = int(Mode.Merged), 2
    q2 = np.vstack([q, q])
    out = np.empty(10, dtype=N.HIT_DTYPE)
    assert N.lib().ott_query_binary(store._handle(), C.byref(d), N.ptr(q2), N.ptr(out), 10, C.byref(n_out), None, None) == -1
    assert b"ott_query_binary: a batch needs OTT_MODE_PER_QUERY" in N.lib().ott_last_error()
    with pytest.raises(OttersError):
        store.set_option("binary_gate", 2)
    # a query after an append; compact() with bit rows resident
    store.add_vector([0.0])
    refused(lambda: run(store, q, nb, MIN, 5), "the bit rows cover 100 rows, the store holds 101 (rows were appended since ott_store_set_binary: set them again)")
    assert store.binary_info()["n_bits"] == nb  # the rows are left in place
    words2 = np.vstack([words, q])
    store.set_binary(words2, nb)
    got, _ = run(store, q, nb, MIN, 5)
    same(got, BR.query(words2, q, MIN, 5), "set again")
    assert got[0]["index"][0] == 100 and got[0]["score"][0] == 0.0
    refused(lambda: store.compact(), "ott_store_compact: rows cannot move while bit rows are set", -4)
    store.clear_binary()
    refused(lambda: run(store, q, nb, MIN, 5), "ott_query_binary: no bit rows are set (ott_store_set_binary)")
    store.compact()  # allowed again
    store.close()
    # a multi-GPU device list; a store whose rows are wider than a bit row can be
    multi = VecStore(1, devices=[0, 0])
    multi.add_vectors(np.zeros((n, 1), np.float32))
    refused(lambda: multi.set_binary(words, nb), "ott_store_set_binary: a multi-GPU store is not served", -4)
    refused(lambda: multi.set_binary_sign(), "ott_store_set_binary_sign: a multi-GPU store is not served", -4)
    multi.close()
    wide = VecStore(16385)
    wide.add_vectors(np.zeros((2, 16385), np.float32))
    refused(lambda: wide.set_binary_sign(), "ott_store_set_binary_sign: dim 16385 is above OTT_BINARY_MAX_BITS (16384)")
    wide.close()
