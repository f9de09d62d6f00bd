"""GPU: the parts of ott_query_binary and the bit rows' staging that tests/test_gpu_binary.py never runs, against the
numpy model (tests/binary_ref.py) bit for bit — index, the score's f32 bits, order, count and `query` — on the table route
(binary_gate 0), the gated route (1) and automatic (-1), the route asserted from binary_counters() by test_gpu_binary.gated.

  a. chunk runs that cut 64-row slices: chunks of 8, 100 and 1021 rows, up to 313 runs, four runs in one slice, slices with a few
     surviving lanes; stats.bytes_scanned against the model's count of distinct slices
  b. every tile of the gated route on both sides of each line where the tile or the 48-KiB LDS opt-in changes
  c. the histogram's last level, h[n_bits], beside the gate word
  d. the layout staged in two 32-MiB batches, the second at an offset that is a multiple of nothing but a slice
  e. sign queries that hold NaN, zeros, denormals and infinities
  f. binary calls between grouped, per-query-mask and recommend calls on one store: the scratch they share"""
import numpy as np
import pytest

import binary_ref as BR
import grouped_ref as GR
import masks_ref as MKR
import recommend_ref as RR
import test_gpu_groups_top as GT
import test_gpu_masks as TMK
import test_gpu_recommend as TR
from otters_amd import Cmp, Metric, OttersError, Path, VecStore
from test_gpu_binary import GATES, MAX, MIN, gated, make_store, rows_at_distance, run, same

pytestmark = pytest.mark.gpu


def random_words(rng, n, n_bits):
    """uint64 [n, words]: i.i.d. bits, padding bits zero"""
    W = BR.words(n_bits)
    w = rng.integers(0, 2 ** 64, (n, W), dtype=np.uint64)
    if n_bits % 64:
        w[:, -1] &= np.uint64((1 << (n_bits % 64)) - 1)
    return w


def table_tile(nq):
    return 4 if nq >= 4 else 2 if nq >= 2 else 1


def passes_of(gate, n_bits, nq, k_eff, rows):
    """the passes a call that scores at least one row takes: ceil(nq / tile), the gated route's tile where the call takes it"""
    tile = BR.gate_tile(n_bits, nq) if gate == 1 and BR.gate_eligible(n_bits, nq, k_eff, rows) else table_tile(nq)
    return -(-nq // tile)


# ---- a. chunk runs that start and end inside slices ---------------------------------------------------------------------------------
N_A, BITS_A = 5000, 200


def chunk_masks(rng, n_chunks):
    i = np.arange(n_chunks)
    ends = np.zeros(n_chunks, bool)
    ends[[0, -1]] = True
    all_but_one = np.ones(n_chunks, bool)
    all_but_one[n_chunks // 2] = False
    return {"every second": i % 2 == 0, "one of seven": i % 7 == 3, "first and last": ends, "random": rng.random(n_chunks) < 0.5,
            "all but one": all_but_one, "none": np.zeros(n_chunks, bool)}


def n_runs(mask):
    return int(np.count_nonzero(np.diff(np.r_[False, mask].astype(np.int8)) == 1))


@pytest.mark.parametrize("chunk", [8, 100, 1021])
def test_chunk_runs_that_cut_slices(chunk):
    rng = np.random.default_rng(chunk)
    assert N_A % 64 and chunk % 64 and (chunk != 1021 or N_A % chunk)  # the last slice is partial; so is the last chunk of 1021 rows
    words = random_words(rng, N_A, BITS_A)
    store = make_store(N_A, words, BITS_A, chunk=chunk)
    q = random_words(rng, 5, BITS_A)
    S = BR.scores(words, q)
    n_chunks = -(-N_A // chunk)
    units = BR.units(BITS_A)
    masks = chunk_masks(rng, n_chunks)
    if chunk == 8:  # 313 runs, four of them in every slice
        assert n_runs(masks["every second"]) == 313
        keep = np.repeat(masks["every second"], 8)[:N_A]
        assert all(n_runs(keep[t:t + 64]) == 4 for t in range(0, N_A - 64, 64))
    for name, cm in masks.items():
        keep = np.repeat(cm, chunk)[:N_A]
        kept = int(keep.sum())
        per_pass = BR.run_bytes(keep, units)
        assert (kept == 0) == (name == "none") and per_pass <= BR.layout_bytes(N_A, BITS_A)
        for nq in (1, 3, 5):
            for k in (1, 10, 513):
                for tk in (MIN, MAX):
                    exp = BR.expected(S[:nq], tk, k, keep=keep)
                    for gate in GATES:
                        where = (chunk, name, nq, k, tk, gate)
                        got, stats = gated(store, gate, lambda: run(store, q[:nq], BITS_A, tk, k, chunk_mask=cm), BITS_A, k)
                        same(got, exp, where)
                        assert stats["vectors_compared"] == kept * nq, (where, stats)
                        if kept:
                            assert stats["passes"] == passes_of(gate, BITS_A, nq, min(k, kept), N_A), (where, stats)
                            assert stats["bytes_scanned"] == stats["passes"] * per_pass, (where, stats, per_pass)
                        else:
                            assert stats["passes"] == 0 and stats["bytes_scanned"] == 0 and sum(g.size for g in got) == 0, (where, stats)
    # composed: the chunk mask, a row mask, deleted rows and a filter at once
    cm = masks["random"] if masks["random"].any() else masks["every second"]
    mask = rng.random(N_A) < 0.7
    dead = rng.choice(N_A, 200, replace=False)
    store.delete_rows(dead)
    keep = np.repeat(cm, chunk)[:N_A] & mask
    keep[dead] = False
    flt = (int(Cmp.Gte), 95.0)  # (the distances of i.i.d. rows of 200 bits centre on 100)
    for k in (10, 513):
        for tk in (MIN, MAX):
            exp = BR.expected(S[:3], tk, k, flt[0], flt[1], keep)
            assert 0 < exp[0].size
            for gate in GATES:
                got, stats = gated(store, gate, lambda: run(store, q[:3], BITS_A, tk, k, flt, mask, cm), BITS_A, k)
                same(got, exp, (chunk, "composed", k, tk, gate))
                assert stats["bytes_scanned"] == stats["passes"] * BR.run_bytes(np.repeat(cm, chunk)[:N_A], units)
    store.close()


# ---- b. the gated route's tiles and the LDS opt-in ----------------------------------------------------------------------------------
TILE_BITS = (3070, 3071, 4094, 4095, 6142, 6143, 8190, 8191, 12286, 12287)
N_B = 1025  # 17 slices, the last one partial


def test_the_widths_lie_on_both_sides_of_every_line():
    """(no device work) a tile of 4, 2 and 1 forced by the LDS budget, each with and without the opt-in above 48 KiB of dynamic LDS"""
    seen = {(BR.gate_tile(b, 4), BR.gate_tile(b, 4) * BR.gate_query_lds(b) > 48 * 1024) for b in TILE_BITS}
    assert seen == {(t, big) for t in (4, 2, 1) for big in (False, True)}
    assert [BR.gate_tile(b, 4) for b in TILE_BITS] == [4, 4, 4, 2, 2, 2, 2, 1, 1, 1]
    assert [BR.gate_tile(b, 4) * BR.gate_query_lds(b) for b in (3070, 3071, 6142, 6143, 12286, 12287)] == [49152, 49168, 49152, 49160, 49152, 49156]
    assert BR.gate_tile(4094, 4) * BR.gate_query_lds(4094) == BR.gate_tile(8190, 2) * BR.gate_query_lds(8190) == BR.GATE_LDS_BYTES


@pytest.mark.parametrize("n_bits", TILE_BITS)
def test_gate_tiles_on_both_sides_of_the_lds_lines(n_bits):
    rng = np.random.default_rng(n_bits)
    words = random_words(rng, N_B, n_bits)
    store = make_store(N_B, words, n_bits)
    q = random_words(rng, 7, n_bits)
    q[6] = q[0]  # two equal queries, in different passes at every tile
    S = BR.scores(words, q)
    for nq in (1, 2, 3, 4, 5, 7):
        for k in (1, 10, 512):
            for tk in (MIN, MAX):
                exp = BR.expected(S[:nq], tk, k)
                for gate in GATES:
                    got, stats = gated(store, gate, lambda: run(store, q[:nq], n_bits, tk, k), n_bits, k)
                    same(got, exp, (n_bits, nq, k, tk, gate))
                    if gate == 1:
                        assert stats["passes"] == -(-nq // BR.gate_tile(n_bits, nq)), (n_bits, nq, stats)
                    else:
                        assert stats["passes"] == -(-nq // (4 if nq >= 4 else 2 if nq >= 2 else 1)), (n_bits, nq, stats)
                    assert stats["bytes_scanned"] == stats["passes"] * BR.layout_bytes(N_B, n_bits)
    store.close()


# ---- c. the last level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [1, 64, 65, 128, 4094, 8190, 16382])
def test_the_last_histogram_level(n_bits):
    """distance n_bits under take Min and distance 0 under take Max are level n_bits: h[n_bits], the word in front of the gate word.
    k = 10 is more than the rows, so no gate falls below it"""
    rng = np.random.default_rng(n_bits)
    q_bits = rng.integers(0, 2, (1, n_bits)).astype(bool)
    q = BR.pack(np.vstack([q_bits, ~q_bits]))  # (the complement within n_bits: pack leaves the padding bits zero)
    words = np.vstack([q[:1], q[1:], random_words(rng, 7, n_bits)])
    words = words[rng.permutation(9)]
    store = make_store(9, words, n_bits)
    S = BR.scores(words, q)
    assert sorted(S[0].tolist())[0] == 0.0 and sorted(S[0].tolist())[-1] == float(n_bits)
    for nq in (1, 2):
        for tk in (MIN, MAX):
            exp = BR.expected(S[:nq], tk, 10)
            for b in range(nq):
                assert exp[b].size == 9 and {exp[b]["score"][0], exp[b]["score"][-1]} == {0.0, float(n_bits)}
            for gate in GATES:
                got, _ = gated(store, gate, lambda: run(store, q[:nq], n_bits, tk, 10), n_bits, 10)
                same(got, exp, (n_bits, nq, tk, gate))
    # 70 rows, all the complement: ten of them tie at the last level, the lowest rows win
    words = np.repeat(q[1:], 70, axis=0)
    store.close()
    store = make_store(70, words, n_bits)
    S = BR.scores(words, q)
    assert (S[0] == n_bits).all() and (S[1] == 0).all()
    for nq in (1, 2):
        for tk in (MIN, MAX):
            exp = BR.expected(S[:nq], tk, 10)
            assert exp[0]["index"].tolist() == list(range(10))
            for gate in GATES:
                got, _ = gated(store, gate, lambda: run(store, q[:nq], n_bits, tk, 10), n_bits, 10)
                same(got, exp, (n_bits, "all equal", nq, tk, gate))
    store.close()


# ---- d. the layout staged in two batches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [16384 - 127, 16384 - 128])
def test_staging_in_two_batches(n_bits):
    """258 * 64 + 65 rows, 260 slices, about 34 MB of layout: set_binary and read_binary stage it in two 32-MiB batches.
    16256 bits are 127 units: a slice is 130048 bytes, 258 of them fit a batch with 2048 bytes to spare, so the second batch begins
    at slice 258 = row 16512, byte 33552384: a multiple of no power of two above 2048.  16257 bits are 128 units: a batch is 256
    slices to the byte and the second begins at row 16384.  The ranges and the planted rows lie around each width's own edge"""
    n = 258 * 64 + 65
    per_batch = (32 << 20) // (BR.units(n_bits) * 1024)
    B = per_batch * 64
    assert (BR.units(n_bits), per_batch, (32 << 20) % (BR.units(n_bits) * 1024)) == ((127, 258, 2048) if n_bits == 16256 else (128, 256, 0))
    assert per_batch < -(-n // 64) <= 2 * per_batch and BR.layout_bytes(n, n_bits) > 32 << 20  # two batches
    rng = np.random.default_rng(16257)
    words = random_words(rng, n, n_bits)
    q_bits = rng.integers(0, 2, (2, n_bits)).astype(bool)
    q = BR.pack(q_bits)
    near = np.r_[B - 5:B + 5]                       # the ten best rows of query 0 under take Min, on both sides of the batch edge
    far = np.r_[B - 10:B - 5, B + 5:B + 10]         # ... and under take Max
    words[near] = BR.pack(rows_at_distance(q_bits[0], rng.permutation(10), rng))
    words[far] = BR.pack(rows_at_distance(q_bits[0], n_bits - rng.permutation(10), rng))
    store = make_store(n, words, n_bits)
    assert store.binary_info() == {"n_bits": n_bits, "bytes": BR.layout_bytes(n, n_bits)}
    assert np.array_equal(store.read_binary(), words)
    for first, cnt in ((B - 100, 100), (B, 65), (B - 70, 135), (B - 1, 1), (B, 1), (B - 1, 2), (0, B), (1, n - 1), (n - 1, 1)):
        assert np.array_equal(store.read_binary(first, cnt), words[first:first + cnt]), (first, cnt)
    S = BR.scores(words, q)
    for tk, planted in ((MIN, near), (MAX, far)):
        exp = BR.expected(S, tk, 10)
        assert sorted(exp[0]["index"].tolist()) == planted.tolist()
        assert exp[0]["score"].tolist() == [float(d if tk == MIN else n_bits - d) for d in range(10)]
        for gate in GATES:
            got, _ = gated(store, gate, lambda: run(store, q, n_bits, tk, 10), n_bits, 10)
            same(got, exp, ("two batches", n_bits, tk, gate))
    store.close()


# ---- e. sign queries with special values ----------------------------------------------------------------------------------------------
SPECIAL = np.array([np.nan, 0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 1e-40, -1e-40, np.inf, -np.inf], np.float32)


@pytest.mark.parametrize("dim", [1, 129, 768])
def test_sign_queries_with_special_values(dim):
    rng = np.random.default_rng(dim)
    n = 200
    rows = rng.normal(size=(n, dim)).astype(np.float32)
    at = rng.random((n, dim)) < 0.3
    rows[at] = SPECIAL[rng.integers(0, SPECIAL.size, int(at.sum()))]
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_binary_sign()
    want = BR.pack(BR.sign_bits(rows))
    assert np.array_equal(store.read_binary(), want)
    if dim == 1:  # every special value as a query of its own, and two normal ones
        q = np.r_[SPECIAL, np.float32([1.5, -1.5])][:, None].astype(np.float32)
    else:
        q = rng.normal(size=(4, dim)).astype(np.float32)
        at = rng.random(q.shape) < 0.4
        q[at] = SPECIAL[rng.integers(0, SPECIAL.size, int(at.sum()))]
        for j, v in zip((0, 63, 64, 127, 128, 2, 1, 65, 126), SPECIAL):  # every one of them, at the words' edges
            q[0, j] = v
    assert SPECIAL.view(np.uint32).tolist() == [0x7FC00000, 0, 0x80000000, 1, 0x80000001, 71362, 0x80000000 + 71362, 0x7F800000, 0xFF800000]
    assert BR.sign_bits(SPECIAL).tolist() == [False, False, False, True, False, True, False, True, False]
    q_words = BR.pack(BR.sign_bits(q))
    nq = q.shape[0]
    for tk in (MIN, MAX):
        exp = BR.query(want, q_words, tk, 7)
        for gate in GATES:

            def call():
                p = store.binary_query_sign(q)
                (p.take_max if tk == MAX else p.take_min)(7)
                rb = p.resolve()
                assert rb.n_bits == dim and np.array_equal(rb.words, q_words)  # the host's packing of the query is the device's rule
                hits, counts, stats = store._run_binary(rb)
                return np.split(hits, np.cumsum(counts)[:-1]), stats

            got, _ = gated(store, gate, call, dim, 7)
            same(got, exp, ("sign query", dim, nq, tk, gate))
    store.close()


# ---- f. between the other kinds -------------------------------------------------------------------------------------------------------
def test_binary_calls_between_grouped_masks_and_recommend_calls(oracle):
    """One store, one context: the table route writes d_gtable and leaves it zeroed for grouped search, the masks sweep and
    recommend, which do the same for it; the gated route's pair arrays are the grouped top-k's pair form's (k 600).  Every call is
    held to the model its own test file uses, twice round, with a refused binary call and an overflowing gated call in between"""
    n, dim = 3000, 128
    rng, rows, qd = TMK.corpus(n, dim, 31, nq=5)
    store = VecStore(dim)
    store.add_vectors(rows)
    labels = rng.integers(0, 800, n)  # more than 512 groups: take(600) goes through the pair form, whose arrays the gated route fills
    store.set_groups(labels)
    gid = GR.dense(labels)
    assert gid.max() + 1 > 600
    store.set_binary_sign()
    inv = store.inv_norms()
    want = BR.pack(BR.sign_bits(rows))
    assert np.array_equal(store.read_binary(), want)
    qw = BR.pack(BR.sign_bits(rng.normal(size=(5, dim)).astype(np.float32)))
    S = BR.scores(want, qw)
    metric, take = Metric.DotProduct, 1
    full = {nq: GR.ranking(oracle, rows, qd[:nq], metric, take) for nq in (1, 5)}
    keep_all = np.ones(n, bool)
    masks = TMK.random_masks(rng, n, 5)
    masks_exp = MKR.expected(oracle, rows, qd, masks, metric, take, 20)
    pos, neg = TR.examples(rng, n, 5, 3)
    rec_exp = RR.recommend(oracle, rows, inv, pos, neg, metric, take, 10, flags=RR.FILL)

    def binary(gate, nq, k, tk, where):
        got, stats = gated(store, gate, lambda: run(store, qw[:nq], dim, tk, k), dim, k)
        same(got, BR.expected(S[:nq], tk, k), where)

    def grouped(nq, m, k, where):
        ref, ref_counts, ref_groups = GR.expected(full[nq], gid, keep_all, k, nq, m)
        got, counts, groups = GT.build(store, qd[:nq], metric, m, k, perq=nq > 1).collect_arrays()
        GR.bits_equal(got, ref, where)
        assert list(counts) == ref_counts and np.array_equal(groups, ref_groups), where

    def masks_sweep(where):
        got, st = TMK.run(store, qd, masks, metric, take, 20, TMK.SWEEP)
        TMK.same(got, masks_exp, where)
        assert st["passes"] == 2, st

    def refused(where):
        """rows of 128 bits have no padding bit a query could set: the refusals a 128-bit store has are a path and a tie order it
        does not serve.  Neither reaches the device, neither counts"""
        before = store.binary_counters()
        with pytest.raises(OttersError, match="ott_query_binary: the MFMA path does not serve binary queries"):
            run(store, qw[:2], dim, MIN, 10, path=Path.Mfma)
        store.set_option("tie_order", 1)
        try:
            with pytest.raises(OttersError, match="ott_query_binary: tie_order 1 and 2 are not served"):
                run(store, qw[:2], dim, MIN, 10)
        finally:
            store.set_option("tie_order", 0)
        assert store.binary_counters() == before, where

    def overflow(where):
        store.set_option("binary_gate", 1)
        store.set_option("binary_gate_cap", 4)  # the ten best rows pass every gate: more than four pairs come out
        before = store.binary_counters()
        try:
            got, stats = run(store, qw[:1], dim, MIN, 10)
        finally:
            store.set_option("binary_gate_cap", 0)
        after = store.binary_counters()
        same(got, BR.expected(S[:1], MIN, 10), where)
        assert {c: after[c] - before[c] for c in after} == {"gated_calls": 1, "pairs_emitted": 4, "overflows": 1, "table_calls": 1}, where
        assert stats["passes"] == 2

    try:
        for rnd in range(2):
            binary(0, 5, 10, MIN, (rnd, "table route, k 10"))
            grouped(5, 3, 10, (rnd, "grouped search"))
            binary(0, 2, 600, MAX, (rnd, "table route, k 600: the pair form"))
            masks_sweep((rnd, "masks sweep"))
            binary(1, 3, 10, MIN, (rnd, "gated route"))
            refused((rnd, "refused"))
            RR.same(TR.run(store, pos, neg, metric, take, 10, fill=True), rec_exp, (rnd, "recommend"))
            binary(1, 5, 512, MAX, (rnd, "gated route, k 512"))
            overflow((rnd, "gated route, overflow"))
            grouped(1, 1, 10, (rnd, "grouped search again"))
            grouped(1, 2, 600, (rnd, "grouped search, the pair form"))
    finally:
        store.set_option("masks_sweep", 2)
        store.close()
