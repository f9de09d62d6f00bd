"""CPU: the rounding-sensitive sparse cases (tests/sparse_cases.py: ring_case, ring_large_case, subnormal_case, the large layout's
rows) ARE sensitive — the proof the GPU files rest on (tests/test_gpu_sparse_rounding.py, tests/test_gpu_sparse_large.py; DESIGN.md
3.1s, 3.1p).  numpy only, no GPU part.  The model (tests/sparse_ref.py: scores) runs over the cases, and beside it five MUTATIONS of
the model, each a way a reworked kernel could be wrong while every test with exact inputs still passes:
  (a) the entries added in reversed order
  (b) the product fused into the sum (emulated in f64: the product of two f32 is exact there, the sum rounds once to f64 and once to
      f32 — a mutation, not a reference)
  (c) two alternating accumulators, added at the end
  (d) the second group of SP_U = 8 entries consumed before the first (the register ring rotated wrongly); rows of 16 entries or more
  (e) products and sums below the smallest normal flushed to zero (the subnormal case)
The conditions are on the reference alone: on ring_case, over the (query, row) pairs with at least 16 shared entries, each of (a) to
(d) changes S's bits on at least 1/4 of the pairs; on subnormal_case at least 100 candidate pairs have a non-zero subnormal S and (e)
changes at least half of them.  A GPU test compares every candidate bit for bit, so one differing pair already fails it: the floors
say that a mutated kernel cannot slip through by luck.  The shares measured are printed (pytest -s) and stated beside each floor."""
import numpy as np

import sparse_cases as SC
import sparse_ref as SR

TINY = np.finfo(np.float32).tiny


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def dense_operands(rows, query, vocab):
    """(V, W, shared): row r's values and the query's weight at each of its indices (+0.0 outside the query, as the kernel's table
    holds it), padded with +0.0 to the longest row; shared[r] = the entries row r shares with the query"""
    n, width = len(rows), max(max(len(i) for i, _ in rows), 1)
    w, present = np.zeros(vocab, np.float32), np.zeros(vocab, bool)
    w[query[0].astype(np.int64)] = query[1]
    present[query[0].astype(np.int64)] = True
    V, W, shared = np.zeros((n, width), np.float32), np.zeros((n, width), np.float32), np.zeros(n, np.int64)
    for r, (i, v) in enumerate(rows):
        V[r, : len(i)], W[r, : len(i)] = v, w[i.astype(np.int64)]
        shared[r] = int(present[i.astype(np.int64)].sum())
    return V, W, shared


def serial(V, W, order=None, fused=False, flush=False):
    """S of every row: column after column of `order` (None: ascending), one rounded f32 operation at a time unless `fused`; a padded
    column adds fl(0 x 0) = +0.0, which leaves S's bits alone (S is never -0.0)"""
    S = np.zeros(V.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for p in range(V.shape[1]) if order is None else order:
            if fused:
                S = (S.astype(np.float64) + V[:, p].astype(np.float64) * W[:, p].astype(np.float64)).astype(np.float32)
                continue
            prod = V[:, p] * W[:, p]
            if flush:
                prod = np.where(np.abs(prod) < TINY, np.float32(0.0), prod)
            S = S + prod
            if flush:
                S = np.where(np.abs(S) < TINY, np.float32(0.0), S)
    assert S.dtype == np.float32
    return S


def reversed_rows(rows):
    return [(i[::-1], v[::-1]) for i, v in rows]


def two_accumulators(V, W):
    with np.errstate(all="ignore"):
        return serial(V[:, 0::2], W[:, 0::2]) + serial(V[:, 1::2], W[:, 1::2])


def second_group_first(width):
    return list(range(SC.SP_U, 2 * SC.SP_U)) + list(range(SC.SP_U)) + list(range(2 * SC.SP_U, width))


def test_the_ring_case_has_the_shape_the_kernels_edges_need():
    rows, vocab, queries = SC.ring_case(np.random.default_rng(21))
    lens = np.array([len(i) for i, _ in rows])
    assert vocab == 512 and len(rows) == 301 and set(SC.RING_LENS) <= set(lens.tolist()) and lens[-1] == 0
    assert (lens[128:192] == 2 * SC.SP_U).all() and (lens[192:256] == 2 * SC.SP_U + 1).all()
    for t in (0, 64, 256):  # the lanes of a cycling slice differ
        assert np.unique(lens[t:t + 45]).size >= 10
    for m in (8, 16, 24, 32):  # both sides of every multiple of SP_U up to 32
        assert {m - 1, m, m + 1} <= set(SC.RING_LENS)
    vals = np.concatenate([v for _, v in rows])
    assert ((np.abs(vals) >= 0.5) & (np.abs(vals) < 1.0)).all() and (vals < 0).any() and (vals > 0).any()
    assert (bits(vals) & 0xFF).astype(bool).mean() > 0.98  # full mantissas: the low byte is in use
    assert len(queries) == 5 and len({q[1].tobytes() for q in queries}) == 5
    for qi, qw in queries:
        assert qi.size == 400 == np.unique(qi).size and (np.diff(qi.astype(np.int64)) < 0).any()  # shuffled
        assert ((np.abs(qw) >= 0.5) & (np.abs(qw) < 2.0)).all() and (bits(qw) & 0xFF).astype(bool).mean() > 0.98
    for vocab in (32769, 1 << 20):
        rows, v, queries = SC.ring_large_case(np.random.default_rng(vocab), vocab)
        pool = SC.used_indices(rows)
        assert v == vocab and pool[0] == 0 and pool[-1] == vocab - 1 and pool.size <= 360
        _, counts = np.unique(pool >> 3, return_counts=True)
        assert (counts == 8).sum() >= 30  # eight consecutive indices: one word of presence nibbles


def test_the_dense_evaluation_equals_the_definition_on_the_new_cases():
    cases = [c for c in SC.cpu_cases() if c[0].startswith(("ring", "subnormal"))]
    assert len(cases) == 4
    for name, rows, vocab, queries in cases:
        ptr, idx, val = SR.csr(rows)
        S, cand = SR.scores(ptr, idx, val, queries, vocab)
        Sd, candd = SR.scores(ptr, idx, val, queries, vocab, dense=True)
        assert np.array_equal(bits(S), bits(Sd)) and np.array_equal(cand, candd), name
        assert not np.isnan(S).any() and not (bits(S) == 0x80000000).any(), name
        for b, q in enumerate(queries):  # ... and this file's column-wise statement of it, which the mutations are mutations of
            V, W, shared = dense_operands(rows, q, vocab)
            assert np.array_equal(bits(serial(V, W)), bits(S[b])) and np.array_equal(shared > 0, cand[b]), (name, b)


def test_ring_case_every_mutation_of_the_order_and_the_rounding_changes_the_bits():
    rows, vocab, queries = SC.ring_case(np.random.default_rng(21))
    ptr, idx, val = SR.csr(rows)
    S, _ = SR.scores(ptr, idx, val, queries, vocab)
    Srev, _ = SR.scores(*SR.csr(reversed_rows(rows)), queries, vocab)  # (a) through the model itself
    changed = {m: 0 for m in "abcd"}
    pairs = 0
    for b, q in enumerate(queries):
        V, W, shared = dense_operands(rows, q, vocab)
        long = shared >= 16
        pairs += int(long.sum())
        changed["a"] += int((bits(Srev[b]) != bits(S[b]))[long].sum())
        changed["b"] += int((bits(serial(V, W, fused=True)) != bits(S[b]))[long].sum())
        changed["c"] += int((bits(two_accumulators(V, W)) != bits(S[b]))[long].sum())
        changed["d"] += int((bits(serial(V, W, order=second_group_first(V.shape[1]))) != bits(S[b]))[long].sum())
    share = {m: changed[m] / pairs for m in changed}
    print(f"ring_case: {pairs} (query, row) pairs with 16 shared entries or more; the share whose bits change under "
          f"(a) reversed order {share['a']:.3f}, (b) fused product {share['b']:.3f}, (c) two accumulators {share['c']:.3f}, "
          f"(d) second group of eight first {share['d']:.3f}")
    assert pairs >= 300  # (a query holds 400 of 512 indices: the rows of 23 entries or more, about 95 of the 301, share 16 with most queries)
    # measured: (a) 0.843, (b) 0.686, (c) 0.784, (d) 0.308 of 491 pairs ((d) moves only the first 16 entries: in a row of 300 the later
    # roundings absorb it more often than not); the floor is 1/4
    assert all(s >= 0.25 for s in share.values()), share


def test_the_large_vocab_ring_cases_are_sensitive_too():
    for vocab in (32769, 1 << 20):
        rows, _, queries = SC.ring_large_case(np.random.default_rng(vocab), vocab)
        S, cand = SR.scores(*SR.csr(rows), queries, vocab)
        Srev, _ = SR.scores(*SR.csr(reversed_rows(rows)), queries, vocab)
        lens = np.array([len(i) for i, _ in rows])
        long = cand & (lens >= 24)[None, :]
        assert long.sum() >= 300 and (bits(Srev) != bits(S))[long].mean() >= 0.25, vocab


def test_subnormal_case_a_flush_to_zero_changes_the_bits():
    rows, vocab, queries = SC.subnormal_case(np.random.default_rng(22))
    S, cand = SR.scores(*SR.csr(rows), queries, vocab)
    vals, weights = np.concatenate([v for _, v in rows]), np.concatenate([w for _, w in queries])
    assert ((np.abs(vals) >= 1e-20) & (np.abs(vals) < 1e-19)).all() and ((np.abs(weights) >= 1e-25) & (np.abs(weights) < 1e-19)).all()
    assert {len(i) for i, _ in rows} == set(range(1, 41))
    sub = cand & (S != 0) & (np.abs(S) < TINY)
    changed = 0
    for b, q in enumerate(queries):
        V, W, _ = dense_operands(rows, q, vocab)
        changed += int((bits(serial(V, W, flush=True)) != bits(S[b]))[sub[b]].sum())
    print(f"subnormal_case: {int(sub.sum())} of {int(cand.sum())} candidate pairs have a non-zero subnormal S; (e) a flush to zero changes {changed} of them")
    # measured: 1446 of 1486 candidate pairs, all 1446 changed
    assert sub.sum() >= 100 and changed * 2 >= sub.sum()
    assert not (bits(S) == 0x80000000).any()


def test_a_wrapped_entry_offset_gives_the_long_rows_past_2_32_bytes_other_bits():
    """the large layout (sparse_cases.large_case): slices 512 to 519 lie past byte 2^32 of the index array.  A kernel whose entry byte
    offset wraps mod 2^32 reads, for the long row of slice t, entries of the long row of slice t - 512 (the two rows sit at the same
    lane: 7 x 512 is a multiple of 64) or padding; the rows differ, so S's bits do — and below the line nothing changes"""
    assert SC.LARGE_SLICES * SC.LARGE_SLICE_ENTRIES * 4 > 1 << 32 > 512 * SC.LARGE_SLICE_ENTRIES * 4
    assert (1 << 29) // SC.LARGE_SLICE_ENTRIES == 256 and (1 << 30) // SC.LARGE_SLICE_ENTRIES == 512
    past = [64 * t + SC.large_long_lane(t) for t in range(512, SC.LARGE_SLICES)]
    below = [64 * t + SC.large_long_lane(t) for t in (0, 1, 255, 256, 511)]
    for t in range(512, SC.LARGE_SLICES):
        assert SC.large_long_lane(t) == SC.large_long_lane(t - 512)
        a, b = SC.large_row(64 * t + SC.large_long_lane(t)), SC.large_row(64 * (t - 512) + SC.large_long_lane(t))
        assert a[0].size == b[0].size == SC.LARGE_LONG and (bits(a[1]) != bits(b[1])).mean() > 0.99
    rng = np.random.default_rng(5)
    queries = [SC.ring_query(rng, np.arange(SC.LARGE_VOCAB, dtype=np.uint32), 24000)]
    true = [SC.large_row(r) for r in past + below]
    wrapped = [SC.large_wrapped_row(r) for r in past + below]
    for (ti, tv), (wi, wv) in zip(true[len(past):], wrapped[len(past):]):
        assert np.array_equal(ti, wi) and np.array_equal(bits(tv), bits(wv))  # below the line a wrapped offset is the offset
    # slice 512's first 512 entries lie below the line too; from entry 512 on it reads the long row of slice 0
    assert np.array_equal(wrapped[0][0][:512], true[0][0][:512]) and np.array_equal(wrapped[0][1][512:600], SC.large_row(0)[1][:88])
    S, cand = SR.scores(*SR.csr(true[: len(past)] + wrapped[: len(past)]), queries, SC.LARGE_VOCAB, dense=True)
    assert cand.all() and (bits(S[0, : len(past)]) != bits(S[0, len(past):])).all()
