"""Shared cases of the sparse tests (tests/test_sparse_cpu.py, tests/test_sparse_rounding_cpu.py, tests/test_gpu_sparse.py,
tests/test_gpu_sparse_rounding.py, tests/test_gpu_sparse_large.py): generators of sparse rows and queries, and the case list the CPU
tests hold the plan header's C statement of the score to.

Two families.  random_rows / random_query, ieee_case, divergent_case: values are multiples of 1/4 and weights multiples of 1/2, so
every product and every partial sum is exact, and exact ties in S (and sums that cancel to +0.0) are frequent — these cases test the
selection, the masks and the overlap rule, and say nothing about the order or the rounding of the sum.  ring_case, ring_large_case,
subnormal_case, large_case and cpu_cases()' "rounding": values and weights with full 24-bit mantissas, so every product and every
partial sum rounds and the bits of S depend on the order of the additions, on whether a product is fused into the sum and on whether
subnormals are kept (tests/test_sparse_rounding_cpu.py measures how much, on the model alone)."""
import numpy as np


def random_rows(rng, n, vocab, mean_len, empty_frac=0.1, pool=None):
    """n rows of about mean_len entries: ascending distinct indices (from `pool`, an index array, when given), values in
    -1 .. 1 by quarters, 0.0 among them"""
    rows = []
    for _ in range(n):
        L = 0 if rng.random() < empty_frac else max(1, int(rng.poisson(mean_len)))
        src = rng.integers(0, vocab, L) if pool is None else pool[rng.integers(0, pool.size, L)]
        idx = np.unique(src).astype(np.uint32)
        val = (rng.integers(-4, 5, idx.size) / 4.0).astype(np.float32)
        rows.append((idx, val))
    return rows


def random_query(rng, vocab, L, pool=None):
    """distinct indices in no particular order, weights in -2 .. 2 by halves, 0.0 among them"""
    src = rng.integers(0, vocab, L) if pool is None else pool[rng.integers(0, pool.size, L)]
    idx = np.unique(src).astype(np.uint32)
    rng.shuffle(idx)
    return idx, (rng.integers(-4, 5, idx.size) / 2.0).astype(np.float32)


def used_indices(rows):
    parts = [i for i, _ in rows if len(i)]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint32)


def f32(*x):
    return np.array(x, np.float32)


def u32(*x):
    return np.array(x, np.uint32)


def ieee_case():
    """vocab 31: subnormal products, -0.0, overflow to +-inf, inf - inf (a dropped row), sums that cancel to +0.0, a stored 0.0 at
    a shared index, a row that shares nothing, an empty row"""
    rows = [
        (u32(0), f32(3e38)),                         # 0: 3e38 * 3e38 = +inf
        (u32(0, 1), f32(3e38, 3e38)),                # 1: +inf + (3e38 * -3e38 = -inf) = NaN: dropped
        (u32(1), f32(3e38)),                         # 2: -inf
        (u32(2), f32(1e-20)),                        # 3: 1e-20 * 1e-25 = 1e-45: a subnormal product, kept
        (u32(2, 3), f32(1e-20, -1e-20)),             # 4: two subnormal products that cancel: +0.0, a hit
        (u32(4), f32(-0.0)),                         # 5: -0.0 * 1 = -0.0; +0.0 + -0.0 = +0.0
        (u32(4, 5), f32(1.0, -1.0)),                 # 6: 1 - 1 = +0.0, a hit
        (u32(5), f32(0.0)),                          # 7: a stored 0.0 at a shared index: a hit with S = +0.0
        (u32(6), f32(0.0)),                          # 8: 0.0 * -2 = -0.0 -> S = +0.0
        (u32(7, 8), f32(1.0, 2.0)),                  # 9: shares nothing with the query: no hit
        (u32(), f32()),                              # 10: no entries: no hit
        (u32(4, 5, 6, 30), f32(0.25, 0.5, -0.75, 8.0)),  # 11: an ordinary row; index 30 is the last of the vocab
        (u32(0, 2, 4, 9), f32(1e-38, 1.0, 1.0, 5.0)),    # 12: 3e38 * 1e-38 = 3, + 1e-25 (lost), + 1; index 9 carries weight 0.0
        (u32(9), f32(7.0)),                              # 13: only the index whose weight is 0.0: a hit with S = +0.0
    ]
    q = (u32(30, 0, 1, 2, 3, 4, 5, 6, 9), f32(-0.5, 3e38, -3e38, 1e-25, 1e-25, 1.0, 1.0, -2.0, 0.0))
    q2 = (u32(5, 4), f32(-1.0, 1.0))
    return rows, 31, [q, q2]


def divergent_case(rng, n=200, vocab=32768):
    """rows of 3 entries with one row of 300 among them in the second slice, a slice whose rows are all empty, duplicated rows"""
    rows = random_rows(rng, n, vocab, 3, empty_frac=0.0, pool=np.arange(0, 600, dtype=np.uint32))
    rows = [(i[:3], v[:3]) for i, v in rows]
    long_idx = np.arange(0, 600, 2, dtype=np.uint32)
    rows[70] = (long_idx, (rng.integers(-4, 5, long_idx.size) / 4.0).astype(np.float32))
    for r in range(128, min(192, n)):
        rows[r] = (u32(), f32())
    for r in (5, 66, 199):
        if r < n:
            rows[r] = rows[3]  # duplicates of row 3: ties go to the lower row
    return rows, vocab


# ---- rounding-sensitive cases: full mantissas, so the order of the sum, a fused product and a flush to zero all show in S's bits ---------

SP_U = 8  # ott_sparse.hip: the entries a lane holds in registers while the next SP_U are in flight (the register ring)
# on both sides of every multiple of SP_U up to 32 and of the ring's first turn at 2 SP_U, then rows of many turns
RING_LENS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 64, 100, 300, 511)


def full_mantissa(rng, size, lo, hi):
    """f32 of random sign, magnitudes uniform in [lo, hi): a f64 draw rounded to f32, so all 24 bits of the mantissa are in use"""
    mag = np.minimum(rng.uniform(lo, hi, size).astype(np.float32), np.nextafter(np.float32(hi), np.float32(0.0)))
    return np.where(rng.random(size) < 0.5, -mag, mag).astype(np.float32)


def ring_values(rng, size):
    """stored values of the rounding cases: +-[0.5, 1)"""
    return full_mantissa(rng, size, 0.5, 1.0)


def ring_row(rng, length, pool):
    """`length` distinct ascending indices out of `pool` with ring_values"""
    idx = np.sort(rng.choice(pool, length, replace=False)).astype(np.uint32)
    return idx, ring_values(rng, length)


def ring_query(rng, pool, support):
    """`support` distinct indices of `pool` in shuffled order, weights +-[0.5, 2)"""
    idx = rng.choice(pool, support, replace=False).astype(np.uint32)
    return idx, full_mantissa(rng, support, 0.5, 2.0)


def ring_rows(rng, pool, lens=RING_LENS):
    """301 rows: two slices and a part whose lengths cycle over `lens` (the lanes of one slice differ), a slice of 64 rows of
    2 SP_U entries each, a slice of 64 rows of 2 SP_U + 1, and one empty row at the end"""
    cyc = [lens[i % len(lens)] for i in range(128 + 44)]
    lengths = cyc[:128] + [2 * SP_U] * 64 + [2 * SP_U + 1] * 64 + cyc[128:] + [0]
    return [ring_row(rng, L, pool) for L in lengths]


def ring_case(rng):
    """(rows, vocab, queries): vocab 512, 301 rows (ring_rows), five distinct queries of 400 indices each — the table form fills all
    four slots of a pass with different weights and has a second pass"""
    vocab = 512
    pool = np.arange(vocab, dtype=np.uint32)
    return ring_rows(rng, pool), vocab, [ring_query(rng, pool, 400) for _ in range(5)]


def ring_large_case(rng, vocab):
    """ring_case's values at a large vocab: indices from a pool of 360 — 0, vocab - 1 and forty runs of eight consecutive indices
    that start at a multiple of eight (one word of presence nibbles each) among them — 301 rows of up to 300 entries, five queries
    of 280 indices each"""
    fixed = np.array([0, (vocab - 1) // 8 * 8 - 8])  # the first word of nibbles and the last whole one below vocab - 1
    starts = np.concatenate([fixed, rng.permutation(np.setdiff1d(rng.integers(1, vocab // 8 - 2, 80) * 8, fixed))[:38]])
    runs = (starts[:, None] + np.arange(8)[None, :]).ravel()
    rest = rng.permutation(np.setdiff1d(rng.integers(0, vocab - 1, 200), runs))[:39]
    pool = np.unique(np.concatenate([runs, rest, [vocab - 1]])).astype(np.uint32)
    assert pool.size == 360 and pool[0] == 0 and pool[-1] == vocab - 1
    return ring_rows(rng, pool, tuple(L for L in RING_LENS if L <= 300)), vocab, [ring_query(rng, pool, 280) for _ in range(5)]


def log_uniform(rng, size, lo_exp, hi_exp):
    """f32 of random sign, magnitudes 10^u with u uniform in [lo_exp, hi_exp)"""
    mag = (10.0 ** rng.uniform(lo_exp, hi_exp, size)).astype(np.float32)
    return np.where(rng.random(size) < 0.5, -mag, mag).astype(np.float32)


def subnormal_case(rng):
    """(rows, vocab, queries): values in +-[1e-20, 1e-19), weights in +-[1e-25, 1e-19) (their exponents uniform), so the products lie
    between the smallest subnormal and the smallest normals and most sums are subnormal; 300 rows of 1 to 40 entries, vocab 64,
    five queries of 48 indices"""
    vocab = 64
    pool = np.arange(vocab, dtype=np.uint32)
    rows = []
    for r in range(300):
        idx = np.sort(rng.choice(pool, 1 + r % 40, replace=False)).astype(np.uint32)
        rows.append((idx, full_mantissa(rng, idx.size, 1e-20, 1e-19)))
    queries = []
    for _ in range(5):
        idx = rng.choice(pool, 48, replace=False).astype(np.uint32)
        queries.append((idx, log_uniform(rng, idx.size, -25.0, -19.0)))
    return rows, vocab, queries


# ---- the layout past 2^32 bytes (tests/test_gpu_sparse_large.py) ------------------------------------------------------------
# The smallest layout whose index array crosses 2^32 bytes while the LDS form is still eligible: vocab 32768, 520 slices, one row of
# 32767 entries per slice (at lane 7 t mod 64), so L_t = 32767 for every slice, base_t = t x 64 x 32767 and the padded entries are
# 520 x 64 x 32767 = 1 090 485 760 = 2^30.02.  Entry 2^29 (byte 2^31 of the index array) is position 256 of slice 256, entry 2^30
# (byte 2^32) position 512 of slice 512; the value array starts at byte 4 361 943 040 of the allocation and ends at 8 723 886 080.
LARGE_VOCAB, LARGE_SLICES, LARGE_LONG, LARGE_SEED = 32768, 520, 32767, 0x5A7E
LARGE_ROWS = LARGE_SLICES * 64
LARGE_SLICE_ENTRIES = 64 * LARGE_LONG


def large_long_lane(t):
    return (7 * t) % 64


def large_row(r):
    """row r of the large layout, made from (LARGE_SEED, r) alone: the long row of its slice (every index but one, ring_values) or
    a row of 0 to 3 entries"""
    rng = np.random.default_rng([LARGE_SEED, int(r)])
    if r % 64 == large_long_lane(r // 64):
        idx = np.delete(np.arange(LARGE_VOCAB, dtype=np.uint32), int(rng.integers(0, LARGE_VOCAB)))
        return idx, ring_values(rng, LARGE_LONG)
    return ring_row(rng, int(rng.integers(0, 4)), LARGE_VOCAB)


def large_case():
    """(rows, vocab, queries): 33 280 rows, about 17 M entries; five queries of 24 000 indices each"""
    rng = np.random.default_rng([LARGE_SEED, 1 << 40])
    pool = np.arange(LARGE_VOCAB, dtype=np.uint32)
    return [large_row(r) for r in range(LARGE_ROWS)], LARGE_VOCAB, [ring_query(rng, pool, 24000) for _ in range(5)]


def large_wrapped_row(r, wrap_bytes=1 << 32):
    """row r as a kernel reads it whose entry BYTE offset 4 x (base_t + 64 p + lane) wraps mod wrap_bytes (the row's length comes from
    the lengths array, which is small): entry p is whatever the layout holds at the wrapped offset — an entry of another row, or the
    padding (index 0, value +0.0).  The mutation tests/test_gpu_sparse_large.py exists for, as large_offsets.wrapped_source is for
    the dense kinds"""
    idx, val = (a.copy() for a in large_row(r))
    t, lane = divmod(int(r), 64)
    at = t * LARGE_SLICE_ENTRIES + 64 * np.arange(idx.size, dtype=np.int64) + lane
    wrapped = at % (wrap_bytes // 4)
    moved = np.flatnonzero(wrapped != at)
    src_row = wrapped[moved] // LARGE_SLICE_ENTRIES * 64 + wrapped[moved] % 64
    src_pos = wrapped[moved] % LARGE_SLICE_ENTRIES // 64
    for s in np.unique(src_row):
        s_idx, s_val = large_row(int(s))
        here = src_row == s
        ok = src_pos[here] < s_idx.size
        pos = np.minimum(src_pos[here], max(s_idx.size - 1, 0))
        idx[moved[here]] = np.where(ok, s_idx[pos], 0) if s_idx.size else 0
        val[moved[here]] = np.where(ok, s_val[pos], np.float32(0.0)) if s_idx.size else np.float32(0.0)
    return idx, val


def cpu_cases():
    """[(name, rows, vocab, queries)] for the plan header against the model"""
    rng = np.random.default_rng(20)
    out = []
    rows, vocab, queries = ieee_case()
    out.append(("ieee", rows, vocab, queries))
    rows = random_rows(rng, 300, 31, 6)
    out.append(("vocab31", rows, 31, [random_query(rng, 31, L) for L in (1, 5, 31, 0)]))
    rows = random_rows(rng, 65, 1, 1)
    out.append(("vocab1", rows, 1, [(u32(0), f32(1.5)), (u32(), f32())]))
    rows, vocab = divergent_case(rng)
    out.append(("divergent", rows, vocab, [random_query(rng, vocab, 40, pool=np.arange(0, 600, dtype=np.uint32)) for _ in range(3)]))
    rows = random_rows(rng, 129, 1 << 20, 12)
    pool = used_indices(rows)
    out.append(("vocab2^20", rows, 1 << 20, [random_query(rng, 1 << 20, 30, pool=pool), (u32((1 << 20) - 1), f32(1.0))]))
    # wide magnitudes: products and sums round at every step, so the summation order shows in the bits
    rows = [(i, (v * np.float32(10.0) ** rng.integers(-6, 7, v.size)).astype(np.float32)) for i, v in random_rows(rng, 200, 64, 20)]
    queries = [(i, (w * np.float32(3.0) ** rng.integers(-8, 9, w.size)).astype(np.float32)) for i, w in (random_query(rng, 64, 40) for _ in range(3))]
    out.append(("rounding", rows, 64, queries))
    # full mantissas (tests/test_sparse_rounding_cpu.py proves them sensitive); generators of their own, so the cases above keep their draws
    out.append(("ring",) + ring_case(np.random.default_rng(21)))
    out.append(("subnormal",) + subnormal_case(np.random.default_rng(22)))
    out.append(("ring_vocab32769",) + ring_large_case(np.random.default_rng(23), 32769))
    out.append(("ring_vocab2^20",) + ring_large_case(np.random.default_rng(24), 1 << 20))
    return out
