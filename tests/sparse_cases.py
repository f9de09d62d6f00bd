"""Shared cases of the sparse tests (tests/test_sparse_cpu.py, tests/test_gpu_sparse.py): generators of sparse rows and queries, and
the case list the CPU tests hold the plan header's C statement of the score to.  Values and weights are small multiples of 1/4
unless a case says otherwise, so exact ties in S (and sums that cancel to +0.0) are frequent."""
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
    return out
