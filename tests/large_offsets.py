"""Host side of the large-offset tests (tests/test_gpu_large_offsets.py, tests/test_large_offsets_cpu.py): how a
host model answers for a store far too large to hold or score on the host.  Test infrastructure: numpy only, no GPU.

The identity everything rests on: every query kind applies its row mask before anything else, a pair's score depends on its two
rows alone, and every tie order ends in "the lower row".  So for a sorted row set K the kind's model over the compact rows R[K]
with no mask, its indices mapped through K, IS the kind's answer over the whole store under the row mask K
(tests/test_large_offsets_cpu.py proves it for every model on a store small enough to score whole).

K is made of windows: `half` rows at the start and at the end of the store and on either side of every boundary row — a row
whose byte offset, float offset or id first needs one more bit.  half = 130 is two full 64-row tiles and a part on each side,
unaligned at both ends.

The mutation helpers (wrapped_source, wrapped_rows) model the bug the GPU file exists for: an address `row * ld` computed in
32 bits reads the row `row mod 2^k` instead."""
import numpy as np

HALF = 130


def spans(n, boundaries, half=HALF):
    """[(first, count)] ascending and disjoint: [0, half), [b - half, b + half) per boundary, [n - half, n), clipped and merged"""
    raw = [(0, half)] + [(int(b) - half, int(b) + half) for b in sorted(boundaries)] + [(n - half, n)]
    out = []
    for a, b in sorted((max(a, 0), min(b, n)) for a, b in raw):
        if b <= a:
            continue
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b - a) for a, b in out]


def windows(n, boundaries, half=HALF):
    """(K, words): the kept rows, sorted int64, and the n-bit row mask of K as packed uint64 words (bit r % 64 of word r // 64),
    made from K alone: no array of n elements exists at any point"""
    K = np.concatenate([np.arange(a, a + c, dtype=np.int64) for a, c in spans(n, boundaries, half)])
    words = np.zeros((int(n) + 63) // 64, dtype=np.uint64)
    np.bitwise_or.at(words, K >> 6, np.uint64(1) << (K & 63).astype(np.uint64))
    return K, words


def runs_of(K):
    """[(first, count)] of the runs of consecutive rows in the sorted set K"""
    K = np.asarray(K, np.int64)
    if K.size == 0:
        return []
    cut = np.flatnonzero(np.diff(K) != 1) + 1
    return [(int(part[0]), int(part.size)) for part in np.split(K, cut)]


def window_rows(oracle, K, dim, seed):
    """f32[len(K), dim]: the rows K of the synthetic corpus VecStore.append_random(n, seed) makes on the device, one
    oracle.rand_rows call per window"""
    return np.ascontiguousarray(np.concatenate([oracle.rand_rows(a, c, dim, seed) for a, c in runs_of(K)]))


def compact_of(K, rows):
    """store rows (all of them in K) -> their positions in R[K]"""
    rows = np.asarray(rows, np.int64)
    at = np.searchsorted(K, rows)
    assert np.array_equal(np.asarray(K)[np.minimum(at, len(K) - 1)], rows), "a row outside K"
    return at


def to_store_index(K, hits, base=0):
    """a model's hits over R[K] (a structured array with an "index" field, or a plain index array) with the compact indices mapped
    back to store rows"""
    K = np.asarray(K, np.int64)
    if getattr(hits, "dtype", None) is not None and hits.dtype.names:
        out = hits.copy()
        out["index"] = K[out["index"].astype(np.int64) - int(base)] + int(base)
        return out
    return K[np.asarray(hits, np.int64)]


def mask_bool(words, n):
    """the packed mask as bool[n] (what the Python plans take)"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little", count=int(n)).astype(bool)


# ---- planted rows (section 3 of the GPU file): rows that win by construction -----------------------------------------------------------

def sign_vector(dim, seed):
    return np.where(np.random.default_rng(seed).random(dim) < 0.5, np.float32(-1.0), np.float32(1.0)).astype(np.float32)


def planted(dim, n_planted, metric_name, seed):
    """(query f32[dim], rows f32[n_planted, dim]) for one metric.  Unplanted elements lie in [-1, 1).
    dot:        q = 3 s, row j = c_j s with distinct c_j in [2, 3): score 3 c_j dim >= 6 dim against at most 3 dim
    l2 and l1:  q = 3 s, row j = 3 s - d_j s with distinct d_j in (0, 0.5]: a planted row is d_j away per element, an unplanted
                one more than 2
    cosine:     q = s, row j = s with its first j * (dim // 256) elements negated (dim >= 256, at most 12 rows): cosines
                1 - 2 j (dim // 256) / dim, distinct and >= 1 - 22 / 256 > 0.9, against (hoeffding_cosine_bound) under 0.5"""
    s = sign_vector(dim, seed)
    j = np.arange(n_planted, dtype=np.float32)
    if metric_name == "dot":
        c = (np.float32(2.0) + (j + 1) / np.float32(2 * (n_planted + 1))).astype(np.float32)
        return (np.float32(3.0) * s).astype(np.float32), (c[:, None] * s[None, :]).astype(np.float32)
    if metric_name in ("l2", "l1"):
        d = ((j + 1) / np.float32(2 * (n_planted + 1))).astype(np.float32)
        return (np.float32(3.0) * s).astype(np.float32), ((np.float32(3.0) - d)[:, None] * s[None, :]).astype(np.float32)
    assert metric_name == "cosine"
    rows = np.repeat(s[None, :], n_planted, axis=0).astype(np.float32)
    assert dim >= 256 and n_planted <= 12
    for r in range(n_planted):
        rows[r, : r * (dim // 256)] *= np.float32(-1.0)
    return s.copy(), rows


def hoeffding_cosine_bound(n_rows, dim, cos, norm2_low):
    """an upper bound of P(any of n_rows uniform rows has cosine >= cos against a sign vector): the dot s.x is a sum of dim
    independent terms in [-1, 1], so P(s.x >= t) <= exp(-t^2 / (2 dim)) (Hoeffding); cosine >= cos needs
    s.x >= cos * sqrt(dim) * |x|, and |x|^2 >= norm2_low * dim except with probability exp(-2 dim (1/3 - norm2_low)^2)
    (Hoeffding again: the squares lie in [0, 1] with mean 1/3)"""
    t2 = cos * cos * dim * norm2_low * dim
    return float(n_rows) * (np.exp(-t2 / (2.0 * dim)) + np.exp(-2.0 * dim * (1.0 / 3.0 - norm2_low) ** 2))


# ---- the mutation: addresses that wrap ------------------------------------------------------------------------------------------------

def wrapped_source(rows, wrap_rows):
    """the row a 32-bit wrapped `row * ld` reads instead of `row`: row mod wrap_rows"""
    return np.asarray(rows, np.int64) % int(wrap_rows)


def wrapped_rows(oracle, K, dim, seed, wrap_rows):
    """R[K] as a kernel with wrapped addresses sees it: row r's values are those of row r mod wrap_rows"""
    src = wrapped_source(K, wrap_rows)
    return np.ascontiguousarray(np.concatenate([oracle.rand_rows(int(r), 1, dim, seed) for r in src]))
