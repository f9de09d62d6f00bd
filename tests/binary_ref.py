"""The normative numpy model of ott_query_binary.  Row r carries n_bits bits; bit j lies in bit j % 64 of 64-bit word
j // 64 (np.packbits(..., bitorder="little") viewed as uint64), the bits at and above n_bits zero.  S = float32(popcount(q XOR v)):
the Hamming distance, exact.  Every row the masks leave is a candidate, the filter acts on S, the order is the canonical one (S
under `take`, equal S to the lower row); hit.query = b.  ott_store_set_binary_sign: bit j of row r = row[j] > 0.0 in f32 (NaN, -0.0
and +0.0 give 0).

It also restates what otters_amd/csrc/ott_binary_plan.h decides (units, offsets, the route, the gate's LDS need and capacity), and
simulates the gated sweep: rows reach W workgroups in any interleaving, each workgroup keeps a histogram of the levels it let
through and a gate, recomputes at arbitrary points — and must never drop a row of the model's top-k."""
import numpy as np

import manhattan_ref as M

MAX_BITS, MAX_QUERIES = 16384, 1024
SLICE, UNIT_BITS, UNIT_BYTES = 64, 128, 16
GATE_NQ, GATE_MAX_K, GATE_LDS_BYTES, GATE_MIN_CAP, GATE_MAX_CAP = 4, 512, 64 * 1024, 1 << 20, 1 << 27
MAX_ROWS = 2 ** 32 - 16
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def words(n_bits):
    return (n_bits + 63) // 64


def units(n_bits):
    return (n_bits + UNIT_BITS - 1) // UNIT_BITS


def pack(bits):
    """bool [n, n_bits] -> uint64 [n, words(n_bits)], padding bits zero"""
    bits = np.asarray(bits, bool)
    n, nb = bits.shape
    out = np.zeros((n, words(nb) * 8), np.uint8)
    if nb:
        out[:, : (nb + 7) // 8] = np.packbits(bits, axis=1, bitorder="little")
    return out.view("<u8").reshape(n, words(nb))


def unpack(w, n_bits):
    """uint64 [n, words] -> bool [n, n_bits]"""
    w = np.ascontiguousarray(w, dtype="<u8")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n_bits].astype(bool)


def padding_ok(w, n_bits):
    """per row: no bit at or above n_bits is set in the last word"""
    w = np.asarray(w, np.uint64)
    if n_bits % 64 == 0 or w.shape[0] == 0:
        return np.ones(w.shape[0], bool)
    return (w[:, -1] >> np.uint64(n_bits % 64)) == 0


def popcount_table(x):
    """popcount of every uint64 of x, by a byte table"""
    x = np.ascontiguousarray(x, dtype="<u8")
    return POP8[x.view(np.uint8).reshape(x.shape + (8,))].sum(axis=-1, dtype=np.uint32)


def popcount_unpack(x):
    x = np.ascontiguousarray(x, dtype="<u8")
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.uint32)


def distances(row_words, q_words):
    """[nq, n] uint32 Hamming distances"""
    row_words, q_words = np.asarray(row_words, np.uint64), np.asarray(q_words, np.uint64)
    out = np.zeros((q_words.shape[0], row_words.shape[0]), np.uint32)
    for b in range(q_words.shape[0]):
        out[b] = popcount_table(row_words ^ q_words[b][None, :]).sum(axis=1, dtype=np.uint32) if row_words.size else 0
    return out


def scores(row_words, q_words):
    """[nq, n] f32: S = (float) popcount(q XOR v), exact"""
    return distances(row_words, q_words).astype(np.float32)


def sign_bits(x):
    """ott_store_set_binary_sign's rule: x > 0.0 in f32, decided on the bits so that no denormal mode can change it"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u - np.uint32(1)) < np.uint32(0x7F800000)


def expected(S, take, k, cmp=0, thr=0.0, keep=None):
    """[hits of query b]: rows that survive `keep`, the filter on S, canonical order, cut at k; `query` = b"""
    out = []
    for b in range(S.shape[0]):
        h = M.select_canonical(S[b][None], take, k, cmp, thr, None if keep is None else np.asarray(keep, bool)).copy()
        h["query"] = b
        out.append(h)
    return out


def query(row_words, q_words, take, k, cmp=0, thr=0.0, keep=None):
    return expected(scores(row_words, q_words), take, k, cmp, thr, keep)


# ---- what ott_binary_plan.h decides -------------------------------------------------------------------------------------------------------
def unit_offset(row, p, n_units):
    return ((row // SLICE) * n_units + p) * (SLICE * UNIT_BYTES) + (row % SLICE) * UNIT_BYTES


def word_offset(row, w, n_units):
    return unit_offset(row, w >> 1, n_units) + (w & 1) * 8


def layout_bytes(n_rows, n_bits):
    return ((n_rows + SLICE - 1) // SLICE) * units(n_bits) * SLICE * UNIT_BYTES


def range_bytes(row0, row1, n_units):
    return 0 if row1 <= row0 else ((row1 + SLICE - 1) // SLICE - row0 // SLICE) * n_units * SLICE * UNIT_BYTES


def run_bytes(rows, n_units):
    """what a pass over the kept rows reads (stats.bytes_scanned per pass): a slice is read whole when any kept row lies in it, and
    once.  rows: the kept row indices, a bool mask over the rows, or (start, count) runs as an int array [n, 2]"""
    rows = np.asarray(rows)
    if rows.dtype == np.bool_:
        rows = np.flatnonzero(rows)
    elif rows.ndim == 2:
        rows = np.concatenate([np.arange(s, s + c, dtype=np.int64) for s, c in rows.astype(np.int64)] + [np.zeros(0, np.int64)])
    slices = set((rows.astype(np.int64) // SLICE).tolist())
    return len(slices) * n_units * SLICE * UNIT_BYTES


def layout_image(row_words, n_bits):
    """the device layout of the rows as bytes: what ott_store_set_binary uploads"""
    row_words = np.asarray(row_words, np.uint64)
    n, nu = row_words.shape[0], units(n_bits)
    img = np.zeros(layout_bytes(n, n_bits) // 8, np.uint64)
    for r in range(n):
        for w in range(words(n_bits)):
            img[word_offset(r, w, nu) // 8] = row_words[r, w]
    return img


def gate_query_lds(n_bits):
    return (n_bits + 2) * 4


def gate_tile(n_bits, nq):
    t = GATE_NQ
    while t >= 1:
        if (t <= nq or t == 1) and t * gate_query_lds(n_bits) <= GATE_LDS_BYTES:
            return t
        t >>= 1
    return 0


def gate_capacity(option, nq, rows):
    pairs = nq * rows
    if option:
        return min(option, pairs)
    return min(min(max(pairs // 8, GATE_MIN_CAP), GATE_MAX_CAP), pairs)


def gate_eligible(n_bits, nq, k_eff, rows, cap_option=0):
    return 1 <= k_eff <= GATE_MAX_K and gate_tile(n_bits, nq) != 0 and gate_capacity(cap_option, nq, rows) < MAX_ROWS


# ---- the gated sweep, simulated -----------------------------------------------------------------------------------------------------------
def gate_scan(h, T, k):
    """the smallest level T' <= T with h[0] + .. + h[T'] >= k, or T"""
    c = np.cumsum(h[: T + 1])
    at = np.flatnonzero(c >= k)
    return int(at[0]) if at.size else T


def simulate_gate(levels, k, n_bits, n_groups, rng, tile=64, recompute=0.5, share=0.5):
    """One query's gated sweep over `levels` (the level of every candidate row: the distance, or n_bits - distance for take Max).
    Tiles of `tile` rows go to `n_groups` workgroups in a random interleaving; a workgroup counts the rows of a tile at or inside
    its gate, recomputes the gate with probability `recompute` (a wave that skips the recompute emits under the old gate), reads
    the global gate with probability `share` (a stale read is a skipped one).  Returns the emitted row indices."""
    levels = np.asarray(levels, np.int64)
    n = levels.size
    tiles = [np.arange(t, min(t + tile, n)) for t in range(0, n, tile)]
    order = rng.permutation(len(tiles))
    hist = np.zeros((n_groups, n_bits + 1), np.int64)
    gate = np.full(n_groups, n_bits, np.int64)
    global_gate = n_bits
    emitted = []
    for ti in order:
        g = int(rng.integers(n_groups))
        T = int(gate[g])
        if rng.random() < share:
            T = min(T, global_gate)
        rows = tiles[ti]
        inside = rows[levels[rows] <= T]
        if inside.size == 0:
            continue
        np.add.at(hist[g], levels[inside], 1)
        if rng.random() < recompute:
            T2 = gate_scan(hist[g], T, k)
            if T2 < T:
                gate[g] = min(gate[g], T2)
                global_gate = min(global_gate, T2)
            inside = inside[levels[inside] <= T2]
        emitted.append(inside)
    return np.concatenate(emitted) if emitted else np.zeros(0, np.int64)


def must_emit(levels, k):
    """the rows no gate may drop: every row at or below the k-th smallest level (ties at the k-th level included)"""
    levels = np.asarray(levels, np.int64)
    if levels.size == 0 or k == 0:
        return np.zeros(0, np.int64)
    kth = np.sort(levels)[min(k, levels.size) - 1]
    return np.flatnonzero(levels <= kth)
