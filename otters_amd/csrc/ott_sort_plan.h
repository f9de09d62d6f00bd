// ott_sort_plan.h — what the sort path's host side (ott_sort.hip: k > 512, the reference's default take) decides before it launches
// anything, free of HIP and of ott_store: plain C++17, like ott_mfma_plan.h, so that the CPU suite compiles the very code
// libotters_hip.so ships on its own (tests/test_sort_plan_cpu.py).  Each of these is written here once, for large_k_slice,
// run_large_k and sort_group_pairs:
//   * the radix sort's pass plan of every result order, and the bits of the row and query fields it sorts on;
//   * which kernel sweeps, over how many queries at a time;
//   * whether a slice takes the rank sort, and the layout of its control block;
//   * the two-phase prefix and the height of a row slice;
//   * the groups' extents from their start words, and the 2-MB pieces a large result travels in;
//   * what a slice reports as bytes scanned.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

#include "../../include/otters_hip.h"  // (and through it stdint.h)
#include "ott_exact_plan.h"            // small_variant_fits, exact_bytes_scanned: the sweep is the exact path's

namespace ott {

// ---- the radix sort's pass plan ----------------------------------------------------------------------------------------------------
// RS_THREADS x RS_ITEMS is the block shape of rs_pass_kernel (ott_sort.hip, which derives its wave count from it): here because
// the tile, and with it the size of the sort's scratch, follows from it
constexpr int RS_THREADS = 512;
constexpr int RS_ITEMS = 8;
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;  // 4096 pairs
constexpr int RS_MAXP = 16;

struct RsPass {
    uint32_t src;    // 0 = key (u64), 1 = query id (u32)
    uint32_t shift;
    uint32_t mask;   // (1 << width) - 1, width <= 8
    uint32_t desc;   // 1 = larger digit first
};
struct RsPlan {
    RsPass pass[RS_MAXP];
    uint32_t n_pass;
    uint32_t abl;  // timing ablations (store option mfma_abl, results then WRONG): 1 no look-back, 2 no stores, 4 no loads, 8 no ranking
};
// control block in device memory: [0, P*256) digit counts -> exclusive starts, then per pass: skip flag, buffer parity
struct RsCtl {
    uint32_t start[RS_MAXP * 256];  // histogram, then (rs_scan_kernel) the exclusive scan: where digit d of pass p starts
    uint32_t skip[RS_MAXP];         // 1 = every pair has the same digit at this position
    uint32_t parity[RS_MAXP + 1];   // number of passes that really ran before pass p (buffer A if even, B if odd); [n_pass] = total
    uint32_t ticket[RS_MAXP];       // next tile index of pass p
    uint32_t error;                 // a look-back gave up
};

inline size_t rs_tiles(uint64_t n) { return (size_t)((n + RS_TILE - 1) / RS_TILE); }
inline size_t rs_tmp_bytes(uint64_t n) { return ((sizeof(RsCtl) + 255) & ~(size_t)255) + rs_tiles(n) * 256 * sizeof(uint64_t); }

// bits [lo, hi) of the source word, LSD; false once the plan is full — a plan is never cut short silently
inline bool rs_add_digits(RsPlan& pl, uint32_t src, uint32_t lo, uint32_t hi, bool desc) {
    for (uint32_t b = lo; b < hi; b += 8) {
        if (pl.n_pass >= (uint32_t)RS_MAXP) return false;
        const uint32_t w = hi - b < 8 ? hi - b : 8;
        pl.pass[pl.n_pass++] = RsPass{src, b, (1u << w) - 1u, desc ? 1u : 0u};
    }
    return true;
}

// Bits needed for the largest value of a field, counted up from `from` and never beyond 32.  The query field: from 0 (one query:
// largest index 0, no bits).  The key's row field: from 1; its largest value is n - 1 + tie_off (the field is row + tie_off), or
// id_span - 1 for grouped pairs.
inline uint32_t index_bits(uint64_t largest, uint32_t from) {
    uint32_t b = from;
    while (b < 32 && (largest >> b) != 0) b++;
    return b;
}
inline uint32_t query_bits(uint32_t nq) { return nq > 1 ? index_bits((uint64_t)(nq - 1), 0) : 0u; }
inline uint32_t row_bits(uint64_t largest) { return index_bits(largest, 1); }

enum SortOrder {
    SORT_SCORE,            // first phase, merged: only the k-th best SCORE is wanted (the order among equal scores is the final sort's business)
    SORT_SCORE_BY_QUERY,   // first phase, per query: the same, grouped by query
    SORT_MERGED,           // best first overall: canonical (tie_sh = 0) or the reference's visit order among equal scores (tie_sh = 3)
    SORT_BY_QUERY,         // grouped by query, each group key descending; also the grouped pairs of ott_group.hip (rbits of id_span)
};
// The pass plan (least significant digit first) of a result order over pairs (key = ord(score) << 32 | ~row, query): only the low
// `rbits` bits of ~row, which can differ between rows of this store, and the `qbits` bits of the query are sorted on.  False if
// the plan would not fit RS_MAXP passes; the worst case is the reference's visit order with every field at its widest:
// 1 (the 3 row bits inside a block) + 4 (32 query bits) + 4 (29 row bits) + 4 (32 score bits) = 13.
inline bool sort_order_plan(SortOrder order, uint32_t rbits, uint32_t qbits, uint32_t tie_sh, uint32_t abl, RsPlan& plan) {
    plan = RsPlan();
    plan.abl = abl;  // (diagnostics only; 0 in normal use)
    const bool score_only = order == SORT_SCORE || order == SORT_SCORE_BY_QUERY, by_query = order == SORT_SCORE_BY_QUERY || order == SORT_BY_QUERY;
    // merged, among equal scores: canonical (sh = 0) = lower row, then lower query — LSD: query first; the reference's visit
    // order (sh = 3) = 8-row block, then query, then row within the block
    const uint32_t sh = order == SORT_MERGED && tie_sh < rbits ? tie_sh : 0u;
    bool ok = rs_add_digits(plan, 0, 0, sh, true);
    if (!by_query && !score_only) ok = ok && rs_add_digits(plan, 1, 0, qbits, false);
    if (!score_only) ok = ok && rs_add_digits(plan, 0, sh, rbits, true);  // ~row: the lower row first among equal scores
    ok = ok && rs_add_digits(plan, 0, 32, 64, true);                      // the score ordinal
    // grouped by query, each group key descending (one query: row order IS the visit order): key first, then the query
    if (by_query) ok = ok && rs_add_digits(plan, 1, 0, qbits, false);
    return ok;
}

// ---- the scoring sweep -------------------------------------------------------------------------------------------------------------
// rows8 (eight lanes per row, a workgroup per 64-row tile, up to 8 queries per pass) wherever it fits, which a small store nearly
// always does; else the streaming kernel, one query or four at a time.  `tiles`: 64-row tiles of the WHOLE plan (the two phases'
// sub-plans are smaller still).
struct SweepShape {
    bool rows8;
    uint32_t tile;    // queries per launch: t8 (1, 2, 4, 8) under rows8, else 1 or 4
    uint32_t passes;  // launches, = corpus passes one sweep makes (stats)
};
inline SweepShape sweep_shape(uint32_t nq, uint32_t dimq, uint32_t tiles, int exact_small) {
    SweepShape w;
    w.rows8 = small_variant_fits(dimq, tiles) && exact_small != 0 && exact_small != 1;
    w.tile = w.rows8 || nq == 1 ? 1u : 4u;
    while (w.rows8 && w.tile < nq && w.tile < 8) w.tile <<= 1;
    w.passes = (nq + w.tile - 1) / w.tile;
    return w;
}
inline uint64_t sort_bytes_scanned(uint32_t passes, uint64_t rows_scored, uint32_t dim, uint32_t metric) {
    return exact_bytes_scanned(passes, rows_scored, dim, metric);  // the same sweep, the same bytes
}

// ---- small results, sorted by rank (small_rank_kernel) -----------------------------------------------------------------------------
constexpr uint32_t SMALL_PAIRS = 16384;
constexpr uint32_t SMALL_PERQ_MAX = 1024;  // PER_QUERY: queries (their extents are prefix-summed in LDS)
// merged: the order word holds row bits + query bits below the score, so they must fit 32; gated slices (run_large_k) sort by radix
inline bool small_path_ok(uint64_t pairs, uint32_t nq, bool perq, uint32_t rbits, uint32_t qbits, int small_sort, bool gated) {
    return pairs <= SMALL_PAIRS && (perq ? nq <= SMALL_PERQ_MAX : rbits + qbits <= 32) && small_sort != 0 && !gated;
}
// [cursor (8 B) | pad | tickets (64 x 4) | rank (cap x 4) | hist (nq x 4)]: one memset
struct SmallCtl {
    size_t cursor, ticket, rank, hist, total;
};
inline SmallCtl small_ctl_layout(uint64_t cap, uint32_t nq) {
    const size_t ticket = 64, rank = ticket + 64 * 4, hist = rank + (size_t)cap * 4;
    return SmallCtl{0, ticket, rank, hist, hist + (size_t)nq * 4};
}

// ---- two phases, row slices --------------------------------------------------------------------------------------------------------
// Rows of the first phase (0 = one phase): m = sqrt(k x pairs per group) balances the two lists; a multiple of 64, at least 4096,
// and only if it is at most a quarter of the rows.  The flat fill pass of the reference tie order (every score ranks the same)
// has no bound to use and stays single-phase.
inline uint64_t prefix_rows(uint64_t rows_scored, uint32_t nq, bool perq, uint64_t k_eff, bool enabled, bool flat) {
    if (!enabled || flat || rows_scored == 0) return 0;
    const double pairs = (double)rows_scored * (perq ? 1.0 : (double)nq);
    const double f = sqrt((double)k_eff / pairs);
    if (f > 0.25) return 0;
    uint64_t m_rows = ((uint64_t)ceil(f * (double)rows_scored) + 63) & ~63ull;
    if (m_rows < 4096) m_rows = 4096;
    return m_rows * 4 > rows_scored ? 0 : m_rows;
}
// rows of a slice of at most `slice_pairs` (row, query) pairs: whole 64-row tiles, at least one
inline uint64_t slice_rows(uint32_t nq, uint64_t slice_pairs) {
    const uint64_t r = (slice_pairs / nq) & ~63ull;
    return r < 64 ? 64 : r;
}

// ---- result groups -----------------------------------------------------------------------------------------------------------------
// Extents of the query groups of n entries sorted by query, from group_start_kernel's words (start[q] = first entry of query q,
// 0xFFFFFFFF = none): first[q] (a query without entries: where the next one starts), count[q] = the group's size, at most k.
// Returns the sum of the counts.
inline uint64_t group_extents(const std::vector<uint32_t>& start, uint64_t n, uint64_t k, std::vector<uint64_t>& first, std::vector<uint64_t>& count) {
    first.assign(start.size(), 0);
    count.assign(start.size(), 0);
    uint64_t next = n, total = 0;  // next: start of the next query that has entries
    for (size_t q = start.size(); q-- > 0;) {
        first[q] = next;
        if (start[q] == 0xFFFFFFFFu) continue;
        count[q] = next - start[q] < k ? next - start[q] : k;
        first[q] = next = start[q];
        total += count[q];
    }
    return total;
}
// Large results (256k hits and more) come over in 2-MB pieces; pieces never straddle two lists: (list, offset, n) in order, src =
// the piece's place among all groups' hits back to back
constexpr size_t COPY_PIECE = (size_t)128 * 1024;  // hits per piece (2 MB)
struct CopyPiece {
    uint32_t g;
    uint64_t at, n, src;
};
inline std::vector<CopyPiece> copy_pieces(const std::vector<uint64_t>& count, uint64_t piece) {
    std::vector<CopyPiece> pieces;
    uint64_t o = 0;
    for (uint32_t g = 0; g < count.size(); g++) {
        for (uint64_t at = 0; at < count[g]; at += piece) pieces.push_back({g, at, piece < count[g] - at ? piece : count[g] - at, o + at});
        o += count[g];
    }
    return pieces;
}

}  // namespace ott
