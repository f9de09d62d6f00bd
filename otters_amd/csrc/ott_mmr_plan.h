// ott_mmr_plan.h — what the host decides for ott_query_mmr (ott_mmr.hip) before it launches anything: the refusals,
// the output capacity a call needs, the layout of the context's scratch, the pair kernel's grid and which pairs a workgroup owns,
// the greedy kernel's thread count and rounds.  HIP-free: tests/test_mmr_cpu.py compiles it with the host compiler under
// AddressSanitizer and walks it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace ott {

constexpr uint32_t MMR_MAX_FETCH = 1024;         // OTT_MMR_MAX_FETCH: one thread per candidate in the greedy kernel
constexpr uint32_t MMR_DIMQ_MAX = 2048;          // row floats (padded to 8) the pair kernel keeps in LDS per selected row: ott_store_score_rows' limit
constexpr uint64_t MMR_PAIR_MAX = 256ull << 20;  // bytes of pair scores a call may ask for: nq x fetch_k^2 x 4
constexpr uint32_t MMR_SEL = 8;                  // pair kernel: the "queries" of a workgroup are this many candidates' rows, in LDS
constexpr uint32_t MMR_COLS = 64;                // ... scored against this many candidates: eight waves x eight 8-lane groups
constexpr uint32_t MMR_PAIR_THREADS = 8 * MMR_COLS;

// ---- the refusals (in the order the call makes them; all before any device work) ----------------------------------------------------
enum MmrRefusal {
    MMR_OK = 0,
    MMR_BAD_K,          // OTT_ERR_INVALID: k == 0
    MMR_BAD_FETCH,      // OTT_ERR_INVALID: fetch_k < k or fetch_k > MMR_MAX_FETCH
    MMR_BAD_LAMBDA,     // OTT_ERR_INVALID: lambda outside [0, 1] or NaN
    MMR_MERGED_BATCH,   // OTT_ERR_UNSUPPORTED: OTT_MODE_MERGED with nq > 1
    MMR_MULTI_GPU,      // OTT_ERR_UNSUPPORTED: candidate rows lie on different shards
    MMR_ROW_TOO_LONG,   // OTT_ERR_UNSUPPORTED: rows of more than MMR_DIMQ_MAX floats
    MMR_PAIRS_TOO_BIG,  // OTT_ERR_UNSUPPORTED: nq x fetch_k^2 x 4 above MMR_PAIR_MAX
};
inline bool mmr_refusal_is_invalid(MmrRefusal r) { return r == MMR_BAD_K || r == MMR_BAD_FETCH || r == MMR_BAD_LAMBDA; }

// what the descriptor and the scalar arguments alone decide (no store is looked at)
inline MmrRefusal mmr_check_args(uint64_t k, uint64_t fetch_k, float lambda) {
    if (k == 0) return MMR_BAD_K;
    if (fetch_k < k || fetch_k > MMR_MAX_FETCH) return MMR_BAD_FETCH;
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return MMR_BAD_LAMBDA;  // (false for NaN)
    return MMR_OK;
}
inline uint64_t mmr_pair_bytes(uint32_t nq, uint64_t fetch_k) { return (uint64_t)nq * fetch_k * fetch_k * 4; }
// ... and what the store decides; fetch_k <= MMR_MAX_FETCH here, so the product fits 64 bits
inline MmrRefusal mmr_check_store(bool per_query, uint32_t nq, bool multi_gpu, uint32_t dimq, uint64_t fetch_k) {
    if (!per_query && nq > 1) return MMR_MERGED_BATCH;
    if (multi_gpu) return MMR_MULTI_GPU;
    if (dimq > MMR_DIMQ_MAX) return MMR_ROW_TOO_LONG;
    if (mmr_pair_bytes(nq, fetch_k) > MMR_PAIR_MAX) return MMR_PAIRS_TOO_BIG;
    return MMR_OK;
}
// hits the caller's buffer must hold: min(k, rows) per query (rows: the store's, or the distinct listed ids)
inline uint64_t mmr_cap_needed(uint64_t k, uint64_t rows, bool per_query, uint32_t nq) { return (k < rows ? k : rows) * (per_query ? nq : 1u); }

// ---- the scratch of a call (one block of the query context) -------------------------------------------------------------------------
// [rows: nq x fetch_k u64 | rel: nq x fetch_k f32 | n: nq u32 | picks: nq x k u32 | values: nq x k f32 | pairs: nq x fetch_k x fetch_k f32]
// The first three are uploaded together (upload_bytes, from off_rows), picks and values come back together (result_bytes, from
// off_picks).  Query q's candidates start at q x fetch_k, its pair scores at q x fetch_k^2 with a row pitch of fetch_k.
struct MmrLayout {
    size_t off_rows, off_rel, off_n, off_picks, off_vals, off_pairs, total;
    size_t upload_bytes, result_bytes;
};
inline size_t mmr_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline MmrLayout mmr_layout(uint32_t nq, uint64_t fetch_k, uint64_t k) {
    MmrLayout L;
    const size_t c = (size_t)nq * fetch_k, o = (size_t)nq * k;
    L.off_rows = 0;
    L.off_rel = c * 8;
    L.off_n = L.off_rel + c * 4;
    L.upload_bytes = L.off_n + (size_t)nq * 4;
    L.off_picks = mmr_align(L.upload_bytes);
    L.off_vals = L.off_picks + o * 4;
    L.result_bytes = o * 8;
    L.off_pairs = mmr_align(L.off_vals + o * 4);
    L.total = L.off_pairs + (size_t)mmr_pair_bytes(nq, fetch_k);
    return L;
}

// ---- the pair kernel's grid ---------------------------------------------------------------------------------------------------------
// One workgroup owns MMR_SEL selected rows x MMR_COLS candidates of one query.  The grid is sized by the longest candidate list of the
// call (n_max); a workgroup whose tile starts past its own query's list has nothing to do.  Flat, query-major: block b is query
// b / (sel_tiles x col_tiles), selected-row tile (b / col_tiles) % sel_tiles, candidate tile b % col_tiles.  Never more than nq x fetch_k^2
// blocks, which MMR_PAIR_MAX keeps at 2^26: far below the 2^31 a grid may have.
struct MmrGrid {
    uint32_t sel_tiles, col_tiles;
    uint64_t blocks;
};
inline MmrGrid mmr_pair_grid(uint32_t nq, uint32_t n_max) {
    MmrGrid g;
    g.sel_tiles = (n_max + MMR_SEL - 1) / MMR_SEL;
    g.col_tiles = (n_max + MMR_COLS - 1) / MMR_COLS;
    g.blocks = (uint64_t)nq * g.sel_tiles * g.col_tiles;
    return g;
}
inline void mmr_block(const MmrGrid& g, uint64_t b, uint32_t* q, uint32_t* sel0, uint32_t* col0) {
    const uint64_t per_q = (uint64_t)g.sel_tiles * g.col_tiles;
    *q = (uint32_t)(b / per_q);
    const uint32_t t = (uint32_t)(b % per_q);
    *sel0 = (t / g.col_tiles) * MMR_SEL;
    *col0 = (t % g.col_tiles) * MMR_COLS;
}
inline size_t mmr_pair_lds_bytes(uint32_t dimq) { return (size_t)MMR_SEL * dimq * 4; }
// pair scores are only read by rounds after the first: nothing to fill for one pick or one candidate
inline bool mmr_needs_pairs(uint64_t k, uint32_t n_max) { return k > 1 && n_max > 1; }

// ---- the greedy kernel --------------------------------------------------------------------------------------------------------------
// one workgroup per query, one thread per candidate in whole waves
inline uint32_t mmr_greedy_threads(uint32_t n_max) {
    const uint32_t t = (n_max + 63u) & ~63u;
    return t < 64 ? 64u : t;
}
inline uint32_t mmr_rounds(uint64_t k, uint32_t n) { return k < n ? (uint32_t)k : n; }

}  // namespace ott
