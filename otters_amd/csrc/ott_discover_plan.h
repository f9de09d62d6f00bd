// ott_discover_plan.h — what the host decides for ott_query_discover (ott_discover.hip) before it launches
// anything: the refusals, the slot layout (pair i in slots 2i and 2i + 1, the target behind the pairs), the passes of the sweep,
// k_eff, the bytes of the context's scratch and the level cut of the (wins, score) order.  HIP-free: tests/test_discover_cpu.py
// compiles it with the host compiler under AddressSanitizer and walks it.  disc_level_cut runs on the device too.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OTT_DISC_HD __host__ __device__
#else
#define OTT_DISC_HD
#endif

namespace ott {

constexpr uint32_t DISC_MAX_PAIRS = 32;              // OTT_DISCOVER_MAX_PAIRS: the pairs' rows ride in the kernel arguments
constexpr uint32_t DISC_MAX_SLOTS = 2 * DISC_MAX_PAIRS + 1;
constexpr uint64_t DISC_NO_ROW = ~0ull;              // OTT_NO_ROW
constexpr uint32_t DISC_NQ = 4;                      // slots per pass of the sweep (ott_sweep_dev.h: SW_NQ): two whole pairs
constexpr uint64_t DISC_MAX_ROWS = 0xFFFFFFF0ull;    // 2^32 - 16: the keys hold ~row in 32 bits
constexpr uint32_t DISC_LEVELS = DISC_MAX_PAIRS + 1; // wins 0 .. 32

// ---- the refusals (in the order the call makes them; all before any device work) ----------------------------------------------------
enum DiscRefusal {
    DISC_OK = 0,
    DISC_BAD_PAIRS,      // OTT_ERR_INVALID: n_pairs == 0 or above DISC_MAX_PAIRS
    DISC_NULL_LIST,      // OTT_ERR_INVALID: a list pointer NULL
    DISC_BAD_FLAGS,      // OTT_ERR_INVALID: nonzero flags
    DISC_MANY_QUERIES,   // OTT_ERR_INVALID: d->nq > 1
    DISC_NULL_QUERY,     // OTT_ERR_INVALID: d->nq == 1 without d->queries, or d->queries with d->nq == 0
    DISC_BOTH_TARGETS,   // OTT_ERR_INVALID: a vector target together with a target row
    DISC_BAD_MIN_WINS,   // OTT_ERR_INVALID: min_wins > n_pairs
    DISC_PER_QUERY,      // OTT_ERR_UNSUPPORTED: OTT_MODE_PER_QUERY
    DISC_MFMA,           // OTT_ERR_UNSUPPORTED: OTT_PATH_MFMA
    DISC_MULTI_GPU,      // OTT_ERR_UNSUPPORTED: the examples' rows lie on different shards
    DISC_TOO_MANY_ROWS,  // OTT_ERR_UNSUPPORTED: a store of more than DISC_MAX_ROWS rows
    DISC_BAD_ID,         // OTT_ERR_INVALID: an id >= the store's length (the target row included)
    DISC_SAME_ROW,       // OTT_ERR_INVALID: a pair with the same row on both sides
    DISC_SMALL_CAP,      // OTT_ERR_INVALID: cap < k_eff
    DISC_NULL_OUT,       // OTT_ERR_INVALID: out == NULL with cap > 0
};
inline bool disc_refusal_is_invalid(DiscRefusal r) {
    return r != DISC_OK && !(r == DISC_PER_QUERY || r == DISC_MFMA || r == DISC_MULTI_GPU || r == DISC_TOO_MANY_ROWS);
}

// what the lists' shape, the flags and the descriptor alone decide (no store is looked at)
inline DiscRefusal disc_check_args(uint64_t n_pairs, bool positive_null, bool negative_null, uint32_t flags, uint32_t nq, bool queries_null, bool has_target_row,
                                   uint64_t min_wins, bool per_query, bool mfma) {
    if (n_pairs == 0 || n_pairs > DISC_MAX_PAIRS) return DISC_BAD_PAIRS;
    if (positive_null || negative_null) return DISC_NULL_LIST;
    if (flags != 0) return DISC_BAD_FLAGS;
    if (nq > 1) return DISC_MANY_QUERIES;
    if ((nq == 1) == queries_null) return DISC_NULL_QUERY;
    if (nq == 1 && has_target_row) return DISC_BOTH_TARGETS;
    if (min_wins > n_pairs) return DISC_BAD_MIN_WINS;
    if (per_query) return DISC_PER_QUERY;
    if (mfma) return DISC_MFMA;
    return DISC_OK;
}
// ... and what the store decides
inline DiscRefusal disc_check_store(bool multi_gpu, uint64_t len) {
    if (multi_gpu) return DISC_MULTI_GPU;
    if (len > DISC_MAX_ROWS) return DISC_TOO_MANY_ROWS;
    return DISC_OK;
}

// ---- the slots -------------------------------------------------------------------------------------------------------------------------
// Slot 2i is pair i's positive, slot 2i + 1 its negative: nothing is deduplicated, a row may fill several slots.  A target (a stored
// row or the caller's vector) takes slot 2 * n_pairs.  rows[] holds the slots a kernel gathers from the store: the pairs', and the
// target ROW's; a vector target's slot goes up from the host.
enum DiscTarget { DISC_TARGET_NONE = 0, DISC_TARGET_ROW = 1, DISC_TARGET_VECTOR = 2 };
struct DiscSlots {
    uint32_t rows[DISC_MAX_SLOTS];
    uint32_t n_pairs;
    uint32_t n_gather;  // 2 * n_pairs, + 1 with a target row
    uint32_t n_slots;   // 2 * n_pairs, + 1 with any target
    uint32_t target;    // DiscTarget
};
// Pair by pair: the positive's id, the negative's id, then the pair itself; the target row last.  *bad: the id a refusal is about.
inline DiscRefusal disc_slots(const uint64_t* positive, const uint64_t* negative, uint32_t n_pairs, uint64_t target_row, bool vector_target, uint64_t len, DiscSlots* sl,
                              uint64_t* bad) {
    sl->n_pairs = n_pairs;
    for (uint32_t i = 0; i < n_pairs; i++) {
        *bad = positive[i];
        if (positive[i] >= len) return DISC_BAD_ID;
        *bad = negative[i];
        if (negative[i] >= len) return DISC_BAD_ID;
        if (positive[i] == negative[i]) return DISC_SAME_ROW;
        sl->rows[2 * i] = (uint32_t)positive[i];
        sl->rows[2 * i + 1] = (uint32_t)negative[i];
    }
    sl->n_gather = sl->n_slots = 2 * n_pairs;
    sl->target = vector_target ? DISC_TARGET_VECTOR : DISC_TARGET_NONE;
    if (vector_target) sl->n_slots++;
    if (!vector_target && target_row != DISC_NO_ROW) {
        *bad = target_row;
        if (target_row >= len) return DISC_BAD_ID;
        sl->rows[sl->n_gather++] = (uint32_t)target_row;
        sl->n_slots++;
        sl->target = DISC_TARGET_ROW;
    }
    return DISC_OK;
}
// the slot of the target, or none
inline uint32_t disc_target_slot(const DiscSlots& sl) { return sl.target != DISC_TARGET_NONE ? 2 * sl.n_pairs : 0xFFFFFFFFu; }

// ---- the run ---------------------------------------------------------------------------------------------------------------------------
inline uint64_t disc_k_eff(uint64_t k, uint64_t len) { return k < len ? k : len; }
inline DiscRefusal disc_check_out(uint64_t k_eff, uint64_t cap, bool out_null) {
    if (cap < k_eff) return DISC_SMALL_CAP;
    if (out_null && cap != 0) return DISC_NULL_OUT;
    return DISC_OK;
}
// DISC_NQ slots per pass, always (there are at least two slots): with an odd number of pairs the target rides in the last pass's
// free pair of slots, otherwise it takes a pass of its own
inline uint32_t disc_passes(uint32_t n_pairs, bool has_target) { return (2 * n_pairs + (has_target ? 1u : 0u) + DISC_NQ - 1) / DISC_NQ; }

// The context's scratch beside the state and key tables: a header, then the rows above the cut level (with a target) or one byte
// of wins per row (without one: the hits' wins are looked up there).
// header: DISC_HDR_WORDS words — hist[0 .. 32] the candidates per wins level, then the list's cursor.
constexpr uint32_t DISC_HDR_WORDS = 64;
constexpr uint32_t DISC_HDR_CURSOR = DISC_LEVELS;
struct DiscAbove {  // a candidate above the cut level
    uint32_t wins, pad;
    uint64_t key;   // ord(T) << 32 | ~row
};
inline size_t disc_state_bytes(uint64_t len) { return (size_t)len * 8; }
inline size_t disc_key_bytes(uint64_t len) { return (size_t)len * 8; }
inline size_t disc_hdr_bytes() { return (size_t)DISC_HDR_WORDS * 4; }
inline size_t disc_list_off() { return disc_hdr_bytes(); }
// with a target: [header | k_eff list entries]; without: [header | one byte of wins per row]
inline size_t disc_wins_off() { return disc_list_off(); }
inline size_t disc_scratch_bytes(bool has_target, uint64_t len, uint64_t k_eff) {
    return ((has_target ? disc_list_off() + (size_t)k_eff * sizeof(DiscAbove) : disc_wins_off() + (size_t)len) + 15) & ~(size_t)15;
}

// ---- the level cut ---------------------------------------------------------------------------------------------------------------------
// hist[w] = candidates with w wins, w <= n_levels - 1.  The cut level L* is the highest level with count(wins >= L*) >= k_eff, or 0
// if there is none; *n_above = count(wins > L*), below k_eff by construction (k_eff >= 1).  The hits are the n_above rows above the
// level, in (wins, score, row) order, and then the best k_eff - n_above rows OF the level.
OTT_DISC_HD inline uint32_t disc_level_cut(const uint32_t* hist, uint32_t n_levels, uint64_t k_eff, uint64_t* n_above) {
    uint64_t above = 0;
    for (uint32_t l = n_levels; l-- > 1;) {
        if (above + hist[l] >= k_eff) {
            *n_above = above;
            return l;
        }
        above += hist[l];
    }
    *n_above = above;
    return 0;
}

}  // namespace ott
