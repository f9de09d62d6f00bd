// ott_masks_plan.h — what the host decides for ott_query_masks (ott_masks.hip) before it launches anything: the
// argument refusals, the order of the queries (stable by mask id, so that queries of one mask share passes and by-mask-group
// runs), the permutation back to the caller's order, whether the masks sweep may serve the call, and the auto rule between the
// sweep and the by-mask-group route.  HIP-free: tests/test_masks_cpu.py compiles it with the host compiler under AddressSanitizer
// + UBSan and walks it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace ott {

constexpr uint32_t MASKS_NO_MASK = 0xFFFFFFFFu;     // OTT_NO_MASK
constexpr uint32_t MASKS_SLOT_BASE = 0x80000000u;   // OTT_MASK_SLOT_BASE
constexpr uint32_t MASKS_SLOTS = 64;                // OTT_MASK_SLOTS
constexpr uint32_t MASKS_MAX_QUERIES = 1024;        // OTT_MASKS_MAX_QUERIES
constexpr uint32_t MASKS_NQ = 4;                    // queries per pass of the sweep (ott_sweep_dev.h: SW_NQ)
constexpr uint64_t MASKS_MAX_ROWS = 0xFFFFFFF0ull;  // 2^32 - 16: the keys hold ~row in 32 bits
// k_eff > 512 takes the top-k's pair form (every surviving (query, row) becomes a 12-byte pair before the sort): the sweep serves
// it only while the pairs of the whole batch stay below this (768 MB of pairs); above, the by-mask-group route answers
constexpr uint64_t MASKS_MAX_SORT_PAIRS = 1ull << 26;

// ---- the refusals (in the order the call makes them; all OTT_ERR_INVALID, all before any device work) -------------------------------
enum MasksRefusal {
    MASKS_OK = 0,
    MASKS_NO_QUERIES,   // nq == 0
    MASKS_TOO_MANY,     // nq > MASKS_MAX_QUERIES
    MASKS_MERGED,       // d->mode != OTT_MODE_PER_QUERY
    MASKS_NULL_MAP,     // mask_of_query == NULL
    MASKS_NULL_MASKS,   // masks == NULL with n_masks > 0
    MASKS_BAD_INDEX,    // an entry >= n_masks that is neither a slot reference nor OTT_NO_MASK (*bad_query says which)
    MASKS_BAD_SLOT,     // a slot reference at or above MASKS_SLOTS
    MASKS_EMPTY_SLOT,   // a reference to a slot that was never filled (masks_check_slots: this one needs the store)
};

inline bool masks_is_slot(uint32_t v) { return v != MASKS_NO_MASK && v >= MASKS_SLOT_BASE; }

// what the arguments alone decide (no store is looked at)
inline MasksRefusal masks_check_args(uint32_t nq, bool per_query, const uint32_t* mask_of_query, bool masks_null, uint32_t n_masks, uint32_t* bad_query) {
    if (nq == 0) return MASKS_NO_QUERIES;
    if (nq > MASKS_MAX_QUERIES) return MASKS_TOO_MANY;
    if (!per_query) return MASKS_MERGED;
    if (!mask_of_query) return MASKS_NULL_MAP;
    if (masks_null && n_masks != 0) return MASKS_NULL_MASKS;
    for (uint32_t b = 0; b < nq; b++) {
        const uint32_t v = mask_of_query[b];
        if (bad_query) *bad_query = b;
        if (v == MASKS_NO_MASK) continue;
        if (masks_is_slot(v)) {
            if (v - MASKS_SLOT_BASE >= MASKS_SLOTS) return MASKS_BAD_SLOT;
        } else if (v >= n_masks) {
            return MASKS_BAD_INDEX;
        }
    }
    return MASKS_OK;
}
// ... and what the store's slots decide: slot_bits[i] = the rows slot i covers, 0 = never filled (or dropped since)
inline MasksRefusal masks_check_slots(uint32_t nq, const uint32_t* mask_of_query, const uint64_t* slot_bits, uint32_t* bad_query) {
    for (uint32_t b = 0; b < nq; b++) {
        const uint32_t v = mask_of_query[b];
        if (masks_is_slot(v) && slot_bits[v - MASKS_SLOT_BASE] == 0) {
            if (bad_query) *bad_query = b;
            return MASKS_EMPTY_SLOT;
        }
    }
    return MASKS_OK;
}

// ---- the order of the queries ----------------------------------------------------------------------------------------------------------
// order[i] = the caller's query at position i, stable by mask id (host masks by index, then the slots, then the queries without a
// mask); place[b] = the position of the caller's query b (the inverse).  group_start: the positions where a new mask id starts,
// n_distinct + 1 entries; passes of MASKS_NQ consecutive positions.
struct MasksPlan {
    std::vector<uint32_t> order, place, group_start;
    uint32_t n_distinct = 0, largest_group = 0, passes = 0;
};
inline void masks_plan_build(const uint32_t* mask_of_query, uint32_t nq, MasksPlan& pl) {
    pl.order.resize(nq);
    pl.place.resize(nq);
    std::iota(pl.order.begin(), pl.order.end(), 0u);
    std::stable_sort(pl.order.begin(), pl.order.end(), [mask_of_query](uint32_t a, uint32_t b) { return mask_of_query[a] < mask_of_query[b]; });
    pl.group_start.clear();
    pl.largest_group = 0;
    for (uint32_t i = 0; i < nq; i++) {
        pl.place[pl.order[i]] = i;
        if (i == 0 || mask_of_query[pl.order[i]] != mask_of_query[pl.order[i - 1]]) pl.group_start.push_back(i);
    }
    pl.n_distinct = (uint32_t)pl.group_start.size();
    pl.group_start.push_back(nq);
    for (uint32_t g = 0; g < pl.n_distinct; g++) pl.largest_group = std::max(pl.largest_group, pl.group_start[g + 1] - pl.group_start[g]);
    pl.passes = (nq + MASKS_NQ - 1) / MASKS_NQ;
}

// ---- the route ---------------------------------------------------------------------------------------------------------------------------
// The masks sweep serves the canonical tie order on path AUTO or EXACT (path: 0 AUTO, 1 EXACT, 2 MFMA) of a single-GPU store of
// fewer than 2^32 - 16 rows; everything else is answered by mask group.
inline bool masks_sweep_eligible(int tie_order, uint32_t path, bool multi_gpu, uint64_t n, uint64_t k_eff, uint32_t nq) {
    if (tie_order != 0 || path == 2 || multi_gpu || n == 0 || n >= MASKS_MAX_ROWS) return false;
    return k_eff <= 512 || (uint64_t)nq * n <= MASKS_MAX_SORT_PAIRS;
}

// Option masks_sweep = 2 (auto).  Measured on the MI355X by benchmarks/masks_batch.py against the by-mask-group route of the same
// process and build (profiles/masks_batch/README.md: the table, the spreads and how these constants follow from it).  A shape goes
// to the sweep only where the sweep's median lay below the loop's by more than the spread of the two measurements, for EVERY kind
// of mask measured (the rule does not see a mask's selectivity); every shape that was not measured, or was not faster, stays with
// the loop.  What measured faster is a box: every mask its own (queries that share a mask are ONE batch run on the loop, which the
// sweep's four-query passes do not beat), stores of 250 000 to 1 000 000 rows, rows of 128 to 768 floats, 16 to 64 queries — all
// eight corners measured, 1.2x to 3.9x; inside the box the rule interpolates, outside it never extrapolates.
constexpr uint64_t MASKS_AUTO_MIN_ROWS = 250000;   // profiles/masks_batch/README.md: 10 000 x 768 measured level or slower (0.95x .. 1.05x); nothing between was measured
constexpr uint64_t MASKS_AUTO_MAX_ROWS = 1000000;  // profiles/masks_batch/README.md: 2 000 000 x 768 loses at 1 % masks (0.95x), 4 000 000 x 768 wins nowhere
constexpr uint32_t MASKS_AUTO_MIN_DIM = 128;       // profiles/masks_batch/README.md: the shortest rows measured
constexpr uint32_t MASKS_AUTO_MAX_DIM = 768;       // profiles/masks_batch/README.md: the longest rows measured
constexpr uint32_t MASKS_AUTO_MIN_NQ = 16;         // profiles/masks_batch/README.md: the smallest batch measured
constexpr uint32_t MASKS_AUTO_MAX_NQ = 64;         // profiles/masks_batch/README.md: the largest batch measured
constexpr uint32_t MASKS_AUTO_MAX_GROUP = 1;       // profiles/masks_batch/README.md: masks shared by 8 queries lose 1.2x .. 4.4x on random masks (only tenant masks won)
inline bool masks_auto_takes_sweep(uint64_t n, uint32_t dim, uint32_t nq, uint32_t n_distinct, uint32_t largest_group) {
    (void)n_distinct;  // (with largest_group <= 1 it is nq)
    return n >= MASKS_AUTO_MIN_ROWS && n <= MASKS_AUTO_MAX_ROWS && dim >= MASKS_AUTO_MIN_DIM && dim <= MASKS_AUTO_MAX_DIM && nq >= MASKS_AUTO_MIN_NQ &&
           nq <= MASKS_AUTO_MAX_NQ && largest_group <= MASKS_AUTO_MAX_GROUP;
}
// option masks_sweep: 0 = always by mask group, 1 = the sweep wherever eligible, 2 = auto
inline bool masks_takes_sweep(int option, bool eligible, uint64_t n, uint32_t dim, uint32_t nq, uint32_t n_distinct, uint32_t largest_group) {
    if (!eligible || option == 0) return false;
    return option == 1 || masks_auto_takes_sweep(n, dim, nq, n_distinct, largest_group);
}

// ---- the scratch of a call ----------------------------------------------------------------------------------------------------------------
// [join: words of n rows | union: words of n rows | the host masks, n_masks x mask_words]
inline uint64_t masks_words(uint64_t bits) { return (bits + 63) / 64; }
inline uint64_t masks_scratch_bytes(uint64_t n, uint32_t n_masks, uint64_t mask_bits) { return (2 * masks_words(n) + (uint64_t)n_masks * masks_words(mask_bits)) * 8; }

// one mask word with every bit at and beyond `bits` set: rows at and beyond a mask's bit count are kept (src/vec.rs:234); `words`
// nullptr = no mask, all ones.  The device's union kernel computes the same (ott_masks.hip: mask_word_ext).
inline uint64_t masks_word_ext(const uint64_t* words, uint64_t bits, uint64_t w) {
    if (!words || w * 64 >= bits) return ~0ull;
    uint64_t x = words[w];
    if (bits - w * 64 < 64) x |= ~0ull << (bits - w * 64);
    return x;
}

}  // namespace ott
