// ott_boost_plan.h — what the host decides for ott_query_boost (ott_boost.hip) before it launches anything: the
// term checks and every refusal with its text, the pass count, whether the sweep's top-k can serve the call, the bytes the stats
// report, and the HOST STATEMENT OF THE FORMULA — the final score F of one (query, row) pair, one IEEE f32 operation at a time, in
// the contract's order.  The device epilogue (boost_sweep_kernel) computes the same operations with the _rn intrinsics.  HIP-free:
// tests/test_boost_cpu.py compiles it with the host compiler under AddressSanitizer + UBSan, walks it, and holds the formula to the
// numpy model (tests/boost_ref.py) bit for bit.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace ott {

constexpr uint32_t BOOST_MAX_TERMS = 8;             // OTT_BOOST_MAX_TERMS
constexpr uint32_t BOOST_MAX_QUERIES = 1024;        // OTT_BOOST_MAX_QUERIES
constexpr uint32_t BOOST_SLOTS = 64;                // OTT_MASK_SLOTS
constexpr uint32_t BOOST_NQ = 4;                    // queries per pass of the sweep (ott_sweep_dev.h: SW_NQ)
constexpr uint64_t BOOST_MAX_ROWS = 0xFFFFFFF0ull;  // 2^32 - 16: the keys hold ~row in 32 bits
// k_eff > 512 takes the top-k's pair form (every surviving (query, row) becomes a 12-byte pair before the sort): served only while
// the pairs of the whole batch stay below this (ott_masks_plan.h: MASKS_MAX_SORT_PAIRS, the same top-k)
constexpr uint64_t BOOST_MAX_SORT_PAIRS = 1ull << 26;

enum : uint32_t { BOOST_SUM = 0, BOOST_MULT = 1 };                        // ott_boost_combine
enum : uint32_t { BOOST_VALUE = 0, BOOST_LIN_DECAY = 1, BOOST_MASK = 2 };  // ott_boost_kind
enum : uint32_t { BOOST_DT_INT32 = 0, BOOST_DT_INT64 = 1, BOOST_DT_FLOAT32 = 2, BOOST_DT_FLOAT64 = 3, BOOST_DT_DATETIME = 5 };  // ott_dtype

// ott_boost_term's layout (include/otters_hip.h), restated so that this header stays free of the public one
struct BoostTerm {
    uint32_t kind;
    uint32_t source;
    float weight;
    float scale;
    double origin;
    float missing;
    uint32_t reserved;
};
static_assert(sizeof(BoostTerm) == 32 && offsetof(BoostTerm, weight) == 8 && offsetof(BoostTerm, scale) == 12 && offsetof(BoostTerm, origin) == 16 &&
                  offsetof(BoostTerm, missing) == 24 && offsetof(BoostTerm, reserved) == 28,
              "ott_boost_term is 32 bytes, offsets 0 4 8 12 16 24 28");

// ---- the refusals, in the order the call makes them; all before any device work ------------------------------------------------------
enum BoostRefusal {
    BOOST_OK = 0,
    // what the arguments alone decide (boost_check_args: no store is looked at)
    BOOST_NO_QUERIES,        // nq == 0
    BOOST_TOO_MANY_QUERIES,  // nq > BOOST_MAX_QUERIES
    BOOST_MERGED,            // OTT_MODE_MERGED with nq > 1
    BOOST_TOO_MANY_TERMS,    // n_terms > BOOST_MAX_TERMS
    BOOST_NULL_TERMS,        // terms == NULL with n_terms > 0
    BOOST_BAD_COMBINE,
    BOOST_BAD_SCORE_WEIGHT,  // not finite
    BOOST_BAD_KIND,          // from here on *bad_term says which term
    BOOST_RESERVED,          // reserved != 0
    BOOST_BAD_WEIGHT,        // not finite
    BOOST_BAD_ORIGIN,        // VALUE, LIN_DECAY: not finite
    BOOST_BAD_MISSING,       // VALUE, LIN_DECAY: not finite
    BOOST_BAD_SCALE,         // LIN_DECAY: not finite or <= 0
    BOOST_BAD_SLOT,          // MASK: slot >= BOOST_SLOTS
    BOOST_MFMA,              // OTT_PATH_MFMA                                                     (OTT_ERR_UNSUPPORTED)
    // what the store decides (boost_check_store, boost_check_sources, boost_check_cap)
    BOOST_MULTI_GPU,         //                                                                   (OTT_ERR_UNSUPPORTED)
    BOOST_TIE_ORDER,         // tie_order 1 or 2                                                  (OTT_ERR_UNSUPPORTED)
    BOOST_TOO_MANY_ROWS,     // n >= BOOST_MAX_ROWS                                               (OTT_ERR_UNSUPPORTED)
    BOOST_UNKNOWN_COLUMN,    // VALUE, LIN_DECAY: source is no column id
    BOOST_COLUMN_LENGTH,     // ... or a column whose length differs from the store's
    BOOST_EMPTY_SLOT,        // MASK: the slot was never filled (or was dropped since)
    BOOST_CAP,               // cap < nq * min(k, rows)
    BOOST_TOO_MANY_PAIRS,    // k_eff > 512 with more than BOOST_MAX_SORT_PAIRS (query, row) pairs  (OTT_ERR_UNSUPPORTED)
};

// ott_status of a refusal: OTT_ERR_INVALID (-1) or OTT_ERR_UNSUPPORTED (-4)
inline int boost_refusal_status(BoostRefusal r) {
    switch (r) {
        case BOOST_OK: return 0;
        case BOOST_MFMA: case BOOST_MULTI_GPU: case BOOST_TIE_ORDER: case BOOST_TOO_MANY_ROWS: case BOOST_TOO_MANY_PAIRS: return -4;
        default: return -1;
    }
}

inline const char* boost_kind_name(uint32_t kind) { return kind == BOOST_VALUE ? "VALUE" : kind == BOOST_LIN_DECAY ? "LIN_DECAY" : "MASK"; }

// the message of a refusal; `nq`, `n_terms`, the term index `bad` and the term itself where the refusal names them (t may be NULL
// for the refusals in front of BOOST_BAD_KIND)
inline std::string boost_refusal_text(BoostRefusal r, uint32_t nq, uint32_t n_terms, uint32_t bad, const BoostTerm* t) {
    const std::string name = "ott_query_boost: ";
    const std::string term = name + "term " + std::to_string(bad) + (t && t->kind <= BOOST_MASK ? std::string(" (") + boost_kind_name(t->kind) + ")" : std::string()) + ": ";
    switch (r) {
        case BOOST_OK: return std::string();
        case BOOST_NO_QUERIES: return "No queries provided";  // src/vec.rs:188-190
        case BOOST_TOO_MANY_QUERIES: return name + std::to_string(nq) + " queries are above OTT_BOOST_MAX_QUERIES (" + std::to_string(BOOST_MAX_QUERIES) + ")";
        case BOOST_MERGED: return name + "a batch needs OTT_MODE_PER_QUERY (a merged list over several boosted queries is not served)";
        case BOOST_TOO_MANY_TERMS: return name + std::to_string(n_terms) + " terms are above OTT_BOOST_MAX_TERMS (" + std::to_string(BOOST_MAX_TERMS) + ")";
        case BOOST_NULL_TERMS: return name + "terms is NULL";
        case BOOST_BAD_COMBINE: return name + "unknown combine (OTT_BOOST_SUM or OTT_BOOST_MULT)";
        case BOOST_BAD_SCORE_WEIGHT: return name + "score_weight is not finite";
        case BOOST_BAD_KIND: return term + "unknown kind " + std::to_string(t ? t->kind : 0u);
        case BOOST_RESERVED: return term + "reserved must be 0";
        case BOOST_BAD_WEIGHT: return term + "weight is not finite";
        case BOOST_BAD_ORIGIN: return term + "origin is not finite";
        case BOOST_BAD_MISSING: return term + "missing is not finite";
        case BOOST_BAD_SCALE: return term + "scale must be finite and above 0";
        case BOOST_BAD_SLOT: return term + "slot " + std::to_string(t ? t->source : 0u) + " is not below OTT_MASK_SLOTS (" + std::to_string(BOOST_SLOTS) + ")";
        case BOOST_MFMA: return name + "the MFMA path does not serve boosted queries (a boosted score has no certified bound); use path AUTO or EXACT";
        case BOOST_MULTI_GPU: return name + "a multi-GPU store is not served (the columns and mask slots of a boost live on one GPU)";
        case BOOST_TIE_ORDER: return name + "tie_order 1 and 2 are not served: the reference has no boosted ranking to reproduce; use the canonical order";
        case BOOST_TOO_MANY_ROWS: return name + "a store of 2^32 - 16 rows or more is not served (the keys hold the row in 32 bits)";
        case BOOST_UNKNOWN_COLUMN: return term + "unknown column id " + std::to_string(t ? t->source : 0u);
        case BOOST_COLUMN_LENGTH: return term + "the length of column " + std::to_string(t ? t->source : 0u) + " no longer matches the store";
        case BOOST_EMPTY_SLOT:
            return term + "slot " + std::to_string(t ? t->source : 0u) +
                   " was never filled, or was dropped when the rows moved (ott_store_eval_row_mask_slot, ott_store_write_row_mask_slot)";
        case BOOST_CAP: return name + "output capacity is smaller than nq * min(k, rows)";
        case BOOST_TOO_MANY_PAIRS:
            return name + "k above 512 is served only up to 2^26 (query, row) pairs; send fewer queries per call";
    }
    return std::string();
}

inline bool boost_finite(double x) { return x - x == 0.0; }  // false for NaN and the infinities

// what the arguments alone decide.  mode: 0 MERGED, 1 PER_QUERY; path: 0 AUTO, 1 EXACT, 2 MFMA
inline BoostRefusal boost_check_args(uint32_t nq, uint32_t mode, uint32_t path, uint32_t combine, float score_weight, const BoostTerm* terms, uint32_t n_terms,
                                     uint32_t* bad_term) {
    if (bad_term) *bad_term = 0;
    if (nq == 0) return BOOST_NO_QUERIES;
    if (nq > BOOST_MAX_QUERIES) return BOOST_TOO_MANY_QUERIES;
    if (mode != 1 && nq > 1) return BOOST_MERGED;
    if (n_terms > BOOST_MAX_TERMS) return BOOST_TOO_MANY_TERMS;
    if (!terms && n_terms != 0) return BOOST_NULL_TERMS;
    if (combine > BOOST_MULT) return BOOST_BAD_COMBINE;
    if (!boost_finite(score_weight)) return BOOST_BAD_SCORE_WEIGHT;
    for (uint32_t j = 0; j < n_terms; j++) {
        const BoostTerm& t = terms[j];
        if (bad_term) *bad_term = j;
        if (t.kind > BOOST_MASK) return BOOST_BAD_KIND;
        if (t.reserved != 0) return BOOST_RESERVED;
        if (!boost_finite(t.weight)) return BOOST_BAD_WEIGHT;
        if (t.kind != BOOST_MASK) {
            if (!boost_finite(t.origin)) return BOOST_BAD_ORIGIN;
            if (!boost_finite(t.missing)) return BOOST_BAD_MISSING;
        }
        if (t.kind == BOOST_LIN_DECAY && !(boost_finite(t.scale) && t.scale > 0.0f)) return BOOST_BAD_SCALE;
        if (t.kind == BOOST_MASK && t.source >= BOOST_SLOTS) return BOOST_BAD_SLOT;
    }
    if (bad_term) *bad_term = 0;
    if (path == 2) return BOOST_MFMA;
    return BOOST_OK;
}

// ... what the store decides
inline BoostRefusal boost_check_store(bool multi_gpu, int tie_order, uint64_t n_rows) {
    if (multi_gpu) return BOOST_MULTI_GPU;
    if (tie_order != 0) return BOOST_TIE_ORDER;
    if (n_rows >= BOOST_MAX_ROWS) return BOOST_TOO_MANY_ROWS;
    return BOOST_OK;
}
// column_rows[c] = the rows column c holds (n_columns of them); slot_bits[i] = the rows slot i covers, 0 = never filled
inline BoostRefusal boost_check_sources(const BoostTerm* terms, uint32_t n_terms, const uint64_t* column_rows, uint64_t n_columns, uint64_t n_rows,
                                        const uint64_t* slot_bits, uint32_t* bad_term) {
    for (uint32_t j = 0; j < n_terms; j++) {
        const BoostTerm& t = terms[j];
        if (bad_term) *bad_term = j;
        if (t.kind == BOOST_MASK) {
            if (slot_bits[t.source] == 0) return BOOST_EMPTY_SLOT;
        } else {
            if (t.source >= n_columns) return BOOST_UNKNOWN_COLUMN;
            if (column_rows[t.source] != n_rows) return BOOST_COLUMN_LENGTH;
        }
    }
    return BOOST_OK;
}
// k_eff = min(k, rows the chunk mask leaves)
inline BoostRefusal boost_check_cap(uint64_t cap, uint32_t nq, uint64_t k_eff, uint64_t n_rows) {
    if (cap < k_eff * nq) return BOOST_CAP;
    if (k_eff > 512 && (uint64_t)nq * n_rows > BOOST_MAX_SORT_PAIRS) return BOOST_TOO_MANY_PAIRS;
    return BOOST_OK;
}

// ---- passes and the stats' bytes ------------------------------------------------------------------------------------------------------
inline uint32_t boost_passes(uint32_t nq) { return (nq + BOOST_NQ - 1) / BOOST_NQ; }
inline uint32_t boost_elem_size(uint32_t dtype) { return dtype == BOOST_DT_INT32 || dtype == BOOST_DT_FLOAT32 ? 4u : 8u; }
// the masks sweep's figure (row bytes, + 4 for cosine's inverse norm) plus, per row and pass, the element sizes of the VALUE and
// LIN_DECAY columns; column_dtype[c] = the dtype of column c
inline uint64_t boost_bytes_scanned(uint32_t passes, uint64_t rows_scored, uint32_t dim, bool cosine, const BoostTerm* terms, uint32_t n_terms,
                                    const uint32_t* column_dtype) {
    uint64_t per_row = (uint64_t)dim * 4 + (cosine ? 4 : 0);
    for (uint32_t j = 0; j < n_terms; j++)
        if (terms[j].kind != BOOST_MASK) per_row += boost_elem_size(column_dtype[terms[j].source]);
    return (uint64_t)passes * rows_scored * per_row;
}

// ---- the formula ------------------------------------------------------------------------------------------------------------------------
// One rounded f32 operation at a time: boost_fl keeps the host compiler from contracting a product into the sum behind it,
// whatever -ffp-contract says (the device code uses __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn for the same reason).
inline float boost_fl(float x) {
    volatile float v = x;
    return v;
}
// a column's element as f64 by the IEEE conversion (exact for INT32 and FLOAT32, round to nearest even for INT64 / DATETIME)
inline double boost_column_f64(uint32_t dtype, const void* vals, uint64_t row) {
    switch (dtype) {
        case BOOST_DT_INT32: return (double)((const int32_t*)vals)[row];
        case BOOST_DT_FLOAT32: return (double)((const float*)vals)[row];
        case BOOST_DT_FLOAT64: return ((const double*)vals)[row];
        default: return (double)((const int64_t*)vals)[row];  // Int64 / DateTime
    }
}
// g of a VALUE or LIN_DECAY term for a row whose element is x (is_null: the row's NULL bit)
inline float boost_g_value(const BoostTerm& t, bool is_null, double x) {
    if (is_null) return t.missing;
    const float v = (float)(x - t.origin);  // the subtraction in f64, ONE rounding to f32
    if (t.kind == BOOST_VALUE) return v;
    const float u = boost_fl(fabsf(v) / t.scale);
    return u >= 1.0f ? 0.0f : boost_fl(1.0f - u);  // a NaN u fails the comparison and gives NaN
}
// g of a MASK term: 1 where the slot's bit is set and for rows at or beyond the slot's bit count (src/vec.rs:234)
inline float boost_g_mask(const uint64_t* words, uint64_t bits, uint64_t row) {
    if (row >= bits) return 1.0f;
    return ((words[row >> 6] >> (row & 63)) & 1) ? 1.0f : 0.0f;
}
// B = c_0, then B = fl(B + c_j), with c_j = fl(weight_j * g_j); n_terms >= 1
inline float boost_sum(const BoostTerm* terms, const float* g, uint32_t n_terms) {
    float B = boost_fl(terms[0].weight * g[0]);
    for (uint32_t j = 1; j < n_terms; j++) B = boost_fl(B + boost_fl(terms[j].weight * g[j]));
    return B;
}
// the final score of a pair whose exact-path score is S
inline float boost_final(uint32_t combine, float score_weight, float S, uint32_t n_terms, float B) {
    const float Sw = boost_fl(score_weight * S);
    if (n_terms == 0) return Sw;
    if (combine == BOOST_SUM) return boost_fl(Sw + B);
    return boost_fl(Sw * boost_fl(1.0f + B));
}

}  // namespace ott
