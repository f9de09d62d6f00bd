// ott_recommend_plan.h — what the host decides for ott_query_recommend (ott_recommend.hip) before it launches
// anything: the refusals, the example layout (distinct positives, then distinct negatives), the passes of the sweep, k_eff, whether
// a second top-k round can and does run, and the bytes of the context's scratch; and, at the end, what ott_query_recommend_strategy
//  adds for the strategies sum_scores and average_vector.  HIP-free: tests/test_recommend_cpu.py and
// tests/test_recommend_strategy_cpu.py compile it with the host compiler under AddressSanitizer and walk it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace ott {

constexpr uint32_t REC_MAX_EXAMPLES = 64;           // OTT_RECOMMEND_MAX_EXAMPLES: the distinct examples of a call ride in the kernel arguments
constexpr uint32_t REC_FILL = 1u;                   // OTT_RECOMMEND_FILL
constexpr uint32_t REC_NQ = 4;                      // examples per pass of the sweep (ott_sweep_dev.h: SW_NQ)
constexpr uint64_t REC_MAX_ROWS = 0xFFFFFFF0ull;    // 2^32 - 16: the keys hold ~row in 32 bits

// ---- the refusals (in the order the call makes them; all before any device work) ----------------------------------------------------
enum RecRefusal {
    REC_OK = 0,
    REC_NO_POSITIVE,   // OTT_ERR_INVALID: n_positive == 0
    REC_NULL_LIST,     // OTT_ERR_INVALID: a list pointer NULL with a count above 0
    REC_BAD_FLAGS,     // OTT_ERR_INVALID: unknown flag bits
    REC_HAS_QUERIES,   // OTT_ERR_INVALID: d->nq != 0 or d->queries != NULL
    REC_PER_QUERY,     // OTT_ERR_UNSUPPORTED: OTT_MODE_PER_QUERY
    REC_MFMA,          // OTT_ERR_UNSUPPORTED: OTT_PATH_MFMA
    REC_MULTI_GPU,     // OTT_ERR_UNSUPPORTED: the examples' rows lie on different shards
    REC_TOO_MANY_ROWS, // OTT_ERR_UNSUPPORTED: a store of more than REC_MAX_ROWS rows
    REC_BAD_ID,        // OTT_ERR_INVALID: an id >= the store's length
    REC_TOO_MANY,      // OTT_ERR_INVALID: more than REC_MAX_EXAMPLES distinct examples
    REC_BOTH_SIDES,    // OTT_ERR_INVALID: a row listed as both positive and negative
    REC_SMALL_CAP,     // OTT_ERR_INVALID: cap < k_eff
    REC_NULL_OUT,      // OTT_ERR_INVALID: out == NULL with cap > 0
    // ott_query_recommend_strategy alone
    REC_BAD_STRATEGY,  // OTT_ERR_INVALID: no such strategy
    REC_MFMA_L1,       // OTT_ERR_UNSUPPORTED: average_vector on OTT_PATH_MFMA with the Manhattan metric (ott_query's refusal)
};
inline bool rec_refusal_is_invalid(RecRefusal r) {
    return r != REC_OK && !(r == REC_PER_QUERY || r == REC_MFMA || r == REC_MULTI_GPU || r == REC_TOO_MANY_ROWS || r == REC_MFMA_L1);
}

// what the lists' shape, the flags and the descriptor alone decide (no store is looked at)
inline RecRefusal rec_check_args(bool positive_null, uint64_t n_positive, bool negative_null, uint64_t n_negative, uint32_t flags, bool has_queries, bool per_query,
                                 bool mfma) {
    if (n_positive == 0) return REC_NO_POSITIVE;
    if (positive_null || (negative_null && n_negative != 0)) return REC_NULL_LIST;
    if (flags & ~REC_FILL) return REC_BAD_FLAGS;
    if (has_queries) return REC_HAS_QUERIES;
    if (per_query) return REC_PER_QUERY;
    if (mfma) return REC_MFMA;
    return REC_OK;
}
// ... and what the store decides
inline RecRefusal rec_check_store(bool multi_gpu, uint64_t len) {
    if (multi_gpu) return REC_MULTI_GPU;
    if (len > REC_MAX_ROWS) return REC_TOO_MANY_ROWS;
    return REC_OK;
}

// ---- the examples --------------------------------------------------------------------------------------------------------------------
// Distinct positives in the order of their first occurrence, then the distinct negatives: slot e of the sweep's query block is
// rows[e], positive iff e < first_neg.  Rows stay below REC_MAX_ROWS (rec_check_store), so 32 bits hold them.
struct RecExamples {
    uint32_t rows[REC_MAX_EXAMPLES];
    uint32_t n, first_neg;
};
// Lists of any length: a scan of the at most REC_MAX_EXAMPLES distinct ids per listed id.  *bad: the id a refusal is about.
inline RecRefusal rec_examples(const uint64_t* positive, uint64_t n_positive, const uint64_t* negative, uint64_t n_negative, uint64_t len, RecExamples* ex,
                               uint64_t* bad) {
    ex->n = ex->first_neg = 0;
    for (int side = 0; side < 2; side++) {
        const uint64_t* ids = side == 0 ? positive : negative;
        const uint64_t n_ids = side == 0 ? n_positive : n_negative;
        const uint32_t lo = side == 0 ? 0u : ex->first_neg;  // duplicates are looked for in [lo, n): the list's own side
        for (uint64_t i = 0; i < n_ids; i++) {
            const uint64_t id = ids[i];
            *bad = id;
            if (id >= len) return REC_BAD_ID;
            bool seen = false;
            for (uint32_t e = 0; e < ex->n && !seen; e++)
                if (ex->rows[e] == (uint32_t)id) {
                    if (e < lo) return REC_BOTH_SIDES;
                    seen = true;
                }
            if (seen) continue;
            if (ex->n == REC_MAX_EXAMPLES) return REC_TOO_MANY;
            ex->rows[ex->n++] = (uint32_t)id;
        }
        if (side == 0) ex->first_neg = ex->n;
    }
    return REC_OK;
}

// ---- the run ---------------------------------------------------------------------------------------------------------------------------
inline uint64_t rec_k_eff(uint64_t k, uint64_t len) { return k < len ? k : len; }
inline RecRefusal rec_check_out(uint64_t k_eff, uint64_t cap, bool out_null) {
    if (cap < k_eff) return REC_SMALL_CAP;
    if (out_null && cap != 0) return REC_NULL_OUT;
    return REC_OK;
}
// one example takes the sweep's single-query kernel, more take REC_NQ per pass
inline uint32_t rec_tile(uint32_t n_examples) { return n_examples == 1 ? 1u : REC_NQ; }
inline uint32_t rec_passes(uint32_t n_examples) { return n_examples == 1 ? 1u : (n_examples + REC_NQ - 1) / REC_NQ; }
// rows of the zero-padded query block the examples' rows are gathered into (upload_exact_inputs' nq_pad)
inline uint32_t rec_slots(uint32_t n_examples) { return (n_examples + 7u) & ~7u; }
// a second round (the negative side) CAN run: the flag is set and there are negatives.  Then the state table outlives the first
// keys kernel; otherwise that kernel is the last to read it and leaves it zeroed
inline bool rec_fill_possible(uint32_t flags, const RecExamples& ex) { return (flags & REC_FILL) != 0 && ex.first_neg < ex.n; }
// ... and DOES run: the positive side returned fewer than k_eff.  It asks for the rest
inline uint64_t rec_second_k(bool fill_possible, uint64_t k_eff, uint64_t n_first) { return fill_possible && n_first < k_eff ? k_eff - n_first : 0; }

// the context's scratch: the rows' {bp, bn} states (the key table is grouped search's, under its own protocol)
inline size_t rec_state_bytes(uint64_t len) { return (size_t)len * 8; }
inline size_t rec_key_bytes(uint64_t len) { return (size_t)len * 8; }

// ---- strategies (ott_query_recommend_strategy) -------------------------------------------------------------------------
constexpr uint32_t REC_BEST_SCORE = 0;      // OTT_RECOMMEND_BEST_SCORE: ott_query_recommend itself
constexpr uint32_t REC_AVERAGE_VECTOR = 1;  // OTT_RECOMMEND_AVERAGE_VECTOR: one ordinary query with a vector built from the examples
constexpr uint32_t REC_SUM_SCORES = 2;      // OTT_RECOMMEND_SUM_SCORES: the sweep with a running f32 sum per row
constexpr uint32_t REC_SUM_MARK = 1u;       // the state's second word once a lane wrote the row: S's bits alone may be 0

inline bool rec_strategy_known(uint32_t strategy) { return strategy <= REC_SUM_SCORES; }
// the flags a strategy takes: best_score its fill bit, the other two none
inline uint32_t rec_strategy_flags(uint32_t strategy) { return strategy == REC_BEST_SCORE ? REC_FILL : 0u; }
// the MFMA path: never for the sweeps; average_vector is ott_query's, which does not score Manhattan there
inline RecRefusal rec_strategy_mfma(uint32_t strategy, bool mfma, bool manhattan) {
    if (!mfma) return REC_OK;
    if (strategy == REC_AVERAGE_VECTOR) return manhattan ? REC_MFMA_L1 : REC_OK;
    return REC_MFMA;
}
// what the strategy, the lists' shape, the flags and the descriptor alone decide for average_vector and sum_scores, in the order
// the call refuses (best_score is handed to ott_query_recommend whole: rec_check_args)
inline RecRefusal rec_strategy_check_args(uint32_t strategy, bool positive_null, uint64_t n_positive, bool negative_null, uint64_t n_negative, uint32_t flags,
                                          bool has_queries, bool per_query, bool mfma, bool manhattan) {
    if (!rec_strategy_known(strategy)) return REC_BAD_STRATEGY;
    if (n_positive == 0) return REC_NO_POSITIVE;
    if (positive_null || (negative_null && n_negative != 0)) return REC_NULL_LIST;
    if (flags & ~rec_strategy_flags(strategy)) return REC_BAD_FLAGS;
    if (has_queries) return REC_HAS_QUERIES;
    if (per_query) return REC_PER_QUERY;
    return rec_strategy_mfma(strategy, mfma, manhattan);
}
// the refusals' texts (the two with an id in them are put together by the caller)
inline const char* rec_strategy_text(RecRefusal r) {
    switch (r) {
        case REC_BAD_STRATEGY: return "ott_query_recommend_strategy: unknown strategy";
        case REC_NO_POSITIVE: return "ott_query_recommend_strategy: at least one positive example is needed";
        case REC_NULL_LIST: return "ott_query_recommend_strategy: an example list is NULL";
        case REC_BAD_FLAGS: return "ott_query_recommend_strategy: flags must be 0 (OTT_RECOMMEND_FILL belongs to best_score)";
        case REC_HAS_QUERIES: return "ott_query_recommend_strategy: the examples are the queries; d->queries must be NULL and d->nq 0";
        case REC_PER_QUERY: return "ott_query_recommend_strategy: the examples make ONE query; PER_QUERY is not served";
        case REC_MFMA: return "ott_query_recommend_strategy: the MFMA path does not serve sum_scores; use path AUTO or EXACT";
        case REC_MFMA_L1: return "ott_query_recommend_strategy: the MFMA path does not score the Manhattan metric; use path AUTO or EXACT";
        case REC_MULTI_GPU: return "ott_query_recommend_strategy: a multi-GPU store is not served (the examples' rows lie on different shards)";
        case REC_TOO_MANY_ROWS: return "ott_query_recommend_strategy: a store of more than 2^32 - 16 rows is not served";
        case REC_TOO_MANY: return "ott_query_recommend_strategy: more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples";
        case REC_SMALL_CAP: return "ott_query_recommend_strategy: output capacity is smaller than min(k, rows)";
        case REC_NULL_OUT: return "ott_query_recommend_strategy: out is NULL";
        default: return "";
    }
}
// sum_scores: slot e adds its pair score when it is a positive, subtracts it when a negative
constexpr bool rec_slot_positive(uint32_t e, uint32_t first_neg) { return e < first_neg; }  // (constexpr: the sweep kernel calls it too)
// average_vector: the context's id-mask scratch [every row but the examples | that & the caller's mask (compose_row_mask) | the vector]
inline uint64_t rec_mask_words(uint64_t len) { return (len + 63) / 64; }
inline size_t rec_mask_bytes(uint64_t len, uint32_t dim) { return (size_t)rec_mask_words(len) * 16 + (size_t)dim * 4; }
// ... its first block on the host, as the device leaves it: ones (past the store's end too, like the live mask), the examples' bits cleared
inline void rec_mask_fill(const RecExamples& ex, uint64_t len, uint64_t* words) {
    for (uint64_t w = 0; w < rec_mask_words(len); w++) words[w] = ~0ull;
    for (uint32_t e = 0; e < ex.n; e++)
        if (ex.rows[e] < len) words[ex.rows[e] >> 6] &= ~(1ull << (ex.rows[e] & 63));
}

}  // namespace ott
