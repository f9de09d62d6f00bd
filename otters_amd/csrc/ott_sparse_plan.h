// ott_sparse_plan.h — what the host decides for sparse rows and ott_query_sparse (ott_sparse.hip) before it touches
// the device: every check of ott_store_set_sparse and of a sparse query with its refusal and text, the sliced-ELL layout arithmetic
// (64 rows per slice, 64-bit offsets), the form of the weight lookup and its passes, the bytes the stats report, and the HOST
// STATEMENT OF THE SCORE: S of one (query, row) pair, one IEEE f32 operation at a time, in the row's index order, with the overlap
// rule beside it.  sparse_score is the definition; sparse_score_dense is what the kernel evaluates (every entry times a dense
// weight table, the overlap tracked apart) and gives the same bits: tests/test_sparse_cpu.py holds both to the numpy model
// (tests/sparse_ref.py) bit for bit and compiles this header under AddressSanitizer + UBSan.  HIP-free.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace ott {

constexpr uint32_t SPARSE_MAX_VOCAB = 1u << 20;      // OTT_SPARSE_MAX_VOCAB
constexpr uint32_t SPARSE_MAX_QUERIES = 1024;        // OTT_SPARSE_MAX_QUERIES
constexpr uint32_t SPARSE_SLICE = 64;                // rows per slice: lane = row
constexpr uint32_t SPARSE_LDS_MAX_VOCAB = 32768;     // the LDS form's last vocab: 128 KiB of weights + 4 KiB of presence bits of 160 KiB
constexpr uint32_t SPARSE_TABLE_NQ = 4;              // queries per pass of the table form: one 16-byte gather serves four
constexpr uint64_t SPARSE_MAX_ROWS = 0xFFFFFFF0ull;  // 2^32 - 16: the keys hold ~row in 32 bits
constexpr uint64_t SPARSE_MAX_SORT_PAIRS = 1ull << 26;  // k_eff > 512: the top-k's pair form (ott_boost_plan.h: BOOST_MAX_SORT_PAIRS, the same top-k)

// ---- the refusals, all before any device work ------------------------------------------------------------------------------------------
enum SparseRefusal {
    SPARSE_OK = 0,
    // ott_store_set_sparse (sparse_check_set); a, b in the text: see sparse_refusal_text
    SPARSE_SET_MULTI_GPU,     //                                                                          (OTT_ERR_UNSUPPORTED)
    SPARSE_SET_VOCAB,         // vocab == 0 or above SPARSE_MAX_VOCAB
    SPARSE_SET_LENGTH,        // n != the store's length
    SPARSE_SET_NULL,          // indptr NULL, or indices / values NULL with entries
    SPARSE_SET_INDPTR0,       // indptr[0] != 0
    SPARSE_SET_INDPTR_ORDER,  // indptr decreases at row a
    SPARSE_SET_INDEX_RANGE,   // index b of row a is not below vocab
    SPARSE_SET_INDEX_ORDER,   // the indices of row a are not strictly ascending at entry b
    SPARSE_SET_VALUE,         // the value of entry b of row a is not finite
    // ott_query_sparse: what the arguments alone decide (sparse_check_query_args)
    SPARSE_Q_NO_QUERIES,
    SPARSE_Q_TOO_MANY_QUERIES,
    SPARSE_Q_MERGED,          // OTT_MODE_MERGED with nq > 1
    SPARSE_Q_METRIC,          // not OTT_METRIC_DOT
    SPARSE_Q_MFMA,            //                                                                          (OTT_ERR_UNSUPPORTED)
    SPARSE_Q_NULL,            // q_indptr NULL, or q_indices / q_values NULL with entries
    SPARSE_Q_INDPTR0,
    SPARSE_Q_INDPTR_ORDER,    // q_indptr decreases at query a
    // ... what the store decides (sparse_check_store, sparse_check_query, sparse_check_cap)
    SPARSE_Q_MULTI_GPU,       //                                                                          (OTT_ERR_UNSUPPORTED)
    SPARSE_Q_NO_ROWS,         // the store has no sparse rows
    SPARSE_Q_STALE,           // rows were appended since ott_store_set_sparse
    SPARSE_Q_TIE_ORDER,       //                                                                          (OTT_ERR_UNSUPPORTED)
    SPARSE_Q_TOO_MANY_ROWS,   //                                                                          (OTT_ERR_UNSUPPORTED)
    SPARSE_Q_INDEX_RANGE,     // index b of query a is not below the store's vocab
    SPARSE_Q_INDEX_DUP,       // index b appears twice in query a
    SPARSE_Q_WEIGHT,          // a weight of query a is not finite
    SPARSE_Q_CAP,             // cap < nq * min(k, rows)
    SPARSE_Q_TOO_MANY_PAIRS,  //                                                                          (OTT_ERR_UNSUPPORTED)
    // ott_store_read_sparse
    SPARSE_READ_RANGE,        // first_row + n_rows is beyond the sparse rows
    SPARSE_READ_CAP,          // entry_cap is below the a entries of the range
};

// ott_status of a refusal: OTT_ERR_INVALID (-1) or OTT_ERR_UNSUPPORTED (-4)
inline int sparse_refusal_status(SparseRefusal r) {
    switch (r) {
        case SPARSE_OK: return 0;
        case SPARSE_SET_MULTI_GPU: case SPARSE_Q_MFMA: case SPARSE_Q_MULTI_GPU: case SPARSE_Q_TIE_ORDER: case SPARSE_Q_TOO_MANY_ROWS: case SPARSE_Q_TOO_MANY_PAIRS:
            return -4;
        default: return -1;
    }
}

// the message of a refusal; a and b are what the refusal names (a row or query and an entry or index, or two counts); query_fn: the
// entry point a query's refusal names (ott_query_sparse_idf makes the same checks under its own name)
inline std::string sparse_refusal_text(SparseRefusal r, uint64_t a, uint64_t b, const char* query_fn = "ott_query_sparse") {
    const std::string set = "ott_store_set_sparse: ", q = std::string(query_fn) + ": ", rd = "ott_store_read_sparse: ";
    const std::string A = std::to_string(a), B = std::to_string(b);
    switch (r) {
        case SPARSE_OK: return std::string();
        case SPARSE_SET_MULTI_GPU: return set + "a multi-GPU store is not served (sparse rows live on one GPU)";
        case SPARSE_SET_VOCAB: return set + "vocab " + A + " is not in 1 .. OTT_SPARSE_MAX_VOCAB (" + std::to_string(SPARSE_MAX_VOCAB) + "); remap the indices";
        case SPARSE_SET_LENGTH: return set + A + " sparse rows for a store of " + B + " rows";
        case SPARSE_SET_NULL: return set + "indptr, indices or values is NULL";
        case SPARSE_SET_INDPTR0: return set + "indptr[0] is " + A + ", not 0";
        case SPARSE_SET_INDPTR_ORDER: return set + "indptr decreases at row " + A;
        case SPARSE_SET_INDEX_RANGE: return set + "index " + B + " of row " + A + " is not below vocab";
        case SPARSE_SET_INDEX_ORDER: return set + "the indices of row " + A + " are not strictly ascending at entry " + B + " (sort them and merge duplicates)";
        case SPARSE_SET_VALUE: return set + "the value of entry " + B + " of row " + A + " is not finite";
        case SPARSE_Q_NO_QUERIES: return "No queries provided";  // src/vec.rs:188-190
        case SPARSE_Q_TOO_MANY_QUERIES: return q + A + " queries are above OTT_SPARSE_MAX_QUERIES (" + std::to_string(SPARSE_MAX_QUERIES) + ")";
        case SPARSE_Q_MERGED: return q + "a batch needs OTT_MODE_PER_QUERY (a merged list over several sparse queries is not served)";
        case SPARSE_Q_METRIC: return q + "the metric must be OTT_METRIC_DOT (a sparse score is a dot product over the shared indices)";
        case SPARSE_Q_MFMA: return q + "the MFMA path does not serve sparse queries (no plane holds sparse rows); use path AUTO or EXACT";
        case SPARSE_Q_NULL: return q + "q_indptr, q_indices or q_values is NULL";
        case SPARSE_Q_INDPTR0: return q + "q_indptr[0] is " + A + ", not 0";
        case SPARSE_Q_INDPTR_ORDER: return q + "q_indptr decreases at query " + A;
        case SPARSE_Q_MULTI_GPU: return q + "a multi-GPU store is not served (sparse rows live on one GPU)";
        case SPARSE_Q_NO_ROWS: return q + "no sparse rows are set (ott_store_set_sparse)";
        case SPARSE_Q_STALE:
            return q + "the sparse rows cover " + A + " rows, the store holds " + B + " (rows were appended since ott_store_set_sparse: set them again)";
        case SPARSE_Q_TIE_ORDER: return q + "tie_order 1 and 2 are not served: the reference has no sparse ranking to reproduce; use the canonical order";
        case SPARSE_Q_TOO_MANY_ROWS: return q + "a store of 2^32 - 16 rows or more is not served (the keys hold the row in 32 bits)";
        case SPARSE_Q_INDEX_RANGE: return q + "index " + B + " of query " + A + " is not below the store's vocab";
        case SPARSE_Q_INDEX_DUP: return q + "index " + B + " appears twice in query " + A;
        case SPARSE_Q_WEIGHT: return q + "the weight of index " + B + " of query " + A + " is not finite";
        case SPARSE_Q_CAP: return q + "output capacity is smaller than nq * min(k, rows)";
        case SPARSE_Q_TOO_MANY_PAIRS: return q + "k above 512 is served only up to 2^26 (query, row) pairs; send fewer queries per call";
        case SPARSE_READ_RANGE: return rd + "rows " + A + " .. " + B + " are beyond the sparse rows";
        case SPARSE_READ_CAP: return rd + "entry_cap is too small: the range holds " + A + " entries";
    }
    return std::string();
}

inline bool sparse_finite(float x) { return x - x == 0.0f; }  // false for NaN and the infinities

// ott_store_set_sparse's checks, in order; *a and *b get what the text names.  store_len: ott_store_len
inline SparseRefusal sparse_check_set(bool multi_gpu, const uint64_t* indptr, const uint32_t* indices, const float* values, uint64_t n, uint32_t vocab,
                                      uint64_t store_len, uint64_t* a, uint64_t* b) {
    *a = *b = 0;
    if (multi_gpu) return SPARSE_SET_MULTI_GPU;
    if (vocab == 0 || vocab > SPARSE_MAX_VOCAB) return *a = vocab, SPARSE_SET_VOCAB;
    if (n != store_len) return *a = n, *b = store_len, SPARSE_SET_LENGTH;
    if (!indptr) return SPARSE_SET_NULL;
    if (indptr[0] != 0) return *a = indptr[0], SPARSE_SET_INDPTR0;
    for (uint64_t r = 0; r < n; r++)
        if (indptr[r + 1] < indptr[r]) return *a = r, SPARSE_SET_INDPTR_ORDER;
    if (indptr[n] != 0 && (!indices || !values)) return SPARSE_SET_NULL;
    for (uint64_t r = 0; r < n; r++)
        for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++) {
            *a = r;
            *b = e - indptr[r];
            if (indices[e] >= vocab) return *b = indices[e], SPARSE_SET_INDEX_RANGE;
            if (e > indptr[r] && indices[e] <= indices[e - 1]) return SPARSE_SET_INDEX_ORDER;
            if (!sparse_finite(values[e])) return SPARSE_SET_VALUE;
        }
    *a = *b = 0;
    return SPARSE_OK;
}

// what a query's arguments alone decide.  mode: 0 MERGED, 1 PER_QUERY; metric: 2 = DOT; path: 2 = MFMA
inline SparseRefusal sparse_check_query_args(uint32_t nq, uint32_t mode, uint32_t metric, uint32_t path, const uint64_t* q_indptr, const uint32_t* q_indices,
                                             const float* q_values, uint64_t* a) {
    *a = 0;
    if (nq == 0) return SPARSE_Q_NO_QUERIES;
    if (nq > SPARSE_MAX_QUERIES) return *a = nq, SPARSE_Q_TOO_MANY_QUERIES;
    if (mode != 1 && nq > 1) return SPARSE_Q_MERGED;
    if (metric != 2) return SPARSE_Q_METRIC;
    if (path == 2) return SPARSE_Q_MFMA;
    if (!q_indptr) return SPARSE_Q_NULL;
    if (q_indptr[0] != 0) return *a = q_indptr[0], SPARSE_Q_INDPTR0;
    for (uint32_t b = 0; b < nq; b++)
        if (q_indptr[b + 1] < q_indptr[b]) return *a = b, SPARSE_Q_INDPTR_ORDER;
    if (q_indptr[nq] != 0 && (!q_indices || !q_values)) return SPARSE_Q_NULL;
    return SPARSE_OK;
}
// ... what the store decides.  sparse_rows: the rows the sparse rows cover; has_sparse: they are set
inline SparseRefusal sparse_check_store(bool multi_gpu, bool has_sparse, uint64_t sparse_rows, uint64_t store_rows, int tie_order, uint64_t* a, uint64_t* b) {
    *a = *b = 0;
    if (multi_gpu) return SPARSE_Q_MULTI_GPU;
    if (!has_sparse) return SPARSE_Q_NO_ROWS;
    if (sparse_rows != store_rows) return *a = sparse_rows, *b = store_rows, SPARSE_Q_STALE;
    if (tie_order != 0) return SPARSE_Q_TIE_ORDER;
    if (store_rows >= SPARSE_MAX_ROWS) return SPARSE_Q_TOO_MANY_ROWS;
    return SPARSE_OK;
}
// ... the queries' entries against the store's vocab: range, duplicates (order is free: the summation follows the row), finite weights
inline SparseRefusal sparse_check_query(uint32_t nq, const uint64_t* q_indptr, const uint32_t* q_indices, const float* q_values, uint32_t vocab, uint64_t* a,
                                        uint64_t* b) {
    std::vector<uint32_t> seen(vocab, 0);  // the query (+ 1) that used the index last
    for (uint32_t qi = 0; qi < nq; qi++)
        for (uint64_t e = q_indptr[qi]; e < q_indptr[qi + 1]; e++) {
            *a = qi;
            *b = q_indices[e];
            if (q_indices[e] >= vocab) return SPARSE_Q_INDEX_RANGE;
            if (seen[q_indices[e]] == qi + 1) return SPARSE_Q_INDEX_DUP;
            seen[q_indices[e]] = qi + 1;
            if (!sparse_finite(q_values[e])) return SPARSE_Q_WEIGHT;
        }
    *a = *b = 0;
    return SPARSE_OK;
}
// k_eff = min(k, rows the chunk mask leaves)
inline SparseRefusal sparse_check_cap(uint64_t cap, uint32_t nq, uint64_t k_eff, uint64_t n_rows) {
    if (cap < k_eff * nq) return SPARSE_Q_CAP;
    if (k_eff > 512 && (uint64_t)nq * n_rows > SPARSE_MAX_SORT_PAIRS) return SPARSE_Q_TOO_MANY_PAIRS;
    return SPARSE_OK;
}

// ---- the sliced-ELL layout ----------------------------------------------------------------------------------------------------------------
// Slice t holds rows 64 t .. 64 t + 63; L_t = the largest entry count among them; entry p of row r lies at base_t + p * 64 + (r & 63)
// of the index array and of the value array.  One allocation: [indices u32 x padded | values f32 x padded | bases u64 x (slices + 1) |
// lengths u32 x 64 slices].  Every offset is 64-bit.
inline uint64_t sparse_slices(uint64_t n_rows) { return (n_rows + SPARSE_SLICE - 1) / SPARSE_SLICE; }
inline uint64_t sparse_entry_offset(uint64_t base, uint64_t p, uint64_t row) { return base + p * SPARSE_SLICE + (row & (SPARSE_SLICE - 1)); }
// L_t of slice t from the CSR's row pointer
inline uint64_t sparse_slice_len(const uint64_t* indptr, uint64_t n_rows, uint64_t t) {
    uint64_t L = 0;
    const uint64_t r1 = (t + 1) * SPARSE_SLICE < n_rows ? (t + 1) * SPARSE_SLICE : n_rows;
    for (uint64_t r = t * SPARSE_SLICE; r < r1; r++)
        if (indptr[r + 1] - indptr[r] > L) L = indptr[r + 1] - indptr[r];
    return L;
}
// base_out[slices + 1]: the slices' bases, base_out[slices] = padded_entries (returned)
inline uint64_t sparse_slice_bases(const uint64_t* indptr, uint64_t n_rows, uint64_t* base_out) {
    const uint64_t ns = sparse_slices(n_rows);
    uint64_t at = 0;
    for (uint64_t t = 0; t < ns; t++) {
        base_out[t] = at;
        at += SPARSE_SLICE * sparse_slice_len(indptr, n_rows, t);
    }
    base_out[ns] = at;
    return at;
}
struct SparseLayout {
    uint64_t n_slices, padded_entries;
    uint64_t off_values, off_bases, off_lengths, bytes;  // byte offsets in the allocation (the indices are at 0)
};
inline SparseLayout sparse_layout(uint64_t n_rows, uint64_t padded_entries) {
    SparseLayout l;
    l.n_slices = sparse_slices(n_rows);
    l.padded_entries = padded_entries;
    l.off_values = padded_entries * 4;
    l.off_bases = padded_entries * 8;  // (a multiple of 8 * 64)
    l.off_lengths = l.off_bases + (l.n_slices + 1) * 8;
    l.bytes = l.off_lengths + l.n_slices * SPARSE_SLICE * 4;
    return l;
}
// the layout bytes of slices [t0, t1): their entries, lengths and bases
inline uint64_t sparse_slice_bytes(const uint64_t* base, uint64_t t0, uint64_t t1) { return (base[t1] - base[t0]) * 8 + (t1 - t0) * (SPARSE_SLICE * 4 + 8); }

// ---- the form of the weight lookup and its passes -----------------------------------------------------------------------------------------
// LDS form: the query's dense f32 table and a presence bitmap in LDS, one query per pass, one workgroup per CU.  Table form: a device
// table [vocab][4] f32 with presence nibbles beside it, four queries per pass.  Both give the same bits.  option: the store's
// sparse_table (-1 automatic, 0 the LDS form wherever eligible, 1 always the table form).
// AUTOMATIC, per (vocab class, nq class), is whichever form measured faster on the MI355X (benchmarks/sparse.py, profiles/sparse/README.md:
// 250k and 1M rows, 64 and 128 entries per row, uniform and skewed lengths, vocab 30522, ms per call, LDS form / table form):
//   nq  1: 0.075 / 0.170, 0.185 / 0.357, 0.102 / 0.299, 0.362 / 0.712, 0.169 / 0.587, 0.450 / 1.029, 0.281 / 1.115, 0.909 / 2.019 — the LDS form, 1.9 to 4.0 x
//   nq  4: 0.206 / 0.176, 0.660 / 0.368, 0.325 / 0.309, 1.364 / 0.710, 0.615 / 0.604, 1.715 / 1.038, 1.035 / 1.130, 3.567 / 2.035 — the table form in 7 of 8
//          cells (up to 1.9 x on skewed lengths, where a lane gathers its entries but the LDS form streams the padding four times); the
//          LDS form is 8 % ahead on 1M uniform rows of 128 entries
//   nq 64: 2.824 / 2.391, 10.07 / 5.344, 4.663 / 4.482, 21.35 / 10.96, 9.352 / 9.210, 27.01 / 16.15, 16.10 / 17.66, 56.52 / 31.68 — the table form in 7 of 8
// (the spread of the three runs is at most 0.07 ms and at most 4 % of the median in every cell).  So: the table form from four queries on, the
// LDS form below (two and three queries were not measured: the LDS form, which keeps no table resident).  Above 32768 there is no choice.
constexpr uint32_t SPARSE_AUTO_TABLE_FROM_NQ = 4;
inline bool sparse_lds_eligible(uint32_t vocab) { return vocab <= SPARSE_LDS_MAX_VOCAB; }
inline bool sparse_take_table(int option, uint32_t vocab, uint32_t nq) {
    if (!sparse_lds_eligible(vocab)) return true;
    if (option >= 0) return option == 1;
    return nq >= SPARSE_AUTO_TABLE_FROM_NQ;
}
inline uint32_t sparse_passes(bool table_form, uint32_t nq) { return table_form ? (nq + SPARSE_TABLE_NQ - 1) / SPARSE_TABLE_NQ : nq; }
inline uint32_t sparse_vocab_pad(uint32_t vocab) { return (vocab + 31u) & ~31u; }
inline size_t sparse_lds_bytes(uint32_t vocab) { return (size_t)sparse_vocab_pad(vocab) * 4 + sparse_vocab_pad(vocab) / 8; }  // weights | presence bits
inline size_t sparse_table_bytes(uint32_t vocab) { return (size_t)vocab * 16 + (size_t)((vocab + 7) / 8) * 4; }              // float4 per index | a nibble per index
inline uint64_t sparse_bytes_scanned(uint32_t passes, uint64_t slice_bytes) { return (uint64_t)passes * slice_bytes; }

// ---- the score ------------------------------------------------------------------------------------------------------------------------------
// One rounded f32 operation at a time: sparse_fl keeps the host compiler from contracting the product into the sum, whatever
// -ffp-contract says (the device code uses __fmul_rn / __fadd_rn).
inline float sparse_fl(float x) {
    volatile float v = x;
    return v;
}
// THE DEFINITION.  Row entries (idx ascending, val), query entries (q_idx distinct in any order, q_w): S = +0.0f, then for j ascending,
// wherever idx[j] is one of the query's, S = fl(S + fl(val[j] * w)).  *overlap: at least one index is shared (the row is a candidate,
// whatever the values are).  A NaN S drops the row: the caller's test.
inline float sparse_score(const uint32_t* idx, const float* val, uint64_t len, const uint32_t* q_idx, const float* q_w, uint64_t q_len, bool* overlap) {
    float S = 0.0f;
    bool any = false;
    for (uint64_t j = 0; j < len; j++)
        for (uint64_t e = 0; e < q_len; e++)
            if (q_idx[e] == idx[j]) {
                S = sparse_fl(S + sparse_fl(val[j] * q_w[e]));
                any = true;
                break;
            }
    *overlap = any;
    return S;
}
// WHAT THE KERNEL EVALUATES: every entry times table[idx] (0.0f outside the query), the overlap from present[idx].  Stored values
// are finite and S starts at +0.0, so fl(val * 0.0f) = +-0.0 never changes S's bits (S is never -0.0: x + y is -0.0 only when both
// are) and the result is the definition's, bit for bit.
inline float sparse_score_dense(const uint32_t* idx, const float* val, uint64_t len, const float* table, const uint8_t* present, bool* overlap) {
    float S = 0.0f;
    bool any = false;
    for (uint64_t j = 0; j < len; j++) {
        S = sparse_fl(S + sparse_fl(val[j] * table[idx[j]]));
        any = any || present[idx[j]] != 0;
    }
    *overlap = any;
    return S;
}

// ---- document frequencies and IDF weights -----------------------------------------------------------------------------------
// df[i] = the LIVE rows whose sparse row stores index i (a stored 0.0 counts), n_docs = the live rows.  The kernel counts with integer
// adds, in a histogram private to the workgroup in LDS (vocab <= 32768: the budget of the sweep's LDS form) or with global atomics
// (any vocab); both give the same words.  option: the store's sparse_df_lds (-1 automatic, 0 never, 1 wherever it fits).
// AUTOMATIC is the LDS form wherever it fits, as measured on the MI355X (benchmarks/hybrid.py, profiles/hybrid/README.md: 250k and 1M
// Zipfian rows of 64 entries, vocab 30522, per build end to end): about 80 us against 19 ms of the global form on 250k rows, about
// 125 us against 74 ms on 1M rows — ten indices are stored by more than half of those rows, so the global form's adds meet on a few
// words.  Above 32768 there is no choice.
inline size_t sparse_df_lds_bytes(uint32_t vocab) { return (size_t)sparse_vocab_pad(vocab) * 4; }
inline bool sparse_df_take_lds(int option, uint32_t vocab) {
    if (!sparse_lds_eligible(vocab)) return false;
    return option != 0;
}
// idf(i) = (float) log(1 + (n_docs - df + 0.5) / (df + 0.5)): f64, every operation rounded, the C library's log, one rounding to f32
inline float sparse_idf(uint64_t n_docs, uint32_t df) {
    volatile double a = (double)(n_docs - df);  // (df <= n_docs: both count live rows)
    a = a + 0.5;
    volatile double b = (double)df + 0.5;
    volatile double c = a / b;
    c = 1.0 + c;
    return (float)log(c);
}
// the weight a query entry gets under OTT_HYBRID_IDF: one f32 multiplication
inline float sparse_idf_weight(float w, float idf) { return sparse_fl(w * idf); }

}  // namespace ott
