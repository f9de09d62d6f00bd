// ott_binary_plan.h — what the host decides for bit rows and ott_query_binary (ott_binary.hip) before it touches the
// device: every check of ott_store_set_binary and of a binary query with its refusal and text, the transposed slice layout (64 rows
// per slice, 16-byte units, 64-bit offsets), which route answers a call (the key table or the gated sweep), the gated route's LDS
// need, eligibility and pair capacity, the bytes the stats report, the sign rule of ott_store_set_binary_sign, and the HOST STATEMENT
// OF THE SCORE: the Hamming distance of two bit rows.  tests/binary_ref.py is the numpy model; tests/test_binary_cpu.py compiles this
// header into a host program and holds it to the model.  HIP-free.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>

namespace ott {

constexpr uint32_t BINARY_MAX_BITS = 16384;          // OTT_BINARY_MAX_BITS
constexpr uint32_t BINARY_MAX_QUERIES = 1024;        // OTT_BINARY_MAX_QUERIES
constexpr uint32_t BINARY_SLICE = 64;                // rows per slice: lane = row
constexpr uint32_t BINARY_UNIT_BITS = 128;           // one 16-byte load per lane
constexpr uint32_t BINARY_UNIT_BYTES = 16;
constexpr uint64_t BINARY_MAX_ROWS = 0xFFFFFFF0ull;  // 2^32 - 16: the keys hold ~row in 32 bits
constexpr uint64_t BINARY_MAX_SORT_PAIRS = 1ull << 26;  // k_eff > 512 on the table route: the top-k's pair form (ott_sparse_plan.h: SPARSE_MAX_SORT_PAIRS)
constexpr uint32_t BINARY_TABLE_NQ = 4;              // queries per pass of the table route
constexpr uint32_t BINARY_GATE_NQ = 4;               // ... and, at most, of the gated route (fewer where the histograms would not fit)
constexpr uint32_t BINARY_GATE_MAX_K = 512;          // the gated route's last k_eff
constexpr uint32_t BINARY_GATE_LDS_BYTES = 64 * 1024;  // what the gated kernel's histograms and gate words may take of a workgroup's LDS
constexpr uint64_t BINARY_GATE_MIN_CAP = 1ull << 20;   // the plan's pair capacity never goes below this (or the call's pairs)
constexpr uint64_t BINARY_GATE_MAX_CAP = 1ull << 27;   // ... nor above this: 2^27 pairs are 3.2 GB of pair arrays (two key and two query arrays) before the sort's scratch

// ---- the refusals, all before any device work ------------------------------------------------------------------------------------------
enum BinaryRefusal {
    BINARY_OK = 0,
    // ott_store_set_binary / ott_store_set_binary_sign
    BINARY_SET_MULTI_GPU,     //                                                                          (OTT_ERR_UNSUPPORTED)
    BINARY_SET_BITS,          // n_bits == 0 or above BINARY_MAX_BITS
    BINARY_SET_LENGTH,        // n != the store's length
    BINARY_SET_NULL,          // words NULL with rows
    BINARY_SET_PADDING,       // a bit at or above n_bits is set in the last word of row a
    BINARY_SIGN_MULTI_GPU,    //                                                                          (OTT_ERR_UNSUPPORTED)
    BINARY_SIGN_DIM,          // dim above BINARY_MAX_BITS
    // ott_query_binary: what the arguments alone decide
    BINARY_Q_NO_QUERIES,
    BINARY_Q_TOO_MANY_QUERIES,
    BINARY_Q_MERGED,          // OTT_MODE_MERGED with nq > 1
    BINARY_Q_METRIC,          // not OTT_METRIC_MANHATTAN
    BINARY_Q_MFMA,            //                                                                          (OTT_ERR_UNSUPPORTED)
    BINARY_Q_NULL,            // q_words NULL
    // ... what the store decides
    BINARY_Q_MULTI_GPU,       //                                                                          (OTT_ERR_UNSUPPORTED)
    BINARY_Q_NO_ROWS,         // the store has no bit rows
    BINARY_Q_STALE,           // rows were appended since ott_store_set_binary
    BINARY_Q_TIE_ORDER,       //                                                                          (OTT_ERR_UNSUPPORTED)
    BINARY_Q_TOO_MANY_ROWS,   //                                                                          (OTT_ERR_UNSUPPORTED)
    BINARY_Q_PADDING,         // a bit at or above n_bits is set in the last word of query a
    BINARY_Q_CAP,             // cap < nq * min(k, rows)
    BINARY_Q_TOO_MANY_PAIRS,  //                                                                          (OTT_ERR_UNSUPPORTED)
    // ott_store_read_binary
    BINARY_READ_RANGE,        // first_row + n_rows is beyond the bit rows
};

// ott_status of a refusal: OTT_ERR_INVALID (-1) or OTT_ERR_UNSUPPORTED (-4)
inline int binary_refusal_status(BinaryRefusal r) {
    switch (r) {
        case BINARY_OK: return 0;
        case BINARY_SET_MULTI_GPU: case BINARY_SIGN_MULTI_GPU: case BINARY_Q_MFMA: case BINARY_Q_MULTI_GPU: case BINARY_Q_TIE_ORDER: case BINARY_Q_TOO_MANY_ROWS:
        case BINARY_Q_TOO_MANY_PAIRS:
            return -4;
        default: return -1;
    }
}

// the message of a refusal; a and b are what the refusal names (a row or query, or two counts)
inline std::string binary_refusal_text(BinaryRefusal r, uint64_t a, uint64_t b) {
    const std::string set = "ott_store_set_binary: ", sign = "ott_store_set_binary_sign: ", q = "ott_query_binary: ", rd = "ott_store_read_binary: ";
    const std::string A = std::to_string(a), B = std::to_string(b), MAXB = std::to_string(BINARY_MAX_BITS);
    switch (r) {
        case BINARY_OK: return std::string();
        case BINARY_SET_MULTI_GPU: return set + "a multi-GPU store is not served (bit rows live on one GPU)";
        case BINARY_SET_BITS: return set + "n_bits " + A + " is not in 1 .. OTT_BINARY_MAX_BITS (" + MAXB + ")";
        case BINARY_SET_LENGTH: return set + A + " bit rows for a store of " + B + " rows";
        case BINARY_SET_NULL: return set + "words is NULL";
        case BINARY_SET_PADDING: return set + "row " + A + " has a bit set at or above n_bits (" + B + ") in its last word; padding bits must be zero";
        case BINARY_SIGN_MULTI_GPU: return sign + "a multi-GPU store is not served (bit rows live on one GPU)";
        case BINARY_SIGN_DIM: return sign + "dim " + A + " is above OTT_BINARY_MAX_BITS (" + MAXB + ")";
        case BINARY_Q_NO_QUERIES: return "No queries provided";  // src/vec.rs:188-190
        case BINARY_Q_TOO_MANY_QUERIES: return q + A + " queries are above OTT_BINARY_MAX_QUERIES (" + std::to_string(BINARY_MAX_QUERIES) + ")";
        case BINARY_Q_MERGED: return q + "a batch needs OTT_MODE_PER_QUERY (a merged list over several binary queries is not served)";
        case BINARY_Q_METRIC: return q + "the metric must be OTT_METRIC_MANHATTAN (the Hamming distance is the L1 distance of the bit rows)";
        case BINARY_Q_MFMA: return q + "the MFMA path does not serve binary queries (no plane holds bit rows); use path AUTO or EXACT";
        case BINARY_Q_NULL: return q + "q_words is NULL";
        case BINARY_Q_MULTI_GPU: return q + "a multi-GPU store is not served (bit rows live on one GPU)";
        case BINARY_Q_NO_ROWS: return q + "no bit rows are set (ott_store_set_binary)";
        case BINARY_Q_STALE:
            return q + "the bit rows cover " + A + " rows, the store holds " + B + " (rows were appended since ott_store_set_binary: set them again)";
        case BINARY_Q_TIE_ORDER: return q + "tie_order 1 and 2 are not served: the reference has no binary ranking to reproduce; use the canonical order";
        case BINARY_Q_TOO_MANY_ROWS: return q + "a store of 2^32 - 16 rows or more is not served (the keys hold the row in 32 bits)";
        case BINARY_Q_PADDING: return q + "query " + A + " has a bit set at or above n_bits (" + B + ") in its last word; padding bits must be zero";
        case BINARY_Q_CAP: return q + "output capacity is smaller than nq * min(k, rows)";
        case BINARY_Q_TOO_MANY_PAIRS: return q + "k above 512 is served only up to 2^26 (query, row) pairs; send fewer queries per call";
        case BINARY_READ_RANGE: return rd + "rows " + A + " .. " + B + " are beyond the bit rows";
    }
    return std::string();
}

// ---- the words of a bit row -------------------------------------------------------------------------------------------------------------
// Bit j of a row lies in bit j % 64 of 64-bit word j / 64 (the project's mask convention); a row is ceil(n_bits / 64) words at the
// ABI and ceil(n_bits / 128) 16-byte units on the device, the bits above n_bits zero in both.
inline uint32_t binary_words(uint32_t n_bits) { return (n_bits + 63u) / 64u; }
inline uint32_t binary_units(uint32_t n_bits) { return (n_bits + BINARY_UNIT_BITS - 1u) / BINARY_UNIT_BITS; }
// the bits of the last word that belong to the row (all 64 where n_bits is a multiple of 64)
inline uint64_t binary_last_word_mask(uint32_t n_bits) { return (n_bits & 63u) ? ((1ull << (n_bits & 63u)) - 1ull) : ~0ull; }
// the first of `n` rows of `words` whose last word has a padding bit set, or n
inline uint64_t binary_first_bad_padding(const uint64_t* words, uint64_t n, uint32_t n_bits) {
    const uint64_t W = binary_words(n_bits), bad = ~binary_last_word_mask(n_bits);
    if (bad == 0) return n;
    for (uint64_t r = 0; r < n; r++)
        if (words[r * W + W - 1] & bad) return r;
    return n;
}

// ott_store_set_binary's checks, in order.  store_len: ott_store_len
inline BinaryRefusal binary_check_set(bool multi_gpu, const uint64_t* words, uint64_t n, uint32_t n_bits, uint64_t store_len, uint64_t* a, uint64_t* b) {
    *a = *b = 0;
    if (multi_gpu) return BINARY_SET_MULTI_GPU;
    if (n_bits == 0 || n_bits > BINARY_MAX_BITS) return *a = n_bits, BINARY_SET_BITS;
    if (n != store_len) return *a = n, *b = store_len, BINARY_SET_LENGTH;
    if (n != 0 && !words) return BINARY_SET_NULL;
    const uint64_t r = binary_first_bad_padding(words, n, n_bits);
    if (r != n) return *a = r, *b = n_bits, BINARY_SET_PADDING;
    return BINARY_OK;
}
inline BinaryRefusal binary_check_sign(bool multi_gpu, uint32_t dim, uint64_t* a) {
    *a = 0;
    if (multi_gpu) return BINARY_SIGN_MULTI_GPU;
    if (dim > BINARY_MAX_BITS) return *a = dim, BINARY_SIGN_DIM;
    return BINARY_OK;
}
// what a query's arguments alone decide.  mode: 0 MERGED, 1 PER_QUERY; metric: 3 = MANHATTAN; path: 2 = MFMA
constexpr uint32_t BINARY_METRIC_MANHATTAN = 3;
inline BinaryRefusal binary_check_query_args(uint32_t nq, uint32_t mode, uint32_t metric, uint32_t path, const void* q_words, uint64_t* a) {
    *a = 0;
    if (nq == 0) return BINARY_Q_NO_QUERIES;
    if (nq > BINARY_MAX_QUERIES) return *a = nq, BINARY_Q_TOO_MANY_QUERIES;
    if (mode != 1 && nq > 1) return BINARY_Q_MERGED;
    if (metric != BINARY_METRIC_MANHATTAN) return BINARY_Q_METRIC;
    if (path == 2) return BINARY_Q_MFMA;
    if (!q_words) return BINARY_Q_NULL;
    return BINARY_OK;
}
// ... what the store decides.  binary_rows: the rows the bit rows cover; has_binary: they are set
inline BinaryRefusal binary_check_store(bool multi_gpu, bool has_binary, uint64_t binary_rows, uint64_t store_rows, int tie_order, uint64_t* a, uint64_t* b) {
    *a = *b = 0;
    if (multi_gpu) return BINARY_Q_MULTI_GPU;
    if (!has_binary) return BINARY_Q_NO_ROWS;
    if (binary_rows != store_rows) return *a = binary_rows, *b = store_rows, BINARY_Q_STALE;
    if (tie_order != 0) return BINARY_Q_TIE_ORDER;
    if (store_rows >= BINARY_MAX_ROWS) return BINARY_Q_TOO_MANY_ROWS;
    return BINARY_OK;
}
inline BinaryRefusal binary_check_query(const uint64_t* q_words, uint32_t nq, uint32_t n_bits, uint64_t* a, uint64_t* b) {
    *a = *b = 0;
    const uint64_t bad = binary_first_bad_padding(q_words, nq, n_bits);
    if (bad != nq) return *a = bad, *b = n_bits, BINARY_Q_PADDING;
    return BINARY_OK;
}
// k_eff = min(k, rows the chunk mask leaves)
inline BinaryRefusal binary_check_cap(uint64_t cap, uint32_t nq, uint64_t k_eff, uint64_t n_rows) {
    if (cap < k_eff * nq) return BINARY_Q_CAP;
    if (k_eff > 512 && (uint64_t)nq * n_rows > BINARY_MAX_SORT_PAIRS) return BINARY_Q_TOO_MANY_PAIRS;
    return BINARY_OK;
}

// ---- the device layout --------------------------------------------------------------------------------------------------------------------
// Slice t holds rows 64 t .. 64 t + 63, transposed: unit p (16 bytes = bits 128 p .. 128 p + 127) of its 64 rows lies in 64
// consecutive units, so the 64 lanes of a wave, lane = row, read unit p of their rows with one 16-byte load each: a coalesced
// 1-KiB wave load, and every lane holds its own row's bits (no cross-lane reduction).  Rows are padded to whole units with zero
// bits; the last slice is padded with zero rows that no lane ever claims.  Every offset is 64-bit.
inline uint64_t binary_slices(uint64_t n_rows) { return (n_rows + BINARY_SLICE - 1) / BINARY_SLICE; }
inline uint64_t binary_slice_bytes(uint32_t units) { return (uint64_t)units * BINARY_SLICE * BINARY_UNIT_BYTES; }
// the byte offset of unit p of row `row`
inline uint64_t binary_unit_offset(uint64_t row, uint32_t p, uint32_t units) {
    return ((row / BINARY_SLICE) * units + p) * (uint64_t)(BINARY_SLICE * BINARY_UNIT_BYTES) + (row & (BINARY_SLICE - 1)) * BINARY_UNIT_BYTES;
}
// ... of 64-bit word w of that row (word w is half w & 1 of unit w / 2)
inline uint64_t binary_word_offset(uint64_t row, uint32_t w, uint32_t units) { return binary_unit_offset(row, w >> 1, units) + (uint64_t)(w & 1u) * 8u; }
inline uint64_t binary_layout_bytes(uint64_t n_rows, uint32_t n_bits) { return binary_slices(n_rows) * binary_slice_bytes(binary_units(n_bits)); }
// the layout bytes of the slices rows [row0, row1) lie in
inline uint64_t binary_range_bytes(uint64_t row0, uint64_t row1, uint32_t units) {
    if (row1 <= row0) return 0;
    return ((row1 + BINARY_SLICE - 1) / BINARY_SLICE - row0 / BINARY_SLICE) * binary_slice_bytes(units);
}
// the layout bytes of the slices the chunk runs touch (a slice two runs share counts once).  runs: n_runs (start, count) pairs of
// rows, ascending and disjoint (ott_run's two fields)
inline uint64_t binary_run_bytes(const uint64_t* runs, size_t n_runs, uint32_t units) {
    uint64_t bytes = 0, done = 0;  // slices below `done` are counted
    for (size_t i = 0; i < n_runs; i++) {
        const uint64_t start = runs[2 * i], count = runs[2 * i + 1];
        uint64_t t0 = start / BINARY_SLICE;
        const uint64_t t1 = (start + count + BINARY_SLICE - 1) / BINARY_SLICE;
        if (t0 < done) t0 = done;
        if (t1 > t0) bytes += binary_range_bytes(t0 * BINARY_SLICE, t1 * BINARY_SLICE, units);
        if (t1 > done) done = t1;
    }
    return bytes;
}
inline uint64_t binary_bytes_scanned(uint32_t passes, uint64_t slice_bytes) { return (uint64_t)passes * slice_bytes; }

// ---- the route ------------------------------------------------------------------------------------------------------------------------------
// TABLE route: the sweep writes a key per (query, row) into the context's key table and the shared top-k reads it back; serves every
// call.  GATED route: the selection is fused into the sweep — per workgroup and query of the pass a histogram of the distances let
// through and a gate word in LDS, candidates appended to the pair arrays, one sort behind the sweep — and no key table exists.
// The histogram of one query: n_bits + 1 levels and the gate word, 4 bytes each.
inline size_t binary_gate_query_lds(uint32_t n_bits) { return ((size_t)n_bits + 2u) * 4u; }
// queries per pass of the gated route: the most of 4, 2, 1 — at most nq — whose histograms fit the LDS budget; 0 = none fits
inline uint32_t binary_gate_tile(uint32_t n_bits, uint32_t nq) {
    for (uint32_t t = BINARY_GATE_NQ; t >= 1; t >>= 1)
        if ((t <= nq || t == 1) && t * binary_gate_query_lds(n_bits) <= BINARY_GATE_LDS_BYTES) return t;
    return 0;
}
inline size_t binary_gate_lds_bytes(uint32_t n_bits, uint32_t tile) { return tile * binary_gate_query_lds(n_bits); }
// The pair capacity the plan chooses: every pair where the call has at most 2^20 of them, else an eighth of them, at least 2^20 and at
// most 2^27 (whatever the call's size the arrays stay below a few GB; a context that cannot allocate them answers on the table route).
// The corpora of benchmarks/binary.py emit 1.3 to 2 % of their pairs on 1M rows and 0.23 to 0.29 % on 10M rows at k = 10, 13 to 27 %
// and 4.5 to 5.1 % at k = 100 (64 queries with k = 100 on 1M rows overflowed); a call that emits more than the capacity is answered by
// the table route.  option: the store's binary_gate_cap (0 = the plan's).
inline uint64_t binary_gate_capacity(uint64_t option, uint32_t nq, uint64_t rows) {
    const uint64_t pairs = (uint64_t)nq * rows;
    if (option) return option < pairs ? option : pairs;
    const uint64_t eighth = pairs / 8;
    uint64_t cap = eighth > BINARY_GATE_MIN_CAP ? eighth : BINARY_GATE_MIN_CAP;
    if (cap > BINARY_GATE_MAX_CAP) cap = BINARY_GATE_MAX_CAP;
    return cap < pairs ? cap : pairs;
}
inline bool binary_gate_eligible(uint32_t n_bits, uint32_t nq, uint64_t k_eff, uint64_t rows, uint64_t cap_option) {
    if (k_eff == 0 || k_eff > BINARY_GATE_MAX_K) return false;
    if (binary_gate_tile(n_bits, nq) == 0) return false;
    return binary_gate_capacity(cap_option, nq, rows) < BINARY_MAX_ROWS;  // (the sort's pair count stays below 2^32 - 16)
}
// option: the store's binary_gate (-1 automatic, 0 never, 1 wherever eligible).
// AUTOMATIC is the table route for every shape, as measured on the MI355X (benchmarks/binary.py, profiles/binary/README.md: 1M and 10M
// rows x 1024 bits, i.i.d. and clustered, k 10 and 100, ms per call, table / gated): 1M rows, 1 query 0.080 / 0.624 and 0.128 / 0.811,
// 4 queries 0.093 / 1.67 and 0.175 / 2.48, 64 queries 0.98 / 9.8 and 2.07 / 16.7; 10M rows, 1 query 0.366 / 1.80 and 0.502 / 5.80, 4 queries
// 0.542 / 5.01 and 0.733 / 19.2, 64 queries 8.1 / 21.8 and 10.8 / 113 — the gated route emits 13k to 29k pairs per query at k = 10 and
// 125k to 510k at k = 100 (the first round of the grid runs under open gates), and its histogram atomics, scans and the sort of the
// pairs cost more than the key table they avoid.  It stays as the option.
constexpr bool BINARY_AUTO_GATE = false;
inline bool binary_take_gate(int option, uint32_t n_bits, uint32_t nq, uint64_t k_eff, uint64_t rows, uint64_t cap_option) {
    if (!binary_gate_eligible(n_bits, nq, k_eff, rows, cap_option)) return false;
    if (option >= 0) return option == 1;
    return BINARY_AUTO_GATE;
}
inline uint32_t binary_passes(uint32_t tile, uint32_t nq) { return (nq + tile - 1) / tile; }

// ---- the score and the sign rule ----------------------------------------------------------------------------------------------------------
// THE DEFINITION: S = (float) popcount(q XOR v) over the row's words; exact in f32 (at most 16384 < 2^24).
inline uint32_t binary_popcount64(uint64_t x) {
    x = x - ((x >> 1) & 0x5555555555555555ull);
    x = (x & 0x3333333333333333ull) + ((x >> 2) & 0x3333333333333333ull);
    x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0Full;
    return (uint32_t)((x * 0x0101010101010101ull) >> 56);
}
inline uint32_t binary_hamming(const uint64_t* q, const uint64_t* v, uint32_t n_bits) {
    uint32_t d = 0;
    for (uint32_t w = 0; w < binary_words(n_bits); w++) d += binary_popcount64(q[w] ^ v[w]);
    return d;
}
// ott_store_set_binary_sign's bit of one f32: x > 0.0f — on the bits, so that no denormal mode can change it: NaN, -0.0, +0.0 and
// every negative give 0; +denormals and +infinity give 1
inline uint32_t binary_sign_bit_of(uint32_t f32_bits) { return (uint32_t)(f32_bits - 1u < 0x7F800000u); }
inline uint32_t binary_sign_bit(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return binary_sign_bit_of(u);
}

}  // namespace ott
