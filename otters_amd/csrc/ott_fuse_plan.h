// ott_fuse_plan.h — what the host decides for ott_query_fuse (ott_fuse.hip) before it launches anything: every
// refusal with its text, the output capacity a call needs, the layout of the context's scratch and of the one upload, the packing of
// an entry's sort key with its 51-bit check, the padded entry count and the LDS it takes, the route decision, and the HOST STATEMENT
// OF THE THREE FORMULAS — the contribution of one entry and the fused score of a row, one IEEE operation at a time, in the
// contract's order.  The device kernel (fuse_kernel) computes the same operations with the _rn intrinsics.  HIP-free:
// tests/test_fuse_cpu.py compiles it with the host compiler under AddressSanitizer + UBSan, walks it, and holds the formulas to the
// numpy model (tests/fuse_ref.py) bit for bit.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace ott {

constexpr uint32_t FUSE_MAX_LEGS = 16;        // OTT_FUSE_MAX_LEGS: legs of one request (4 bits of the key)
constexpr uint32_t FUSE_MAX_FETCH = 512;      // OTT_FUSE_MAX_FETCH: hits a leg contributes (9 bits of the key; query_on's device output limit)
constexpr uint32_t FUSE_MAX_ENTRIES = 8192;   // OTT_FUSE_MAX_ENTRIES: legs_b x fetch of one request (one workgroup's LDS)
constexpr uint32_t FUSE_MAX_REQUESTS = 1024;  // OTT_FUSE_MAX_REQUESTS
constexpr uint32_t FUSE_THREADS = 1024;       // the kernel's workgroup at most: sixteen waves, one per leg in the statistics
constexpr uint32_t FUSE_ENTRY_LDS = 12;       // bytes of LDS per padded entry: a 64-bit key and an f32 contribution
constexpr uint64_t FUSE_ROW_LIMIT = 1ull << 51;  // local rows an entry's key can name

enum : uint32_t { FUSE_RRF = 0, FUSE_DBSF = 1, FUSE_MINMAX = 2 };  // ott_fusion

// ---- the refusals, in the order the call makes them; all before any device work ------------------------------------------------------
enum FuseRefusal {
    FUSE_OK = 0,
    FUSE_NOT_PER_QUERY,      // d->mode != OTT_MODE_PER_QUERY                                     (OTT_ERR_UNSUPPORTED)
    FUSE_NO_REQUESTS,        // n_requests == 0
    FUSE_TOO_MANY_REQUESTS,  // n_requests > FUSE_MAX_REQUESTS
    FUSE_NULL_LEGS,          // legs_per_request == NULL
    FUSE_BAD_FETCH,          // fetch == 0 or > FUSE_MAX_FETCH
    FUSE_BAD_LEGS,           // a request with 0 legs or more than FUSE_MAX_LEGS   (*bad says which request)
    FUSE_TOO_MANY_ENTRIES,   // legs_b x fetch > FUSE_MAX_ENTRIES                  (*bad says which request)
    FUSE_LEG_SUM,            // the legs do not add up to d->nq
    FUSE_BAD_FUSION,         // unknown fusion
    FUSE_BAD_RRF_K,          // RRF: rrf_k not finite or below 0
    FUSE_BAD_WEIGHT,         // a weight that is not finite                        (*bad says which leg)
    FUSE_BAD_K,              // k == 0
    // what the store decides (fuse_check_store, fuse_check_cap)
    FUSE_MULTI_GPU,          //                                                                   (OTT_ERR_UNSUPPORTED)
    FUSE_TOO_MANY_ROWS,      // 2^51 rows or more: the key holds the local row in 51 bits       (OTT_ERR_UNSUPPORTED)
    FUSE_CAP,                // cap < sum over b of min(k, legs_b x min(fetch, rows))
    FUSE_NULL_OUT,           // out == NULL with cap > 0
};

// ott_status of a refusal: OTT_ERR_INVALID (-1) or OTT_ERR_UNSUPPORTED (-4)
inline int fuse_refusal_status(FuseRefusal r) {
    switch (r) {
        case FUSE_OK: return 0;
        case FUSE_NOT_PER_QUERY: case FUSE_MULTI_GPU: case FUSE_TOO_MANY_ROWS: return -4;
        default: return -1;
    }
}

// the message of a refusal; `bad` is the request or leg the refusal names, `v` the count it names
inline std::string fuse_refusal_text(FuseRefusal r, uint64_t bad, uint64_t v) {
    const std::string name = "ott_query_fuse: ";
    switch (r) {
        case FUSE_OK: return std::string();
        case FUSE_NOT_PER_QUERY: return name + "the legs are ranked one by one: d->mode must be OTT_MODE_PER_QUERY";
        case FUSE_NO_REQUESTS: return name + "n_requests must be at least 1";
        case FUSE_TOO_MANY_REQUESTS: return name + std::to_string(v) + " requests are above OTT_FUSE_MAX_REQUESTS (" + std::to_string(FUSE_MAX_REQUESTS) + ")";
        case FUSE_NULL_LEGS: return name + "legs_per_request is NULL";
        case FUSE_BAD_FETCH: return name + "fetch must lie between 1 and OTT_FUSE_MAX_FETCH (" + std::to_string(FUSE_MAX_FETCH) + ")";
        case FUSE_BAD_LEGS:
            return name + "request " + std::to_string(bad) + " has " + std::to_string(v) + " legs; a request takes 1 to OTT_FUSE_MAX_LEGS (" +
                   std::to_string(FUSE_MAX_LEGS) + ")";
        case FUSE_TOO_MANY_ENTRIES:
            return name + "request " + std::to_string(bad) + " has " + std::to_string(v) + " entries (legs x fetch), above OTT_FUSE_MAX_ENTRIES (" +
                   std::to_string(FUSE_MAX_ENTRIES) + ")";
        case FUSE_LEG_SUM: return name + "legs_per_request adds up to " + std::to_string(v) + ", not to d->nq";
        case FUSE_BAD_FUSION: return name + "unknown fusion (OTT_FUSE_RRF, OTT_FUSE_DBSF or OTT_FUSE_MINMAX)";
        case FUSE_BAD_RRF_K: return name + "rrf_k must be finite and at least 0";
        case FUSE_BAD_WEIGHT: return name + "the weight of leg " + std::to_string(bad) + " is not finite";
        case FUSE_BAD_K: return name + "k must be at least 1";
        case FUSE_MULTI_GPU: return name + "a multi-GPU store is not served (the legs' lists lie on different GPUs)";
        case FUSE_TOO_MANY_ROWS: return name + "a store of 2^51 rows or more is not served (an entry's key holds the row in 51 bits)";
        case FUSE_CAP: return name + "output capacity is smaller than the sum over the requests of min(k, legs x min(fetch, rows))";
        case FUSE_NULL_OUT: return name + "out is NULL";
    }
    return std::string();
}

inline bool fuse_finite(float x) { return x - x == 0.0f; }  // false for NaN and the infinities

// what the arguments alone decide (no store is looked at).  *bad / *v: what the message names.
inline FuseRefusal fuse_check_args(bool per_query, const uint32_t* legs_per_request, uint32_t n_requests, uint32_t nq, uint64_t fetch, uint32_t fusion,
                                   float rrf_k, const float* leg_weights, uint64_t k, uint64_t* bad, uint64_t* v) {
    *bad = 0;
    *v = 0;
    if (!per_query) return FUSE_NOT_PER_QUERY;
    if (n_requests == 0) return FUSE_NO_REQUESTS;
    if (n_requests > FUSE_MAX_REQUESTS) { *v = n_requests; return FUSE_TOO_MANY_REQUESTS; }
    if (!legs_per_request) return FUSE_NULL_LEGS;
    if (fetch == 0 || fetch > FUSE_MAX_FETCH) return FUSE_BAD_FETCH;
    uint64_t sum = 0;
    for (uint32_t b = 0; b < n_requests; b++) {
        const uint32_t l = legs_per_request[b];
        *bad = b;
        if (l == 0 || l > FUSE_MAX_LEGS) { *v = l; return FUSE_BAD_LEGS; }
        if ((uint64_t)l * fetch > FUSE_MAX_ENTRIES) { *v = (uint64_t)l * fetch; return FUSE_TOO_MANY_ENTRIES; }
        sum += l;
    }
    *bad = 0;
    if (sum != nq) { *v = sum; return FUSE_LEG_SUM; }
    if (fusion > FUSE_MINMAX) return FUSE_BAD_FUSION;
    if (fusion == FUSE_RRF && !(fuse_finite(rrf_k) && rrf_k >= 0.0f)) return FUSE_BAD_RRF_K;
    if (leg_weights)
        for (uint32_t l = 0; l < nq; l++)
            if (!fuse_finite(leg_weights[l])) { *bad = l; return FUSE_BAD_WEIGHT; }
    if (k == 0) return FUSE_BAD_K;
    return FUSE_OK;
}
// ... and what the store decides
inline FuseRefusal fuse_check_store(bool multi_gpu, uint64_t rows) {
    if (multi_gpu) return FUSE_MULTI_GPU;
    if (rows >= FUSE_ROW_LIMIT) return FUSE_TOO_MANY_ROWS;  // (the last row of 2^51 would share leg 15, position 511's key with the pad)
    return FUSE_OK;
}

// ---- the capacity rule ---------------------------------------------------------------------------------------------------------------
// hits a leg's list holds at most: the first stage's k
inline uint64_t fuse_stride(uint64_t fetch, uint64_t rows) { return fetch < rows ? fetch : rows; }
// hits request b can return at most
inline uint64_t fuse_request_cap(uint64_t k, uint32_t legs, uint64_t stride) {
    const uint64_t e = (uint64_t)legs * stride;
    return k < e ? k : e;
}
inline uint64_t fuse_cap_needed(const uint32_t* legs_per_request, uint32_t n_requests, uint64_t k, uint64_t fetch, uint64_t rows) {
    const uint64_t stride = fuse_stride(fetch, rows);
    uint64_t need = 0;
    for (uint32_t b = 0; b < n_requests; b++) need += fuse_request_cap(k, legs_per_request[b], stride);
    return need;
}
inline FuseRefusal fuse_check_cap(const void* out, uint64_t cap, uint64_t need) {
    if (cap < need) return FUSE_CAP;
    if (!out && cap) return FUSE_NULL_OUT;
    return FUSE_OK;
}

// ---- an entry's key --------------------------------------------------------------------------------------------------------------------
// local row << 13 | leg << 9 | position: sorted ascending, the entries of one row lie together in leg order.  The all-ones key pads.
constexpr uint64_t FUSE_PAD_KEY = ~0ull;
inline bool fuse_key_fits(uint64_t local_row) { return local_row < FUSE_ROW_LIMIT; }
inline uint64_t fuse_key(uint64_t local_row, uint32_t leg, uint32_t pos) { return (local_row << 13) | ((uint64_t)leg << 9) | pos; }
inline uint64_t fuse_key_row(uint64_t key) { return key >> 13; }
inline uint32_t fuse_key_leg(uint64_t key) { return (uint32_t)(key >> 9) & 15u; }
inline uint32_t fuse_key_pos(uint64_t key) { return (uint32_t)key & 511u; }

// ---- padded entry counts, threads, LDS ---------------------------------------------------------------------------------------------
// the bitonic network of a request: the next power of two at or above its entries (legs x stride), 64 at least
inline uint32_t fuse_padded(uint32_t entries) {
    uint32_t p = 64;
    while (p < entries) p <<= 1;
    return p;
}
inline uint32_t fuse_threads(uint32_t padded) { return padded < FUSE_THREADS ? padded : FUSE_THREADS; }
inline size_t fuse_lds_bytes(uint32_t padded) { return (size_t)padded * FUSE_ENTRY_LDS; }

// ---- the scratch of a call (one block of the query context) -------------------------------------------------------------------------
// [blocks: nq x stride ott_hit, sentinel padded | first: n_requests u32 | legs: n_requests u32 | weights: nq f32 |
//  counts: n_requests u32 | hits: n_requests x kout ott_hit]
// Leg l's list starts at l x stride; request b's legs are first[b] .. first[b] + legs[b] - 1.  The device route uploads
// [first | legs | weights] (meta_bytes, from off_first) and the first stage writes the blocks; the host route uploads
// [blocks | first | legs | weights] in one copy (from 0, off_counts_unaligned bytes).  counts and hits come back together.
struct FuseLayout {
    size_t off_blocks, off_first, off_legs, off_weights, off_counts, off_hits, total;
    size_t block_bytes, meta_bytes, upload_bytes, result_bytes;
    uint32_t kout;  // output slots per request: min(k, the largest request's entries)
};
inline size_t fuse_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline FuseLayout fuse_layout(uint32_t nq, uint32_t n_requests, uint64_t stride, uint64_t k, uint32_t max_legs) {
    FuseLayout L;
    const uint64_t most = (uint64_t)max_legs * stride;
    L.kout = (uint32_t)(k < most ? k : most);
    L.off_blocks = 0;
    L.block_bytes = (size_t)nq * stride * 16;
    L.off_first = L.block_bytes;  // (a multiple of 16)
    L.off_legs = L.off_first + (size_t)n_requests * 4;
    L.off_weights = L.off_legs + (size_t)n_requests * 4;
    L.meta_bytes = (size_t)n_requests * 8 + (size_t)nq * 4;
    L.upload_bytes = L.block_bytes + L.meta_bytes;
    L.off_counts = fuse_align(L.upload_bytes);
    L.off_hits = L.off_counts + fuse_align((size_t)n_requests * 4);
    L.result_bytes = fuse_align((size_t)n_requests * 4) + (size_t)n_requests * L.kout * 16;
    L.total = L.off_counts + L.result_bytes;
    return L;
}

// ---- the route ---------------------------------------------------------------------------------------------------------------------
// Device route: the first stage leaves the legs' blocks in the context's scratch (query_on's device output, no host wait) and the
// kernel reads them there.  Host route: the first stage returns to the host, the lists go up in one copy.  Device output ranks
// candidates in the canonical order only, so tie orders 1 and 2 always take the host route.  option: the store's fuse_device
// (-1 automatic, 0 never, 1 wherever eligible).  Automatic stays on the host route: on 1M rows the two routes'
// medians differ by less than the first stage's own run-to-run spread, in either direction (profiles/fuse/README.md).
inline bool fuse_device_eligible(int tie_order, uint64_t stride) { return tie_order == 0 && stride <= FUSE_MAX_FETCH; }
inline bool fuse_take_device(int option, int tie_order, uint64_t stride) {
    if (!fuse_device_eligible(tie_order, stride)) return false;
    return option == 1;
}

// ---- the host statement of the formulas --------------------------------------------------------------------------------------------
// Every operation below is one rounded IEEE operation; the volatile stores keep the host compiler from contracting a multiplication
// and an addition whatever -ffp-contract says (the device code uses the _rn intrinsics for the same reason).
inline float fuse_f32(float x) { volatile float v = x; return v; }
inline double fuse_f64(double x) { volatile double v = x; return v; }

// the sum of n f64 terms in the contract's order: partial t (0 <= t < 64) adds the terms at t, t + 64, ... ascending from +0.0, then
// p[t] += p[t + h] for h = 32, 16, 8, 4, 2, 1
template <typename Term>
inline double fuse_sum64(uint32_t n, Term term) {
    double p[64];
    for (uint32_t t = 0; t < 64; t++) {
        double a = 0.0;
        for (uint32_t i = t; i < n; i += 64) a = fuse_f64(a + term(i));
        p[t] = a;
    }
    for (uint32_t h = 32; h > 0; h >>= 1)
        for (uint32_t t = 0; t < h; t++) p[t] = fuse_f64(p[t] + p[t + h]);
    return p[0];
}

// what a leg's list decides for its entries: nrm = (float)(d / span) with d = s - worst (take Max) or worst - s (take Min), or 0.5
// for every entry when !(span > 0)
struct FuseLegStats {
    double worst, span;
};
inline FuseLegStats fuse_leg_stats(uint32_t fusion, bool take_max, const float* scores, uint32_t n) {
    FuseLegStats st{0.0, 0.0};
    if (n == 0 || fusion == FUSE_RRF) return st;
    if (fusion == FUSE_MINMAX) {  // the list is best first: its best score is the first, its worst the last
        const double best = (double)scores[0], worst = (double)scores[n - 1];
        st.worst = worst;
        st.span = take_max ? fuse_f64(best - worst) : fuse_f64(worst - best);
        return st;
    }
    const double dn = (double)n;
    const double mean = fuse_f64(fuse_sum64(n, [&](uint32_t i) { return (double)scores[i]; }) / dn);
    const double var = fuse_f64(fuse_sum64(n, [&](uint32_t i) {
                                    const double df = fuse_f64((double)scores[i] - mean);
                                    return fuse_f64(df * df);
                                }) / dn);
    const double sd3 = fuse_f64(3.0 * sqrt(var));
    const double lo = fuse_f64(mean - sd3), hi = fuse_f64(mean + sd3);
    st.worst = take_max ? lo : hi;
    st.span = fuse_f64(hi - lo);
    return st;
}
// the contribution of the entry at position r with score s of a leg with weight w
inline float fuse_contribution(uint32_t fusion, bool take_max, float rrf_k, float w, const FuseLegStats& st, uint32_t r, float s) {
    if (fusion == FUSE_RRF) return fuse_f32(w / fuse_f32(rrf_k + (float)(r + 1)));
    float nrm = 0.5f;
    if (st.span > 0.0) {
        const double d = take_max ? fuse_f64((double)s - st.worst) : fuse_f64(st.worst - (double)s);
        nrm = (float)fuse_f64(d / st.span);
    }
    return fuse_f32(w * nrm);
}
// the fused score of a row: +0.0f, then one f32 addition per leg that holds the row, in ascending leg order
inline float fuse_add(float F, float c) { return fuse_f32(F + c); }

}  // namespace ott
