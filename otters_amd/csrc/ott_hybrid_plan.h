// ott_hybrid_plan.h — what the host decides for ott_query_hybrid (ott_fuse.hip) before it launches anything: every
// refusal with its text, the order of a request's legs (its dense legs, then its sparse legs), the output capacity, the take of
// every leg and the layout of the one upload — ott_query_fuse's (ott_fuse_plan.h: FuseLayout) with one byte per leg behind the
// weights.  The formulas are ott_fuse_plan.h's, with the leg's own take in place of the call's; the sparse side's checks are
// ott_sparse_plan.h's, under this entry point's name.  HIP-free: tests/test_hybrid_cpu.py compiles it with the host compiler under
// AddressSanitizer + UBSan and walks it.
#pragma once

#include "ott_fuse_plan.h"
#include "ott_sparse_plan.h"

namespace ott {

constexpr uint32_t HYBRID_IDF = 1u;  // OTT_HYBRID_IDF: bit 0 of sparse_flags

// ---- the refusals, in the order the call makes them; all before any device work ------------------------------------------------------
enum HybridRefusal {
    HYBRID_OK = 0,
    // what the arguments alone decide (hybrid_check_args)
    HYBRID_NOT_PER_QUERY,      // d->mode != OTT_MODE_PER_QUERY                                   (OTT_ERR_UNSUPPORTED)
    HYBRID_NO_REQUESTS,
    HYBRID_TOO_MANY_REQUESTS,
    HYBRID_NULL_LEGS,          // dense_per_request NULL with d->nq != 0, or sparse_per_request NULL with n_sparse != 0
    HYBRID_BAD_FETCH,
    HYBRID_BAD_LEGS,           // a request with 0 legs or more than FUSE_MAX_LEGS, dense plus sparse     (*bad: the request)
    HYBRID_TOO_MANY_ENTRIES,   // legs_b x fetch > FUSE_MAX_ENTRIES                                       (*bad: the request)
    HYBRID_DENSE_SUM,          // dense_per_request does not add up to d->nq
    HYBRID_SPARSE_SUM,         // sparse_per_request does not add up to n_sparse
    HYBRID_BAD_FUSION,
    HYBRID_BAD_RRF_K,
    HYBRID_BAD_WEIGHT,         // a leg weight that is not finite                                         (*bad: the leg)
    HYBRID_BAD_K,
    HYBRID_BAD_SPARSE_CMP,     // sparse_cmp is no ott_cmp
    HYBRID_BAD_FLAGS,          // a bit of sparse_flags other than OTT_HYBRID_IDF
    HYBRID_TOO_MANY_SPARSE,    // n_sparse > SPARSE_MAX_QUERIES
    HYBRID_SPARSE_NULL,        // sq_indptr NULL, or sq_indices / sq_values NULL with entries
    HYBRID_INDPTR0,
    HYBRID_INDPTR_ORDER,       // sq_indptr decreases                                                     (*bad: the sparse query)
    // what the store decides
    HYBRID_MULTI_GPU,          //                                                                 (OTT_ERR_UNSUPPORTED)
    HYBRID_TOO_MANY_ROWS,      // 2^51 rows or more, or 2^32 - 16 or more with sparse legs        (OTT_ERR_UNSUPPORTED)
    HYBRID_TIE_ORDER,          // tie orders 1 and 2, whether or not a sparse leg exists          (OTT_ERR_UNSUPPORTED)
    HYBRID_NO_SPARSE_ROWS,
    HYBRID_STALE,              // rows were appended since ott_store_set_sparse                  (*bad, *v: the two counts)
    HYBRID_INDEX_RANGE,        // index *v of sparse query *bad is not below the vocab
    HYBRID_INDEX_DUP,
    HYBRID_SPARSE_WEIGHT,      // a sparse query's weight is not finite (with OTT_HYBRID_IDF: after the scaling too)
    HYBRID_CAP,
    HYBRID_NULL_OUT,
};

inline int hybrid_refusal_status(HybridRefusal r) {
    switch (r) {
        case HYBRID_OK: return 0;
        case HYBRID_NOT_PER_QUERY: case HYBRID_MULTI_GPU: case HYBRID_TOO_MANY_ROWS: case HYBRID_TIE_ORDER: return -4;
        default: return -1;
    }
}

inline std::string hybrid_refusal_text(HybridRefusal r, uint64_t bad, uint64_t v) {
    const std::string name = "ott_query_hybrid: ";
    const std::string A = std::to_string(bad), B = std::to_string(v);
    switch (r) {
        case HYBRID_OK: return std::string();
        case HYBRID_NOT_PER_QUERY: return name + "the legs are ranked one by one: d->mode must be OTT_MODE_PER_QUERY";
        case HYBRID_NO_REQUESTS: return name + "n_requests must be at least 1";
        case HYBRID_TOO_MANY_REQUESTS: return name + B + " requests are above OTT_FUSE_MAX_REQUESTS (" + std::to_string(FUSE_MAX_REQUESTS) + ")";
        case HYBRID_NULL_LEGS: return name + "dense_per_request or sparse_per_request is NULL although its legs are given";
        case HYBRID_BAD_FETCH: return name + "fetch must lie between 1 and OTT_FUSE_MAX_FETCH (" + std::to_string(FUSE_MAX_FETCH) + ")";
        case HYBRID_BAD_LEGS:
            return name + "request " + A + " has " + B + " legs (dense plus sparse); a request takes 1 to OTT_FUSE_MAX_LEGS (" + std::to_string(FUSE_MAX_LEGS) + ")";
        case HYBRID_TOO_MANY_ENTRIES:
            return name + "request " + A + " has " + B + " entries (legs x fetch), above OTT_FUSE_MAX_ENTRIES (" + std::to_string(FUSE_MAX_ENTRIES) + ")";
        case HYBRID_DENSE_SUM: return name + "dense_per_request adds up to " + B + ", not to d->nq";
        case HYBRID_SPARSE_SUM: return name + "sparse_per_request adds up to " + B + ", not to n_sparse";
        case HYBRID_BAD_FUSION: return name + "unknown fusion (OTT_FUSE_RRF, OTT_FUSE_DBSF or OTT_FUSE_MINMAX)";
        case HYBRID_BAD_RRF_K: return name + "rrf_k must be finite and at least 0";
        case HYBRID_BAD_WEIGHT: return name + "the weight of leg " + A + " is not finite";
        case HYBRID_BAD_K: return name + "k must be at least 1";
        case HYBRID_BAD_SPARSE_CMP: return name + "unknown sparse filter comparator";
        case HYBRID_BAD_FLAGS: return name + "unknown bits in sparse_flags (OTT_HYBRID_IDF is the only one)";
        case HYBRID_TOO_MANY_SPARSE: return name + B + " sparse legs are above OTT_SPARSE_MAX_QUERIES (" + std::to_string(SPARSE_MAX_QUERIES) + ")";
        case HYBRID_SPARSE_NULL: return name + "sq_indptr, sq_indices or sq_values is NULL";
        case HYBRID_INDPTR0: return name + "sq_indptr[0] is " + B + ", not 0";
        case HYBRID_INDPTR_ORDER: return name + "sq_indptr decreases at sparse query " + A;
        case HYBRID_MULTI_GPU: return name + "a multi-GPU store is not served (the legs' lists lie on different GPUs, sparse rows on one)";
        case HYBRID_TOO_MANY_ROWS: return name + "the store holds too many rows (2^51 for the fused key, 2^32 - 16 with sparse legs)";
        case HYBRID_TIE_ORDER: return name + "tie_order 1 and 2 are not served: the reference has no sparse ranking to reproduce; use the canonical order";
        case HYBRID_NO_SPARSE_ROWS: return name + "no sparse rows are set (ott_store_set_sparse)";
        case HYBRID_STALE:
            return name + "the sparse rows cover " + A + " rows, the store holds " + B + " (rows were appended since ott_store_set_sparse: set them again)";
        case HYBRID_INDEX_RANGE: return name + "index " + B + " of sparse query " + A + " is not below the store's vocab";
        case HYBRID_INDEX_DUP: return name + "index " + B + " appears twice in sparse query " + A;
        case HYBRID_SPARSE_WEIGHT: return name + "the weight of index " + B + " of sparse query " + A + " is not finite";
        case HYBRID_CAP: return name + "output capacity is smaller than the sum over the requests of min(k, legs x min(fetch, rows))";
        case HYBRID_NULL_OUT: return name + "out is NULL";
    }
    return std::string();
}

// what the arguments alone decide (no store is looked at).  cmp_max: the last ott_cmp (OTT_CMP_EQ).  *bad / *v: what the message names.
inline HybridRefusal hybrid_check_args(bool per_query, const uint32_t* dense_per_request, const uint32_t* sparse_per_request, uint32_t n_requests, uint32_t nq_dense,
                                       uint32_t n_sparse, uint64_t fetch, uint32_t fusion, float rrf_k, const float* leg_weights, uint64_t k, uint32_t sparse_cmp,
                                       uint32_t cmp_max, uint32_t sparse_flags, const uint64_t* sq_indptr, const uint32_t* sq_indices, const float* sq_values,
                                       uint64_t* bad, uint64_t* v) {
    *bad = 0;
    *v = 0;
    if (!per_query) return HYBRID_NOT_PER_QUERY;
    if (n_requests == 0) return HYBRID_NO_REQUESTS;
    if (n_requests > FUSE_MAX_REQUESTS) { *v = n_requests; return HYBRID_TOO_MANY_REQUESTS; }
    if ((!dense_per_request && nq_dense) || (!sparse_per_request && n_sparse)) return HYBRID_NULL_LEGS;
    if (fetch == 0 || fetch > FUSE_MAX_FETCH) return HYBRID_BAD_FETCH;
    uint64_t dsum = 0, ssum = 0;
    for (uint32_t b = 0; b < n_requests; b++) {
        const uint64_t nd = dense_per_request ? dense_per_request[b] : 0, ns = sparse_per_request ? sparse_per_request[b] : 0, l = nd + ns;
        *bad = b;
        if (l == 0 || l > FUSE_MAX_LEGS) { *v = l; return HYBRID_BAD_LEGS; }
        if (l * fetch > FUSE_MAX_ENTRIES) { *v = l * fetch; return HYBRID_TOO_MANY_ENTRIES; }
        dsum += nd;
        ssum += ns;
    }
    *bad = 0;
    if (dsum != nq_dense) { *v = dsum; return HYBRID_DENSE_SUM; }
    if (ssum != n_sparse) { *v = ssum; return HYBRID_SPARSE_SUM; }
    if (fusion > FUSE_MINMAX) return HYBRID_BAD_FUSION;
    if (fusion == FUSE_RRF && !(fuse_finite(rrf_k) && rrf_k >= 0.0f)) return HYBRID_BAD_RRF_K;
    if (leg_weights)
        for (uint64_t l = 0; l < dsum + ssum; l++)
            if (!fuse_finite(leg_weights[l])) { *bad = l; return HYBRID_BAD_WEIGHT; }
    if (k == 0) return HYBRID_BAD_K;
    if (sparse_cmp > cmp_max) return HYBRID_BAD_SPARSE_CMP;
    if (sparse_flags & ~HYBRID_IDF) return HYBRID_BAD_FLAGS;
    if (n_sparse > SPARSE_MAX_QUERIES) { *v = n_sparse; return HYBRID_TOO_MANY_SPARSE; }
    if (n_sparse) {
        if (!sq_indptr) return HYBRID_SPARSE_NULL;
        if (sq_indptr[0] != 0) { *v = sq_indptr[0]; return HYBRID_INDPTR0; }
        for (uint32_t q = 0; q < n_sparse; q++)
            if (sq_indptr[q + 1] < sq_indptr[q]) { *bad = q; return HYBRID_INDPTR_ORDER; }
        if (sq_indptr[n_sparse] != 0 && (!sq_indices || !sq_values)) return HYBRID_SPARSE_NULL;
    }
    return HYBRID_OK;
}

// a refusal of the sparse side's own checks (sparse_check_store, sparse_check_query) under this entry point's name; a, b are theirs
inline HybridRefusal hybrid_from_sparse(SparseRefusal r) {
    switch (r) {
        case SPARSE_OK: return HYBRID_OK;
        case SPARSE_Q_MULTI_GPU: return HYBRID_MULTI_GPU;
        case SPARSE_Q_NO_ROWS: return HYBRID_NO_SPARSE_ROWS;
        case SPARSE_Q_STALE: return HYBRID_STALE;
        case SPARSE_Q_TIE_ORDER: return HYBRID_TIE_ORDER;
        case SPARSE_Q_TOO_MANY_ROWS: return HYBRID_TOO_MANY_ROWS;
        case SPARSE_Q_INDEX_RANGE: return HYBRID_INDEX_RANGE;
        case SPARSE_Q_INDEX_DUP: return HYBRID_INDEX_DUP;
        case SPARSE_Q_WEIGHT: return HYBRID_SPARSE_WEIGHT;
        default: return HYBRID_SPARSE_NULL;  // (the argument checks ran before: not reached)
    }
}
// what the store decides before its sparse rows are looked at.  A tie order other than the canonical one refuses the whole call.
inline HybridRefusal hybrid_check_store(bool multi_gpu, uint64_t rows, int tie_order) {
    if (multi_gpu) return HYBRID_MULTI_GPU;
    if (rows >= FUSE_ROW_LIMIT) return HYBRID_TOO_MANY_ROWS;
    if (tie_order != 0) return HYBRID_TIE_ORDER;
    return HYBRID_OK;
}

// ---- a request's legs ------------------------------------------------------------------------------------------------------------------
// Request b's legs are first[b] .. first[b] + nd_b + ns_b - 1: its dense legs in the caller's order, then its sparse legs in the
// caller's order.  dense_at[i] / sparse_at[j]: the leg of the call's i-th dense query / j-th sparse query; total[b] = nd_b + ns_b.
inline uint32_t hybrid_leg_order(const uint32_t* dense_per_request, const uint32_t* sparse_per_request, uint32_t n_requests, uint32_t* first, uint32_t* total,
                                 uint32_t* dense_at, uint32_t* sparse_at) {
    uint32_t at = 0, i = 0, j = 0, most = 0;
    for (uint32_t b = 0; b < n_requests; b++) {
        const uint32_t nd = dense_per_request ? dense_per_request[b] : 0, ns = sparse_per_request ? sparse_per_request[b] : 0;
        first[b] = at;
        total[b] = nd + ns;
        for (uint32_t x = 0; x < nd; x++) dense_at[i++] = at++;
        for (uint32_t x = 0; x < ns; x++) sparse_at[j++] = at++;
        if (nd + ns > most) most = nd + ns;
    }
    return most;  // the legs of the call's largest request
}

// ---- the scratch and the upload ----------------------------------------------------------------------------------------------------------
// ott_query_fuse's block with take[legs] (one byte per leg, 1 = the leg is best first under take Max) behind the weights:
// [blocks | first | legs | weights | take | pad] go up in one copy, [counts | hits] come back.
struct HybridLayout {
    FuseLayout f;
    size_t off_take;
};
inline HybridLayout hybrid_layout(uint32_t legs, uint32_t n_requests, uint64_t stride, uint64_t k, uint32_t max_legs) {
    HybridLayout L;
    L.f = fuse_layout(legs, n_requests, stride, k, max_legs);
    L.off_take = L.f.off_weights + (size_t)legs * 4;
    L.f.meta_bytes += ((size_t)legs + 3) & ~(size_t)3;
    L.f.upload_bytes = L.f.block_bytes + L.f.meta_bytes;
    L.f.off_counts = fuse_align(L.f.upload_bytes);
    L.f.off_hits = L.f.off_counts + fuse_align((size_t)n_requests * 4);
    L.f.total = L.f.off_counts + L.f.result_bytes;
    return L;
}

}  // namespace ott
