// ott_gather.hip — candidate id lists: ott_query_ids ranks, and ott_store_score_rows scores, only the rows a
// caller lists.  The work follows the list, not the store.
//
// exact_gather8_kernel is exact_rows8_kernel's geometry with ONE indirection: a workgroup of eight waves owns 64 SLOTS of the
// ascending, duplicate-free id list instead of 64 consecutive rows; an 8-lane group owns one listed row, lane c carries chain c of
// the reference's f32x8 (src/vec_compute.rs:9-22), the cross-lane sum is wide's reduce_add in either order, the remainder is
// sequential, the queries sit in LDS.  Same additions in the same order as rows8, so the same bits.  Ascending ids keep the
// candidate key order (better score, lower row, lower query), so the block lists feed launch_merge unchanged.
//
// A ranked query that the kernel does not serve (tie_order 1 / 2, Path.Mfma, k > 128, more than 65536 ids, a multi-GPU store,
// option id_gather = 0) takes the FALLBACK: set_bits_kernel turns the list into a device row mask and the query runs today's
// code with that mask joined where every row mask reaches the kernels (compose_row_mask, ott_api.hip).
#include <string.h>

#include <algorithm>
#include <atomic>
#include <numeric>
#include <vector>

#include "ott_internal.h"
#include "ott_exact_dev.h"

namespace ott {

constexpr int G8_WAVES = 8;
constexpr int G8_UNROLL = 12;
constexpr uint32_t G8_QMAX = 2048;       // query floats per query kept in LDS
constexpr uint32_t G8_MAX_TILES = 1024;  // tiles of 64 slots per launch (and per ranked query: what the block-list chain takes)
constexpr uint64_t G8_AUTO_MAX_IDS = 10000;  // option id_gather = -1: longer lists take the mask route (measured: see ott_query_ids)
constexpr int G8_SMEM_MAX = (8 * (int)G8_QMAX + 8 * 64 + 128) * 4;  // 8 queries of 2048 floats + scores + validity + rows: 68 KB

struct GatherParams {
    const float* rows;
    const float* inv;
    const float* queries;  // [nq_pad * dimq], zero padded
    const float* qinv;     // [nq_pad]
    const uint64_t* row_mask;  // the composed mask (caller & live), or nullptr; never read by the raw-score form
    uint64_t row_mask_bits;
    const uint64_t* ids;   // [n_ids] ascending (ranked: also duplicate-free); every id < the store's length (checked on the host)
    uint64_t n_ids;
    uint64_t slot0;        // first slot of this launch (raw scores: launches of at most G8_MAX_TILES tiles)
    Cand* lists;
    unsigned long long* scored;  // ranked, with a mask: += the slots that passed it (pass 0 only); nullptr = not counted
    float* raw_out;        // raw scores: [nq][raw_stride]
    const uint64_t* pos;   // raw scores: slot -> position in the caller's list
    uint64_t raw_stride;
    uint32_t ld, dim, dimq;
    uint32_t q0, nq_total;
    uint32_t metric, take_max, cmp, reduce;
    float thr;
    uint32_t k, list_stride;
};

// NQ queries share a pass (1, 2, 4 or 8), PERQ = one list per query, RAW = no filter, no lists: every slot's score goes to
// raw_out[query][pos[slot]].  Dynamic LDS: [NQ x dimq query floats | NQ x 64 scores | 64 validity words | 64 row words].
template <int MK, int E, int NQ, bool PERQ, bool RAW = false>
__global__ __launch_bounds__(64 * G8_WAVES) void exact_gather8_kernel(GatherParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sQ = smem;                                          // [NQ][dimq]
    float* sS = smem + (size_t)NQ * p.dimq;                    // [NQ][64]
    uint32_t* sV = reinterpret_cast<uint32_t*>(sS + NQ * 64);  // [64]
    uint32_t* sR = sV + 64;                                    // [64]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane >> 3, c = lane & 7;
    const float* Q = p.queries + (size_t)p.q0 * p.dimq;
    const uint32_t nq_here = (p.nq_total - p.q0) < (uint32_t)NQ ? (p.nq_total - p.q0) : (uint32_t)NQ;
    float qinv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) qinv[q] = (uint32_t)q < nq_here ? p.qinv[p.q0 + q] : 0.0f;
    // (the uploaded query block is zero padded to a multiple of 8 queries: rows past nq_here read as zeros)
    for (uint32_t i = threadIdx.x; i < (uint32_t)NQ * p.dimq; i += 64 * G8_WAVES) sQ[i] = Q[i];

    // tile -> 64 slots of the list (the grid covers only tiles that start inside it)
    const uint64_t s0 = p.slot0 + (uint64_t)blockIdx.x * 64;
    const uint32_t cnt = (p.n_ids - s0) < 64 ? (uint32_t)(p.n_ids - s0) : 64u;
    const uint32_t lslot = 8u * (uint32_t)wave + (uint32_t)grp;  // this lane group's slot within the tile
    bool valid = lslot < cnt;
    const uint64_t my_slot = s0 + (valid ? lslot : cnt - 1);     // a slot past the list's end is clamped for the loads, invalid for the epilogue
    const uint64_t my_row = p.ids[my_slot];
    if constexpr (!RAW) {
        if (p.row_mask != nullptr && valid && my_row < p.row_mask_bits) valid = (p.row_mask[my_row >> 6] >> (my_row & 63)) & 1;  // src/vec.rs:231-237
    }
    const float* rp = p.rows + my_row * (uint64_t)p.ld;
    float vinv = 0.0f;
    if (p.metric == OTT_METRIC_COSINE) vinv = p.inv[my_row];
    __syncthreads();  // the queries are in LDS

    // the row against every query of the pass: the eight chains, wide's reduce_add, the remainder (ott_exact_dev.h: rows8_scores)
    float scq[NQ];
    rows8_scores<MK, NQ, G8_UNROLL>(sQ, p.dimq, rp, p.dim, lane, p.reduce, p.metric == OTT_METRIC_COSINE, qinv, vinv, scq);
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const float sc = scq[q];
        if constexpr (RAW) {
            if (c == 0 && valid && (uint32_t)q < nq_here) p.raw_out[(uint64_t)(p.q0 + q) * p.raw_stride + p.pos[my_slot]] = sc;
        } else {
            if (c == 0) sS[q * 64 + lslot] = sc;
        }
    }
    if constexpr (RAW) {
        return;
    } else {
        if (c == 0) {
            sV[lslot] = valid ? 1u : 0u;
            sR[lslot] = (uint32_t)my_row;
        }
        __syncthreads();

        // lane = slot of the tile: filter, key, block list(s), as rows8 builds them.  Merged: wave 0 folds the NQ x 64 candidates into
        // one list; per query: wave q builds query q's list
        const bool take_max = p.take_max != 0;
        const bool ok = sV[lane] != 0;
        const uint32_t row = sR[lane];
        if (wave == 0 && p.scored != nullptr && p.q0 == 0) {
            const uint32_t n_ok = (uint32_t)__popcll(__ballot(ok));
            if (lane == 0 && n_ok) atomicAdd(p.scored, (unsigned long long)n_ok);
        }
        auto cand_of = [&](int q, bool& pass, uint64_t& key) {
            const float s = sS[q * 64 + lane];
            pass = ok && !(s != s) && cmp_holds(s, p.cmp, p.thr);  // NaN dropped: vec_compute.rs:237
            key = ((uint64_t)ord_of(s, take_max) << 32) | (uint32_t)(~row);
        };
        if constexpr (PERQ) {
            if (wave >= NQ || (uint32_t)wave >= nq_here) return;
            bool pass;
            uint64_t key;
            cand_of(wave, pass, key);
            WaveList<E> L;
            wl_init(L);
            uint64_t tk = 0;
            uint32_t tq = 0xFFFFFFFFu;
            wl_fill_sorted(L, tk, tq, p.k, pass, key, p.q0 + wave, lane, 0u);
            Cand* dst = p.lists + ((size_t)(p.q0 + wave) * gridDim.x + blockIdx.x) * p.list_stride;
#pragma unroll
            for (int e = 0; e < E; e++) {
                Cand cd;
                cd.key = L.key[e];
                cd.q = L.q[e];
                cd.pad = 0;
                dst[e * 64 + lane] = cd;
            }
        } else {
            if (wave != 0) return;
            WaveList<E> L;
            wl_init(L);
            uint64_t tk = 0;
            uint32_t tq = 0xFFFFFFFFu;
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                if ((uint32_t)q >= nq_here) break;
                bool pass;
                uint64_t key;
                cand_of(q, pass, key);
                if (q == 0) wl_fill_sorted(L, tk, tq, p.k, pass, key, p.q0 + q, lane, 0u);
                else wl_offer_block(L, tk, tq, p.k, pass, key, p.q0 + q, lane, 0u);
            }
            Cand* dst = p.lists + (size_t)blockIdx.x * p.list_stride;
#pragma unroll
            for (int e = 0; e < E; e++) {
                Cand cd;
                cd.key = L.key[e];
                cd.q = L.q[e];
                cd.pad = 0;
                dst[e * 64 + lane] = cd;
            }
        }
    }
}

// the fallback's mask: bit ids[i] of `words` is set (the words were zeroed on the stream before); ids[i] < the store's length
__global__ __launch_bounds__(256) void set_bits_kernel(uint64_t* __restrict__ words, const uint64_t* __restrict__ ids, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = ids[i];
        atomicOr(reinterpret_cast<unsigned long long*>(words) + (r >> 6), 1ull << (r & 63));
    }
}

namespace {

uint32_t pow2ceil(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

template <int MK, int E, int NQ, bool PERQ, bool RAW>
int launch_g8(ott_store* s, const GatherParams& p, uint32_t grid) {
    const size_t smem = ((size_t)NQ * p.dimq + (size_t)NQ * 64 + 128) * 4;
    auto kern = exact_gather8_kernel<MK, E, NQ, PERQ, RAW>;
    if (smem > 48 * 1024) {  // more dynamic LDS than the default limit: the opt-in, once per device
        static std::atomic<uint64_t> attr_set{0};
        if (attr_needed(attr_set, s->device)) {
            OTT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, G8_SMEM_MAX));
            attr_done(attr_set, s->device);
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * G8_WAVES), smem, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

template <int MK>
int launch_gather_mk(ott_store* s, const GatherParams& p, uint32_t nq_tile, int E, bool perq, bool raw, uint32_t grid) {
    perq = perq && nq_tile > 1;  // (a one-query pass builds the one list either way: the caller points it at the query's slot)
#define OTT_G8(NQv, Ev, PQ) \
    if (!raw && nq_tile == NQv && E == Ev && perq == PQ) return launch_g8<MK, Ev, NQv, PQ, false>(s, p, grid);
    OTT_G8(1, 1, false) OTT_G8(2, 1, false) OTT_G8(4, 1, false) OTT_G8(8, 1, false)
    OTT_G8(1, 2, false) OTT_G8(2, 2, false) OTT_G8(4, 2, false) OTT_G8(8, 2, false)
    OTT_G8(2, 1, true) OTT_G8(4, 1, true) OTT_G8(8, 1, true)
    OTT_G8(2, 2, true) OTT_G8(4, 2, true) OTT_G8(8, 2, true)
#undef OTT_G8
#define OTT_G8R(NQv) \
    if (raw && nq_tile == NQv) return launch_g8<MK, 1, NQv, false, true>(s, p, grid);
    OTT_G8R(1) OTT_G8R(2) OTT_G8R(4) OTT_G8R(8)
#undef OTT_G8R
    return fail(OTT_ERR_INVALID, "launch_gather: no kernel for this (nq_tile, E, mode)");
}

int launch_gather(ott_store* s, const GatherParams& p, uint32_t nq_tile, int E, bool perq, bool raw, uint32_t grid) {
    switch (metric_kind(p.metric)) {
        case MK_L2: return launch_gather_mk<MK_L2>(s, p, nq_tile, E, perq, raw, grid);
        case MK_L1: return launch_gather_mk<MK_L1>(s, p, nq_tile, E, perq, raw, grid);
        default: return launch_gather_mk<MK_DOT>(s, p, nq_tile, E, perq, raw, grid);
    }
}

// one block up, one copy: [queries (zero padded to 8 x dimq) | qinv | ids | pos (raw scores)]
int upload_gather_inputs(ott_store* s, const float* queries, uint32_t nq, const uint64_t* ids, const uint64_t* pos, uint64_t n_ids, GatherParams& p) {
    const uint32_t nq_pad = (nq + 7u) & ~7u;
    const size_t q_bytes = (size_t)nq_pad * s->dimq * 4, qi_bytes = (size_t)nq_pad * 4, id_bytes = (size_t)n_ids * 8;
    const size_t off_qi = q_bytes, off_ids = (off_qi + qi_bytes + 15) & ~(size_t)15, off_pos = off_ids + id_bytes;
    const size_t total = off_pos + (pos ? id_bytes : 0);
    int rc = s->h_stage.ensure(total);
    if (rc) return rc;
    char* hs = (char*)s->h_stage.p;
    memset(hs, 0, off_ids);
    for (uint32_t i = 0; i < nq; i++) {
        memcpy((float*)hs + (size_t)i * s->dimq, queries + (size_t)i * s->dim, (size_t)s->dim * 4);
        ((float*)(hs + off_qi))[i] = host_inv_norm_exact(queries + (size_t)i * s->dim, s->dim);
    }
    memcpy(hs + off_ids, ids, id_bytes);
    if (pos) memcpy(hs + off_pos, pos, id_bytes);
    if ((rc = s->d_queries.ensure(total))) return rc;
    OTT_HIP(hipMemcpyAsync(s->d_queries.p, hs, total, hipMemcpyHostToDevice, s->stream));
    const char* dq = (const char*)s->d_queries.p;
    p.queries = (const float*)dq;
    p.qinv = (const float*)(dq + off_qi);
    p.ids = (const uint64_t*)(dq + off_ids);
    p.pos = pos ? (const uint64_t*)(dq + off_pos) : nullptr;
    return OTT_OK;
}

void fill_gather_params(const ott_store* s, uint32_t nq, uint32_t metric, uint64_t n_ids, GatherParams& p) {
    memset(&p, 0, sizeof(p));
    p.rows = s->d_rows;
    p.inv = s->d_inv;
    p.n_ids = n_ids;
    p.ld = s->ld;
    p.dim = s->dim;
    p.dimq = s->dimq;
    p.nq_total = nq;
    p.metric = metric;
    p.reduce = s->reduce;
}

// The ranked query on the gather kernel.  ids: ascending, duplicate-free, every id < s->n, ids of chunks the chunk mask clears
// already dropped, at most 64 x G8_MAX_TILES of them; k_eff <= 128.  The context's `mu` is the caller's.
int run_gather(ott_store* s, const ott_query_desc* d, const std::vector<uint64_t>& ids, uint64_t k_eff, ott_hit* out, uint64_t* n_out,
               uint64_t* n_per_query, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    memset(&st, 0, sizeof(st));
    const uint32_t nq = d->nq;
    const bool perq = d->mode == OTT_MODE_PER_QUERY;
    const uint64_t n_u = ids.size(), cs = s->chunk_size;
    st.path_used = OTT_PATH_EXACT;
    st.total_chunks = s->n ? (s->n + cs - 1) / cs : 0;
    for (uint64_t i = 0; i < n_u; i++) st.evaluated_chunks += (i == 0 || ids[i] / cs != ids[i - 1] / cs) ? 1 : 0;
    st.pruned_chunks = st.total_chunks - st.evaluated_chunks;
    if (n_u == 0 || k_eff == 0) {
        st.total_ns = now_ns() - t0;
        if (stats_out) *stats_out = st;
        return OTT_OK;
    }
    const uint64_t* d_mask = nullptr;
    uint64_t mask_bits = 0;
    if ((rc = compose_row_mask(s, d, &d_mask, &mask_bits))) return rc;

    const int E = k_eff <= 64 ? 1 : 2;
    const uint32_t KS = 64 * E;
    const uint32_t n_tiles = (uint32_t)((n_u + 63) / 64);
    const uint32_t tile = pow2ceil(nq) < 8u ? pow2ceil(nq) : 8u;
    const uint32_t passes = (nq + tile - 1) / tile;
    GatherParams p;
    fill_gather_params(s, nq, d->metric, n_u, p);
    if ((rc = upload_gather_inputs(s, d->queries, nq, ids.data(), nullptr, n_u, p))) return rc;
    p.row_mask = d_mask;
    p.row_mask_bits = mask_bits;
    p.take_max = d->take == OTT_TAKE_MAX;
    p.cmp = d->filter_cmp;
    p.thr = d->filter_thr;
    p.k = (uint32_t)k_eff;
    p.list_stride = KS;
    const size_t n_lists_total = perq ? (size_t)nq * n_tiles : (size_t)passes * n_tiles;
    if ((rc = s->d_lists.ensure(n_lists_total * KS * sizeof(Cand)))) return rc;
    const uint32_t groups = perq ? nq : 1;
    // results block in pinned host memory, as run_exact lays it out: [counts (groups x u64, padded to 64 B) | hits (groups x KS) | scored]
    const size_t cnt_pad = (((size_t)groups * sizeof(uint64_t)) + 63) & ~(size_t)63;
    const size_t res_bytes = cnt_pad + (size_t)groups * KS * sizeof(ott_hit);
    if ((rc = s->h_hits.ensure(res_bytes + 8))) return rc;
    void* mapped = nullptr;
    OTT_HIP(hipHostGetDevicePointer(&mapped, s->h_hits.p, 0));
    uint64_t* d_counts = (uint64_t*)mapped;
    ott_hit* d_hits = (ott_hit*)((char*)mapped + cnt_pad);
    if (d_mask) {  // rows the mask drops are not counted as compared
        if ((rc = s->d_gather.ensure(64))) return rc;
        OTT_HIP(hipMemsetAsync(s->d_gather.p, 0, 8, s->stream));
        p.scored = (unsigned long long*)s->d_gather.p;
    }
    const bool timing = stats_out != nullptr;
    if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
    for (uint32_t ps = 0; ps < passes; ps++) {
        p.q0 = ps * tile;
        // merged: one list group per pass.  per query: list (query, tile) lives at (query * n_tiles + tile) * KS; a one-query
        // pass runs the single-list kernel, so it is pointed at its query's slot (q0 == ps there)
        p.lists = (Cand*)s->d_lists.p + ((perq && tile > 1) ? 0 : (size_t)ps * n_tiles * KS);
        if ((rc = launch_gather(s, p, tile, E, perq, false, n_tiles))) return rc;
    }
    if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
    if (perq)
        rc = launch_merge(s, (const Cand*)s->d_lists.p, n_tiles, KS, (uint64_t)n_tiles * KS, nq, (uint32_t)k_eff, E, p.take_max != 0, s->base_offset, d_hits, KS,
                          d_counts, 0);
    else
        rc = launch_merge(s, (const Cand*)s->d_lists.p, passes * n_tiles, KS, 0, 1, (uint32_t)k_eff, E, p.take_max != 0, s->base_offset, d_hits, KS, d_counts, 0);
    if (rc) return rc;
    if (timing) OTT_HIP(hipEventRecord(s->ev[5], s->stream));
    char* hh = (char*)s->h_hits.p;
    if (d_mask) OTT_HIP(hipMemcpyAsync(hh + res_bytes, s->d_gather.p, 8, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    uint64_t scored = n_u;
    if (d_mask) memcpy(&scored, hh + res_bytes, 8);
    st.passes = passes;
    st.vectors_compared = scored * nq;  // listed rows after unique, chunk filter and mask, per query (sum chunk.len * nq elsewhere)
    st.bytes_scanned = (uint64_t)passes * scored * ((uint64_t)s->dim * 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));
    const uint64_t* counts = (const uint64_t*)hh;
    const ott_hit* hits = (const ott_hit*)(hh + cnt_pad);
    uint64_t total = 0;
    for (uint32_t g = 0; g < groups; g++) {
        const uint64_t cg = counts[g];
        if (cg) memcpy(out + total, hits + (size_t)g * KS, (size_t)cg * sizeof(ott_hit));
        if (n_per_query && perq) n_per_query[g] = cg;
        total += cg;
    }
    if (n_out) *n_out = total;
    if (timing) read_exact_events(s, &st);
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

// The fallback: the list as a device row mask in the context's scratch, then today's query with it (query_on -> compose_row_mask).
int run_ids_as_mask(ott_store* s, const ott_query_desc* d, const std::vector<uint64_t>& ids, ott_hit* out, uint64_t cap, uint64_t* n_out,
                    uint64_t* n_per_query, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t words = (s->n + 63) / 64;
    // [id mask | id mask & caller mask (compose_row_mask) | the ids]
    if ((rc = s->d_idmask.ensure((size_t)words * 16 + ids.size() * 8))) return rc;
    uint64_t* d_words = (uint64_t*)s->d_idmask.p;
    uint64_t* d_ids = d_words + 2 * words;
    OTT_HIP(hipMemsetAsync(d_words, 0, (size_t)words * 8, s->stream));
    if (!ids.empty()) {
        if ((rc = s->h_stage.ensure(ids.size() * 8))) return rc;
        memcpy(s->h_stage.p, ids.data(), ids.size() * 8);
        OTT_HIP(hipMemcpyAsync(d_ids, s->h_stage.p, ids.size() * 8, hipMemcpyHostToDevice, s->stream));
        uint64_t blocks = (ids.size() + 255) / 256;
        if (blocks > (uint64_t)s->n_cu * 8) blocks = (uint64_t)s->n_cu * 8;
        hipLaunchKernelGGL(set_bits_kernel, dim3((uint32_t)blocks), dim3(256), 0, s->stream, d_words, (const uint64_t*)d_ids, (uint64_t)ids.size());
        OTT_HIP(hipGetLastError());
        OTT_HIP(hipStreamSynchronize(s->stream));  // (h_stage is the query's own staging next)
    }
    IdMaskGuard guard{s};
    s->cur_idmask = d_words;
    return query_on(s, d, out, nullptr, cap, n_out, n_per_query, nullptr, stats_out);
}

// scores of rows `ids` (any order, duplicates allowed) for every query on a context the caller holds: out[q * n_ids + i]
int score_rows_on(ott_store* s, const float* queries, uint32_t nq, uint32_t metric, const uint64_t* ids, uint64_t n_ids, float* out_scores) {
    int rc;
    OTT_HIP(use_device(s));
    // slots in ascending row order (neighbouring slots share lines and pages), pos: slot -> the caller's position
    std::vector<uint64_t> pos(n_ids), sorted(n_ids);
    std::iota(pos.begin(), pos.end(), (uint64_t)0);
    std::stable_sort(pos.begin(), pos.end(), [ids](uint64_t a, uint64_t b) { return ids[a] < ids[b]; });
    for (uint64_t i = 0; i < n_ids; i++) sorted[i] = ids[pos[i]];
    GatherParams p;
    fill_gather_params(s, nq, metric, n_ids, p);
    if ((rc = upload_gather_inputs(s, queries, nq, sorted.data(), pos.data(), n_ids, p))) return rc;
    const size_t out_bytes = (size_t)nq * n_ids * 4;
    if ((rc = s->d_gather.ensure(64 + out_bytes))) return rc;
    p.raw_out = (float*)((char*)s->d_gather.p + 64);
    p.raw_stride = n_ids;
    const uint32_t tile = pow2ceil(nq) < 8u ? pow2ceil(nq) : 8u;
    const uint64_t per_launch = 64ull * G8_MAX_TILES;
    for (uint32_t q0 = 0; q0 < nq; q0 += tile)
        for (uint64_t s0 = 0; s0 < n_ids; s0 += per_launch) {  // no size limit: launches of at most G8_MAX_TILES tiles
            p.q0 = q0;
            p.slot0 = s0;
            const uint64_t left = n_ids - s0 < per_launch ? n_ids - s0 : per_launch;
            if ((rc = launch_gather(s, p, tile, 1, false, true, (uint32_t)((left + 63) / 64)))) return rc;
        }
    OTT_HIP(hipMemcpyAsync(out_scores, p.raw_out, out_bytes, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    return OTT_OK;
}

}  // namespace

int check_ids(const char* who, const uint64_t* ids, uint64_t n_ids, uint64_t len) {
    if (n_ids && !ids) return fail(OTT_ERR_INVALID, std::string(who) + ": ids is NULL");
    for (uint64_t i = 0; i < n_ids; i++)
        if (ids[i] >= len)
            return fail(OTT_ERR_INVALID, std::string(who) + ": row " + std::to_string(ids[i]) + " is out of range (the store holds " + std::to_string(len) + " rows)");
    return OTT_OK;
}

// The ranked query over a list on a context whose `mu` the caller holds (and the owner's `rw`, shared): the gather kernel or the mask
// route.  u: ascending, duplicate-free, every id < the store's length; d->k = min(k, pool) >= 1; n_listed: the ids as the caller listed them.
int query_ids_on(ott_store* ctx, const ott_query_desc* d, std::vector<uint64_t>& u, uint64_t n_listed, ott_hit* out, uint64_t cap, uint64_t* n_out,
                 uint64_t* n_per_query, ott_stats* stats) {
    // The gather kernel serves the canonical order, the lists rows8 builds (k <= 128), up to 1024 tiles of 64 ids, up to 16 queries
    // (two passes of eight, as rows8) of up to 2048 floats, on path AUTO or EXACT; everything else takes the mask.
    // AUTO (id_gather = -1): the gather for lists of up to 10000 ids, the mask above.  Measured on 10M x 768, cosine top-10, one
    // query, random ids, against a caller-built row mask over the store (profiles/idlist/README.md): 100 ids 0.048 against 0.465 ms,
    // 1000 ids 0.054 / 0.485, 10000 ids 0.388 / 0.561 — and 65536 ids 2.84 / 0.95: the kernels take 50 us there, the host's sort
    // of the list 2.7 ms.  The crossover lies near 12500 ids; 10000 is the largest size at which the gather measured faster.
    const uint64_t k_eff = d->k;
    const bool eligible = ctx->opt.tie_order == 0 && ctx->opt.id_gather != 0 && (ctx->opt.id_gather == 1 || n_listed <= G8_AUTO_MAX_IDS) &&
                          d->path != OTT_PATH_MFMA && k_eff <= 128 && u.size() <= 64ull * G8_MAX_TILES && ctx->dimq <= G8_QMAX && d->nq <= 16;
    if (!eligible) return run_ids_as_mask(ctx, d, u, out, cap, n_out, n_per_query, stats);
    if (d->chunk_mask) {  // a host pointer: ids of cleared chunks go here
        const uint64_t cs = ctx->chunk_size;
        u.erase(std::remove_if(u.begin(), u.end(), [&](uint64_t r) { const uint64_t c = r / cs; return !((d->chunk_mask[c >> 6] >> (c & 63)) & 1); }), u.end());
    }
    return run_gather(ctx, d, u, k_eff, out, n_out, n_per_query, stats);
}

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_ids(ott_store* s, const ott_query_desc* d, const uint64_t* ids, uint64_t n_ids, ott_hit* out, uint64_t cap, uint64_t* n_out,
                  uint64_t* n_per_query, ott_stats* stats) {
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_ids: out is NULL");
    if ((rc = check_ids("ott_query_ids", ids, n_ids, ott_store_len(s)))) return rc;  // before any device work (staged rows count)
    if (n_out) *n_out = 0;
    if (n_per_query)
        for (uint32_t i = 0; i < d->nq; i++) n_per_query[i] = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    // ascending and duplicate-free: order and duplicates in the list do not matter, and ascending rows keep the candidate key order
    std::vector<uint64_t> u(ids, ids + n_ids);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    const bool perq = d->mode == OTT_MODE_PER_QUERY;
    const uint64_t pool = perq ? (uint64_t)u.size() : (uint64_t)u.size() * d->nq;
    const uint64_t k_eff = d->k < pool ? d->k : pool;
    if (cap < (perq ? k_eff * d->nq : k_eff)) return fail(OTT_ERR_INVALID, "ott_query_ids: output capacity is smaller than min(k, ids*nq)");
    if (k_eff == 0) return OTT_OK;  // an empty list, or k == 0: a valid query with no hits
    ott_query_desc d2 = *d;
    d2.k = k_eff;  // at most `pool` pairs can pass: the same hits, and the paths below size their buffers by the list
    if (s->multi) return multi_query_ids(s, &d2, u, out, cap, n_out, n_per_query, stats);
    ott::host::SharedLock rd;  // the corpus cannot change while this query runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    CtxLease ctx(s);
    return query_ids_on(ctx.c, &d2, u, n_ids, out, cap, n_out, n_per_query, stats);
}

int ott_store_score_rows(ott_store* s, const float* queries, uint32_t nq, uint32_t metric, const uint64_t* ids, uint64_t n_ids, float* out_scores) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_score_rows: store is NULL");
    if (nq == 0) return fail(OTT_ERR_INVALID, "No queries provided");
    if (!queries) return fail(OTT_ERR_INVALID, "ott_store_score_rows: queries is NULL");
    if (metric > OTT_METRIC_MANHATTAN) return fail(OTT_ERR_INVALID, "ott_store_score_rows: unknown metric");
    int rc = check_ids("ott_store_score_rows", ids, n_ids, ott_store_len(s));
    if (rc) return rc;
    if (n_ids == 0) return OTT_OK;
    if (!out_scores) return fail(OTT_ERR_INVALID, "ott_store_score_rows: out_scores is NULL");
    if (s->multi) return multi_score_rows(s, queries, nq, metric, ids, n_ids, out_scores);
    if (s->dimq > G8_QMAX) return fail(OTT_ERR_UNSUPPORTED, "ott_store_score_rows: rows of more than 2048 floats are not served");
    ott::host::SharedLock rd;
    if ((rc = lock_store_shared(s, rd))) return rc;
    CtxLease ctx(s);
    return score_rows_on(ctx.c, queries, nq, metric, ids, n_ids, out_scores);
}

}  // extern "C"
