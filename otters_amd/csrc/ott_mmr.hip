// ott_mmr.hip — MMR diversity re-ranking: ott_query_mmr picks d->k of a query's best fetch_k hits greedily, each
// pick the most relevant and the least similar to what is already picked.
//
// The first stage is the library's own query (query_on, or query_ids_on with an id list) on the call's context, host output: its
// hits ARE the candidates, on every path and tie order.  Their rows and relevances go back up in one copy.
// mmr_pair_kernel fills P[s][c] = score(stored row of candidate s as the query, stored row of candidate c) across the GPU: the gather
// kernel's RAW geometry (eight lanes per row, rows8_scores of ott_exact_dev.h — the same additions in the same order, so the exact
// path's bits), except that the eight "queries" of a workgroup are eight candidates' rows read from the store BY ID into LDS.
// mmr_greedy_kernel runs the selection: one workgroup per query, one thread per candidate, every round in the one launch.
// Host decisions (refusals, scratch layout, grids): ott_mmr_plan.h.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "ott_internal.h"
#include "ott_exact_dev.h"

namespace ott {

constexpr int MMR_UNROLL = 12;  // rows8_scores' unroll, as the gather kernel's

struct MmrPairParams {
    const float* rows;
    const float* inv;
    const uint64_t* cand;  // [nq][fetch] local rows of the candidates; every one < the store's length (checked on the host)
    const uint32_t* n;     // [nq] candidates of each query
    float* pairs;          // [nq][fetch][fetch]
    uint32_t fetch, ld, dim, dimq;
    uint32_t sel_tiles, col_tiles;
    uint32_t metric, reduce;
};

// Dynamic LDS: [MMR_SEL x dimq] the selected rows, zero padded.  Block -> (query, selected-row tile, candidate tile): mmr_block.
template <int MK>
__global__ __launch_bounds__(MMR_PAIR_THREADS) void mmr_pair_kernel(MmrPairParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sQ = smem;  // [MMR_SEL][dimq]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane >> 3, c = lane & 7;
    const uint32_t per_q = p.sel_tiles * p.col_tiles;
    const uint32_t q = blockIdx.x / per_q, t = blockIdx.x % per_q;
    const uint32_t sel0 = (t / p.col_tiles) * MMR_SEL, col0 = (t % p.col_tiles) * MMR_COLS;
    const uint32_t n = p.n[q];
    if (sel0 >= n || col0 >= n) return;  // the grid is sized by the call's longest list (uniform: before any barrier)
    const uint64_t* cand = p.cand + (size_t)q * p.fetch;
    const uint32_t n_sel = (n - sel0) < MMR_SEL ? (n - sel0) : MMR_SEL;

    // the selected rows into LDS, by id (a row past the list's end repeats the last one: scored, never stored)
    float qinv[MMR_SEL];
#pragma unroll
    for (uint32_t j = 0; j < MMR_SEL; j++) {
        const uint64_t r = cand[sel0 + (j < n_sel ? j : n_sel - 1)];
        qinv[j] = p.metric == OTT_METRIC_COSINE ? p.inv[r] : 0.0f;
        const float* src = p.rows + r * (uint64_t)p.ld;
        for (uint32_t i = threadIdx.x; i < p.dimq; i += MMR_PAIR_THREADS) sQ[j * p.dimq + i] = i < p.dim ? src[i] : 0.0f;
    }
    const uint32_t col = col0 + 8u * (uint32_t)wave + (uint32_t)grp;  // this lane group's candidate
    const bool valid = col < n;
    const uint64_t my_row = cand[valid ? col : n - 1];  // clamped for the loads, invalid for the store
    const float* rp = p.rows + my_row * (uint64_t)p.ld;
    const float vinv = p.metric == OTT_METRIC_COSINE ? p.inv[my_row] : 0.0f;
    __syncthreads();  // the selected rows are in LDS

    float sc[MMR_SEL];
    rows8_scores<MK, (int)MMR_SEL, MMR_UNROLL>(sQ, p.dimq, rp, p.dim, lane, p.reduce, p.metric == OTT_METRIC_COSINE, qinv, vinv, sc);
    if (c == 0 && valid) {
        float* dst = p.pairs + ((size_t)q * p.fetch + sel0) * p.fetch + col;
#pragma unroll
        for (uint32_t j = 0; j < MMR_SEL; j++)
            if (j < n_sel) dst[(size_t)j * p.fetch] = sc[j];
    }
}

struct MmrGreedyParams {
    const float* pairs;  // [nq][fetch][fetch]
    const float* rel;    // [nq][fetch]
    const uint32_t* n;   // [nq]
    uint32_t* picks;     // [nq][k] positions in the candidate list, in pick order
    float* values;       // [nq][k]
    uint32_t fetch, k, take_max;
    float lam, om;
};

__device__ __forceinline__ float mmr_value_out(float v) { return v != v ? __uint_as_float(0x7FC00000u) : v; }  // a NaN value: one bit pattern

// One workgroup per query, thread c = candidate c (blockDim.x = whole waves, >= the query's candidates).  A round: row s of P
// (coalesced), the running redundancy, the value, the workgroup-wide best of (ordinal << 32) | ~position by wave reduction and one
// LDS exchange (two buffers in turn, so one barrier per round), every thread reads the winner.  Picks and values wait in LDS and are
// written once at the end.
__global__ __launch_bounds__(MMR_MAX_FETCH) void mmr_greedy_kernel(MmrGreedyParams p) {
    __shared__ unsigned long long sW[2][MMR_MAX_FETCH / 64];
    __shared__ uint32_t sPick[MMR_MAX_FETCH];
    __shared__ float sVal[MMR_MAX_FETCH];
    const uint32_t q = blockIdx.x, c = threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const uint32_t n = p.n[q];
    const uint32_t rounds = p.k < n ? p.k : n;
    if (rounds == 0) return;
    const bool tmax = p.take_max != 0;
    const float* P = p.pairs + (size_t)q * p.fetch * p.fetch;
    const bool mine = c < n;
    float lr = 0.0f, red = 0.0f;  // lam * g(rel_c); the running redundancy (set by round 1)
    if (mine) {
        const float r = p.rel[(size_t)q * p.fetch + c];
        lr = __fmul_rn(p.lam, tmax ? r : -r);
    }
    bool open = mine;  // not picked yet
    if (c == 0) {      // pick 0 is candidate 0
        sPick[0] = 0;
        sVal[0] = mmr_value_out(lr);
        open = false;
    }
    uint32_t s = 0;
    for (uint32_t r = 1; r < rounds; r++) {
        float value = 0.0f;
        unsigned long long key = 0ull;  // a picked candidate and a thread without one rank below every open candidate
        if (open) {
            const float pv = P[(size_t)s * p.fetch + c];
            const float x = tmax ? pv : -pv;
            if (r == 1) red = x;
            else if (x != x) {}
            else if (red != red) red = x;
            else red = x > red ? x : red;
            value = __fsub_rn(lr, __fmul_rn(p.om, red));
            const uint32_t o = value != value ? 0u : ord_of(value, true);  // a NaN value ranks below every other
            key = ((unsigned long long)o << 32) | (uint32_t)(~c);
        }
        unsigned long long best = key;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(best, off);
            best = other > best ? other : best;
        }
        if (lane == 0) sW[r & 1][wave] = best;
        __syncthreads();
        best = 0ull;
        for (uint32_t w = 0; w < n_waves; w++) {
            const unsigned long long other = sW[r & 1][w];
            best = other > best ? other : best;
        }
        s = ~(uint32_t)best;  // fewer picks than candidates so far: an open candidate exists, and its key is not 0
        if (s >= n) s = 0;    // (never taken; keeps the next round's read inside P whatever the keys held)
        if (open && c == s) {
            sPick[r] = c;
            sVal[r] = mmr_value_out(value);
            open = false;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < rounds; i += blockDim.x) {
        p.picks[(size_t)q * p.k + i] = sPick[i];
        p.values[(size_t)q * p.k + i] = sVal[i];
    }
}

namespace {

template <int MK>
int launch_pairs_mk(ott_store* s, const MmrPairParams& p, uint32_t grid) {
    const size_t smem = mmr_pair_lds_bytes(p.dimq);
    auto kern = mmr_pair_kernel<MK>;
    if (smem > 48 * 1024) {  // more dynamic LDS than the default limit: the opt-in, once per device
        static std::atomic<uint64_t> attr_set{0};
        if (attr_needed(attr_set, s->device)) {
            OTT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mmr_pair_lds_bytes(MMR_DIMQ_MAX)));
            attr_done(attr_set, s->device);
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(MMR_PAIR_THREADS), smem, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

int launch_pairs(ott_store* s, const MmrPairParams& p, uint32_t grid) {
    switch (metric_kind(p.metric)) {
        case MK_L2: return launch_pairs_mk<MK_L2>(s, p, grid);
        case MK_L1: return launch_pairs_mk<MK_L1>(s, p, grid);
        default: return launch_pairs_mk<MK_DOT>(s, p, grid);
    }
}

const char* refusal_text(MmrRefusal r) {
    switch (r) {
        case MMR_BAD_K: return "ott_query_mmr: k must be at least 1";
        case MMR_BAD_FETCH: return "ott_query_mmr: fetch_k must lie between k and OTT_MMR_MAX_FETCH (1024)";
        case MMR_BAD_LAMBDA: return "ott_query_mmr: lambda must lie in [0, 1]";
        case MMR_MERGED_BATCH: return "ott_query_mmr: OTT_MODE_MERGED takes one query; use OTT_MODE_PER_QUERY for one MMR per query";
        case MMR_MULTI_GPU: return "ott_query_mmr: not on a multi-GPU store (candidate rows lie on different shards)";
        case MMR_ROW_TOO_LONG: return "ott_query_mmr: rows of more than 2048 floats are not served";
        case MMR_PAIRS_TOO_BIG: return "ott_query_mmr: nq x fetch_k^2 pair scores take more than 256 MiB; lower fetch_k or split the batch";
        default: return "";
    }
}

// The second stage on a context the caller holds: `cand` holds the first stage's hits grouped by query, per[q] of them for query q
// (every per[q] <= fetch_k).  Writes the picks to out / out_values in pick order.
int run_mmr_select(ott_store* s, const ott_query_desc* d, uint64_t fetch_k, float lambda, const std::vector<ott_hit>& cand, const std::vector<uint64_t>& per,
                   ott_hit* out, uint64_t* n_out, uint64_t* n_per_query, float* out_values, bool timing, uint64_t* kernel_ns) {
    int rc;
    OTT_HIP(use_device(s));
    const uint32_t nq = d->nq;
    const uint64_t k = d->k;
    const MmrLayout L = mmr_layout(nq, fetch_k, k);
    if ((rc = s->h_stage.ensure(L.upload_bytes))) return rc;
    char* hs = (char*)s->h_stage.p;
    uint64_t* h_rows = (uint64_t*)(hs + L.off_rows);
    float* h_rel = (float*)(hs + L.off_rel);
    uint32_t* h_n = (uint32_t*)(hs + L.off_n);
    uint32_t n_max = 0;
    uint64_t at = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t nc = per[q];
        if (nc > fetch_k) return fail(OTT_ERR_HIP, "ott_query_mmr: the first stage returned more hits than fetch_k");
        h_n[q] = (uint32_t)nc;
        n_max = std::max(n_max, (uint32_t)nc);
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t r = cand[at + i].index - s->base_offset;
            if (r >= s->n) return fail(OTT_ERR_HIP, "ott_query_mmr: the first stage returned a row outside the store");  // (nothing is launched on it)
            h_rows[(size_t)q * fetch_k + i] = r;
            h_rel[(size_t)q * fetch_k + i] = cand[at + i].score;
        }
        at += nc;
    }
    if ((rc = s->d_mmr.ensure(L.total))) return rc;
    char* dm = (char*)s->d_mmr.p;
    OTT_HIP(hipMemcpyAsync(dm, hs, L.upload_bytes, hipMemcpyHostToDevice, s->stream));
    if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
    if (mmr_needs_pairs(k, n_max)) {
        const MmrGrid g = mmr_pair_grid(nq, n_max);
        MmrPairParams pp;
        memset(&pp, 0, sizeof(pp));
        pp.rows = s->d_rows;
        pp.inv = s->d_inv;
        pp.cand = (const uint64_t*)(dm + L.off_rows);
        pp.n = (const uint32_t*)(dm + L.off_n);
        pp.pairs = (float*)(dm + L.off_pairs);
        pp.fetch = (uint32_t)fetch_k;
        pp.ld = s->ld;
        pp.dim = s->dim;
        pp.dimq = s->dimq;
        pp.sel_tiles = g.sel_tiles;
        pp.col_tiles = g.col_tiles;
        pp.metric = d->metric;
        pp.reduce = s->reduce;
        if ((rc = launch_pairs(s, pp, (uint32_t)g.blocks))) return rc;
    }
    MmrGreedyParams gp;
    memset(&gp, 0, sizeof(gp));
    gp.pairs = (const float*)(dm + L.off_pairs);
    gp.rel = (const float*)(dm + L.off_rel);
    gp.n = (const uint32_t*)(dm + L.off_n);
    gp.picks = (uint32_t*)(dm + L.off_picks);
    gp.values = (float*)(dm + L.off_vals);
    gp.fetch = (uint32_t)fetch_k;
    gp.k = (uint32_t)k;
    gp.take_max = d->take == OTT_TAKE_MAX;
    gp.lam = lambda;
    gp.om = 1.0f - lambda;
    hipLaunchKernelGGL(mmr_greedy_kernel, dim3(nq), dim3(mmr_greedy_threads(n_max)), 0, s->stream, gp);
    OTT_HIP(hipGetLastError());
    if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
    if ((rc = s->h_hits.ensure(L.result_bytes))) return rc;
    OTT_HIP(hipMemcpyAsync(s->h_hits.p, dm + L.off_picks, L.result_bytes, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    if (timing) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s->ev[3], s->ev[4]) == hipSuccess) *kernel_ns = (uint64_t)(ms * 1e6);
    }
    const uint32_t* picks = (const uint32_t*)s->h_hits.p;
    const float* vals = (const float*)((const char*)s->h_hits.p + (L.off_vals - L.off_picks));
    uint64_t total = 0;
    at = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t rounds = mmr_rounds(k, h_n[q]);
        for (uint32_t i = 0; i < rounds; i++) {
            const uint32_t pos = picks[(size_t)q * k + i];
            if (pos >= h_n[q]) return fail(OTT_ERR_HIP, "ott_query_mmr: the selection returned a position outside the candidate list");
            out[total + i] = cand[at + pos];
            if (out_values) out_values[total + i] = vals[(size_t)q * k + i];
        }
        if (n_per_query && d->mode == OTT_MODE_PER_QUERY) n_per_query[q] = rounds;
        total += rounds;
        at += h_n[q];
    }
    if (n_out) *n_out = total;
    return OTT_OK;
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_mmr(ott_store* s, const ott_query_desc* d, const uint64_t* ids, uint64_t n_ids, uint64_t fetch_k, float lambda, ott_hit* out, uint64_t cap,
                  uint64_t* n_out, uint64_t* n_per_query, float* out_values, ott_stats* stats) {
    if (!d) return fail(OTT_ERR_INVALID, "ott_query_mmr: desc is NULL");
    MmrRefusal why = mmr_check_args(d->k, fetch_k, lambda);  // before the store is looked at
    if (why != MMR_OK) return fail(OTT_ERR_INVALID, refusal_text(why));
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_mmr: out is NULL");
    const uint64_t len = ott_store_len(s);
    if ((rc = check_ids("ott_query_mmr", ids, n_ids, len))) return rc;
    const bool perq = d->mode == OTT_MODE_PER_QUERY;
    if ((why = mmr_check_store(perq, d->nq, s->multi != nullptr, s->dimq, fetch_k)) != MMR_OK) return fail(OTT_ERR_UNSUPPORTED, refusal_text(why));
    // ascending and duplicate-free, as ott_query_ids takes a list
    std::vector<uint64_t> u;
    if (ids) {
        u.assign(ids, ids + n_ids);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
    }
    const uint64_t rows = ids ? (uint64_t)u.size() : len;
    if (cap < mmr_cap_needed(d->k, rows, perq, d->nq)) return fail(OTT_ERR_INVALID, "ott_query_mmr: output capacity is smaller than min(k, rows) per query");
    if (n_out) *n_out = 0;
    if (n_per_query)
        for (uint32_t i = 0; i < d->nq; i++) n_per_query[i] = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    const uint64_t t0 = now_ns();
    const uint64_t n_first = fetch_k < rows ? fetch_k : rows;  // the first stage's hits per query
    if (n_first == 0) return OTT_OK;                           // an empty store or an empty list: a valid query with no hits

    ott::host::SharedLock rd;  // the corpus cannot change between the two stages
    if ((rc = lock_store_shared(s, rd))) return rc;
    CtxLease ctx(s);  // one query context for both stages
    // first stage: the same descriptor with k = fetch_k, through the query's own internals (every path, the cascade, the tie orders)
    ott_query_desc d1 = *d;
    d1.k = n_first;
    std::vector<ott_hit> cand((size_t)n_first * d->nq);
    std::vector<uint64_t> per(d->nq, 0);
    uint64_t n_cand = 0;
    ott_stats st;
    memset(&st, 0, sizeof(st));
    ott_stats* st1 = stats ? &st : nullptr;  // (kernel timing costs event records: only when the caller asked for stats)
    if (ids) rc = query_ids_on(ctx.c, &d1, u, n_ids, cand.data(), cand.size(), &n_cand, per.data(), st1);
    else rc = query_on(ctx.c, &d1, cand.data(), nullptr, cand.size(), &n_cand, per.data(), nullptr, st1);
    if (rc) return rc;
    if (!perq) per[0] = n_cand;  // (one query: its hits are the list)
    uint64_t kernel_ns = 0;
    if (n_cand && (rc = run_mmr_select(ctx.c, d, fetch_k, lambda, cand, per, out, n_out, n_per_query, out_values, stats != nullptr, &kernel_ns))) return rc;
    st.merge_ns += kernel_ns;
    st.total_ns = now_ns() - t0;
    if (stats) *stats = st;
    return OTT_OK;
}

}  // extern "C"
