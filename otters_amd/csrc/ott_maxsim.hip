// ott_maxsim.hip — late-interaction (MaxSim) search over grouped rows: the nq query vectors are the TOKENS of one
// query, a group's score is the sum over the tokens of the best score among the group's surviving rows, the top-k is over groups.
//
//   maxsim_sweep_kernel   group_sweep_kernel's streaming geometry and K loop (lane = row, 64-row tiles per wave, 128-B stages through
//                         the swizzled LDS tile, tokens through the constant address space, a persistent grid over the run lists of
//                         surviving chunks, the scoring terms of ott_exact_dev.h: the bits are the oracle's).  Epilogue per (row,
//                         token of the pass): composed row mask, NaN drop, o = ord_of(score, take) — 32 bits, never 0 for a non-NaN —
//                         and table[token][gid[row]] = max(itself, o): a relaxed agent-scope load, then atomicMax on the 32-bit slot
//                         only when o is larger.  0 = empty slot.  No score filter here: the filter is on the SUM.
//                         FOLD (diagnostic build only until it is measured, option maxsim_fold): rows of a document are normally
//                         appended together, so most lanes of a wave share their neighbour's group and the first tiles of a
//                         group would issue up to 64 same-address atomics per token.  Before the
//                         atomic every token's ordinal is folded over runs of adjacent lanes with equal gid (a segmented max in six
//                         ds_bpermute steps, the gid shuffles shared by the tokens) and only the head lane of a run touches memory.
//                         Max is order-free and only lanes of one group are ever joined, so the table cannot differ.  A wave
//                         without two equal neighbours (a shuffled layout) skips the fold after one shuffle and a ballot.
//   maxsim_reduce_kernel  one lane per group: the group's nq slots in token order, sum = best[0]; sum = sum + best[t] (f32, round to
//                         nearest, this order); dropped on an empty slot (a token without a score: the group has no surviving row,
//                         or every one of them scored NaN for it), a NaN sum (+inf + -inf) or a failed filter; else
//                         key = ord_of(sum) << 32 | ~gid into the [n_groups] table of 8-byte keys (0 = dropped).  Zeroes the slots it
//                         read: the next query's sweep needs no memset.
//
// The key table has exactly the shape grouped search takes its top-k from, so the rest is ott_group.hip's: group_select_kernel +
// launch_merge (base offset 0: a hit's index is the group) for k_eff <= 512, group_compact_kernel + sort_group_pairs above.
//
// Tokens per pass: 4 (one for a single token), group_sweep_kernel's measured sweet spot — 36 + 32 live floats per lane; the
// epilogue adds an ordinal per token and the fold's two shuffle temporaries (profiles/maxsim/resource_usage.txt: 159 VGPRs, 161
// with the fold, no scratch).
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ott_internal.h"
#include "ott_exact_dev.h"

namespace ott {

constexpr int MS_KC = 32;                    // floats per row per stage: one 128-B line
constexpr int MS_WAVES = 4;
constexpr int MS_STAGE_FLOATS = 64 * MS_KC;  // per wave: 8 KB
constexpr int MS_SMEM = MS_WAVES * MS_STAGE_FLOATS * 4;
constexpr int MS_BLOCKS_PER_CU = 2;          // the persistent grid of exact_kernel
constexpr uint32_t MS_NQ = 4;                // tokens per pass
constexpr bool MS_FOLD = false;              // the product's epilogue: the plain one until the A/B of profiles/maxsim/README.md is measured
constexpr uint64_t MS_TABLE_MAX = 1ull << 31;  // bytes of the (token, group) table: all tokens are held at once

struct MaxsimParams {
    const float* rows;
    const float* inv;
    const float* queries;  // [nq_pad * dimq], zero padded
    const float* qinv;     // [nq_pad]
    const uint64_t* row_mask;
    uint64_t row_mask_bits;
    const ott_run* runs;
    const uint32_t* tile_prefix;  // [n_runs + 1]
    const uint32_t* gid;          // [n] dense group ids, every one < n_groups (checked on the host when they were set)
    uint32_t* table;              // [nq_total][n_groups] best ordinal per (token, group); 0 = empty
    uint32_t n_groups;
    uint32_t ld, dim, dimq;
    uint32_t n_runs, n_tiles;
    uint32_t q0, nq_total;
    uint32_t metric, take_max, reduce;
};

template <int MK, int NQ, bool FOLD>
__global__ __launch_bounds__(64 * MS_WAVES) void maxsim_sweep_kernel(MaxsimParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* st = smem + wave * MS_STAGE_FLOATS;
    const bool take_max = p.take_max != 0;
    const uint32_t nq_here = (p.nq_total - p.q0) < (uint32_t)NQ ? (p.nq_total - p.q0) : (uint32_t)NQ;
    // wave-uniform, read-only inputs through the CONSTANT address space: always scalar loads (see exact_kernel)
    typedef __attribute__((address_space(4))) const float* CF32;
    typedef __attribute__((address_space(4))) const uint32_t* CU32;
    typedef __attribute__((address_space(4))) const ott_run* CRUN;
    const CF32 Q = (CF32)(p.queries + (size_t)p.q0 * p.dimq);
    const CU32 tile_prefix = (CU32)p.tile_prefix;
    const CRUN runs = (CRUN)p.runs;
    float qinv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) qinv[q] = (uint32_t)q < nq_here ? p.qinv[p.q0 + q] : 0.0f;

    const uint32_t gw = blockIdx.x * MS_WAVES + wave, nw = gridDim.x * MS_WAVES;
    const int sw = (lane >> 1) & 7;
    const uint32_t nstages = (p.ld + MS_KC - 1) / MS_KC;
    const int lrow = lane >> 3;  // row within an 8-row load group
    const int lslot = lane & 7;  // 16-B slot within the 128-B line
    // its float offset, kept inside a short row (dim < 29): the staging loads are unconditional, so a slot past the row's end must
    // not make the LAST row of the store read past the allocation
    const uint32_t lsl4 = ((uint32_t)lslot * 4 < p.ld) ? (uint32_t)lslot * 4 : 0u;

    for (uint32_t t = gw; t < p.n_tiles; t += nw) {
        // tile -> run of surviving chunks (wave-uniform scalar search)
        uint32_t lo = 0, hi = p.n_runs;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tile_prefix[mid] <= t) lo = mid;
            else hi = mid;
        }
        const uint64_t run_start = runs[lo].start, run_count = runs[lo].count;
        const uint64_t off = (uint64_t)(t - tile_prefix[lo]) * 64;
        const uint64_t row0 = run_start + off;
        const uint32_t cnt = (run_count - off) < 64 ? (uint32_t)(run_count - off) : 64u;
        const uint64_t my_row = row0 + lane;
        bool valid = (uint32_t)lane < cnt;
        if (p.row_mask != nullptr && valid && my_row < p.row_mask_bits)
            valid = (p.row_mask[my_row >> 6] >> (my_row & 63)) & 1;  // src/vec.rs:231-237
        if (__ballot(valid) == 0) continue;  // whole tile masked: its rows are never read

        // the row's group and inverse norm are fetched now and used after the K loop: their latency hides behind the stages
        float vinv = 0.0f;
        uint32_t g = 0xFFFFFFFFu;  // no group's id (ids stay below n_groups <= 2^32 - 1): a lane without a row joins no run
        if (valid) {
            g = p.gid[my_row];
            if (p.metric == OTT_METRIC_COSINE) vinv = p.inv[my_row];
        }
        float acc[NQ][8];
        float tail[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            tail[q] = 0.0f;
#pragma unroll
            for (int l = 0; l < 8; l++) acc[q][l] = 0.0f;
        }
        // Branch-free staging: every load is always issued (rows past a short tile's end are clamped to its last row, a column
        // group past `ld` in the last stage re-reads stage 0) and the out-of-range values are zeroed when they go to LDS
        v4f R[8];
        const float* rp[8];
        bool rok[8];
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint32_t row = 8 * m + lrow;
            rok[m] = row < cnt;
            rp[m] = p.rows + (row0 + (rok[m] ? row : cnt - 1)) * (uint64_t)p.ld + lsl4;
        }
        auto load_stage = [&](uint32_t s) {
            const uint32_t soff = (s * MS_KC + lslot * 4 < p.ld) ? s * MS_KC : 0u;
#pragma unroll
            for (int m = 0; m < 8; m++) R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rp[m] + soff));  // streamed once per pass
        };
        load_stage(0);
        for (uint32_t s = 0; s < nstages; s++) {
            const bool cok = s * MS_KC + lslot * 4 < p.ld;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int row = 8 * m + lrow;
                const bool ok = rok[m] & cok;
                const v4f v = R[m];
                *reinterpret_cast<float4*>(st + row * MS_KC + ((lslot ^ ((row >> 1) & 7)) << 2)) =
                    make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
            }
            wave_sync();
            if (s + 1 < nstages) load_stage(s + 1);
#pragma unroll
            for (int j = 0; j < MS_KC / 8; j++) {
                const uint32_t col = s * MS_KC + 8 * j;
                if (col < p.dim) {
                    const float4 a = *reinterpret_cast<const float4*>(st + lane * MS_KC + (((2 * j) ^ sw) << 2));
                    const float4 b = *reinterpret_cast<const float4*>(st + lane * MS_KC + (((2 * j + 1) ^ sw) << 2));
                    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    if (col + 8 <= p.dim) {
                        // one chunks_exact(8) step: acc = acc + term(q, v)   (vec_compute.rs:12-13, 39-42); every slot of the
                        // pass is computed (the token block is zero padded): no per-token branch
#pragma unroll
                        for (int q = 0; q < NQ; q++) {
                            const CF32 qp = Q + (size_t)q * p.dimq + col;
#pragma unroll
                            for (int l = 0; l < 8; l++) acc[q][l] = __fadd_rn(acc[q][l], exact_term<MK>(qp[l], x[l]));
                        }
                    } else {
                        // remainder: sequential sum of the last dim % 8 terms (vec_compute.rs:15-21, 44-53)
                        const uint32_t nt = p.dim - col;
#pragma unroll
                        for (int q = 0; q < NQ; q++) {
                            const CF32 qp = Q + (size_t)q * p.dimq + col;
#pragma unroll
                            for (int l = 0; l < 7; l++)
                                if ((uint32_t)l < nt) tail[q] = __fadd_rn(tail[q], exact_term<MK>(qp[l], x[l]));
                        }
                    }
                }
            }
            wave_sync();
        }

        // score -> ordinal (0 = nothing to offer: no row, a token past the query's last, a NaN score)
        uint32_t o[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            float s = __fadd_rn(reduce8(acc[q], p.reduce), tail[q]);
            if (p.metric == OTT_METRIC_COSINE) s = __fmul_rn(__fmul_rn(s, qinv[q]), vinv);  // vec_compute.rs:31
            o[q] = (valid && (uint32_t)q < nq_here && !(s != s)) ? ord_of(s, take_max) : 0u;  // NaN dropped: vec_compute.rs:237
        }
        bool head = true;
        if constexpr (FOLD) {
            // runs of adjacent lanes with one gid: after the step of distance d a lane holds the max over the lanes of its run among
            // [lane, lane + 2d) (a lane d further on with the same gid outside the run may join too: it is the same slot's)
            const uint32_t gprev = __shfl_up(g, 1);
            head = lane == 0 || gprev != g;
            if (__ballot(!head) != 0) {
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t og = __shfl_down(g, d);
                    const bool join = lane + d < 64 && og == g;
#pragma unroll
                    for (int q = 0; q < NQ; q++) {
                        const uint32_t oo = __shfl_down(o[q], d);
                        if (join && oo > o[q]) o[q] = oo;
                    }
                }
            }
        }
        if (head && valid) {
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                if (o[q] != 0) {
                    uint32_t* slot = p.table + (size_t)(p.q0 + q) * p.n_groups + g;
                    // the load goes past this CU's vector L1 (agent scope), so it sees what other CUs' atomics left; a value that
                    // is stale all the same is a smaller one (slots only rise) and costs an atomic, never a result
                    if (o[q] > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, o[q]);
                }
            }
        }
    }
}

// One lane per group.  keys: [n_groups] 8-byte keys, zero when the kernel starts (d_gtable's protocol): only kept groups are written.
__global__ __launch_bounds__(256) void maxsim_reduce_kernel(uint32_t* table, uint32_t n_groups, uint32_t nq, uint32_t take_max, uint32_t cmp, float thr,
                                                            unsigned long long* keys) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const bool tmax = take_max != 0;
    bool complete = true;
    float acc = 0.0f;
    for (uint32_t t = 0; t < nq; t++) {
        uint32_t* slot = table + (size_t)t * n_groups + g;
        const uint32_t o = *slot;
        if (o == 0) {
            complete = false;
        } else {
            *slot = 0u;
            const float b = score_of(o, tmax);
            acc = t == 0 ? b : __fadd_rn(acc, b);  // starts from best[0], not from 0.0: a -0.0 stays -0.0
        }
    }
    if (complete && !(acc != acc) && cmp_holds(acc, cmp, thr)) keys[g] = ((unsigned long long)ord_of(acc, tmax) << 32) | (uint32_t)(~(uint32_t)g);
}

namespace {

uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <int MK, bool FOLD>
int launch_sweep_mk(ott_store* s, const MaxsimParams& p, uint32_t nq_tile, uint32_t grid) {
    if (nq_tile == 1) hipLaunchKernelGGL((maxsim_sweep_kernel<MK, 1, FOLD>), dim3(grid), dim3(64 * MS_WAVES), MS_SMEM, s->stream, p);
    else hipLaunchKernelGGL((maxsim_sweep_kernel<MK, (int)MS_NQ, FOLD>), dim3(grid), dim3(64 * MS_WAVES), MS_SMEM, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

template <bool FOLD>
int launch_sweep_fold(ott_store* s, const MaxsimParams& p, uint32_t nq_tile, uint32_t grid) {
    switch (metric_kind(p.metric)) {
        case MK_L2: return launch_sweep_mk<MK_L2, FOLD>(s, p, nq_tile, grid);
        case MK_L1: return launch_sweep_mk<MK_L1, FOLD>(s, p, nq_tile, grid);
        default: return launch_sweep_mk<MK_DOT, FOLD>(s, p, nq_tile, grid);
    }
}

int launch_sweep(ott_store* s, const MaxsimParams& p, uint32_t nq_tile, uint32_t grid) {
#ifdef OTT_MFMA_DEBUG_BUILD
    // the diagnostic build carries both epilogues (option maxsim_fold: the A/B of benchmarks/maxsim.py)
    if (s->opt.maxsim_fold >= 0 && (s->opt.maxsim_fold != 0) != MS_FOLD) return launch_sweep_fold<!MS_FOLD>(s, p, nq_tile, grid);
#endif
    return launch_sweep_fold<MS_FOLD>(s, p, nq_tile, grid);
}

// The query on a context whose `mu` the caller holds (and the owner's `rw`, shared).  k_eff = min(k, n_groups) >= 1.
int run_maxsim(ott_store* s, const ott_query_desc* d, uint64_t k_eff, ott_hit* out, uint64_t* n_out, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    memset(&st, 0, sizeof(st));
    const uint32_t nq = d->nq, ng = s->n_groups;
    RunPlan pl;
    make_run_plan(s, d->chunk_mask, pl);
    st.path_used = OTT_PATH_EXACT;
    st.total_chunks = pl.total_chunks;
    st.evaluated_chunks = pl.evaluated;
    st.pruned_chunks = pl.total_chunks - pl.evaluated;
    st.vectors_compared = pl.rows_scored * nq;
    if (pl.rows_scored == 0) {
        st.total_ns = now_ns() - t0;
        if (stats_out) *stats_out = st;
        return OTT_OK;
    }
    const uint64_t* d_mask = nullptr;
    uint64_t mask_bits = 0;
    if ((rc = compose_row_mask(s, d, &d_mask, &mask_bits))) return rc;
    const std::vector<uint32_t> prefix = tile_prefix(pl, 64);
    const uint32_t n_tiles = prefix.back();
    if ((rc = upload_exact_inputs(s, d->queries, nq, pl, prefix))) return rc;

    const uint32_t tile = nq == 1 ? 1u : MS_NQ;
    const uint32_t passes = (nq + tile - 1) / tile;
    // both tables are zero when a query finds them: zeroed when they are (re)allocated or a query failed half way, the ordinals
    // left zeroed by the reduce kernel, the keys by the select / compact kernel
    const size_t ord_bytes = (size_t)nq * ng * 4, key_bytes = (size_t)ng * 8;
    if (s->d_mstable.cap < ord_bytes || !s->mstable_clean) {
        if ((rc = s->d_mstable.ensure(ord_bytes))) return rc;
        OTT_HIP(hipMemsetAsync(s->d_mstable.p, 0, s->d_mstable.cap, s->stream));
    }
    s->mstable_clean = false;
    if (s->d_gtable.cap < key_bytes || !s->gtable_clean) {
        if ((rc = s->d_gtable.ensure(key_bytes))) return rc;
        OTT_HIP(hipMemsetAsync(s->d_gtable.p, 0, s->d_gtable.cap, s->stream));
    }
    s->gtable_clean = false;
    uint32_t* table = (uint32_t*)s->d_mstable.p;
    unsigned long long* keys = (unsigned long long*)s->d_gtable.p;

    MaxsimParams p;
    memset(&p, 0, sizeof(p));
    p.rows = s->d_rows;
    p.inv = s->d_inv;
    p.queries = (const float*)s->d_queries.p;
    p.qinv = (const float*)((const char*)s->d_queries.p + s->in_off_qinv);
    p.row_mask = d_mask;
    p.row_mask_bits = mask_bits;
    p.runs = (const ott_run*)((const char*)s->d_queries.p + s->in_off_runs);
    p.tile_prefix = (const uint32_t*)((const char*)s->d_queries.p + s->in_off_prefix);
    p.gid = s->d_gid;
    p.table = table;
    p.n_groups = ng;
    p.ld = s->ld;
    p.dim = s->dim;
    p.dimq = s->dimq;
    p.n_runs = (uint32_t)pl.runs.size();
    p.n_tiles = n_tiles;
    p.nq_total = nq;
    p.metric = d->metric;
    p.take_max = d->take == OTT_TAKE_MAX;
    p.reduce = s->reduce;
    // the persistent grid of the grouped sweep: a workgroup of four waves per four tiles, at most MS_BLOCKS_PER_CU per CU
    uint32_t grid = (n_tiles + MS_WAVES - 1) / MS_WAVES;
    const uint32_t grid_cap = (uint32_t)s->n_cu * MS_BLOCKS_PER_CU;
    if (grid > grid_cap) grid = grid_cap;
    if (grid < 1) grid = 1;

    const bool lists_path = k_eff <= 512;
    const int E = lists_path ? list_E(k_eff) : 1;
    const uint32_t KS = 64u * (uint32_t)E;
    const uint32_t n_lists = group_select_lists(ng);
    if (lists_path) {
        if ((rc = s->d_lists.ensure((size_t)n_lists * KS * sizeof(Cand)))) return rc;
    } else {
        if ((rc = ensure_group_pairs(s, ng))) return rc;
        if ((rc = s->d_gctl.ensure(64))) return rc;
        OTT_HIP(hipMemsetAsync(s->d_gctl.p, 0, 8, s->stream));
    }
    const bool timing = stats_out != nullptr;
    if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
    for (uint32_t ps = 0; ps < passes; ps++) {
        p.q0 = ps * tile;
        if ((rc = launch_sweep(s, p, tile, grid))) return rc;
    }
    hipLaunchKernelGGL(maxsim_reduce_kernel, dim3((ng + 255) / 256), dim3(256), 0, s->stream, table, ng, nq, p.take_max, (uint32_t)d->filter_cmp, d->filter_thr, keys);
    OTT_HIP(hipGetLastError());
    if (lists_path) {
        if ((rc = launch_group_select(s, keys, ng, 0, 1, (uint32_t)k_eff, E, (Cand*)s->d_lists.p, n_lists))) return rc;
    } else {
        if ((rc = launch_group_compact(s, keys, ng, 0, 1, (uint64_t*)s->l_keysA.p, (uint32_t*)s->l_qA.p, (unsigned long long*)s->d_gctl.p, ng))) return rc;
    }
    if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
    st.passes = passes;
    st.bytes_scanned = (uint64_t)passes * pl.rows_scored * ((uint64_t)s->dim * 4 + 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));  // (+ 4: the group id)

    uint64_t total = 0;
    if (lists_path) {
        // results block in pinned host memory, as run_groups lays it out: [count (u64, padded to 64 B) | hits (KS)]
        const size_t cnt_pad = 64;
        if ((rc = s->h_hits.ensure(cnt_pad + (size_t)KS * sizeof(ott_hit)))) return rc;
        void* mapped = nullptr;
        OTT_HIP(hipHostGetDevicePointer(&mapped, s->h_hits.p, 0));
        if ((rc = launch_merge(s, (const Cand*)s->d_lists.p, n_lists, KS, (uint64_t)n_lists * KS, 1, (uint32_t)k_eff, E, p.take_max != 0, 0 /* index = group */,
                               (ott_hit*)((char*)mapped + cnt_pad), KS, (uint64_t*)mapped, 0)))
            return rc;
        if (timing) OTT_HIP(hipEventRecord(s->ev[5], s->stream));
        OTT_HIP(hipStreamSynchronize(s->stream));
        s->mstable_clean = true;
        s->gtable_clean = true;
        const char* hh = (const char*)s->h_hits.p;
        total = *(const uint64_t*)hh;
        if (total > k_eff) total = k_eff;
        if (total) memcpy(out, hh + cnt_pad, (size_t)total * sizeof(ott_hit));
    } else {
        unsigned long long n_pairs = 0;
        OTT_HIP(hipMemcpyAsync(&n_pairs, s->d_gctl.p, 8, hipMemcpyDeviceToHost, s->stream));
        OTT_HIP(hipStreamSynchronize(s->stream));
        s->mstable_clean = true;
        s->gtable_clean = true;
        if (n_pairs > ng) n_pairs = ng;
        std::vector<std::vector<ott_hit>> lists;
        if ((rc = sort_group_pairs(s, n_pairs, 1, p.take_max != 0, k_eff, lists, ng))) return rc;
        if (timing) {
            OTT_HIP(hipEventRecord(s->ev[5], s->stream));
            OTT_HIP(hipStreamSynchronize(s->stream));
        }
        std::vector<ott_hit>& l = lists[0];
        for (ott_hit& h : l) h.index -= s->base_offset;  // the sort path's hits are rows of the store; these are groups
        if (!l.empty()) memcpy(out, l.data(), l.size() * sizeof(ott_hit));
        total = l.size();
    }
    if (n_out) *n_out = total;
    if (timing) read_exact_events(s, &st);
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_maxsim(ott_store* s, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, ott_stats* stats) {
    // what the descriptor alone decides comes first: these refusals need no store
    if (d && d->mode == OTT_MODE_PER_QUERY)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim: the query vectors are the tokens of ONE query; PER_QUERY (a batch of token sets) is not served");
    if (d && d->path == OTT_PATH_MFMA) return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim: the MFMA path does not serve late-interaction queries; use path AUTO or EXACT");
    if (!s) return fail(OTT_ERR_INVALID, "ott_query_maxsim: store is NULL");
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (s->multi)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim: a multi-GPU store is not served (a group may span shards: the maxima would have to be joined before the sum)");
    if (s->n_groups == 0) return fail(OTT_ERR_INVALID, "ott_query_maxsim: no group ids are set (ott_store_set_groups)");
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (s->gid_n != ott_store_len(s))  // staged rows count: they were appended
        return fail(OTT_ERR_INVALID, "ott_query_maxsim: the group ids cover " + std::to_string(s->gid_n) + " rows, the store holds " + std::to_string(ott_store_len(s)) +
                                         " (rows were appended since ott_store_set_groups: set them again)");
    const auto table_fits = [&](uint32_t n_groups) { return (uint64_t)d->nq * n_groups * 4 <= MS_TABLE_MAX; };
    const char* too_big = "ott_query_maxsim: tokens x groups x 4 bytes is above 2 GiB (the table holds every token's maxima at once); use fewer tokens or groups";
    if (!table_fits(s->n_groups)) return fail(OTT_ERR_UNSUPPORTED, too_big);
    ott::host::SharedLock rd;  // the corpus and the group ids cannot change while this query runs
    if ((rc = ott::host::lock_shared_clean(s->rw, rd, [s] { return s->pend.count() != 0; }, [s] { return store_flush(s); }))) return rc;
    // what the checks above read without the lock is read again, and k_eff only here: a set_groups may have come in between
    if (s->n_groups == 0) return fail(OTT_ERR_INVALID, "ott_query_maxsim: no group ids are set (ott_store_set_groups)");
    if (s->gid_n != s->n) return fail(OTT_ERR_INVALID, "ott_query_maxsim: the group ids no longer cover the store's rows (set them again)");
    if (!table_fits(s->n_groups)) return fail(OTT_ERR_UNSUPPORTED, too_big);
    const uint64_t k_eff = d->k < s->n_groups ? d->k : s->n_groups;
    if (cap < k_eff) return fail(OTT_ERR_INVALID, "ott_query_maxsim: output capacity is smaller than min(k, n_groups)");
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_maxsim: out is NULL");
    if (k_eff == 0) return OTT_OK;
    ott_store* ctx = ctx_acquire(s);
    rc = run_maxsim(ctx, d, k_eff, out, n_out, stats);
    ctx_release(ctx);
    return rc;
}

}  // extern "C"
