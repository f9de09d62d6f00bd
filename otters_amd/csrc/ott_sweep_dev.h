// ott_sweep_dev.h — the streaming tile loop of every sweep that is "the loop plus an epilogue": group_sweep_kernel (ott_group.hip),
// group_top_sweep_kernel (ott_group_top.hip) and maxsim_sweep_kernel (ott_maxsim.hip) over grouped rows; recommend_sweep_kernel,
// recommend_sum_sweep_kernel (ott_recommend.hip) and discover_sweep_kernel (ott_discover.hip), which read no group ids; and
// masks_sweep_kernel (ott_masks.hip), a row mask per query.  launch_sweep, below the loop, is the one launch of all of them.
// exact_kernel's streaming geometry with every variant stripped: lane = row, 64-row tiles per wave, 128-B stages through the swizzled LDS tile, queries through the constant address space, a persistent grid over the run lists
// of surviving chunks, the scoring terms of ott_exact_dev.h, so the bits are the oracle's.  A kernel is sweep_tiles plus its epilogue;
// what guards the loop against reading past the allocation (lsl4, the clamp to the tile's last row) exists here and nowhere else.
// exact_kernel and exact_rows8_kernel (ott_exact.hip) keep their own loop: it carries the prune checkpoints, the int8 and dump forms.
//
// Queries per pass: 4 (one for a single query).  A lane keeps 8 accumulators and a tail per query beside the 32 staging registers
// of the next stage: 4 queries are 36 + 32 live floats, which exact_kernel measured as the sweet spot of this geometry (an 8-wide
// pass needs 233 VGPRs and ran slower than two 4-wide ones).
#pragma once

#include <type_traits>

#include "ott_exact_dev.h"

namespace ott {

constexpr int SW_KC = 32;                    // floats per row per stage: one 128-B line
constexpr int SW_WAVES = 4;
constexpr int SW_STAGE_FLOATS = 64 * SW_KC;  // per wave: 8 KB
constexpr int SW_SMEM = SW_WAVES * SW_STAGE_FLOATS * 4;
constexpr int SW_BLOCKS_PER_CU = 2;          // the persistent grid of exact_kernel
constexpr uint32_t SW_NQ = 4;                // queries per pass of a batch

// what every sweep reads; filled by sweep_prologue (ott_group.hip)
struct SweepParams {
    const float* rows;
    const float* inv;
    const float* queries;  // [nq_pad * dimq], zero padded
    const float* qinv;     // [nq_pad]
    const uint64_t* row_mask;
    uint64_t row_mask_bits;
    const ott_run* runs;
    const uint32_t* tile_prefix;  // [n_runs + 1]
    const uint32_t* gid;          // [n] dense group ids, every one < n_groups (checked on the host when they were set); nullptr = none are read
    uint32_t ld, dim, dimq;
    uint32_t n_runs, n_tiles;
    uint32_t q0, nq_total;
    uint32_t metric, take_max, reduce;
};

// The body of a sweep kernel (a workgroup of SW_WAVES waves, SW_SMEM bytes of dynamic LDS).  For every tile of the wave that is not
// wholly masked: epi(my_row, valid, g, s, nq_here) — the lane's row, whether it has one that passed the composed row mask, its group
// (0xFFFFFFFF without a row: no group's id, ids stay below n_groups <= 2^32 - 1), the NQ scores of the pass (those from nq_here on
// are of the zero padding) and the number of queries the pass really has.
template <int MK, int NQ, class Epilogue>
__device__ __forceinline__ void sweep_tiles(const SweepParams& p, Epilogue&& epi) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* st = smem + wave * SW_STAGE_FLOATS;
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

    const uint32_t gw = blockIdx.x * SW_WAVES + wave, nw = gridDim.x * SW_WAVES;
    const int sw = (lane >> 1) & 7;
    const uint32_t nstages = (p.ld + SW_KC - 1) / SW_KC;
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
        uint32_t g = 0xFFFFFFFFu;
        if (valid) {
            if (p.gid != nullptr) g = p.gid[my_row];  // (wave-uniform: a sweep over a store without groups, ott_recommend.hip, has no ids)
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
            const uint32_t soff = (s * SW_KC + lslot * 4 < p.ld) ? s * SW_KC : 0u;
#pragma unroll
            for (int m = 0; m < 8; m++) R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rp[m] + soff));  // streamed once per pass
        };
        load_stage(0);
        for (uint32_t s = 0; s < nstages; s++) {
            const bool cok = s * SW_KC + lslot * 4 < p.ld;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int row = 8 * m + lrow;
                const bool ok = rok[m] & cok;
                const v4f v = R[m];
                *reinterpret_cast<float4*>(st + row * SW_KC + ((lslot ^ ((row >> 1) & 7)) << 2)) =
                    make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
            }
            wave_sync();
            if (s + 1 < nstages) load_stage(s + 1);
#pragma unroll
            for (int j = 0; j < SW_KC / 8; j++) {
                const uint32_t col = s * SW_KC + 8 * j;
                if (col < p.dim) {
                    const float4 a = *reinterpret_cast<const float4*>(st + lane * SW_KC + (((2 * j) ^ sw) << 2));
                    const float4 b = *reinterpret_cast<const float4*>(st + lane * SW_KC + (((2 * j + 1) ^ sw) << 2));
                    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    if (col + 8 <= p.dim) {
                        // one chunks_exact(8) step: acc = acc + term(q, v)   (vec_compute.rs:12-13, 39-42); every slot of the
                        // pass is computed (the query block is zero padded): no per-query branch
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

        float sc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            sc[q] = __fadd_rn(reduce8(acc[q], p.reduce), tail[q]);
            if (p.metric == OTT_METRIC_COSINE) sc[q] = __fmul_rn(__fmul_rn(sc[q], qinv[q]), vinv);  // vec_compute.rs:31
        }
        epi(my_row, valid, g, sc, nq_here);
    }
}

// The one launch of a sweep kernel.  kernel_of(MK, NQ), both as std::integral_constant<int, .>, names the instance: write it with
// OTT_SWEEP_KERNEL(kernel template, further template arguments ...).  tile: the queries of a pass, 1 or SW_NQ.  HAS_NQ1 = false: the
// kind has no single-query kernel (ott_discover.hip: a pass holds whole pairs) and only NQ = SW_NQ is instantiated.
template <bool HAS_NQ1 = true, class Params, class KernelOf>
int launch_sweep(hipStream_t stream, const Params& p, uint32_t tile, uint32_t grid, KernelOf kernel_of) {
    const auto pick = [&](auto mk) -> void (*)(Params) {
        if constexpr (HAS_NQ1) {
            if (tile == 1) return kernel_of(mk, std::integral_constant<int, 1>{});
        }
        return kernel_of(mk, std::integral_constant<int, (int)SW_NQ>{});
    };
    void (*kernel)(Params);
    switch (metric_kind(p.metric)) {
        case MK_L2: kernel = pick(std::integral_constant<int, MK_L2>{}); break;
        case MK_L1: kernel = pick(std::integral_constant<int, MK_L1>{}); break;
        default: kernel = pick(std::integral_constant<int, MK_DOT>{}); break;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * SW_WAVES), SW_SMEM, stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}
#define OTT_SWEEP_KERNEL(name, ...) [](auto mk, auto nq) { return &name<decltype(mk)::value, decltype(nq)::value, ##__VA_ARGS__>; }

}  // namespace ott
