// ott_exact_dev.h — device helpers of the exact-order kernels, shared by ott_exact.hip (exact_kernel, exact_rows8_kernel, the merge
// kernels), ott_gather.hip (exact_gather8_kernel) and ott_mmr.hip (mmr_pair_kernel): the candidate order, the wave-wide sorted
// candidate list, the score filter, the per-element term of every metric, wide's horizontal sum and the per-row step of the kernels
// that read scattered rows with eight lanes per row.  Inline only: a kernel that includes this compiles
// to what it compiled to when the code stood in ott_exact.hip.
#pragma once

#include "ott_internal.h"

namespace ott {

// Candidate order.  sh = 0: the canonical total order (better score, lower row, lower query).  sh = 3 (store option
// tie_order = reference): better score, then the reference's VISIT order — 8-row block, then query, then row within the block
// (src/vec.rs:222-303: blocks of eight rows, every query per block, lanes in order; the remainder rows all share the last
// block index, where the same three keys give query-then-row) — so that among equal scores the first one the reference's
// collector would have seen ranks first.  key = ord << 32 | ~row: key >> 3 is (ord, ~block), key & 7 is ~(row & 7).
__device__ __forceinline__ bool before(uint64_t ak, uint32_t aq, uint64_t bk, uint32_t bq, uint32_t sh) {
    const uint64_t ah = ak >> sh, bh = bk >> sh;
    return ah > bh || (ah == bh && (aq < bq || (aq == bq && ak > bk)));
}

__device__ __forceinline__ uint32_t rl32(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ uint64_t rl64(uint64_t v, int src) {
    return ((uint64_t)rl32((uint32_t)(v >> 32), src) << 32) | rl32((uint32_t)v, src);
}

__device__ __forceinline__ void wave_sync() {
    // orders this wave's LDS writes before its later LDS reads (DS ops of one wave execute in
    // order; this only stops the compiler from moving them across)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sorted candidate list spread over a wave: position p = e*64 + lane
template <int E>
struct WaveList {
    uint64_t key[E];
    uint32_t q[E];
};

template <int E>
__device__ __forceinline__ void wl_init(WaveList<E>& L) {
#pragma unroll
    for (int e = 0; e < E; e++) {
        L.key[e] = 0;  // sentinel: worse than any real candidate (real ord >= 1)
        L.q[e] = 0xFFFFFFFFu;
    }
}

template <int E>
__device__ __forceinline__ void wl_insert(WaveList<E>& L, uint64_t xk, uint32_t xq, int lane, uint32_t sh) {
    int pos = 0;
#pragma unroll
    for (int e = 0; e < E; e++) pos += __popcll(__ballot(before(L.key[e], L.q[e], xk, xq, sh)));
#pragma unroll
    for (int e = E - 1; e >= 0; e--) {
        uint64_t upk = __shfl_up(L.key[e], 1);
        uint32_t upq = __shfl_up(L.q[e], 1);
        if (e > 0) {
            uint64_t pk = rl64(L.key[e - 1], 63);
            uint32_t pq = rl32(L.q[e - 1], 63);
            if (lane == 0) {
                upk = pk;
                upq = pq;
            }
        }
        int p = e * 64 + lane;
        if (p == pos) {
            L.key[e] = xk;
            L.q[e] = xq;
        } else if (p > pos) {
            L.key[e] = upk;
            L.q[e] = upq;
        }
    }
}

// key of the current k-th entry (position k-1)
template <int E>
__device__ __forceinline__ void wl_tau(const WaveList<E>& L, uint32_t k, uint64_t& tk, uint32_t& tq) {
    uint32_t p = k - 1;
#pragma unroll
    for (int e = 0; e < E; e++)
        if ((int)(p >> 6) == e) {
            tk = rl64(L.key[e], p & 63);
            tq = rl32(L.q[e], p & 63);
        }
}

template <int E>
__device__ __forceinline__ void wl_offer(WaveList<E>& L, uint64_t& tk, uint32_t& tq, uint32_t k, bool pass, uint64_t key,
                                         uint32_t q, int lane, uint32_t sh) {
    pass = pass && before(key, q, tk, tq, sh);
    uint64_t m = __ballot(pass);
    while (m) {
        int src = __builtin_ctzll(m);
        m &= m - 1;
        uint64_t xk = rl64(key, src);
        uint32_t xq = rl32(q, src);
        if (before(xk, xq, tk, tq, sh)) {
            wl_insert(L, xk, xq, lane, sh);
            wl_tau(L, k, tk, tq);
        }
    }
}

// Bitonic sort of one (key, q) entry per lane, best first (entries that are not `pass` become the sentinel and sort last).
__device__ __forceinline__ void wave_sort_desc(uint64_t& sk, uint32_t& sq, int lane, uint32_t sh) {
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1) {
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const uint64_t ok = __shfl_xor(sk, j);
            const uint32_t oq = __shfl_xor(sq, j);
            const bool mine_first = before(sk, sq, ok, oq, sh);               // my entry ranks before the partner's
            const bool want_first = ((lane & j) == 0) == ((lane & k2) == 0);  // this lane keeps the better one of the pair
            if (mine_first != want_first && !(sk == ok && sq == oq)) {
                sk = ok;
                sq = oq;
            }
        }
    }
}

// One register of 64 entries that is BITONIC (e.g. the lane-wise better halves of a descending and an ascending sequence)
// into descending order: the last six steps of the sort above.
__device__ __forceinline__ void wave_bitonic_merge_desc(uint64_t& sk, uint32_t& sq, int lane, uint32_t sh) {
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const uint64_t ok = __shfl_xor(sk, j);
        const uint32_t oq = __shfl_xor(sq, j);
        const bool mine_first = before(sk, sq, ok, oq, sh);
        const bool want_first = (lane & j) == 0;
        if (mine_first != want_first && !(sk == ok && sq == oq)) {
            sk = ok;
            sq = oq;
        }
    }
}

// A SORTED register of 64 candidates (best first, sentinels behind the real ones) into the sorted list, as a block: register
// by register, the better halves of (list register, reversed block) stay, the worse halves move on to the next register, each
// half put back in order by a bitonic merge — 3 + 36 shuffles per register whatever the number of candidates, where
// inserting them one by one costs a ballot, a shift of the whole list and a new threshold EACH (round 3: a wave of a 1M-row
// store sees 500 rows, so at k = 100 a fifth of them entered its list that way: top-100 on 1M x 128 took 200 us, top-10 88).
template <int E>
__device__ __forceinline__ void wl_merge_sorted(WaveList<E>& L, uint64_t sk, uint32_t sq, int lane, uint32_t sh) {
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint64_t rk = __shfl(sk, 63 - lane);
        const uint32_t rq = __shfl(sq, 63 - lane);
        const bool mine = before(L.key[e], L.q[e], rk, rq, sh);
        uint64_t hk = mine ? L.key[e] : rk, lk = mine ? rk : L.key[e];
        uint32_t hq = mine ? L.q[e] : rq, lq = mine ? rq : L.q[e];
        wave_bitonic_merge_desc(hk, hq, lane, sh);
        wave_bitonic_merge_desc(lk, lq, lane, sh);
        L.key[e] = hk;
        L.q[e] = hq;
        sk = lk;
        sq = lq;
    }
}

// wl_offer for a tile with MANY candidates above the threshold (the first tiles of a wave, the lists of the other waves at the
// block fold): sort them once and merge the block; few candidates: one at a time as before.
constexpr int WL_BLOCK_MIN = 12;
template <int E>
__device__ __forceinline__ void wl_offer_block(WaveList<E>& L, uint64_t& tk, uint32_t& tq, uint32_t k, bool pass, uint64_t key, uint32_t q, int lane,
                                               uint32_t sh) {
    pass = pass && before(key, q, tk, tq, sh);
    if (__popcll(__ballot(pass)) < WL_BLOCK_MIN) {
        wl_offer(L, tk, tq, k, pass, key, q, lane, sh);
        return;
    }
    uint64_t sk = pass ? key : 0ull;
    uint32_t sq = pass ? q : 0xFFFFFFFFu;
    wave_sort_desc(sk, sq, lane, sh);
    wl_merge_sorted(L, sk, sq, lane, sh);
    wl_tau(L, k, tk, tq);
}

// First offer into an EMPTY one-entry-per-lane list (k <= 64): the sorted candidates ARE the list — 21 shuffle steps instead
// of up to 64 one-at-a-time insertions (a wave's first tile; for a store of one tile per wave that is the whole query).
// (Longer lists, k > 64: the 64 sorted candidates are positions 0 .. 63, the rest stays empty.  Inserting a tile's 64 rows one
// by one — at k > 64 every row of a wave's first tile is a candidate — was most of the 33 us rows8 took for a top-100 on a
// 10k-row store against 10 for a top-10.)
template <int E>
__device__ __forceinline__ void wl_fill_sorted(WaveList<E>& L, uint64_t& tk, uint32_t& tq, uint32_t k, bool pass, uint64_t key, uint32_t q, int lane,
                                               uint32_t sh) {
    uint64_t sk = pass ? key : 0ull;
    uint32_t sq = pass ? q : 0xFFFFFFFFu;
    wave_sort_desc(sk, sq, lane, sh);
    L.key[0] = (uint32_t)lane < k ? sk : 0ull;
    L.q[0] = (uint32_t)lane < k ? sq : 0xFFFFFFFFu;
#pragma unroll
    for (int e = 1; e < E; e++) {
        L.key[e] = 0ull;
        L.q[e] = 0xFFFFFFFFu;
    }
    wl_tau(L, k, tk, tq);
}

__device__ __forceinline__ bool cmp_holds(float s, uint32_t cmp, float thr) {
    // src/vec_compute.rs:56-64: ordered compares (false on NaN)
    switch (cmp) {
        case OTT_CMP_LT: return s < thr;
        case OTT_CMP_GT: return s > thr;
        case OTT_CMP_LTE: return s <= thr;
        case OTT_CMP_GTE: return s >= thr;
        case OTT_CMP_EQ: return s == thr;
        default: return true;
    }
}

typedef float v4f __attribute__((ext_vector_type(4)));

// Metric kind of the exact family (template parameter MK of exact_kernel / exact_rows8_kernel): the per-element term that the
// eight chains and the remainder add up.  Dot and cosine share MK_DOT (cosine scales the sum by the inverse norms afterwards).
// MK_L1 is the Manhattan metric, an extension whose contract the project defines in the reference's style:
//     manhattan(q, v) = reduce_add(acc) + tail
//       acc[l] = 0;  for each chunk j of chunks_exact(8), in order:  acc[l] = acc[l] + |q[8j+l] - v[8j+l]|
//       tail   = 0;  for each remainder element i, in order:          tail   = tail + |q[i] - v[i]|
// IEEE f32 round-to-nearest-even throughout (the subtraction rounds, abs is exact, the add rounds), nothing fused, no flush;
// reduce_add is reduce8 in the store's order and the final add __fadd_rn(reduce8(acc), tail), as for dot and L2.  inf - inf
// gives NaN (the pair is dropped), an infinite difference or an overflowing sum +inf (a valid score).
constexpr int MK_DOT = 0, MK_L2 = 1, MK_L1 = 2;
static inline int metric_kind(uint32_t metric) {
    return metric == OTT_METRIC_EUCLIDEAN ? MK_L2 : metric == OTT_METRIC_MANHATTAN ? MK_L1 : MK_DOT;
}
template <int MK>
__device__ __forceinline__ float exact_term(float qv, float x) {
    if constexpr (MK == MK_L2) {
        const float d = __fsub_rn(qv, x);  // vec_compute.rs:39-42
        return __fmul_rn(d, d);
    } else if constexpr (MK == MK_L1) {
        return fabsf(__fsub_rn(qv, x));    // |q - v|: the subtraction rounds, abs is exact, so |q - v| == |v - q| bit for bit
    } else {
        return __fmul_rn(qv, x);           // vec_compute.rs:12-13
    }
}

// wide::f32x8::reduce_add (see oracle/otters_oracle.h for the two orders)
__device__ __forceinline__ float reduce8(const float* l, uint32_t mode) {
    if (mode == OTT_REDUCE_SEQ4) {
        float a = __fadd_rn(__fadd_rn(__fadd_rn(l[0], l[1]), l[2]), l[3]);
        float b = __fadd_rn(__fadd_rn(__fadd_rn(l[4], l[5]), l[6]), l[7]);
        return __fadd_rn(a, b);
    }
    return __fadd_rn(__fadd_rn(__fadd_rn(l[0], l[4]), __fadd_rn(l[2], l[6])),
                     __fadd_rn(__fadd_rn(l[1], l[5]), __fadd_rn(l[3], l[7])));
}

// The per-row step of the eight-lanes-per-row kernels that read scattered rows (exact_gather8_kernel, ott_gather.hip; mmr_pair_kernel,
// ott_mmr.hip): one row against NQ queries that sit in LDS ([NQ][dimq], zero padded).  Lane c = lane & 7 of the row's 8-lane group
// carries chain c of the reference's f32x8: acc = acc + q[8j + c] * v[8j + c], j ascending (vec_compute.rs:12-13, 39-42), the
// cross-lane sum is wide's reduce_add in either order, the remainder is sequential and every lane of the group computes it
// (vec_compute.rs:15-21, 44-53); cosine scales the sum by the query's and then the row's inverse norm (vec_compute.rs:31).  Every
// lane of the group ends with the same sc[q].  The rows are scattered: a wave instruction touches 8 rows x 32 B, and the four steps
// that share a 128-B line hit in the vector L1.
template <int MK, int NQ, int UNROLL>
__device__ __forceinline__ void rows8_scores(const float* sQ, uint32_t dimq, const float* rp, uint32_t dim, int lane, uint32_t reduce, bool cosine,
                                             const float* qinv, float vinv, float* sc) {
    const int c = lane & 7;
    const uint32_t full = dim >> 3;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = 0.0f;
    auto step = [&](uint32_t jj, float xv) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float qv = sQ[(uint32_t)q * dimq + 8 * jj + c];
            acc[q] = __fadd_rn(acc[q], exact_term<MK>(qv, xv));
        }
    };
    uint32_t j = 0;
    for (; j + UNROLL <= full; j += UNROLL) {
        float x[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) x[u] = rp[8 * (j + u) + c];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) step(j + u, x[u]);
    }
    for (; j < full; j++) step(j, rp[8 * j + c]);
    float tail[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) tail[q] = 0.0f;
    const uint32_t nt = dim & 7u;
    for (uint32_t l = 0; l < nt; l++) {
        const float xv = rp[8 * full + l];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float qv = sQ[(uint32_t)q * dimq + 8 * full + l];
            tail[q] = __fadd_rn(tail[q], exact_term<MK>(qv, xv));
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        // wide::f32x8::reduce_add across the group's eight lanes
        float sum;
        if (reduce == OTT_REDUCE_SEQ4) {
            const int b = lane & ~7;
            float l8[8];
#pragma unroll
            for (int i = 0; i < 8; i++) l8[i] = __shfl(acc[q], b + i);
            sum = reduce8(l8, OTT_REDUCE_SEQ4);
        } else {
            const float s1 = __fadd_rn(acc[q], __shfl_xor(acc[q], 4));  // l_c + l_{c^4}
            const float s2 = __fadd_rn(s1, __shfl_xor(s1, 2));          // (l0+l4)+(l2+l6) on even-pair lanes, (l1+l5)+(l3+l7) on the others
            sum = __fadd_rn(s2, __shfl_xor(s2, 1));                     // (a + b == b + a bit for bit)
        }
        float v = __fadd_rn(sum, tail[q]);
        if (cosine) v = __fmul_rn(__fmul_rn(v, qinv[q]), vinv);  // vec_compute.rs:31
        sc[q] = v;
    }
}

}  // namespace ott
