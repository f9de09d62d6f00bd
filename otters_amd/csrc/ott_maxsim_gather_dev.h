// ott_maxsim_gather_dev.h — what maxsim_gather_kernel (ott_maxsim_gather.hip) and maxsim_gather_batch_kernel (ott_maxsim_batch.hip)
// share on the device, written once: the join of a group's running maxima over the row groups of a wave and over the waves, and
// the sum of one query's maxima in token order that makes the group's key.  The per-row body in front of them — one 32-row step of
// the workgroup — is ott_maxsim_gather_step.inc, shared as text (why: its header).  Both kernels keep their tokens in LDS as
// [dimq][NT + MG_PAD] floats, then [NT] inverse norms, then [MG_WAVES][NT] maxima (mg_lds_bytes).
#pragma once

#include "ott_internal.h"
#include "ott_exact_dev.h"

namespace ott {

constexpr int MG_UNROLL = 8;  // row elements a lane has in flight

// The join: over the wave's eight row groups by shuffles (the lanes of one group agree already); lane 0 leaves the wave's maxima in
// sB[wave][NT].  The caller's barrier comes next, mg_joined reads behind it.
template <int NT>
__device__ __forceinline__ void mg_join_wave(const uint32_t (&best)[NT], uint32_t* sB, int wave, int lane) {
#pragma unroll
    for (int q = 0; q < NT; q++) {
        uint32_t b = best[q];
#pragma unroll
        for (int d = 8; d < 64; d <<= 1) {
            const uint32_t ob = (uint32_t)__shfl_xor((int)b, d);
            if (ob > b) b = ob;
        }
        if (lane == 0) sB[wave * NT + q] = b;
    }
}
template <int NT>
__device__ __forceinline__ uint32_t mg_joined(const uint32_t* sB, uint32_t t) {
    uint32_t m = sB[t];
#pragma unroll
    for (int w = 1; w < (int)MG_WAVES; w++) m = sB[w * NT + t] > m ? sB[w * NT + t] : m;
    return m;
}

// One pass holds every token of the query: the sum of the joined maxima in token order, started from best[0] (a -0.0 stays -0.0),
// as maxsim_reduce_kernel makes it.  The group's key, or 0 = dropped (a token without a best, a NaN sum, the filter).
template <int NT>
__device__ __forceinline__ unsigned long long mg_sum_key(const uint32_t* sB, uint32_t n_tokens, bool take_max, uint32_t cmp, float thr, uint32_t gid) {
    bool complete = true;
    float sum = 0.0f;
    for (uint32_t t = 0; t < n_tokens; t++) {
        const uint32_t o = mg_joined<NT>(sB, t);
        if (o == 0) {
            complete = false;
        } else {
            const float b = score_of(o, take_max);
            sum = t == 0 ? b : __fadd_rn(sum, b);
        }
    }
    if (complete && !(sum != sum) && cmp_holds(sum, cmp, thr)) return ((unsigned long long)ord_of(sum, take_max) << 32) | (uint32_t)(~gid);
    return 0ull;
}

}  // namespace ott
