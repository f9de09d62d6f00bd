// ott_prune.h — the row-tail bound of the exact scorer's pruned sweep.  Host and device code; no other
// project header, so that the CPU suite can compile it on its own (tests/test_exact_prune_bound.py).
//
// After the first m dims of a row (whole chunks of eight: no remainder term yet) the exact-order kernel holds the eight
// partial accumulators acc[l] of the reference's f32x8 sum and, for this test only, vsq = the row's prefix sum of squares
// (a sequential fmaf chain).  With the query-side upper bounds qt >= ||q[m:]|| and qn >= ||q|| (prune_query_bounds) and the
// row's stored inverse norm vinv = 1 / fl(sqrt(fl(sum v^2))) (inv_norm_kernel), prune_score_bound returns a float b with
//     final score <= b  (upper = true, Take Max)      final score >= b  (upper = false, Take Min)
// in f32::total_cmp order, where "final score" is the bit-exact score the kernel would compute after the remaining dims —
// or NaN where no bound is claimed (the row is always finished).  A row whose bound ranks strictly below a proven lower
// bound of the final k-th best cannot be in the result.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define OTT_PRUNE_HD __host__ __device__
#else
#define OTT_PRUNE_HD
#endif

namespace ott {

OTT_PRUNE_HD inline uint32_t prune_f2u(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}
OTT_PRUNE_HD inline float prune_u2f(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// the float next to a finite x toward +inf / -inf
OTT_PRUNE_HD inline float prune_next_up(float x) {
    if (x == 0.0f) return prune_u2f(1u);  // smallest positive subnormal
    const uint32_t b = prune_f2u(x);
    return prune_u2f(x > 0.0f ? b + 1u : b - 1u);
}
OTT_PRUNE_HD inline float prune_next_down(float x) { return -prune_next_up(-x); }

// the smallest float >= x / the largest float <= x (x finite; beyond the f32 range: +-inf)
OTT_PRUNE_HD inline float prune_f32_up(double x) {
    const float f = (float)x;
    return (double)f < x ? prune_next_up(f) : f;
}
OTT_PRUNE_HD inline float prune_f32_down(double x) {
    const float f = (float)x;
    return (double)f > x ? prune_next_down(f) : f;
}

// Host: upper bounds of ||q[m:dim]|| and ||q||.  Every square of a float is exact in double and a sum of dim <= 2^16 of them
// is within dim * 2^-53 of its value: 2^-30 covers that and the square root.  False: the query does not allow pruning
// (a non-finite element, a zero query, or a norm above 2^50 — no partial sum of a row with a norm below 2^51 then comes near
// the f32 range).
inline bool prune_query_bounds(const float* q, uint32_t dim, uint32_t m, double* qt, double* qn) {
    double t = 0.0, n = 0.0;
    for (uint32_t i = 0; i < dim; i++) {
        const double x = (double)q[i];
        if (!(x - x == 0.0)) return false;
        n += x * x;
        if (i >= m) t += x * x;
    }
    *qt = sqrt(t * (1.0 + 0x1p-30)) * (1.0 + 0x1p-30);
    *qn = sqrt(n * (1.0 + 0x1p-30)) * (1.0 + 0x1p-30);
    return n > 0.0 && *qn <= 0x1p50;
}

// The bound.  u = 2^-24, N = dim/8 + 9, products of subnormals lose at most 2^-150 each:
//   final dot S <= sum(acc) + ||q_t|| ||v_t|| + 2 N u ||q|| ||v|| + dim 2^-148
//   ||v||^2   <= (1/vinv)^2 (1 + 2 (dim + 8) u) + dim 2^-148        (sequential f32 sum of squares, two correct roundings)
//   ||v_p||^2 >= vsq (1 - 2 (m + 1) u) - m 2^-148                   (sequential fmaf chain of m terms)
//   ||v_t||^2  = ||v||^2 - ||v_p||^2
// evaluated in double with a relative slack of 2^-40 (and 2^-50 on the difference) for the double roundings, rounded
// outward to f32; cosine then applies the kernel's own two roundings, (S * qinv) * vinv, which are monotone for positive
// scales.  A zero bound is returned as +0 (upper) / -0 (lower): total_cmp orders -0 below +0.
OTT_PRUNE_HD inline float prune_score_bound(const float acc[8], float vsq, float vinv, uint32_t m, uint32_t dim, double qt, double qn,
                                            float qinv, bool cosine, bool upper) {
    const float nan = prune_u2f(0x7FC00000u);
    if (!(vinv >= 0x1p-50f && vinv <= 3.4028234e38f)) return nan;  // zero, tiny, huge, inf or NaN norm: no bound
    if (!(vsq >= 0.0f && vsq <= 3.4028234e38f)) return nan;
    if (cosine && !(qinv > 0.0f && qinv <= 3.4028234e38f)) return nan;
    double P = 0.0, Pa = 0.0;
    for (int l = 0; l < 8; l++) {
        const double a = (double)acc[l];
        if (!(a - a == 0.0)) return nan;
        P += a;
        Pa += fabs(a);
    }
    const double u = 0x1p-24;
    const double iv = 1.0 / (double)vinv;
    const double vn2 = iv * iv * (1.0 + 2.0 * ((double)dim + 8.0) * u) + (double)dim * 0x1p-148;
    double vp2 = (double)vsq * (1.0 - 2.0 * ((double)m + 1.0) * u) - (double)m * 0x1p-148;
    if (vp2 < 0.0) vp2 = 0.0;
    double vt2 = vn2 - vp2 + (vn2 + vp2) * 0x1p-50;
    if (vt2 < 0.0) vt2 = 0.0;
    const double T = qt * sqrt(vt2);
    const double G = 2.0 * ((double)(dim / 8) + 9.0) * u * qn * sqrt(vn2);
    const double r = T + G + (Pa + T + G) * 0x1p-40 + (double)dim * 0x1p-147;
    float S = upper ? prune_f32_up(P + r) : prune_f32_down(P - r);
    if (cosine) {
#if defined(__HIP_DEVICE_COMPILE__)
        S = __fmul_rn(__fmul_rn(S, qinv), vinv);
#else
        volatile float t1 = S * qinv;  // (two separate f32 roundings, as in the kernel)
        S = t1 * vinv;
#endif
    }
    if (S == 0.0f) S = upper ? 0.0f : -0.0f;
    return S;
}

}  // namespace ott
