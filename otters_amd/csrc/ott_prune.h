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

// ---- the tail sign sketch ("the sketch form") --------------------------------------------------------------
// Per row, for the dims of stages sk0 .. nst-1 (32 dims each; dims past `dim` count as zero and are excluded): one sign word
// per stage (bit b of word j = the f32 sign bit of v[32 (sk0 + j) + b], so -0 counts as negative), a = an f32 close to the
// mean of |v_i| over those dims, and rho = an f32 with rho >= ||v_t - a s|| in real arithmetic, s_i = -1 where the bit is set,
// +1 elsewhere.  v_i - a s_i = s_i (|v_i| - a) holds for every finite v_i, -0 included, so ||v_t - a s||^2 = sum (|v_i| - a)^2
// = sum v_i^2 - 2 a sum |v_i| + n a^2.  The three sums are taken in double (every square and product of floats is exact there,
// n <= 2^16 additions lose at most n 2^-53 of the sum of the magnitudes each), the cancellation is paid for by adding 2^-34 of
// the magnitudes, and the root is inflated by 2^-30 and rounded up.  A tail that holds a NaN or an inf, or whose rho leaves the
// f32 range: a = 0, rho = +inf — no bound is ever claimed from such a sketch.
// Layout of a row's sketch line (u32 words): [a | rho | word 0 .. word W-1], pitch = prune_sketch_pitch(W) words (16-B lines).
OTT_PRUNE_HD inline uint32_t prune_sketch_stage0(uint32_t nst) { return nst - (nst + 3) / 4; }
OTT_PRUNE_HD inline uint32_t prune_sketch_pitch(uint32_t n_words) { return (n_words + 2 + 3) & ~3u; }

// The sketch's running sums over the tail dims, taken in dim order: one element (its f32 bits), then the end.
struct PruneSketchSums {
    double s1 = 0.0, s2 = 0.0;  // sum |v_i|, sum v_i^2
    bool finite = true;
};
OTT_PRUNE_HD inline void prune_sketch_add(PruneSketchSums& t, uint32_t bits) {
    if ((bits & 0x7F800000u) == 0x7F800000u) t.finite = false;
    const double x = (double)prune_u2f(bits & 0x7FFFFFFFu);
    t.s1 += x;
    t.s2 += x * x;
}
// n: the tail's real dims.  Writes a and rho.
OTT_PRUNE_HD inline void prune_sketch_finish(const PruneSketchSums& t, uint32_t n, float* a_out, float* rho_out) {
    float a = 0.0f, rho = prune_u2f(0x7F800000u);
    if (t.finite) {
        a = n ? (float)(t.s1 / (double)n) : 0.0f;  // (any non-negative finite a gives a valid sketch: rho is taken for THIS a)
        const double ad = (double)a;
        const double mag = t.s2 + 2.0 * ad * t.s1 + (double)n * ad * ad;
        double r2 = t.s2 - 2.0 * ad * t.s1 + (double)n * ad * ad;
        r2 = (r2 > 0.0 ? r2 : 0.0) + mag * 0x1p-34;
        const double r = sqrt(r2) * (1.0 + 0x1p-30);
        if (r <= 3.4028234e38) rho = prune_f32_up(r);
        else a = 0.0f;
    }
    *a_out = a;
    *rho_out = rho;
}

// v: the row (at least `dim` floats), first: the sketch's first dim (a multiple of 32).  Writes pitch words to `line`.
OTT_PRUNE_HD inline void prune_sketch_row(const float* v, uint32_t dim, uint32_t first, uint32_t n_words, uint32_t* line) {
    PruneSketchSums t;
    for (uint32_t j = 0; j < n_words; j++) {
        uint32_t w = 0;
        for (uint32_t b = 0; b < 32; b++) {
            const uint32_t i = first + 32 * j + b;
            if (i >= dim) break;
            const uint32_t bits = prune_f2u(v[i]);
            w |= (bits >> 31) << b;
            prune_sketch_add(t, bits);
        }
        line[2 + j] = w;
    }
    float a, rho;
    prune_sketch_finish(t, dim > first ? dim - first : 0u, &a, &rho);
    line[0] = prune_f2u(a);
    line[1] = prune_f2u(rho);
    for (uint32_t j = 2 + n_words; j < prune_sketch_pitch(n_words); j++) line[j] = 0u;
}

// Host: an upper bound of sum |q[m:dim]| (double, inflated like the norms), m a multiple of 32
inline double prune_query_l1(const float* q, uint32_t dim, uint32_t m) {
    double t = 0.0;
    for (uint32_t i = m; i < dim; i++) t += fabs((double)q[i]);
    return t * (1.0 + 0x1p-30);
}

// The sketch form of the bound.  The kernel stops at dim m (a multiple of 32 at or after the sketch's first dim) with the eight
// chains acc[l], and has summed, in f32 and in any order, D = sum over the n_t = dim - m tail dims of q_i s_i (each term exact).
// With v_t = a s + r over those dims (r is a part of the sketched remainder, so ||r|| <= rho):
//   q_t . v_t  =  a (q_t . s) + q_t . r  <=  a (D + n_t u' ||q_t||_1) + ||q_t|| rho,      u' = 2^-24 (1 + 2^-6)
//   final dot S <= sum(acc) + q_t . v_t + 2 N u ||q|| ||v|| + dim 2^-148                   (as in prune_score_bound)
// (a D is exact in double: two 24-bit significands.)  q1 >= ||q[m:]||_1 (prune_query_l1), qt, qn as for prune_score_bound.
// The same evaluation in double with slack, the same outward rounding, cosine scaling and zero rule.
OTT_PRUNE_HD inline float prune_score_bound_sketch(const float acc[8], float vinv, float a, float rho, float D, uint32_t m, uint32_t dim,
                                                   double qt, double q1, double qn, float qinv, bool cosine, bool upper) {
    const float nan = prune_u2f(0x7FC00000u);
    if (!(vinv >= 0x1p-50f && vinv <= 3.4028234e38f)) return nan;  // zero, tiny, huge, inf or NaN norm: no bound
    if (!(rho >= 0.0f && rho <= 3.4028234e38f)) return nan;        // no sketch of this tail
    if (!(a >= 0.0f && a <= 3.4028234e38f)) return nan;
    if (!(D - D == 0.0f)) return nan;
    if (cosine && !(qinv > 0.0f && qinv <= 3.4028234e38f)) return nan;
    double P = 0.0, Pa = 0.0;
    for (int l = 0; l < 8; l++) {
        const double x = (double)acc[l];
        if (!(x - x == 0.0)) return nan;
        P += x;
        Pa += fabs(x);
    }
    const double u = 0x1p-24;
    const double iv = 1.0 / (double)vinv;
    const double vn2 = iv * iv * (1.0 + 2.0 * ((double)dim + 8.0) * u) + (double)dim * 0x1p-148;
    const double nt = (double)(dim > m ? dim - m : 0u);
    const double C = (double)a * (double)D;                                     // the centre of the tail: exact
    const double W = (double)a * (nt * u * (1.0 + 0x1p-6) * q1) + qt * (double)rho;  // its half width
    const double G = 2.0 * ((double)(dim / 8) + 9.0) * u * qn * sqrt(vn2);
    const double r = W + G + (Pa + fabs(C) + W + G) * 0x1p-40 + (double)dim * 0x1p-147;
    float S = upper ? prune_f32_up(P + C + r) : prune_f32_down(P + C - r);
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
