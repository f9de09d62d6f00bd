// ott_i8_check.h — the int8 operand of ONE query, and the pruned exact sweep's check of its survivors on the int8 plane
// ("survivors on the int8 plane").  Host and device code over ott_prune.h and ott_mfma_plan.h only, so that the
// CPU suite can compile it on its own (tests/test_exact_i8_check_cpu.py, tests/host/exact_i8_check_walk.cpp).
//
// The store's int8 plane holds every row as rint(v_i / s_v) with one scale s_v per row (ott_planes.hip).  A single query meets
// it as an int8 operand of its own — the query pre-scaled by 1 / ||q|| for cosine, one scale s_Q, element = rint(q_i pf / s_Q)
// — and the approximate score of a row is (float)(q~ . v~) x ((s_v [x 1 / ||v||]) x s_Q).  The int8 level's error model
// (ott_mfma_plan.h: error_model, i8_c_eps_units) bounds |approximate - exact-order f32 score| from the plane's and the query's
// MEASURED quantisation losses.  Two callers: the single-query int8 sweep of the batch path (run_i8_single, ott_mfma.hip), and
// the head form of the pruned exact sweep, which scores the rows that passed its four-bit bound on the plane before it reads
// their f32 rows (ott_exact.hip: pq_refine).  Both quantise with i8_quant_elem, so one error model covers both.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ott_mfma_plan.h"
#include "ott_prune.h"

namespace ott {

// one element of the operand: rint(q pf / s_Q) clamped to +-127 (a NaN becomes 0); inv_sq = 1 / s_Q, rounded once.  Written
// without library calls — the host quantises a query in front of every launch, and 768 calls each of rintf, fminf and fmaxf were
// most of 11 us there: the value is clamped first (rounding a value of at most 127 to nearest cannot leave the range, so clamp and
// round commute), then rounded to nearest even by adding and subtracting 1.5 x 2^23, which is exact for |x| < 2^22 in the default
// rounding mode (nothing in this project is built with -ffast-math: the sum is not reassociated)
OTT_PRUNE_HD inline int32_t i8_quant_elem(float q, float pf, float inv_sq) {
    const float xe = q * pf;
    float t = xe * inv_sq;
    t = t == t ? (t < -127.0f ? -127.0f : t > 127.0f ? 127.0f : t) : 0.0f;
    const float biased = t + 12582912.0f;
    return (int32_t)(biased - 12582912.0f);
}
// four elements as one little-endian word of the operand (what v_dot4 meets a word of the plane with)
OTT_PRUNE_HD inline uint32_t i8_quant_word(const float q4[4], float pf, float inv_sq) {
    uint32_t w = 0;
    for (int j = 0; j < 4; j++) w |= ((uint32_t)i8_quant_elem(q4[j], pf, inv_sq) & 0xFFu) << (8 * j);
    return w;
}

// the query side of the int8 level: what the operand is made with and what the error model takes
struct I8Query {
    float pf;      // the pre-scale: 1 / ||q|| (reference order) for cosine, 1 otherwise
    float s_q;     // s_Q = max |q_i pf| / 127 (1 for an all-zero or non-finite maximum)
    float inv_sq;  // 1 / s_Q
    float qnorm;   // upper bound of ||q||
    float qrel;    // measured ||q pf - s_Q q~|| / ||q pf||, rounded up, at most 1
    bool regular;  // query_regular(qnorm): inside the error model
};
// q8: dim int8 elements of the operand, or nullptr where the caller quantises elsewhere (the pruned sweep's kernel does, with
// i8_quant_word over the same pf and inv_sq)
inline I8Query i8_query_quant(const float* q, uint32_t dim, bool cosine, float q_inv, int8_t* q8) {
    // (four partial sums each: one dependent chain of 768 double additions is a microsecond of its own)
    double n2[4] = {0.0, 0.0, 0.0, 0.0};
    float amax = 0.0f;
    for (uint32_t i = 0; i < dim; i++) {
        n2[i & 3] += (double)q[i] * q[i];
        const float a = fabsf(q[i]);
        if (a > amax) amax = a;  // (a NaN is dropped, as fmaxf drops it)
    }
    I8Query x;
    x.qnorm = (float)(sqrt((n2[0] + n2[1]) + (n2[2] + n2[3])) * (1.0 + 1e-6));
    x.regular = query_regular(x.qnorm);
    x.pf = cosine ? q_inv : 1.0f;
    const float e_max = amax * x.pf;
    x.s_q = (e_max > 0.0f && e_max < __builtin_inff()) ? e_max / 127.0f : 1.0f;
    x.inv_sq = 1.0f / x.s_q;
    double se4[4] = {0.0, 0.0, 0.0, 0.0}, sx4[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < dim; i++) {
        const int32_t t = i8_quant_elem(q[i], x.pf, x.inv_sq);
        if (q8) q8[i] = (int8_t)t;
        const float xe = q[i] * x.pf;
        const double df = (double)xe - (double)x.s_q * (double)t;
        se4[i & 3] += df * df;
        sx4[i & 3] += (double)xe * (double)xe;
    }
    const double se = (se4[0] + se4[1]) + (se4[2] + se4[3]), sx = (sx4[0] + sx4[1]) + (sx4[2] + sx4[3]);
    x.qrel = sx > 0.0 ? (float)(sqrt(se / sx) * 1.0001) : 0.0f;
    if (!(x.qrel <= 1.0f)) x.qrel = 1.0f;
    return x;
}

// ---- the pruned sweep's check ------------------------------------------------------------------------------------------------------
// The bound the check drops against: what finalize_kernel certifies the int8 level with — eps_c + eps_r + 1.001 x this query's
// measured loss, for dot times the norms (the store's largest, max_norm()) — rounded outward.  ok = false: the query is outside
// the error model (not query_regular, a measured loss above what eps_r assumes of ||q~||, a bound that is not finite) and the
// sweep runs without the check.  plane_rel: the plane's measured loss (Plane::rel); eps_scale_ppm: the test-only option.
struct I8CheckEps {
    bool ok;
    float eps;
};
inline I8CheckEps i8_check_eps(uint32_t dim, uint32_t metric, int eps_scale_ppm, float plane_rel, const I8Query& x, float vn_max) {
    const I8CheckEps off{false, 0.0f};
    if (metric != OTT_METRIC_COSINE && metric != OTT_METRIC_DOT) return off;
    const ErrorModel em = error_model(2, false, dim, metric, true, eps_scale_ppm, plane_rel);
    if (!x.regular || !(x.qrel <= em.qrel_cap) || !(plane_rel >= 0.0f)) return off;
    double e = (double)em.eps_c + (double)em.eps_r + 1.001 * (double)x.qrel * (double)em.eps_scale;
    if (metric == OTT_METRIC_DOT) e *= (double)x.qnorm * (double)vn_max;
    const float eps = prune_f32_up(e * (1.0 + 1e-6));
    if (!(eps >= 0.0f && eps < __builtin_inff())) return off;
    return I8CheckEps{true, eps};
}

// the row factor of the approximate score, in run_i8_single's order of operations
OTT_PRUNE_HD inline float i8_row_factor(bool cosine, float vinv, float s_v, float s_q) { return ((cosine ? vinv : 1.0f) * s_v) * s_q; }
OTT_PRUNE_HD inline float i8_approx_score(int32_t idot, float row_factor) { return (float)idot * row_factor; }

// the far edge of [approx - eps, approx + eps] on the side the take looks at, one float further out than the rounded sum (NaN
// where the sum is NaN or infinite: no edge, the row is kept)
OTT_PRUNE_HD inline float i8_check_edge(float approx, float eps, bool take_max) {
    return take_max ? prune_next_up(approx + eps) : prune_next_down(approx - eps);
}
// "larger is better" ordinal of a score (ott_internal.h: ord_of)
OTT_PRUNE_HD inline uint32_t i8_check_ord(float f, bool take_max) {
    const uint32_t b = prune_f2u(f);
    const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return take_max ? k : ~k;
}
// The drop rule: a row goes iff the edge ranks STRICTLY below the gate (a score ordinal; 0 = open, nothing ranks below it).  A row
// outside the plane's error model (flag bits 0 / 2) is kept, and so is one whose approximate score is NaN or infinite or whose edge is NaN.
OTT_PRUNE_HD inline bool i8_check_drops(float approx, float eps, bool take_max, uint32_t gate, bool outside) {
    const float b = i8_check_edge(approx, eps, take_max);
    return !outside && approx - approx == 0.0f && b == b && i8_check_ord(b, take_max) < gate;
}

}  // namespace ott
