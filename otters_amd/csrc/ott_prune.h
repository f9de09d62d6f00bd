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
// The b-bit form (prune_score_bound_sketchb): s is replaced by the odd integers kappa_i, |kappa_i| <= kmax = 2^b - 1, and D = the
// kernel's fmaf chain D <- fl(D + q_i kappa_i), one rounding per dim (the product is no longer a float, the fused sum still rounds
// once; no step underflows: D and q_i kappa_i are multiples of 2^-149).  The standard bound of a recursive sum of n_t terms gives
// |D - q_t . kappa| <= n_t u' sum |q_i kappa_i| <= n_t u' kmax ||q_t||_1, so only that term of the half width grows by kmax; kmax = 1
// is the sign form bit for bit.
OTT_PRUNE_HD inline float prune_score_bound_sketchb(const float acc[8], float vinv, float a, float rho, float D, double kmax, uint32_t m,
                                                    uint32_t dim, double qt, double q1, double qn, float qinv, bool cosine, bool upper) {
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
    const double W = (double)a * (nt * u * (1.0 + 0x1p-6) * kmax * q1) + qt * (double)rho;  // its half width (x 1.0 is exact: b = 1)
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

OTT_PRUNE_HD inline float prune_score_bound_sketch(const float acc[8], float vinv, float a, float rho, float D, uint32_t m, uint32_t dim,
                                                   double qt, double q1, double qn, float qinv, bool cosine, bool upper) {
    return prune_score_bound_sketchb(acc, vinv, a, rho, D, 1.0, m, dim, qt, q1, qn, qinv, cosine, upper);
}

// ---- the b-bit tail sketch ("three bits per dim") ---------------------------------------------------------------
// The sign sketch generalised to a signed mid-rise code of b bits per dim: kappa_i = 2 code_i + 1, code_i a two's-complement field
// of b bits, so kappa_i is an odd integer in [-(2^b - 1), 2^b - 1], and the row's tail is v_t = a kappa + r with ||r|| <= rho.
//   b = 1: the sign sketch itself — code = -1 where the sign bit is set, a = the mean of |v_i|, the same line bit for bit.
//   b > 1: Delta = max |v_i| / 2^(b-1) over the sketched dims, code_i = floor(v_i / Delta) clamped to [-2^(b-1), 2^(b-1) - 1],
//          a = Delta / 2: the mid points of 2^b cells of width Delta that cover [-max, max].
// rho is taken for the a and the codes that are stored, whatever rule chose them: ||v_t - a kappa||^2 = sum v_i^2 - 2 a sum v_i kappa_i
// + a^2 sum kappa_i^2, the three sums in double (every term exact), the cancellation paid for with 2^-34 of the magnitudes, the root
// inflated and rounded up exactly as in the sign form.  So a code on a cell boundary, or of a -0, may fall either way (host and
// device need not agree), and any a >= 0 is a valid sketch.  A tail that holds a NaN or an inf, or whose rho leaves the f32 range:
// a = 0, rho = +inf.
// Layout of a line (u32 words): [a | rho | b words per sketched stage] (b = 4: two zero words first), the field of dim 32 s + i at bits b i .. b i + b - 1 of the
// stage's b words taken as one little-endian string of 32 b bits; dims past `dim` hold code 0.  Pitch: whole 16-B lines.
// The first sketched stage: the last quarter of the stages at b = 1, the last 5/8 (rounded up) at b = 3 — at least one stage stays
// in front (the prefix then holds whole chunks of eight: 32 c < dim for every c below the stage count).
// b = 4 ("four bits per dim"): the same code with sixteen cells, in a layout of whole 16-B pieces — [a | rho | 0 | 0], then piece 1 + j
// = the four words of sketched stage j, eight fields per word, none across a word (prune_sketchb_word0: the first code word; the
// pitch, 4 S + 4 words, is what prune_sketch_pitch gives anyway).  At sixteen cells the remainder rho is small enough that the f32
// prefix is the dearer part of a gated row (the byte model), so the sketch starts at stage 1: one stage of the row
// in front (whole chunks of eight, as before), every other stage sketched.  Measured against a quarter and an eighth of the stages
// in front (profiles/exact_sketch4/README.md); experiment builds get those with -DOTT_SK4_STAGE0_DIV=4 or 8.
#ifndef OTT_SK4_STAGE0_DIV
#define OTT_SK4_STAGE0_DIV 0
#endif
OTT_PRUNE_HD inline uint32_t prune_sketchb_stage0(uint32_t nst, uint32_t bits) {
    if (bits <= 1) return prune_sketch_stage0(nst);
    if (bits == 4) {
        const uint32_t div = (uint32_t)(OTT_SK4_STAGE0_DIV), c4 = div ? nst / (div ? div : 1u) : 1u;
        return nst < 2 ? 0u : c4 < 1 ? 1u : c4;
    }
    const uint32_t c = nst - (5 * nst + 7) / 8;
    return (c < 1 && nst >= 2) ? 1u : c;
}
OTT_PRUNE_HD inline uint32_t prune_sketchb_pitch(uint32_t n_stages, uint32_t bits) { return prune_sketch_pitch(n_stages * bits); }
// the line word that holds the first code: behind a and rho, at b = 4 behind the whole first 16-B piece
OTT_PRUNE_HD inline uint32_t prune_sketchb_word0(uint32_t bits) { return bits == 4 ? 4u : 2u; }

// the code of dim i (0 .. 31) of a stage whose b words start at w
OTT_PRUNE_HD inline int32_t prune_sketchb_code(const uint32_t* w, uint32_t i, uint32_t bits) {
    const uint32_t pos = bits * i, lo = pos & 31u;
    uint32_t x = w[pos >> 5] >> lo;
    if (lo + bits > 32u) x |= w[(pos >> 5) + 1] << (32u - lo);
    return (int32_t)(x << (32u - bits)) >> (32u - bits);
}
// the code of a value for the cell width 1 / inv_delta, b > 1 (inv_delta = 0: every code is 0)
OTT_PRUNE_HD inline int32_t prune_sketchb_quant(float v, float inv_delta, uint32_t bits) {
    const float t = floorf(v * inv_delta), hi = (float)((1 << (bits - 1)) - 1), lo = -(float)(1 << (bits - 1));
    if (!(t == t)) return 0;
    return (int32_t)(t > hi ? hi : t < lo ? lo : t);
}
// the cell width's reciprocal and a from the largest magnitude of the tail (finite), b > 1
OTT_PRUNE_HD inline void prune_sketchb_scale(float vmax, uint32_t bits, float* inv_delta, float* a) {
    const float delta = vmax / (float)(1 << (bits - 1));
    float r = delta > 0.0f ? 1.0f / delta : 0.0f;
    if (!(r <= 3.4028234e38f)) r = 3.4028234e38f;  // (a subnormal Delta: the products saturate, the clamp sorts them)
    *inv_delta = r;
    *a = delta * 0.5f;
}

struct PruneSketchSumsB {
    double s1 = 0.0, s1a = 0.0, s2 = 0.0, sk = 0.0;  // sum v_i kappa_i, sum |v_i kappa_i|, sum v_i^2, sum kappa_i^2
    bool finite = true;
};
OTT_PRUNE_HD inline void prune_sketchb_add(PruneSketchSumsB& t, uint32_t vbits, int32_t kappa) {
    if ((vbits & 0x7F800000u) == 0x7F800000u) t.finite = false;
    const double x = (double)prune_u2f(vbits), kd = (double)kappa, p = x * kd;
    t.s1 += p;
    t.s1a += fabs(p);
    t.s2 += x * x;
    t.sk += kd * kd;
}
// a_in: the a the codes were made for (any non-negative finite value).  Writes a and rho.
OTT_PRUNE_HD inline void prune_sketchb_finish(const PruneSketchSumsB& t, float a_in, float* a_out, float* rho_out) {
    float a = 0.0f, rho = prune_u2f(0x7F800000u);
    if (t.finite && a_in >= 0.0f && a_in <= 3.4028234e38f) {
        a = a_in;
        const double ad = (double)a;
        const double mag = t.s2 + 2.0 * ad * t.s1a + t.sk * ad * ad;
        double r2 = t.s2 - 2.0 * ad * t.s1 + t.sk * ad * ad;
        r2 = (r2 > 0.0 ? r2 : 0.0) + mag * 0x1p-34;
        const double r = sqrt(r2) * (1.0 + 0x1p-30);
        if (r <= 3.4028234e38) rho = prune_f32_up(r);
        else a = 0.0f;
    }
    *a_out = a;
    *rho_out = rho;
}
// the sign form's a from the b = 1 sums (sum v_i kappa_i = sum |v_i| there)
OTT_PRUNE_HD inline float prune_sketchb_mean(const PruneSketchSumsB& t, uint32_t n) { return (t.finite && n) ? (float)(t.s1 / (double)n) : 0.0f; }

// v: the row (at least `dim` floats), first: the sketch's first dim (a multiple of 32).  Writes prune_sketchb_pitch words to `line`.
OTT_PRUNE_HD inline void prune_sketchb_row(const float* v, uint32_t dim, uint32_t first, uint32_t n_stages, uint32_t bits, uint32_t* line) {
    const uint32_t pitch = prune_sketchb_pitch(n_stages, bits);
    for (uint32_t j = 2; j < pitch; j++) line[j] = 0u;
    float inv_delta = 0.0f, a_in = 0.0f;
    if (bits > 1) {
        float vmax = 0.0f;
        for (uint32_t i = first; i < dim; i++) {
            const float x = prune_u2f(prune_f2u(v[i]) & 0x7FFFFFFFu);
            if (x > vmax && x <= 3.4028234e38f) vmax = x;
        }
        prune_sketchb_scale(vmax, bits, &inv_delta, &a_in);
    }
    PruneSketchSumsB t;
    for (uint32_t i = first; i < dim && i < first + 32 * n_stages; i++) {
        const uint32_t vb = prune_f2u(v[i]);
        const int32_t code = bits > 1 ? prune_sketchb_quant(v[i], inv_delta, bits) : -(int32_t)(vb >> 31);
        const uint32_t pos = bits * ((i - first) & 31u), lo = pos & 31u;
        uint32_t* w = line + prune_sketchb_word0(bits) + bits * ((i - first) >> 5) + (pos >> 5);
        const uint32_t f = (uint32_t)code & ((1u << bits) - 1u);
        w[0] |= f << lo;
        if (lo + bits > 32u) w[1] |= f >> (32u - lo);
        prune_sketchb_add(t, vb, 2 * code + 1);
    }
    if (bits <= 1) a_in = prune_sketchb_mean(t, dim > first ? dim - first : 0u);
    float a, rho;
    prune_sketchb_finish(t, a_in, &a, &rho);
    line[0] = prune_f2u(a);
    line[1] = prune_f2u(rho);
}

// ---- the head of the four-bit form ("no f32 stage in front") ------------------------------------------------------
// A companion record per row beside its four-bit line, so that a gated row reads no f32 stage at all: the four words of STAGE 0's
// codes, in the layout of a line piece (eight fields per word, code 0 past `dim`), made with the line's own cell width — a value
// beyond the tail's +-max clamps — and rho_all >= ||v - a kappa|| over ALL stages, for the a and the codes that are stored: the
// line's three double sums carried on over stage 0's dims (the tail's dims first, in order, then stage 0's) and finished by
// prune_sketchb_finish with the line's a.  A non-finite value anywhere in the row, or a line without a bound (rho = +inf): rho_all =
// +inf.  The line itself is not touched.  With it the sweep calls prune_score_bound_sketchq with m = 0: an all-zero acc, rho_all,
// K over every stage, qt = qn, and qe1 and the integer sum of the whole query (prune_query_quant with m = 0).
// Host restatement of what tail_sketch_kernel<4> writes (ott_store.hip).  v: the row, nst: its stages, line: its four-bit line
// (prune_sketchb_row with first = 32, nst - 1 stages).
OTT_PRUNE_HD inline void prune_sketch4_head_row(const float* v, uint32_t dim, uint32_t nst, const uint32_t* line, uint32_t codes[4], float* rho_all) {
    const uint32_t first = 32;
    float vmax = 0.0f, inv_delta = 0.0f, a_in = 0.0f;
    for (uint32_t i = first; i < dim; i++) {
        const float x = prune_u2f(prune_f2u(v[i]) & 0x7FFFFFFFu);
        if (x > vmax && x <= 3.4028234e38f) vmax = x;
    }
    prune_sketchb_scale(vmax, 4, &inv_delta, &a_in);
    PruneSketchSumsB t;
    for (uint32_t i = first; i < dim && i < 32 * nst; i++)  // (the codes that are stored: the kernel's own, or a line of the caller's choosing)
        prune_sketchb_add(t, prune_f2u(v[i]), 2 * prune_sketchb_code(line + prune_sketchb_word0(4) + 4 * ((i - first) >> 5), i & 31u, 4) + 1);
    codes[0] = codes[1] = codes[2] = codes[3] = 0u;
    for (uint32_t i = 0; i < first && i < dim; i++) {
        const int32_t code = prune_sketchb_quant(v[i], inv_delta, 4);
        codes[i >> 3] |= ((uint32_t)code & 15u) << (4 * (i & 7u));
        prune_sketchb_add(t, prune_f2u(v[i]), 2 * code + 1);
    }
    const float a = prune_u2f(line[0]), rho = prune_u2f(line[1]);
    float a2, r = prune_u2f(0x7F800000u);
    if (rho <= 3.4028234e38f) prune_sketchb_finish(t, a, &a2, &r);
    *rho_all = r;
}

// ---- the quantised query of the four-bit form ("the integer decode") --------------------------------------------
// The four-bit line stores eight two's-complement codes per word: one operand of a signed 4-bit dot product.  The query's other
// operand: q_i = 2^e qhat_i + e_i with integers |qhat_i| <= 1911 = 7 * 273, split into balanced base-16 digits qhat = 256 d2 + 16 d1
// + d0, every d in [-8, 7].  The digit of dim 32 s + 8 w + j sits at bits 4 j .. 4 j + 3 of word w of stage s, where the code of that
// dim sits in its piece, so sum_i code_i qhat_i = 256 K2 + 16 K1 + K0 with K_d = the dot products of the code words and the digit
// words, exact in i32 (896 dims x 8 x 8 < 2^16), and K = sum_i kappa_i qhat_i = 2 (256 K2 + 16 K1 + K0) + sum_i qhat_i.
// 2^e is a power of two taken from max |q_i| over the WHOLE query, so q_i 2^-e and 2^e qhat_i are exact wherever they do not
// underflow; the quantiser is one function for host and kernel, a single f32 multiply (no contraction) and a round to nearest even.
// A product that underflows, to a subnormal or to zero, rounds to 0 either way.
constexpr int32_t PRUNE_QHAT_MAX = 1911;
OTT_PRUNE_HD inline int32_t prune_quant_q(float q, float inv_scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __fmul_rn(q, inv_scale);
#else
    volatile float t0 = q * inv_scale;
    const float t = t0;
#endif
    const float r = rintf(t);
    if (!(r == r)) return 0;
    return r > (float)PRUNE_QHAT_MAX ? PRUNE_QHAT_MAX : r < -(float)PRUNE_QHAT_MAX ? -PRUNE_QHAT_MAX : (int32_t)r;
}
// the balanced digits of |qhat| <= 1911 (all of [-2184, 1911] has them)
OTT_PRUNE_HD inline void prune_quant_digits(int32_t qhat, int32_t d[3]) {
    d[0] = ((qhat + 8) & 15) - 8;
    const int32_t r1 = (qhat - d[0]) >> 4;  // (exact: a multiple of 16)
    d[1] = ((r1 + 8) & 15) - 8;
    d[2] = (r1 - d[1]) >> 4;
}
// eight consecutive dims of the query (zeros past `dim`) -> their word of each digit plane
OTT_PRUNE_HD inline void prune_quant_word(const float q8[8], float inv_scale, uint32_t out[3]) {
    out[0] = out[1] = out[2] = 0u;
    for (int j = 0; j < 8; j++) {
        int32_t d[3];
        prune_quant_digits(prune_quant_q(q8[j], inv_scale), d);
        for (int k = 0; k < 3; k++) out[k] |= ((uint32_t)d[k] & 15u) << (4 * j);
    }
}
// sum over the eight nibbles of a and b, both signed: what v_dot8_i32_i4 adds to its accumulator (plain C; the kernel calls the
// instruction, tests/test_exact_prune_sketchq_bound.py holds this restatement to the direct sum)
OTT_PRUNE_HD inline int32_t prune_dot8_i4(uint32_t a, uint32_t b, int32_t acc) {
    for (int j = 0; j < 8; j++) acc += ((int32_t)(a << (28 - 4 * j)) >> 28) * ((int32_t)(b << (28 - 4 * j)) >> 28);
    return acc;
}

struct PruneQuant {
    int e;                   // the scale is 2^e
    float scale, inv_scale;  // 2^e and 2^-e, both normal floats
    double qe1;              // >= sum over i >= m of |q_i - 2^e qhat_i| (double, inflated like the norms)
    int32_t qsum;            // sum over i >= m of qhat_i, exact
};
// Host: the scale of a finite query and the two tail sums the bound needs (m a multiple of 32).  The smallest 2^e with
// max |q_i| 2^-e <= 1911.  False — the integer decode is not available for this query — when the query is zero or not finite, or
// when 2^e or 2^-e is not a normal float (max |q_i| below about 2^-116).
inline bool prune_query_quant(const float* q, uint32_t dim, uint32_t m, PruneQuant* out) {
    float mx = 0.0f;
    for (uint32_t i = 0; i < dim; i++) {
        const float x = fabsf(q[i]);
        if (!(x <= 3.4028234e38f)) return false;
        if (x > mx) mx = x;
    }
    if (!(mx > 0.0f)) return false;
    int x2;
    (void)frexp((double)mx, &x2);  // mx = f 2^x2, f in [0.5, 1); 1911 = 0.933.. x 2^11
    int e = x2 - 11;
    if (ldexp((double)mx, -e) > (double)PRUNE_QHAT_MAX) e++;
    if (e < -126 || e > 126) return false;  // 2^e and 2^-e are normal floats exactly for e in [-126, 126]
    out->e = e;
    out->scale = (float)ldexp(1.0, e);
    out->inv_scale = (float)ldexp(1.0, -e);
    double t = 0.0;
    int64_t sum = 0;
    for (uint32_t i = m; i < dim; i++) {
        const int32_t h = prune_quant_q(q[i], out->inv_scale);
        t += fabs((double)q[i] - (double)out->scale * (double)h);  // (2^e qhat and the difference: exact in double)
        sum += h;
    }
    out->qe1 = t * (1.0 + 0x1p-30);
    out->qsum = (int32_t)sum;  // (|sum| <= 1911 dim: the launch carries at most 896 dims; any dim <= 2^20 fits)
    return true;
}

// The bound of the integer decode.  With v_t = a kappa + r, ||r|| <= rho, q_i = 2^e qhat_i + e_i and K = sum qhat_i kappa_i:
//   q_t . v_t = a 2^e K + a (e_t . kappa) + q_t . r  <=  a 2^e K + a kmax qe1 + ||q_t|| rho,        kmax = 15
// C = a 2^e K is exact in double (a has 24 bits, |K| <= 1911 * 15 * 864 < 2^25); the f32 chain's term a n_t u' kmax ||q_t||_1 is
// gone.  Everything else is prune_score_bound_sketchb's: Pa, G, the slack, the outward rounding, the cosine scaling, the zero rule,
// the NaN cases, Take Min as the mirror image.  Valid for every line: a 4-bit code gives |kappa_i| <= 15 whatever it holds.
OTT_PRUNE_HD inline float prune_score_bound_sketchq(const float acc[8], float vinv, float a, float rho, int32_t K, float scale, uint32_t dim,
                                                    double qt, double qe1, double qn, float qinv, bool cosine, bool upper) {
    const float nan = prune_u2f(0x7FC00000u);
    if (!(vinv >= 0x1p-50f && vinv <= 3.4028234e38f)) return nan;  // zero, tiny, huge, inf or NaN norm: no bound
    if (!(rho >= 0.0f && rho <= 3.4028234e38f)) return nan;        // no sketch of this tail
    if (!(a >= 0.0f && a <= 3.4028234e38f)) return nan;
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
    const double C = (double)a * (double)scale * (double)K;              // the centre of the tail: exact
    const double W = (double)a * (15.0 * qe1) + qt * (double)rho;        // its half width
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

// The estimate of the integer decode: the centre of the interval whose ends prune_score_bound_sketchq gives at m = 0 with an
// all-zero acc — C = a 2^e K, exact in double, rounded to f32 once and scaled like a cosine score.  A SELECTION KEY only (the
// estimate pass of the pruned sweep's seed ranks rows by it and scores the best ones exactly): nothing rests on its
// accuracy.  It lies between the two bounds of the same line; on uniform rows it is off by about ||q|| rho / sqrt(dim).  NaN —
// "do not offer this row" — exactly where that bound is NaN at m = 0: a norm, a, rho or (cosine) a query norm that gives no bound.
OTT_PRUNE_HD inline float prune_score_est_sketchq(float vinv, float a, float rho, int32_t K, float scale, float qinv, bool cosine) {
    const float nan = prune_u2f(0x7FC00000u);
    if (!(vinv >= 0x1p-50f && vinv <= 3.4028234e38f)) return nan;
    if (!(rho >= 0.0f && rho <= 3.4028234e38f)) return nan;
    if (!(a >= 0.0f && a <= 3.4028234e38f)) return nan;
    if (cosine && !(qinv > 0.0f && qinv <= 3.4028234e38f)) return nan;
    float S = (float)((double)a * (double)scale * (double)K);
    if (cosine) {
#if defined(__HIP_DEVICE_COMPILE__)
        S = __fmul_rn(__fmul_rn(S, qinv), vinv);
#else
        volatile float t1 = S * qinv;
        S = t1 * vinv;
#endif
    }
    return S;
}

// The sign sketch's own names: the b = 1 case of the functions above (sum v_i kappa_i = sum |v_i| there, sum kappa_i^2 = n, the same
// operations in the same order: the same bits).
typedef PruneSketchSumsB PruneSketchSums;
OTT_PRUNE_HD inline void prune_sketch_add(PruneSketchSums& t, uint32_t bits) { prune_sketchb_add(t, bits, (bits >> 31) ? -1 : 1); }
// n: the tail's real dims (every one of them added).  Writes a and rho.
OTT_PRUNE_HD inline void prune_sketch_finish(const PruneSketchSums& t, uint32_t n, float* a_out, float* rho_out) {
    prune_sketchb_finish(t, prune_sketchb_mean(t, n), a_out, rho_out);
}
// v: the row (at least `dim` floats), first: the sketch's first dim (a multiple of 32).  Writes pitch words to `line`.
OTT_PRUNE_HD inline void prune_sketch_row(const float* v, uint32_t dim, uint32_t first, uint32_t n_words, uint32_t* line) {
    prune_sketchb_row(v, dim, first, n_words, 1, line);
}

}  // namespace ott
