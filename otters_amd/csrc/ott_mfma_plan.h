// ott_mfma_plan.h — what the batch path's host side decides before it launches anything, free of HIP and of ott_store: plain
// C++17 over the public header's enums, like ott_policy.h, so that the CPU suite compiles the very code libotters_hip.so ships on
// its own (tests/test_mfma_plan_cpu.py).  Each of these is written here once, for both runners of ott_mfma.hip (run_mfma,
// run_i8_single) and for ott_policy.h:
//   * the tile geometry of a batch;
//   * how many candidates a level re-scores (its budget);
//   * the bound on |approximate - exact| a level certifies against (DESIGN.md "MFMA path: certification");
//   * which queries that bound covers (query_regular) and the norms it is built from;
//   * the layout of the one pinned block a batch uploads.
// Used from files built with -ffp-contract=off (the Makefile's flag); a driver that wants the same bits is built the same way.
#pragma once
#include <math.h>

#include "../../include/otters_hip.h"  // (and through it stddef.h, stdint.h)

namespace ott {

// ---- tile geometry ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t MFMA_K_STAGE = 32;  // k per stage of the scoring kernel (ott_mfma.hip: MKC)
// level 0 = hi pass (the store's 16-bit hi plane), 1 = split-bf16 / f32-pipe pass, 2 = int8 pass (rows and queries as scaled int8,
// from the store's int8 plane; it shares the hi pass's tile geometry and its measured bound)
constexpr bool level_is_i8(int level) { return level == 2; }
constexpr bool level_is_hi(int level) { return level == 0 || level == 2; }

struct TileGeometry {
    int NB;             // tile variant of mfma_score_kernel: -1 (16 queries), 0 (32), 1 (64), 2 (128), 4 (256)
    uint32_t BN;        // queries per tile
    uint32_t nq_pad;    // the batch, padded to whole tiles
    uint32_t qblk_max;  // query blocks per launch
    uint32_t ldq;       // f32 units per query row (raw block; split operands)
    uint32_t ldh;       // hi pass: operand rows are ldh 16-bit units = ldh / 2 four-byte units (int8: 2 ldh bytes)
    uint32_t passes() const { return (nq_pad / BN + qblk_max - 1) / qblk_max; }  // passes over the plane from HBM
};
inline TileGeometry tile_geometry(uint32_t nq, int level, uint32_t dim) {
    TileGeometry g;
    // tile width: 16 or 32 queries (micro / narrow variants, 4-deep ring), 64, 128 or 256 (the micro tile is f32 only)
    g.NB = (nq <= 16 && !level_is_hi(level)) ? -1 : nq <= 32 ? 0 : nq <= 64 ? 1 : nq <= 128 ? 2 : 4;
    g.BN = g.NB == -1 ? 16u : g.NB == 0 ? 32u : 64u * (uint32_t)g.NB;
    g.nq_pad = (nq + g.BN - 1) / g.BN * g.BN;
    // query blocks per launch (mfma_score_kernel): the 256-wide tile takes up to 4 blocks of one row tile back to back
    g.qblk_max = g.NB != 4 ? 1u : g.nq_pad / g.BN < 4u ? g.nq_pad / g.BN : 4u;
    g.ldq = (dim + MFMA_K_STAGE - 1) / MFMA_K_STAGE * MFMA_K_STAGE;
    g.ldh = level_is_i8(level) ? ((dim + 127u) & ~127u) / 2 : (dim + 63u) & ~63u;
    return g;
}

// ---- candidate budget ------------------------------------------------------------------------------------------------------------
// T = re-scored candidates per query: k plus slack, a multiple of 64.  What each level WANTS before that rounding:
constexpr uint64_t MFMA_T_MAX = 512;    // the most a level re-scores (the 4096-candidate level apart)
constexpr uint64_t MFMA_T_WIDE = 4096;  // the cascade's last level: lists of 64K entries, finalize sorts 4096 candidates in LDS
constexpr uint64_t t_want_split(uint64_t k) { return k + 28; }
// the hi pass's bound is ~100x wider, so it needs every row within it of the k-th score among the re-scored: at least 2k + 56
constexpr uint64_t t_want_hi(uint64_t k) { return 2 * k + 56; }
// (int8: a bound ~15x the half plane's — every row within ~8e-3 of the k-th score must be among the re-scored: 512)
// (the int8 pass: about 2.7 k rows of a uniform 768-d corpus lie within its bound of the k-th score — 4k + 88 re-scored, at most 512;
//  a store whose queries fail at that is asked for 512 from then on, t_min)
constexpr uint64_t t_want_i8(uint64_t k) { return 4 * k + 88 < MFMA_T_MAX ? 4 * k + 88 : MFMA_T_MAX; }
// the list the one-query sweep keeps: 128 candidates while k <= 24 (about 2.7 k rows of a uniform 768-d corpus lie within the bound
// of the k-th score), what the cascade's int8 level would re-score otherwise
constexpr uint64_t SWEEP_T = 128, SWEEP_K_MAX = 24;
constexpr uint64_t I8_K_MAX = 128;  // the int8 level is asked for up to this k
// on a half plane, whose bound is ~8x tighter than bf16's, k + k / 3 + 28 within the 512 is enough (k <= 363 instead of 228: about
// 0.23 k rows lie within the bound of the k-th score on uniform rows)
inline bool mfma_hi_k_ok(uint64_t k, bool half) { return (half ? k + k / 3 + 28 : t_want_hi(k)) <= MFMA_T_MAX; }

struct Budget {
    uint32_t T;    // candidates re-scored per query
    int E;         // finalize_kernel's exact top-k list holds 64 E entries
    bool wide;     // the 4096-candidate level
    uint32_t cap;  // slots of a query's candidate list
    bool k_too_large;
};
// (t_min: the split pass as a later level of the cascade sees the queries whose k-th score sits in a dense neighbourhood —
// that is why the pass before failed them — so it re-scores more: 512 as the second level, 4096 as the third)
// (round 3: the hi pass re-scores `t_min` = 512 per query once it has failed a store's queries at 2k + 56 (ott_api.hip,
//  hi_t512) — what certifies clustered corpora in ONE pass: 20 000 clusters of ~500 near neighbours each, 256 queries,
//  top-100: 10.5 ms with every query through the split pass -> 4.9 ms; on uniform rows it would cost ~0.15 ms of wall per batch)
inline Budget level_budget(int level, uint32_t k, uint32_t t_min, uint64_t rows_scored, bool sweep) {
    Budget b;
    const uint64_t own = sweep ? (k <= SWEEP_K_MAX ? SWEEP_T : t_want_i8(k)) : level_is_i8(level) ? t_want_i8(k) : level_is_hi(level) ? t_want_hi(k) : t_want_split(k);
    // (the sweep takes a t_min above its 128 as it is; the rounds take the larger of t_min and the level's own want)
    const uint64_t want = (sweep ? t_min > SWEEP_T : t_min > own) ? t_min : own;
    b.E = sweep ? 2 : 1;  // (the sweep's wave lists hold at least 128)
    while (64u * b.E < (want < MFMA_T_MAX ? want : MFMA_T_MAX) && b.E < 8) b.E *= 2;
    b.wide = !sweep && !level_is_hi(level) && t_min > MFMA_T_MAX;
    b.T = b.wide ? (uint32_t)MFMA_T_WIDE : 64u * b.E;
    if (b.wide) {  // E now only sizes the exact top-k list
        b.E = 1;
        while (64u * b.E < k && b.E < 8) b.E *= 2;
    }
    b.k_too_large = k > b.T || k > MFMA_T_MAX;
    const uint32_t cap_max = b.wide ? 65536u : 16384u;  // a round leaves ~8 T survivors per query
    // small stores: the list can hold every row, no need for all the slots.  The sweep has no rounds: its list is all there is
    b.cap = sweep ? b.T : 1024;
    while (!sweep && b.cap < rows_scored + 64 && b.cap < cap_max) b.cap <<= 1;
    return b;
}

// ---- error bound on |approx - exact| (see DESIGN.md "MFMA path: certification") ----------------------------------------------------
// The int8 passes' accumulation constant for cosine / dot, in units of 2^-24 relative to ||q|| ||v||: a bound on
// |approximate - EXACT-ORDER f32 score| beyond the measured quantisation losses.  Two sides:
//  * the approximate score: the integer accumulation is exact; one i32 -> f32 conversion, the row factor's two multiplies and the
//    score's one, the per-element rounding of the pre-scaled cosine operand: 16 units cover them;
//  * the exact-order re-score it is compared with (src/vec_compute.rs:9-22) is NOT the real dot product: a lane chain is dim/8
//    rounded products and rounded adds, then three adds of reduce_add, the remainder's chain (at most 7 + 1 adds) and cosine's two
//    multiplies — |fl - real| <= gamma(dim/8 + 6) * sum|q_i v_i| <= (dim/8 + 16) units of ||q|| ||v|| (Higham, recursive summation;
//    the 1 / (1 - n u) factor is inside the slack for every dim the store accepts).
// Round 5 priced the first side only ("pure quantisation"): with int8-REPRESENTABLE rows and queries the measured losses are ~1e-7,
// the bound collapsed to ~17 units, and nearly constant rows — whose lane sums drift by 30-150 units, every add rounding the same
// way — were left outside a "certified" list (tests/adversarial_i8.py, tests/test_gpu_i8_bound.py, profiles/round6/i8_bound.md).
inline float i8_c_eps_units(uint32_t dim) { return 0.125f * (float)dim + 32.0f; }

// upper bound on ||v|| over the store, from its smallest non-zero inverse norm (+inf: no such row)
inline float max_norm(float min_pos_inv) { return min_pos_inv < __builtin_inff() ? (1.0f / min_pos_inv) * 1.000001f : 0.0f; }

// what the relaxed score filter of a candidate pass lets through: the caller's interval widened by eps_max on its closed side(s),
// so that nothing that can pass exactly is dropped
struct FilterInterval {
    float flo, fhi;
};
inline FilterInterval relaxed_filter(uint32_t filter_cmp, float filter_thr, float eps_max) {
    FilterInterval f = {-__builtin_inff(), __builtin_inff()};
    switch (filter_cmp) {
        case OTT_CMP_GT: case OTT_CMP_GTE: f.flo = filter_thr - eps_max; break;
        case OTT_CMP_LT: case OTT_CMP_LTE: f.fhi = filter_thr + eps_max; break;
        case OTT_CMP_EQ: f.flo = filter_thr - eps_max; f.fhi = filter_thr + eps_max; break;
        default: break;
    }
    return f;
}

struct ErrorModel {
    // what finalize_kernel takes (FinalParams): per query it certifies against (eps_c + eps_r + its measured loss) x the norms
    float eps_c;      // accumulation term
    float eps_r;      // hi / int8: rows' share of the rounding loss (||q~|| <= (1 + u) ||q||); 0 otherwise
    float qrel_cap;   // hi / int8: the largest measured loss of a query the relaxed filter assumed (above it: not certified); 0 otherwise
    float eps_scale;  // 1, or what the test-only option eps_scale_ppm shrinks every term of the bound by
    float r_max;      // eps_r + the most any certified query adds
    // the bound over a whole batch (its largest query norm): what the relaxed filter is widened by.  Not finite = the level refuses
    float eps_max(uint32_t metric, float qn_max, float vn_max) const {  // vn_max: max_norm() of the store
        if (metric == OTT_METRIC_COSINE) return eps_c + r_max;
        if (metric == OTT_METRIC_DOT) return (eps_c + r_max) * vn_max * qn_max;
        return eps_c * (qn_max + vn_max) * (qn_max + vn_max) + 2.0f * r_max * qn_max * vn_max;
    }
};
// `plane_rel`: the measured rounding loss of the plane the level streams (hi_rel / i8_rel: max over the store's regular rows);
// `bf3`: level 1 runs on split-bf16 operands rather than the f32 matrix pipe.
inline ErrorModel error_model(int level, bool hi_f16, uint32_t dim, uint32_t metric, bool bf3, int eps_scale_ppm, float plane_rel) {
    const bool i8 = level_is_i8(level), hi = level_is_hi(level);
    const float u = 5.9604645e-8f;  // 2^-24
    // f32 pipe: recursive-summation bounds of both orders.  Split bf16: three products per element are accumulated (3*dim
    // terms), and each element's product loses at most 3 * 2^-16 (1 + 2^-8) of |q_i v_i| to the dropped lo*lo / residual terms
    // Hi pass: |q~.v~ - q.v| = |q~.(v~ - v) + (q~ - q).v| <= ||q~|| ||v~ - v|| + ||q~ - q|| ||v|| with both rounding losses MEASURED
    // (rows: plane_rel; queries: per query, added in finalize_kernel), plus the accumulation terms.
    // what the relaxed filter assumes of any query: the format's worst-case relative rounding loss (bf16 RNE 2^-8, half 2^-11)
    // int8: the queries share ONE scale per batch, so a query's loss depends on its largest element against the batch's; what the
    // relaxed filter assumes of any certified query is a measured loss of at most 2^-6 (uniform 768-d queries measure 4e-3)
    const float fmt_u = i8 ? 0.015625f : hi_f16 ? 4.8828125e-4f : 0.00390625f;
    const float qrel_cap = 1.01f * fmt_u;
    ErrorModel m;
    // test-only option eps_scale_ppm: every term of the bound shrunk on purpose, to show that a VIOLATED bound is noticed (the
    // measured |approximate - exact| / eps of the re-scored candidates exceeds 1) and the query falls through to the next level
    const float esc = eps_scale_ppm == 1000000 ? 1.0f : (float)eps_scale_ppm * 1e-6f;
    m.eps_scale = esc;
    m.eps_c = esc * (i8    ? (metric == OTT_METRIC_EUCLIDEAN ? (2.0f * (float)dim + 32.0f) * u  // (||v||^2 from the stored inverse norm: see below)
                                                            : i8_c_eps_units(dim) * u)
                     : hi  ? (2.5f * (float)dim + 32.0f) * u
                     : bf3 ? (3.75f * (float)dim + 32.0f) * u + 3.03f * 1.52587890625e-5f
                           : ((metric == OTT_METRIC_EUCLIDEAN ? 2.0f : 1.25f) * (float)dim + 32.0f) * u);
    // (squared L2 on the f32 pipe: besides the two summation orders, ||v||^2 comes from the stored inverse norm, whose
    //  sequential f32 sum carries up to dim * 2^-24 of relative error itself)
    m.eps_r = hi ? esc * (1.001f * (1.0f + fmt_u) * plane_rel) : 0.0f;
    m.r_max = hi ? m.eps_r + esc * (1.001f * qrel_cap) : 0.0f;
    m.qrel_cap = hi ? qrel_cap : 0.0f;
    return m;
}

// A query with a non-finite, astronomically large or vanishing (but non-zero) norm is outside the error model: no level certifies
// it, the exact path answers.  `qnorm`: the upper bound on ||q|| (query_norms)
inline bool query_regular(float qnorm) { return qnorm <= 1e18f && (qnorm == 0.0f || qnorm >= 1e-18f); }

// ---- query norms -----------------------------------------------------------------------------------------------------------------
// where the float sum of squares with its worst-case error as margin is a good enough ||q|| (outside it the squares underflow or
// overflow in f32: zero, tiny, huge, non-finite — the f64 sum is taken).  Not query_regular: that one is about the error model.
inline bool f32_norm_usable(float nrm) { return nrm >= 1e-15f && nrm <= 1e18f; }

// Norms of EIGHT queries at a time: the reference-order inverse norm is one dependent float add chain per query
// (src/vec.rs:387-397: sequential sum of squares, separate multiply and add — built with -ffp-contract=off,
// and the baseline x86-64 target has no fused multiply-add anyway), so eight independent chains keep the host core busy.
// The UPPER BOUND on ||q|| the error model needs comes from that same float sum with its worst-case error as margin
// (relative error of a sequential f32 sum of non-negative terms <= dim * 2^-24; of its root, half that); the f64 sum is
// taken only where it is needed: squared L2 (||q||^2 rides in the qinv slot) and queries whose float norm is outside
// [1e-15, 1e18] (the irregular ones).
// 1024 queries x 768 (a C4 shard's batch): the whole host prepare phase in front of the first launch 0.32-0.49 -> 0.18-0.24 ms
// (diagnostic build's host timers, benchmarks/hostprof.py); 256 queries 0.10 -> 0.06 ms.
// qnorm[nq], qinv[nq] (Euclidean: ||q||^2), qamax[nq] if want_amax (the largest |element| of every query: the int8 batch's ONE
// quantisation scale comes from them); returns the largest qnorm.
inline float query_norms(const float* queries, uint32_t nq, uint32_t dim, uint32_t metric, bool want_amax, float* qnorm, float* qinv, float* qamax) {
    constexpr uint32_t G = 8;
    const bool need_f64 = metric == OTT_METRIC_EUCLIDEAN;
    float qn_max = 0.f;
    for (uint32_t i0 = 0; i0 < nq; i0 += G) {
        const uint32_t g = nq - i0 < G ? nq - i0 : G;
        const float* v[G];
        float fs[G];
        double ds[G];
        for (uint32_t a = 0; a < G; a++) {
            v[a] = queries + (size_t)(i0 + (a < g ? a : 0)) * dim;  // (a short last group: the spare chains re-read its first query)
            fs[a] = 0.0f;
            ds[a] = 0.0;
        }
        for (uint32_t j = 0; j < dim; j++)
            for (uint32_t a = 0; a < G; a++) {
                const float x = v[a][j];
                const float sq = x * x;
                fs[a] = fs[a] + sq;
                if (need_f64) ds[a] += (double)x * x;  // (loop-invariant: the compiler makes two loops of it)
            }
        if (want_amax)
            for (uint32_t a = 0; a < g; a++) {
                float m = 0.0f;
                for (uint32_t j = 0; j < dim; j++) m = fmaxf(m, fabsf(v[a][j]));
                qamax[i0 + a] = m;
            }
        for (uint32_t a = 0; a < g; a++) {
            const uint32_t i = i0 + a;
            const float nrm = sqrtf(fs[a]);
            double nd;
            if (need_f64) nd = sqrt(ds[a]);
            else if (f32_norm_usable(nrm)) nd = (double)nrm * (1.0 + (double)dim * 5.9604644775390625e-8);
            else {
                double t = 0.0;
                for (uint32_t j = 0; j < dim; j++) t += (double)v[a][j] * (double)v[a][j];
                nd = sqrt(t);
                ds[a] = t;
            }
            qnorm[i] = (float)(nd * (1.0 + 1e-6));
            if (metric == OTT_METRIC_EUCLIDEAN) qinv[i] = (float)ds[a];  // ||q||^2 rides in the qinv slot
            else qinv[i] = nrm != 0.0f ? 1.0f / nrm : 0.0f;
            if (qnorm[i] > qn_max) qn_max = qnorm[i];
        }
    }
    return qn_max;
}

// ---- the query block -------------------------------------------------------------------------------------------------------------
// ONE input block, staged in pinned memory and uploaded with one copy: Q (zero padded) | qinv | qnorm | tau | cntA | cntB |
// overflow (zeros) | qrel | gate | runs | tile prefix | raw Q.  (Six copies and three memsets were ~50 us of blit kernels in
// front of every batch.)  Byte offsets; the one-query sweep uses it with one row and appends its int8 operand behind `total`.
constexpr size_t QB_CNT_STRIDE = 32;  // a query's list cursor has a 128-byte line of its own (ott_mfma.hip: CNT_STRIDE)
constexpr size_t QB_RUN_BYTES = 16;   // sizeof(ott_run)
struct QueryBlock {
    size_t q_bytes;  // of the operand block at offset 0 (and of the raw block)
    size_t qinv, qnorm, tau, cntA, cntB, over;
    size_t qrel;  // hi pass: measured rounding loss of each operand row
    size_t gate;  // emission threshold of the scoring rounds (select_kernel)
    size_t runs, prefix;
    size_t qraw;  // the raw queries, for the exact re-score: a block of their own where the operand block is not them, else offset 0
    size_t total;
};
inline QueryBlock query_block(uint32_t nq_pad, uint32_t ldq, size_t n_runs, size_t n_prefix, bool own_operand) {
    QueryBlock b;
    const size_t col = (size_t)nq_pad * 4, cnt = (size_t)nq_pad * QB_CNT_STRIDE * 4;
    b.q_bytes = (size_t)nq_pad * ldq * 4;
    b.qinv = b.q_bytes;
    b.qnorm = b.qinv + col;
    b.tau = b.qnorm + col;
    b.cntA = (b.tau + col + 127) & ~(size_t)127;
    b.cntB = b.cntA + cnt;
    b.over = b.cntB + cnt;
    b.qrel = b.over + col;
    b.gate = b.qrel + col;
    b.runs = (b.gate + col + 15) & ~(size_t)15;
    b.prefix = b.runs + n_runs * QB_RUN_BYTES;
    const size_t end = b.prefix + n_prefix * 4;
    b.qraw = own_operand ? (end + 127) & ~(size_t)127 : 0;
    b.total = own_operand ? b.qraw + b.q_bytes : end;
    return b;
}

}  // namespace ott
