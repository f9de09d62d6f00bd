// Stand-alone walk over the estimate that ranks the seed's rows in the pruned sweep's estimate pass (otters_amd/csrc/ott_prune.h:
// prune_score_est_sketchq) and over the plan's rule for that pass (ott_exact_plan.h: prune_plan_seed_est, prune_seed_keep), for the
// sanitizers (CPU only, its own main), in the manner of prune_head_walk.cpp and over its rows and queries: dims 225 .. 896, rows from
// subnormal to near-overflow scales, NaN / inf / signed zeros in stage 0, a stage 0 that dwarfs the tail, a row that is zero outside
// stage 0, queries that stress the quantiser.  Per row and query, cosine and dot: the estimate is NaN exactly where the head form's
// bound (prune_score_bound_sketchq at m = 0) is, and lies between the lower and the upper bound otherwise.
//   c++ -std=c++17 -O1 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I otters_amd/csrc tests/host/prune_seed_est_walk.cpp -o prune_seed_est_walk   (one command line), then ./prune_seed_est_walk
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ott_exact_plan.h"
#include "ott_prune.h"
using namespace ott;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni() {  // [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(rng_state >> 11) / (double)(1ll << 52) - 1.0;
}

// the line and the head of row v, K as the kernel forms it, then the estimate against the two bounds
static int walk_row(const std::vector<float>& q, const std::vector<float>& v, uint32_t dim, unsigned long long* sum, unsigned* n_est) {
    const uint32_t ld = (dim + 3) / 4 * 4, nst = (ld + 31) / 32;
    std::vector<uint32_t> line(prune_sketchb_pitch(nst - 1, 4));  // exactly the line and exactly four code words: a read or write past
    std::vector<uint32_t> codes(4);                               // either is the sanitizer's
    prune_sketchb_row(v.data(), dim, 32, nst - 1, 4, line.data());
    float rho_all;
    prune_sketch4_head_row(v.data(), dim, nst, line.data(), codes.data(), &rho_all);
    double qt, qn;
    PruneQuant x;
    if (!prune_query_bounds(q.data(), dim, 0, &qt, &qn) || !prune_query_quant(q.data(), dim, 0, &x)) return 0;  // (no head form for this query)
    std::vector<uint32_t> planes(12 * nst);
    for (uint32_t i = 0; i < 4 * nst; i++) {
        float q8[8];
        for (uint32_t j = 0; j < 8; j++) q8[j] = 8 * i + j < dim ? q[8 * i + j] : 0.0f;
        uint32_t d3[3];
        prune_quant_word(q8, x.inv_scale, d3);
        for (uint32_t d = 0; d < 3; d++) planes[(i >> 2) * 12 + d * 4 + (i & 3)] = d3[d];
    }
    int K[3] = {0, 0, 0};
    for (uint32_t s = 0; s < nst; s++) {
        const uint32_t* w = s ? line.data() + prune_sketchb_word0(4) + 4 * (s - 1) : codes.data();
        for (uint32_t i = 0; i < 4; i++)
            for (uint32_t d = 0; d < 3; d++) K[d] = prune_dot8_i4(w[i], planes[s * 12 + d * 4 + i], K[d]);
    }
    const int Kq = 2 * (256 * K[2] + 16 * K[1] + K[0]) + x.qsum;
    const float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double nv = 0.0;
    for (uint32_t i = 0; i < dim; i++) nv += (double)v[i] * (double)v[i];
    const float vinv = 1.0f / sqrtf((float)nv), qinv = (float)(1.0 / qn), a = prune_u2f(line[0]);
    for (int cosine = 0; cosine < 2; cosine++) {
        const float up = prune_score_bound_sketchq(acc, vinv, a, rho_all, Kq, x.scale, dim, qt, x.qe1, qn, qinv, cosine != 0, true);
        const float lo = prune_score_bound_sketchq(acc, vinv, a, rho_all, Kq, x.scale, dim, qt, x.qe1, qn, qinv, cosine != 0, false);
        const float est = prune_score_est_sketchq(vinv, a, rho_all, Kq, x.scale, qinv, cosine != 0);
        if ((est == est) != (up == up) || (est == est) != (lo == lo)) return 31;  // NaN exactly where the bound is
        if (est == est && !(lo <= est && est <= up)) return 32;                   // between the two bounds
        if (est == est) (*n_est)++;
        *sum += prune_f2u(est);
    }
    // the refusals on their own: a norm, a, rho or (cosine) a query norm that gives no bound gives no estimate
    const float bad[] = {(float)NAN, (float)INFINITY, 0.0f, 1e-30f, -1.0f};
    for (float b : bad) {
        const float e1 = prune_score_est_sketchq(b, a, rho_all, Kq, x.scale, qinv, true);
        if (e1 == e1) return 33;
        if (!(b == 0.0f || b == 1e-30f)) {  // (a = 0 and rho = 0 are lines like any other)
            const float e2 = prune_score_est_sketchq(vinv, b, rho_all, Kq, x.scale, qinv, false);
            const float e3 = prune_score_est_sketchq(vinv, a, b, Kq, x.scale, qinv, false);
            if (e2 == e2 || e3 == e3) return 34;
        }
        if (b != 1e-30f) {
            const float e4 = prune_score_est_sketchq(vinv, a, rho_all, Kq, x.scale, b, true);
            if (e4 == e4) return 35;
        }
    }
    return 0;
}

int main() {
    unsigned long long sum = 0;
    // the rule: the head form, one list entry per lane, no filter, a tenth of the rows at least 131 072 — and nothing else
    for (int head = 0; head < 2; head++)
        for (int E : {1, 2, 4, 8})
            for (int filtered = 0; filtered < 2; filtered++)
                for (int exact_prune : {-1, 0, 1})
                    for (uint64_t rows : {40320ull, 1310656ull, 1310719ull, 1310720ull, 1310784ull, 10000000ull}) {
                        const PruneIn in{768, 768, OTT_METRIC_COSINE, false, true, false, 0, exact_prune, 1, SketchState{true, true, 4, 92, 1}, rows, E};
                        const PrunePlan pp = prune_plan(in);
                        const bool on = OTT_X_SEED_EST && pp.c != 0 && head && E == 1 && !filtered && rows >= 1310720;
                        const uint64_t got = prune_plan_seed_est(in, pp, head != 0, filtered != 0);
                        if (got != (on ? pp.seed : 0)) return 2;
                        if (got != 0 && (got % 64 != 0 || got < 131072 || got >= rows)) return 3;
                    }
    for (uint64_t k : {1ull, 4ull, 10ull, 16ull, 17ull, 64ull})
        if (OTT_X_SEED_KEEP == 0 && prune_seed_keep(k) != (k < 16 ? (uint32_t)k : 16u)) return 4;
    unsigned n_est = 0;
    for (uint32_t dim : {225u, 256u, 768u, 773u, 896u}) {
        std::vector<std::vector<float>> queries, rows;
        for (int kind = 0; kind < 12; kind++) {
            std::vector<float> q(dim);
            for (auto& x : q) x = (float)uni();
            switch (kind) {
                case 1: q[37] = 0x1p20f; break;
                case 2: for (auto& x : q) x *= 1e-3f; q[3] = 1.0f; break;
                case 3: for (auto& x : q) x *= 1e-3f; q[dim - 2] = -1.0f; break;
                case 4: for (auto& x : q) x = floorf(x * 1800.0f) + 0.5f; q[1] = 1900.5f; break;
                case 5: for (uint32_t i = 32; i < dim; i++) q[i] = 0.0f; break;
                case 6: for (uint32_t i = 32; i < dim; i += 3) q[i] *= 1e-40f; break;
                case 7: for (auto& x : q) x *= 0x1p-126f; break;
                case 8: for (auto& x : q) x *= 0x1p-100f; break;
                case 9: for (auto& x : q) x *= 0x1p40f; break;
                case 10: for (auto& x : q) x *= 0x1p25f; q[41] = 0x1p50f * (1.0f - 0x1p-10f); break;
                case 11: q[5] = (float)NAN; break;
                default: break;
            }
            queries.push_back(q);
        }
        for (int kind = 0; kind < 21; kind++) {
            std::vector<float> v(dim);
            const float scales[] = {1.0f, 1e-20f, 1e-38f, 1e-42f, 1e15f, 1e19f};
            for (auto& x : v) x = (float)uni() * scales[kind % 6];
            switch (kind) {
                case 6: v[3] = (float)NAN; break;                                                       // stage 0
                case 7: v[0] = (float)INFINITY; break;
                case 8: v[31] = -(float)INFINITY; break;
                case 9: v[40] = (float)NAN; break;                                                      // the tail
                case 10: for (uint32_t i = 0; i < 32; i++) v[i] = (i & 1) ? 0.0f : -0.0f; break;
                case 11: for (auto& x : v) x = 0.0f; break;
                case 12: for (uint32_t i = 0; i < 32; i++) v[i] = 3e38f; break;                           // the sums leave the f32 range
                case 13: for (uint32_t i = 0; i < 32; i++) v[i] = (uni() < 0 ? -1.0f : 1.0f) * 1e6f; break;  // every code of the head clamps
                case 14: for (uint32_t i = 32; i < dim; i++) v[i] = 0.0f; break;                          // zero outside stage 0
                case 15: for (uint32_t i = 32; i < dim; i++) v[i] = -0.0f; break;
                case 16: for (auto& x : v) x = (uni() < 0 ? -1.0f : 1.0f) * 0.999f; break;                 // |kappa| = 15 throughout
                case 17: v[4] = 70.0f; v[39] = 40.0f; v[dim - 2] = -55.0f; break;
                case 18: for (auto& x : v) x = 3e38f * (float)uni(); break;
                case 19: for (uint32_t i = 0; i < 32; i++) v[i] *= 1e-30f; break;
                case 20:  // a decoy of the GPU test: one outlier makes the line coarse, every other dim is tiny along the query's signs
                    for (uint32_t i = 0; i < dim; i++) v[i] = (queries[0][i] < 0 ? -1.0f : 1.0f) * 1e-2f;
                    v[40] = 100.0f;
                    break;
                default: break;
            }
            rows.push_back(v);
        }
        for (const auto& q : queries)
            for (const auto& v : rows)
                if (const int rc = walk_row(q, v, dim, &sum, &n_est)) {
                    printf("walk_row: %d at dim %u\n", rc, dim);
                    return rc;
                }
    }
    if (n_est < 500) return 5;  // (the walk is not vacuous: the rows of ordinary scale have an estimate for every query the quantiser accepts)
    printf("prune_seed_est_walk ok %llx, %u estimates\n", sum, n_est);
    return 0;
}
