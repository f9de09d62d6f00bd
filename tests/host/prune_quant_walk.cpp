// Stand-alone walk over the integer decode of otters_amd/csrc/ott_prune.h for the sanitizers (CPU only, its own main): the quantiser,
// the digit planes, the nibble-wise dot products and prune_score_bound_sketchq over the cases of
// tests/test_exact_prune_sketchq_bound.py — dims 225 .. 896, rows from subnormal to near-overflow scales with NaN, inf and signed
// zeros, queries that stress the quantiser, the plan's rule where it refuses:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I otters_amd/csrc tests/host/prune_quant_walk.cpp -o prune_quant_walk   (one command line), then ./prune_quant_walk
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

// the bound of row v for query q at the four-bit form's checkpoint (dim 32), upper and lower; the exact dot product must lie between
static int walk_row(const std::vector<float>& q, const std::vector<float>& v, uint32_t dim, unsigned long long* sum) {
    const uint32_t ld = (dim + 3) / 4 * 4, nst = (ld + 31) / 32, first = 32, m = 32;
    std::vector<uint32_t> line(prune_sketchb_pitch(nst - 1, 4));  // exactly the line: a read or write past it is the sanitizer's
    prune_sketchb_row(v.data(), dim, first, nst - 1, 4, line.data());
    double qt, qn;
    PruneQuant x;
    if (!prune_query_bounds(q.data(), dim, m, &qt, &qn) || !prune_query_quant(q.data(), dim, m, &x)) return 0;
    std::vector<uint32_t> planes(12 * nst);
    int64_t direct = 0;
    for (uint32_t i = 0; i < 4 * nst; i++) {
        float q8[8];
        for (uint32_t j = 0; j < 8; j++) q8[j] = 8 * i + j < dim ? q[8 * i + j] : 0.0f;
        uint32_t d3[3];
        prune_quant_word(q8, x.inv_scale, d3);
        for (uint32_t d = 0; d < 3; d++) planes[(i >> 2) * 12 + d * 4 + (i & 3)] = d3[d];
    }
    int K[3] = {0, 0, 0};
    for (uint32_t s = 1; s < nst; s++) {
        const uint32_t* w = line.data() + prune_sketchb_word0(4) + 4 * (s - 1);
        for (uint32_t i = 0; i < 4; i++)
            for (uint32_t d = 0; d < 3; d++) K[d] = prune_dot8_i4(w[i], planes[s * 12 + d * 4 + i], K[d]);
        for (uint32_t b = 0; b < 32 && 32 * s + b < dim; b++) {
            const int32_t h = prune_quant_q(q[32 * s + b], x.inv_scale);
            int32_t dg[3];
            prune_quant_digits(h, dg);
            if (h < -PRUNE_QHAT_MAX || h > PRUNE_QHAT_MAX || 256 * dg[2] + 16 * dg[1] + dg[0] != h) return 10;
            for (int k = 0; k < 3; k++)
                if (dg[k] < -8 || dg[k] > 7) return 11;
            direct += (int64_t)h * (2 * prune_sketchb_code(w, b, 4) + 1);
        }
    }
    const int Kq = 2 * (256 * K[2] + 16 * K[1] + K[0]) + x.qsum;
    if ((int64_t)Kq != direct) return 12;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t c = 0; c < m; c += 8)
        for (int l = 0; l < 8; l++) {
            volatile float prod = q[c + l] * v[c + l];
            acc[l] = acc[l] + prod;
        }
    double nv = 0.0, dot = 0.0;
    for (uint32_t i = 0; i < dim; i++) {
        nv += (double)v[i] * (double)v[i];
        dot += (double)q[i] * (double)v[i];
    }
    const float vinv = 1.0f / sqrtf((float)nv);
    for (int cosine = 0; cosine < 2; cosine++) {
        const float up = prune_score_bound_sketchq(acc, vinv, prune_u2f(line[0]), prune_u2f(line[1]), Kq, x.scale, dim, qt, x.qe1, qn, (float)(1.0 / qn), cosine != 0, true);
        const float lo = prune_score_bound_sketchq(acc, vinv, prune_u2f(line[0]), prune_u2f(line[1]), Kq, x.scale, dim, qt, x.qe1, qn, (float)(1.0 / qn), cosine != 0, false);
        if ((up == up) != (lo == lo)) return 13;
        if (up == up && !cosine && !((double)lo <= dot && dot <= (double)up)) return 14;  // (the real dot product: inside the bound of the f32 score too)
        if (up == up && lo > up) return 15;
        *sum += prune_f2u(up) ^ prune_f2u(lo);
    }
    return 0;
}

int main() {
    unsigned long long sum = 0;
    // every qhat has its digits; the quantiser on a grid of products, NaN and the infinities included
    for (int32_t h = -PRUNE_QHAT_MAX; h <= PRUNE_QHAT_MAX; h++) {
        int32_t d[3];
        prune_quant_digits(h, d);
        if (256 * d[2] + 16 * d[1] + d[0] != h || d[0] < -8 || d[0] > 7 || d[1] < -8 || d[1] > 7 || d[2] < -8 || d[2] > 7) return 1;
    }
    for (float x : {0.0f, -0.0f, 0.5f, 1.5f, -2.5f, 1911.4f, 1911.6f, -1e30f, 3.4e38f, 1e-45f, (float)NAN, (float)INFINITY, -(float)INFINITY})
        for (float s : {1.0f, 0x1p-126f, 0x1p126f, 0x1p-20f}) {
            const int32_t h = prune_quant_q(x, s);
            if (h < -PRUNE_QHAT_MAX || h > PRUNE_QHAT_MAX) return 2;
            sum += (unsigned)h;
        }
    // the extremes of the i32 sums: all codes -8 / 7 against all digits -8 / 7 over 896 dims
    for (uint32_t a : {0x88888888u, 0x77777777u})
        for (uint32_t b : {0x88888888u, 0x77777777u}) {
            int32_t k = 0;
            for (int i = 0; i < 4 * 28; i++) k = prune_dot8_i4(a, b, k);
            const int ca = a == 0x88888888u ? -8 : 7, cb = b == 0x88888888u ? -8 : 7;
            if (k != 896 * ca * cb) return 3;
        }
    // rows x queries
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
                case 11: q[dim - 1] = (float)NAN; break;
                default: break;
            }
            queries.push_back(q);
        }
        for (int kind = 0; kind < 14; kind++) {
            std::vector<float> v(dim);
            const float scales[] = {1.0f, 1e-20f, 1e-38f, 1e-42f, 1e15f, 1e19f};
            for (auto& x : v) x = (float)uni() * scales[kind % 6];
            switch (kind) {
                case 6: v[40] = (float)NAN; break;
                case 7: v[dim - 1] = (float)INFINITY; break;
                case 8: for (uint32_t i = 32; i < dim; i++) v[i] = (i & 1) ? 0.0f : -0.0f; break;
                case 9: for (auto& x : v) x = 0.0f; break;
                case 10: for (uint32_t i = 0; i < 32; i++) v[i] = 3e38f; break;
                case 11: for (uint32_t i = 32; i < dim; i++) v[i] = (uni() < 0 ? -1.0f : 1.0f) * 0.999f; break;  // |kappa| = 15 throughout
                case 12: v[39] = 40.0f; v[dim - 2] = -55.0f; break;
                case 13: for (auto& x : v) x = 3e38f * (float)uni(); break;
                default: break;
            }
            rows.push_back(v);
        }
        for (const auto& q : queries) {
            // the plan: the four-bit form exactly where the quantiser accepts
            const uint32_t ld = (dim + 3) / 4 * 4, nst = (ld + 31) / 32;
            const PruneIn in{dim, ld, OTT_METRIC_COSINE, false, true, false, 0, 1, 1, SketchState{true, true, 4, 4 * (nst - 1), prune_sketchb_stage0(nst, 4)}, 1ull << 21, 1};
            PrunePlan pp = prune_plan(in);
            PruneQuant x;
            if (!prune_plan_needs_quant(in, pp)) return 4;
            const bool ok = prune_query_quant(q.data(), dim, pp.c * 32, &x);
            if (!ok) pp = prune_plan_quant_refused(in);
            if (ok != pp.sketch || (ok && pp.c != 1) || (!ok && pp.c != nst * 7 / 8)) return 5;
            if (ok && !(x.scale * x.inv_scale == 1.0f && x.qe1 >= 0.0 && fabs((double)x.qsum) <= 1911.0 * dim)) return 6;
            for (const auto& v : rows)
                if (const int rc = walk_row(q, v, dim, &sum)) {
                    printf("walk_row: %d at dim %u\n", rc, dim);
                    return rc;
                }
        }
    }
    printf("prune_quant_walk ok %llx\n", sum);
    return 0;
}
