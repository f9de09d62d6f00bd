// Stand-alone walk over the head of the four-bit sketch (otters_amd/csrc/ott_prune.h: prune_sketch4_head_row) and the head form's
// bound — prune_score_bound_sketchq at m = 0 with an all-zero acc, rho_all and K over every stage — for the sanitizers (CPU only,
// its own main), over the cases of tests/test_exact_prune_head_bound.py: dims 225 .. 896, rows from subnormal to near-overflow
// scales, NaN / inf / signed zeros in stage 0, a stage 0 that dwarfs the tail, a row that is zero outside stage 0, queries that
// stress the quantiser, and the plan's rule (ott_exact_plan.h: prune_plan_head):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I otters_amd/csrc tests/host/prune_head_walk.cpp -o prune_head_walk   (one command line), then ./prune_head_walk
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

// the head of row v beside its line, then the head form's bound for query q, upper and lower; the exact dot product must lie between
static int walk_row(const std::vector<float>& q, const std::vector<float>& v, uint32_t dim, unsigned long long* sum) {
    const uint32_t ld = (dim + 3) / 4 * 4, nst = (ld + 31) / 32;
    std::vector<uint32_t> line(prune_sketchb_pitch(nst - 1, 4));  // exactly the line and exactly four code words: a read or write past
    std::vector<uint32_t> codes(4);                               // either is the sanitizer's
    prune_sketchb_row(v.data(), dim, 32, nst - 1, 4, line.data());
    const std::vector<uint32_t> before = line;
    float rho_all;
    prune_sketch4_head_row(v.data(), dim, nst, line.data(), codes.data(), &rho_all);
    if (line != before) return 20;  // the line is left as it is
    bool finite = true;
    double res = 0.0;
    const double a = (double)prune_u2f(line[0]);
    for (uint32_t i = 0; i < dim; i++) {
        if (!(v[i] - v[i] == 0.0f)) finite = false;
        const uint32_t* w = i < 32 ? codes.data() : line.data() + prune_sketchb_word0(4) + 4 * ((i - 32) >> 5);
        const double r = (double)v[i] - a * (2 * prune_sketchb_code(w, i & 31u, 4) + 1);
        res += r * r;
    }
    for (uint32_t i = dim; i < 32; i++)
        if (prune_sketchb_code(codes.data(), i, 4) != 0) return 21;  // code 0 past dim
    if (!finite && rho_all <= 3.4028234e38f) return 22;              // a non-finite value anywhere: no bound
    if (rho_all <= 3.4028234e38f && !((double)rho_all >= sqrt(res) * (1.0 - 0x1p-40))) return 23;
    if (!(prune_u2f(line[1]) <= 3.4028234e38f) && rho_all <= 3.4028234e38f) return 24;  // a line without a bound: a head without one

    double qt, qn;
    PruneQuant x;
    if (!prune_query_bounds(q.data(), dim, 0, &qt, &qn) || !prune_query_quant(q.data(), dim, 0, &x)) return 0;
    if (qt != qn) return 25;  // m = 0: the tail is the query
    std::vector<uint32_t> planes(12 * nst);
    for (uint32_t i = 0; i < 4 * nst; i++) {
        float q8[8];
        for (uint32_t j = 0; j < 8; j++) q8[j] = 8 * i + j < dim ? q[8 * i + j] : 0.0f;
        uint32_t d3[3];
        prune_quant_word(q8, x.inv_scale, d3);
        for (uint32_t d = 0; d < 3; d++) planes[(i >> 2) * 12 + d * 4 + (i & 3)] = d3[d];
    }
    int K[3] = {0, 0, 0};
    int64_t direct = 0;
    for (uint32_t s = 0; s < nst; s++) {
        const uint32_t* w = s ? line.data() + prune_sketchb_word0(4) + 4 * (s - 1) : codes.data();
        for (uint32_t i = 0; i < 4; i++)
            for (uint32_t d = 0; d < 3; d++) K[d] = prune_dot8_i4(w[i], planes[s * 12 + d * 4 + i], K[d]);
        for (uint32_t b = 0; b < 32 && 32 * s + b < dim; b++) direct += (int64_t)prune_quant_q(q[32 * s + b], x.inv_scale) * (2 * prune_sketchb_code(w, b, 4) + 1);
    }
    const int Kq = 2 * (256 * K[2] + 16 * K[1] + K[0]) + x.qsum;
    if ((int64_t)Kq != direct) return 26;
    const float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double nv = 0.0, dot = 0.0;
    for (uint32_t i = 0; i < dim; i++) {
        nv += (double)v[i] * (double)v[i];
        dot += (double)q[i] * (double)v[i];
    }
    const float vinv = 1.0f / sqrtf((float)nv);
    for (int cosine = 0; cosine < 2; cosine++) {
        const float up = prune_score_bound_sketchq(acc, vinv, prune_u2f(line[0]), rho_all, Kq, x.scale, dim, qt, x.qe1, qn, (float)(1.0 / qn), cosine != 0, true);
        const float lo = prune_score_bound_sketchq(acc, vinv, prune_u2f(line[0]), rho_all, Kq, x.scale, dim, qt, x.qe1, qn, (float)(1.0 / qn), cosine != 0, false);
        if ((up == up) != (lo == lo)) return 27;
        if (up == up && !finite) return 28;
        if (up == up && !cosine && !((double)lo <= dot && dot <= (double)up)) return 29;  // (the real dot product: inside the bound of the f32 score too)
        if (up == up && lo > up) return 30;
        *sum += prune_f2u(up) ^ prune_f2u(lo);
    }
    return 0;
}

int main() {
    unsigned long long sum = 0;
    // the plan's rule: the four-bit plan, the quantiser's yes, a head for every row, the option not 0 — and nothing else
    for (uint32_t bits : {1u, 3u, 4u})
        for (int present = 0; present < 2; present++)
            for (int covers = 0; covers < 2; covers++)
                for (int option = -1; option <= 1; option++)
                    for (int quant_ok = 0; quant_ok < 2; quant_ok++) {
                        const uint32_t nst = 24;
                        const PruneIn in{768, 768, OTT_METRIC_COSINE, false, true, false, 0, 1, 1,
                                         SketchState{true, true, bits, bits * (nst - prune_sketchb_stage0(nst, bits)), prune_sketchb_stage0(nst, bits)}, 1ull << 21, 1};
                        const PrunePlan pp = prune_plan(in);
                        const bool want = bits == 4 && present && covers && option != 0 && quant_ok;
                        if (prune_plan_head(in, pp, quant_ok != 0, HeadState{present != 0, covers != 0, option}) != want) return 1;
                    }
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
        for (int kind = 0; kind < 20; kind++) {
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
                default: break;
            }
            rows.push_back(v);
        }
        for (const auto& q : queries)
            for (const auto& v : rows)
                if (const int rc = walk_row(q, v, dim, &sum)) {
                    printf("walk_row: %d at dim %u\n", rc, dim);
                    return rc;
                }
    }
    printf("prune_head_walk ok %llx\n", sum);
    return 0;
}
