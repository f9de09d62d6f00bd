// Stand-alone walk over the int8 check of the pruned exact sweep's survivors (otters_amd/csrc/ott_i8_check.h: i8_query_quant,
// i8_quant_word, i8_check_eps, i8_check_drops; ott_exact_plan.h: prune_plan_i8_check) for the sanitizers (CPU only, its own
// main), over the cases of tests/test_exact_i8_check_cpu.py: dims 8 .. 896 and their plane pitches, queries from subnormal to
// near-overflow scales with NaN / inf / signed zeros among them, rows quantised the way the plane's builder does, both metrics,
// both takes, gates on and around every row's own ordinal, and the rule's whole table:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I otters_amd/csrc tests/host/exact_i8_check_walk.cpp -o exact_i8_check_walk   (one command line), then ./exact_i8_check_walk
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ott_exact_plan.h"
#include "ott_i8_check.h"
using namespace ott;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni() {  // [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(rng_state >> 11) / (double)(1ll << 52) - 1.0;
}

// a row of the plane as i8_rows_kernel makes it: exactly ld8 bytes, zeros past dim; returns s_v and the measured loss
static float plane_row(const std::vector<float>& v, uint32_t dim, std::vector<int8_t>& out, double* rel) {
    float mx = 0.0f;
    for (uint32_t i = 0; i < dim; i++) mx = fmaxf(mx, fabsf(v[i]));
    float s = mx / 127.0f;
    if (!(s < __builtin_inff())) s = 0.0f;
    const float inv = s > 0.0f ? 1.0f / s : 0.0f;
    double se = 0.0, sx = 0.0;
    for (uint32_t i = 0; i < (uint32_t)out.size(); i++) {
        float t = i < dim ? rintf(v[i] * inv) : 0.0f;
        t = t == t ? fminf(fmaxf(t, -127.0f), 127.0f) : 0.0f;
        out[i] = (int8_t)(int)t;
        if (i < dim) {
            const double df = (double)v[i] - (double)s * (double)(int)t;
            se += df * df;
            sx += (double)v[i] * (double)v[i];
        }
    }
    *rel = sx > 0.0 ? sqrt(se / sx) : 0.0;
    return s;
}

static int walk(uint32_t dim, double qscale, double vscale, int special, unsigned long long* sum) {
    const uint32_t ld8 = (dim + 127u) & ~127u, nw = ld8 / 4;
    std::vector<float> q(dim);
    for (uint32_t i = 0; i < dim; i++) q[i] = (float)(uni() * qscale);
    if (special == 1) q[dim / 2] = NAN;
    if (special == 2) q[0] = INFINITY;
    if (special == 3) for (uint32_t i = 0; i < dim; i += 2) q[i] = -0.0f;
    if (special == 4) for (uint32_t i = 0; i < dim; i++) q[i] = 0.0f;
    double n2 = 0.0;
    for (uint32_t i = 0; i < dim; i++) n2 += (double)q[i] * q[i];
    const float q_inv = n2 > 0.0 && n2 < 1e300 ? (float)(1.0 / sqrt(n2)) : 0.0f;
    for (int cosine = 0; cosine < 2; cosine++) {
        std::vector<int8_t> q8(dim);  // exactly dim elements: a write past them is the sanitizer's
        const I8Query x = i8_query_quant(q.data(), dim, cosine != 0, q_inv, q8.data());
        const I8Query y = i8_query_quant(q.data(), dim, cosine != 0, q_inv, nullptr);
        if (x.s_q != y.s_q || x.qrel != y.qrel || x.regular != y.regular) return 10;
        if (!(x.s_q > 0.0f) || !(x.qrel >= 0.0f && x.qrel <= 1.0f)) return 11;
        // the kernel's word form over a whole plane row of the operand: the same bytes, zeros past dim
        std::vector<uint32_t> qw(nw);
        for (uint32_t i = 0; i < nw; i++) {
            float q4[4];
            for (uint32_t j = 0; j < 4; j++) q4[j] = 4 * i + j < dim ? q[4 * i + j] : 0.0f;
            qw[i] = i8_quant_word(q4, x.pf, x.inv_sq);
        }
        for (uint32_t c = 0; c < ld8; c++) {
            const int8_t b = (int8_t)((qw[c >> 2] >> (8 * (c & 3))) & 0xFFu);
            if (b != (c < dim ? q8[c] : 0) || b < -127) return 12;
        }
        // a few rows, their approximate scores and the rule at gates around them
        const uint32_t metric = cosine ? OTT_METRIC_COSINE : OTT_METRIC_DOT;
        for (int r = 0; r < 6; r++) {
            std::vector<float> v(dim);
            for (uint32_t i = 0; i < dim; i++) v[i] = (float)(uni() * vscale);
            if (r == 4) v[dim - 1] = NAN;
            if (r == 5) v[0] = (float)(vscale * 1e4);  // one huge element: the row loses more than 2^-5
            std::vector<int8_t> img(ld8);
            double rel;
            const float s_v = plane_row(v, dim, img, &rel);
            double nv = 0.0, dot = 0.0;
            for (uint32_t i = 0; i < dim; i++) {
                nv += (double)v[i] * v[i];
                dot += (double)q[i] * v[i];
            }
            const float vinv = nv > 0.0 ? (float)(1.0 / sqrt(nv)) : 0.0f;
            int acc = 0;
            for (uint32_t c = 0; c < ld8; c++) acc += (int)img[c] * (int)(int8_t)((qw[c >> 2] >> (8 * (c & 3))) & 0xFFu);
            const float approx = i8_approx_score(acc, i8_row_factor(cosine != 0, vinv, s_v, x.s_q));
            const bool outside = !(rel <= 0.03125) || !(nv == nv);
            const I8CheckEps e = i8_check_eps(dim, metric, 1000000, (float)(rel * 1.000001) + 1e-30f, x, nv > 0.0 ? (float)(sqrt(nv) * 1.000001) : 0.0f);
            const I8CheckEps none = i8_check_eps(dim, OTT_METRIC_EUCLIDEAN, 1000000, 0.004f, x, 1.0f);
            if (none.ok) return 13;
            if (!x.regular && e.ok) return 14;
            if (!e.ok) continue;
            if (!(e.eps >= 0.0f) || !(e.eps < INFINITY)) return 15;
            const double exact = cosine ? dot * (double)q_inv * (double)vinv : dot;
            for (int take_max = 0; take_max < 2; take_max++) {
                if (i8_check_drops(approx, e.eps, take_max != 0, 0u, outside)) return 16;           // an open gate
                if (i8_check_drops(approx, e.eps, take_max != 0, 0xFFFFFFFFu, true)) return 17;     // a row outside the error model
                if (!outside && exact == exact && fabs(exact) < 3e38 && approx - approx == 0.0f) {
                    // (the real score, not the exact-order one: it lies inside the bound too, by more than the eps_c units between them)
                    const uint32_t o = i8_check_ord((float)exact, take_max != 0);
                    for (uint32_t g = o > 2 ? o - 2 : 1; g <= o && g != 0; g++)
                        if (fabs((double)approx - exact) <= (double)e.eps && i8_check_drops(approx, e.eps, take_max != 0, g, false)) return 18;
                }
                *sum += i8_check_drops(approx, e.eps, take_max != 0, i8_check_ord(approx, take_max != 0), outside) ? 1 : 0;
            }
        }
    }
    return 0;
}

int main() {
    unsigned long long sum = 0;
    const uint32_t dims[] = {8, 29, 96, 127, 128, 129, 232, 256, 768, 773, 896};
    const double scales[] = {1e-30, 1e-6, 1.0, 1e6, 1e18};
    for (uint32_t dim : dims)
        for (double qs : scales)
            for (double vs : scales)
                for (int special = 0; special < 5; special++) {
                    const int rc = walk(dim, qs, vs, special, &sum);
                    if (rc) {
                        printf("FAIL %d: dim %u qscale %g vscale %g special %d\n", rc, dim, qs, vs, special);
                        return rc;
                    }
                }
    // the rule's table, whole
    PruneIn in{};
    int on = 0;
    for (uint32_t c = 0; c < 2; c++)
        for (int head = 0; head < 2; head++)
            for (int E : {1, 2, 4, 8})
                for (int ready = 0; ready < 2; ready++)
                    for (int opt = -1; opt <= 1; opt++)
                        for (int ok = 0; ok < 2; ok++) {
                            in.E = E;
                            const bool run = prune_plan_i8_check(in, PrunePlan{c, true, 64}, head != 0, I8CheckState{ready != 0, opt, ok != 0});
                            if (run != (OTT_X_I8_CHECK != 0 && c != 0 && head && E == 1 && ready && opt != 0 && ok)) return 30;
                            on += run;
                        }
    if (on != (OTT_X_I8_CHECK ? 2 : 0)) return 31;
    printf("exact_i8_check_walk ok (%llu)\n", sum);
    return 0;
}
