// Stand-alone walk over otters_amd/csrc/ott_exact_plan.h for the sanitizers (CPU only, its own main): the grids of
// tests/test_exact_plan_cpu.py, and a result block of exactly the planned size written at the planned offsets:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I otters_amd/csrc tests/host/exact_plan_walk.cpp -o exact_plan_walk   (one command line), then ./exact_plan_walk
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ott_exact_plan.h"
#include "ott_prune.h"
#include "ott_sort_plan.h"
using namespace ott;

int main() {
    unsigned long long sum = 0;
    const uint64_t ks[] = {1, 16, 17, 64, 65, 128, 129, 256, 257, 512, 513, ~0ull};
    const uint32_t nqs[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 1000000};
    // lists or sort
    for (uint64_t k : ks)
        for (uint32_t nq : {1u, 2u, 4u, 5u, 0xFFFFFFFFu})
            for (uint64_t pairs : {1ull << 19, 1ull << 28})
                for (int d = -1; d <= 1; d++)
                    for (int from : {0, 1, 128, 512, -1})
                        for (int fetch = 0; fetch < 2; fetch++) {
                            const ExactRoute r = lists_or_sort(k, nq, pairs / nq + d, from, fetch != 0);
                            if (k > 512 && r == EXACT_LISTS) return 1;
                            if (!fetch && r == EXACT_SORT) return 2;
                            sum += r;
                        }
    // variant, passes, grid, block lists; the block lists and the result block written whole, at the planned offsets
    for (int es : {-1, 0, 1, 2, 3})
        for (uint32_t nq : nqs)
            for (int perq = 0; perq < 2; perq++)
                for (uint64_t k : {10ull, 100ull, 200ull, 300ull})
                    for (uint32_t dimq : {8u, 896u, 904u, 2048u, 2052u})
                        for (uint32_t tiles : {0u, 1u, 79u, 1024u, 1025u, 0xFFFFFFFFu})
                            for (int stream_grid : {1, 512}) {
                                const ExactPlan x = exact_plan(k, nq, perq != 0, dimq, tiles, 2, es, stream_grid);
                                if (x.tile < 1 || x.tile > 8 || (uint64_t)x.passes * x.tile < nq || x.KS != 64u * (uint32_t)x.E || (x.variant && x.E > 2)) return 3;
                                if (x.variant == 1 && (nq != 1 || perq)) return 4;
                                if (x.grid != (x.variant ? (int)tiles : stream_grid)) return 5;
                                sum += exact_n_lists(x, nq, perq != 0, false, 0, 0) + exact_n_lists(x, nq, perq != 0, true, 3, 5) + x.lean;
                                if (nq > 17 || tiles > 1025) continue;
                                const uint32_t groups = perq ? nq : 1;
                                const ExactResult r = exact_result_layout(groups, x.KS);
                                char* blk = (char*)malloc(r.host_bytes);  // counts, pad, every group's KS hits, the tail counter: the last byte included
                                if (!blk) return 6;
                                memset(blk, 1, (size_t)groups * 8);
                                for (uint32_t g = 0; g < groups; g++) memset(blk + r.cnt_pad + (size_t)g * x.KS * sizeof(ott_hit), 2, (size_t)x.KS * sizeof(ott_hit));
                                memset(blk + r.bytes, 3, 8);
                                if (r.cnt_pad % 64 || r.cnt_pad < (size_t)groups * 8 || r.host_bytes != r.bytes + 8) return 7;
                                sum += (unsigned char)blk[r.host_bytes - 1] + (unsigned char)blk[r.cnt_pad];
                                free(blk);
                            }
    // the sort path's sweep and the policy's clause on the same predicate
    for (uint32_t nq : nqs)
        for (uint32_t tiles : {0u, 1024u, 1025u, 0xFFFFFFFFu})
            for (int es : {-1, 0, 1, 2}) {
                const SweepShape w = sweep_shape(nq, 2048, tiles, es);
                if (w.rows8 != (small_variant_fits(2048, tiles) && es != 0 && es != 1)) return 9;
                sum += w.passes + sort_bytes_scanned(w.passes, 1ull << 29, 4096, OTT_METRIC_COSINE) - exact_bytes_scanned(w.passes, 1ull << 29, 4096, OTT_METRIC_COSINE);
            }
    // the pruned sweep
    const uint32_t dims[] = {8, 31, 32, 33, 63, 64, 65, 224, 225, 256, 768, 896, 4096, 65536};
    const uint64_t rows[] = {0, 63, 64, 639, 640, 30080, (1ull << 20) - 1, 1ull << 20, 1310720 - 64, 1310720, 1310720 + 64, 4194304 - 32, 4194304 + 32, 10000000, 1ull << 40, ~0ull};
    for (uint32_t dim : dims) {
        const uint32_t ld = (dim + 3u) & ~3u, nst = (ld + 31) / 32;
        for (uint32_t bits : {0u, 1u, 3u, 4u})
            for (int wv = 0; wv < 3; wv++)
                for (int covers = 0; covers < 2; covers++)
                    for (int ep : {0, 1, -1})
                        for (int esk : {0, -1})
                            for (uint64_t r : rows)
                                for (int E : {1, 2, 4, 8})
                                    for (uint32_t metric = 0; metric < 4; metric++)
                                        for (int flags = 0; flags < 16; flags++) {
                                            const uint32_t st0 = bits ? prune_sketchb_stage0(nst, bits) : 0;
                                            const uint32_t lim = bits == 4 ? OTT_SKETCH4_MAX_WORDS : bits == 3 ? OTT_SKETCH_MAX_WORDS : OTT_SKETCH1_MAX_WORDS;
                                            const uint32_t words = wv == 0 ? (nst - st0) * bits : wv == 1 ? lim : lim + 1;
                                            const PruneIn in{dim, ld, metric, (flags & 1) != 0, (flags & 2) == 0, (flags & 4) != 0, (flags & 8) ? 2u : 0u, ep, esk,
                                                             SketchState{bits != 0, covers != 0, bits, words, st0}, r, E};
                                            const PrunePlan p = prune_plan(in);
                                            if (!p.c) continue;
                                            if (flags || ep == 0 || (metric != OTT_METRIC_COSINE && metric != OTT_METRIC_DOT)) return 10;
                                            if (p.c >= nst || 32 * p.c > dim - dim % 8 || p.seed % 64 || p.seed < 64) return 11;
                                            if (p.sketch && (p.c != st0 || !covers || !bits || words > lim || esk == 0)) return 12;
                                            sum += p.c + p.seed;
                                        }
    }
    for (uint32_t nq : nqs)
        for (uint32_t dimq : {8u, 896u, 904u})
            for (size_t n_runs : {(size_t)0, (size_t)2, (size_t)3, ~(size_t)0}) sum += exact_lean(nq, dimq, n_runs);
    printf("exact_plan_walk ok (%llu)\n", sum);
    return 0;
}
