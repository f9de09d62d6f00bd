// Stand-alone walk over otters_amd/csrc/ott_sort_plan.h on exactly-sized heap blocks, for the sanitizers (CPU only, its own main):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I otters_amd/csrc tests/host/sort_plan_walk.cpp -o sort_plan_walk   (one command line), then ./sort_plan_walk
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "ott_sort_plan.h"
using namespace ott;

int main() {
    const uint32_t nqs[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 255, 256, 257, 1024, 1025, 1u << 20, 0xFFFFFFFFu};
    const uint64_t rowmax[] = {0, 1, 2, 7, 8, 255, 256, 65535, 65536, (1ull << 24) - 1, 1ull << 31, (1ull << 32) - 1, (1ull << 32) + 5, ~0ull};
    unsigned long long sum = 0;
    for (uint32_t nq : nqs)
        for (uint64_t rm : rowmax)
            for (uint32_t tie_sh : {0u, 3u})
                for (int order = 0; order < 4; order++) {
                    std::unique_ptr<RsPlan> plan(new RsPlan);  // exactly sized: a seventeenth pass would be written past the block
                    if (!sort_order_plan((SortOrder)order, row_bits(rm), query_bits(nq), tie_sh, 0, *plan)) return 1;
                    if (plan->n_pass > (uint32_t)RS_MAXP) return 2;
                    for (uint32_t i = 0; i < plan->n_pass; i++) sum += plan->pass[i].mask + plan->pass[i].shift;
                }
    {  // a plan filled to the brim, then one more digit
        std::unique_ptr<RsPlan> plan(new RsPlan());
        if (!rs_add_digits(*plan, 0, 0, 64, true) || !rs_add_digits(*plan, 1, 0, 32, false) || !rs_add_digits(*plan, 0, 0, 32, true)) return 3;
        if (rs_add_digits(*plan, 1, 0, 9, false) || plan->n_pass != 16) return 4;
    }
    for (uint32_t nq : nqs)
        for (uint32_t tiles : {0u, 1u, 1024u, 1025u, 0xFFFFFFFFu})
            for (int es : {-1, 0, 1, 2}) {
                const SweepShape w = sweep_shape(nq, 2048, tiles, es);
                sum += w.tile + w.passes + sort_bytes_scanned(w.passes, 1ull << 29, 4096, OTT_METRIC_COSINE);
            }
    for (uint64_t rows : {(uint64_t)0, (uint64_t)1, (uint64_t)4095, (uint64_t)16384, (uint64_t)16385, (uint64_t)65536, (uint64_t)90000, (uint64_t)10000000, (uint64_t)1 << 29, (uint64_t)1 << 40})
        for (uint32_t nq : {1u, 3u, 16u, 0xFFFFFFFFu})
            for (uint64_t k : {(uint64_t)0, (uint64_t)513, (uint64_t)600, (uint64_t)3000, rows / 16, rows, ~(uint64_t)0})
                for (int f = 0; f < 8; f++) sum += prefix_rows(rows, nq, f & 1, k, f & 2, f & 4);
    for (uint32_t nq : nqs) sum += slice_rows(nq, 1ull << 14) + slice_rows(nq, 1ull << 29);
    for (uint64_t cap : {0ull, 1ull, 700ull, 16384ull})
        for (uint32_t nq : {1u, 23u, 1024u}) {
            const SmallCtl c = small_ctl_layout(cap, nq);
            char* blk = (char*)malloc(c.total);  // every field at its offset, the last byte of the block included
            memset(blk + c.cursor, 1, 8);
            memset(blk + c.ticket, 2, 64 * 4);
            memset(blk + c.rank, 3, cap * 4);
            memset(blk + c.hist, 4, (size_t)nq * 4);
            sum += (unsigned char)blk[c.total - 1] + small_path_ok(cap, nq, nq > 1, 14, query_bits(nq), 1, false);
            free(blk);
        }
    for (uint32_t nq : {1u, 2u, 5u, 64u, 1025u})
        for (uint64_t k : {1ull, 40ull, 1ull << 40})
            for (int pattern = 0; pattern < 4; pattern++) {
                std::vector<uint32_t> start(nq);
                const uint64_t n = 100ull * nq;
                for (uint32_t q = 0; q < nq; q++) start[q] = (pattern == 1 && q % 2) || (pattern == 2 && q + 1 < nq) || (pattern == 3) ? 0xFFFFFFFFu : 100u * q;
                if (pattern == 2 && nq > 1) start[nq - 1] = 0;
                std::vector<uint64_t> first, count;
                const uint64_t total = group_extents(start, pattern == 3 ? 0 : n, k, first, count);
                uint64_t s2 = 0;
                for (uint32_t q = 0; q < nq; q++) {
                    if (first[q] + count[q] > n) return 5;
                    s2 += count[q];
                }
                if (s2 != total) return 6;
                for (uint64_t piece : {(uint64_t)COPY_PIECE, (uint64_t)7, (uint64_t)1}) {
                    if (total / piece > 100000) continue;
                    const std::vector<CopyPiece> pc = copy_pieces(count, piece);
                    std::vector<char> dst((size_t)total);  // the pieces tile [0, total) exactly
                    uint64_t at = 0;
                    for (const CopyPiece& p : pc) {
                        if (p.src != at || p.at + p.n > count[p.g]) return 7;
                        memset(dst.data() + p.src, 1, (size_t)p.n);
                        at += p.n;
                    }
                    if (at != total) return 8;
                }
            }
    {
        std::vector<uint64_t> count = {0, 1, COPY_PIECE, COPY_PIECE + 1, 3 * COPY_PIECE};
        if (copy_pieces(count, COPY_PIECE).size() != 7) return 9;
    }
    sum += rs_tmp_bytes(0) + rs_tmp_bytes(1ull << 30) + rs_tiles(4097);
    printf("sort_plan_walk ok (%llu)\n", sum);
    return 0;
}
