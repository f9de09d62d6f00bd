// Stand-alone walk over the index arithmetic of the pruned exact sweep's narrow finish (otters_amd/csrc/ott_finish_few.h; the
// kernel side is ott_exact.hip: pq_finish_few) for the sanitizers (CPU only, its own main).  It plays a wave — 64 lanes, eight load
// instructions per round, an 8-KB stage buffer — for n = 1 .. 16 queued rows, pstage 0 and 1 and every ld from 1 to 896, with the n
// rows as SEPARATE heap buffers of exactly ld floats, so that a load outside a row's own bytes is the sanitizer's:
//   c++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I otters_amd/csrc tests/host/finish_few_walk.cpp -o finish_few_walk   (one command line), then ./finish_few_walk
// Checked per (n, pstage, ld): every (row < n, stage, 16-B slot) of a round is stored exactly once and read by its lane from where it
// was stored; a lane consumes its stages in ascending order, each of pstage .. nstages - 1 exactly once; every load starts inside
// [0, ld) of one of the n rows (the store's ld is a multiple of four floats, so a 16-B piece that starts inside ends inside; an ld
// that is not is walked with the piece cut at ld); a clamped stage is never consumed; and what the lane reads is the row's own
// value, or zero past ld.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ott_finish_few.h"
using namespace ott;

static int fail(const char* what, uint32_t n, uint32_t pstage, uint32_t ld) {
    printf("FAIL %s: n %u pstage %u ld %u\n", what, n, pstage, ld);
    return 1;
}

// the value element c of queued row i holds: never zero, distinct per (row, column)
static float val(uint32_t i, uint32_t c) { return (float)(1 + i * 1024 + c); }

static int walk(uint32_t n, uint32_t pstage, uint32_t ld, unsigned long long* loads, unsigned long long* consumed) {
    const uint32_t nstages = (ld + FF_KC - 1) / FF_KC;
    if (pstage >= nstages) return 0;  // (no stage behind the checkpoint: the sweep has no such plan)
    std::vector<std::unique_ptr<float[]>> rows;
    for (uint32_t i = 0; i < n; i++) {
        rows.emplace_back(new float[ld]);
        for (uint32_t c = 0; c < ld; c++) rows[i][c] = val(i, c);
    }
    const uint32_t G = ff_groups(n), S = ff_stages(n);
    if (G * S != 8 || 8 * G < n) return fail("groups and stages", n, pstage, ld);
    std::vector<float> st(64 * FF_KC);
    std::vector<int> stamp(64 * FF_KC / 4);  // per 16-B slot of the buffer: (stage + 1) * 64 + row + 1 of what was stored, 0 = zero-filled filler
    std::vector<uint32_t> next_stage(n, pstage);
    const uint32_t rounds = ff_rounds(n, pstage, nstages);
    for (uint32_t r = 0; r < rounds; r++) {
        std::fill(stamp.begin(), stamp.end(), -1);
        std::vector<int> stored(n * S * 8, 0);
        for (uint32_t m = 0; m < 8; m++) {
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t lrow = lane >> 3, lslot = lane & 7;
                const uint32_t j = ff_load_slab(m, n), g = ff_load_group(m, n);
                if (j >= S || g >= G) return fail("slab or group out of range", n, pstage, ld);
                const uint32_t i = ff_load_row(m, n, lrow);
                const bool rok = i < n;
                const uint32_t s = ff_stage(n, pstage, r, j), sc = ff_stage_clamp(s, nstages);
                if (sc >= nstages) return fail("clamped stage outside the row", n, pstage, ld);
                const uint32_t off = ff_slot_off(lslot, ld) + ff_col_off(sc, lslot, ld);
                if (off >= ld) return fail("load offset outside [0, ld)", n, pstage, ld);
                // the load: up to four floats from the row's own buffer (ASan holds every one of them to the allocation)
                const float* src = rows[rok ? i : 0].get() + off;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                for (uint32_t c = 0; c < 4 && off + c < ld; c++) v[c] = src[c];
                (*loads)++;
                const bool ok = rok && ff_col_ok(s, lslot, ld);
                const uint32_t at = ff_store_off(m, lrow, lslot);
                if (at % 4 || at + 4 > 64 * FF_KC) return fail("store outside the stage buffer", n, pstage, ld);
                if (stamp[at / 4] != -1) return fail("two pieces stored to one slot in a round", n, pstage, ld);
                for (uint32_t c = 0; c < 4; c++) st[at + c] = ok ? v[c] : 0.f;
                stamp[at / 4] = ok ? (int)((s + 1) * 64 + i + 1) : 0;
                if (ok) {
                    if (s >= nstages) return fail("a clamped stage stored as data", n, pstage, ld);
                    if (off != s * FF_KC + lslot * 4) return fail("a row's piece loaded from the wrong offset", n, pstage, ld);
                    stored[(i * S + j) * 8 + lslot]++;
                }
            }
        }
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = 0; j < S; j++)
                for (uint32_t sl = 0; sl < 8; sl++) {
                    const uint32_t s = ff_stage(n, pstage, r, j);
                    const int want = (s < nstages && s * FF_KC + sl * 4 < ld) ? 1 : 0;
                    if (stored[(i * S + j) * 8 + sl] != want) return fail("a (row, stage, slot) not stored exactly once", n, pstage, ld);
                }
        // consumption: every lane, its row of slab 0, 1, .. while the stage exists (lanes past n walk a slab row too and are not offered)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t li = lane & (8 * G - 1);
            for (uint32_t j = 0; j < S && ff_stage(n, pstage, r, j) < nstages; j++) {
                const uint32_t s = ff_stage(n, pstage, r, j);
                if (ff_stage_clamp(s, nstages) != s) return fail("a clamped stage consumed", n, pstage, ld);
                if (lane < n) {
                    if (s != next_stage[lane]) return fail("stages not consumed in ascending order, each once", n, pstage, ld);
                    next_stage[lane] = s + 1;
                }
                for (uint32_t sl = 0; sl < 8; sl++) {
                    const uint32_t at = ff_read_off(li, n, j, sl);
                    if (at % 4 || at + 4 > 64 * FF_KC) return fail("read outside the stage buffer", n, pstage, ld);
                    if (lane >= n) continue;
                    const bool data = s * FF_KC + sl * 4 < ld;
                    if (stamp[at / 4] != (data ? (int)((s + 1) * 64 + lane + 1) : 0)) return fail("a lane reads what was not stored for it", n, pstage, ld);
                    for (uint32_t c = 0; c < 4; c++) {
                        const uint32_t col = s * FF_KC + sl * 4 + c;
                        if (st[at + c] != (col < ld ? val(lane, col) : 0.f)) return fail("a lane reads another value than its row's", n, pstage, ld);
                    }
                    (*consumed)++;
                }
            }
        }
    }
    for (uint32_t i = 0; i < n; i++)
        if (next_stage[i] != nstages) return fail("a row's stages not all consumed", n, pstage, ld);
    return 0;
}

int main() {
    unsigned long long loads = 0, consumed = 0, cases = 0;
    for (uint32_t n = 1; n <= FF_MAX_ROWS; n++)
        for (uint32_t pstage = 0; pstage < 2; pstage++)
            for (uint32_t ld = 1; ld <= 896; ld++) {
                if (walk(n, pstage, ld, &loads, &consumed)) return 1;
                cases++;
            }
    printf("finish_few_walk ok: %llu cases, %llu loads, %llu pieces consumed\n", cases, loads, consumed);
    return 0;
}
