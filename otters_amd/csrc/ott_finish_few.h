// ott_finish_few.h — the index arithmetic of the pruned exact sweep's narrow finish (ott_exact.hip: pq_finish_few; DESIGN.md 3.1b,
// "a few queued rows").  Host and device code with no other header behind it, so that the CPU suite can walk it on its own
// (tests/host/finish_few_walk.cpp, tests/test_exact_finish_few_cpu.py).
//
// pq_finish finishes n queued rows as one dense tile of 64: per 128-B stage eight wave instructions of 8 rows x 128 B, every
// group of eight rows past n re-reading the first queued row, and the next stage asked for only when this one has arrived.  With
// n <= 16 the same eight instructions and the same 8-KB stage buffer hold SEVERAL stages of the n rows at once: G = 1 row group
// of eight for n <= 8, G = 2 for n <= 16, so S = 8 / G stages per round.  Instruction m of a round loads row group m % G of
// the round's stage m / G; its 8 x 128 B land where pq_finish puts instruction m's — row 8 m + lrow of the stage buffer, 16-B
// slots XOR-swizzled by that row — which makes the buffer S slabs of 8 G rows, slab j = the round's stage j.  Lane i < n then
// walks row i of slab 0, 1, .. in stage order.  A stage past the row's last is clamped to the last one (the bytes are the row's
// own) and never consumed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OTT_FF_HD __host__ __device__
#else
#define OTT_FF_HD
#endif

namespace ott {

constexpr uint32_t FF_MAX_ROWS = 16;  // the most rows the narrow finish takes
constexpr uint32_t FF_KC = 32;        // floats of a row per stage: one 128-B line (ott_exact.hip: KC)

// row groups of eight per stage, and the stages one round holds
OTT_FF_HD inline uint32_t ff_gshift(uint32_t n) { return n <= 8 ? 0u : 1u; }  // log2 G
OTT_FF_HD inline uint32_t ff_groups(uint32_t n) { return 1u << ff_gshift(n); }
OTT_FF_HD inline uint32_t ff_stages(uint32_t n) { return 8u >> ff_gshift(n); }
// rounds that cover stages pstage .. nstages - 1
OTT_FF_HD inline uint32_t ff_rounds(uint32_t n, uint32_t pstage, uint32_t nstages) {
    const uint32_t S = ff_stages(n);
    return nstages > pstage ? (nstages - pstage + S - 1) / S : 0u;
}
// what instruction m = 0 .. 7 of a round loads: the round's stage j (slab j) and the row group
OTT_FF_HD inline uint32_t ff_load_slab(uint32_t m, uint32_t n) { return m >> ff_gshift(n); }
OTT_FF_HD inline uint32_t ff_load_group(uint32_t m, uint32_t n) { return m & (ff_groups(n) - 1u); }
// the queued row a lane of instruction m loads for (lrow = lane / 8); a row past n re-reads the first queued row and is zero-filled
OTT_FF_HD inline uint32_t ff_load_row(uint32_t m, uint32_t n, uint32_t lrow) { return 8u * ff_load_group(m, n) + lrow; }
// stage s of round r, slab j; clamped for the load
OTT_FF_HD inline uint32_t ff_stage(uint32_t n, uint32_t pstage, uint32_t r, uint32_t j) { return pstage + r * ff_stages(n) + j; }
OTT_FF_HD inline uint32_t ff_stage_clamp(uint32_t s, uint32_t nstages) { return s < nstages ? s : nstages - 1u; }
// float offset inside a row of the 16-B piece a lane loads (lslot = lane % 8) at the clamped stage sc.  A slot past a short row's
// end (ld < 29) reads slot 0, a piece past ld the same slot of stage 0 — pq_finish's own clamps: every byte is the row's own
OTT_FF_HD inline uint32_t ff_slot_off(uint32_t lslot, uint32_t ld) { return lslot * 4u < ld ? lslot * 4u : 0u; }
OTT_FF_HD inline uint32_t ff_col_off(uint32_t sc, uint32_t lslot, uint32_t ld) { return sc * FF_KC + lslot * 4u < ld ? sc * FF_KC : 0u; }
// whether the piece is the row's data at the UNCLAMPED stage s (the zero-fill rule's column half; the row half is row < n)
OTT_FF_HD inline bool ff_col_ok(uint32_t s, uint32_t lslot, uint32_t ld) { return s * FF_KC + lslot * 4u < ld; }
// float offset in the wave's stage buffer: a 16-B slot of a row of 32 floats, swizzled by the buffer row
OTT_FF_HD inline uint32_t ff_buf_off(uint32_t brow, uint32_t slot) { return brow * FF_KC + ((slot ^ ((brow >> 1) & 7u)) << 2); }
// where a lane of instruction m stores its piece, and where lane i reads 16-B slot `slot` of its row in slab j
OTT_FF_HD inline uint32_t ff_store_off(uint32_t m, uint32_t lrow, uint32_t lslot) { return ff_buf_off(8u * m + lrow, lslot); }
OTT_FF_HD inline uint32_t ff_read_off(uint32_t i, uint32_t n, uint32_t j, uint32_t slot) { return ff_buf_off(((j * 8u) << ff_gshift(n)) + i, slot); }

}  // namespace ott
