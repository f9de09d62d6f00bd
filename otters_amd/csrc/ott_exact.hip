// ott_exact.hip — exact-order streaming scorer + fused wavefront top-k (gfx950).
//
// Replaces the scoring loop of VecQueryPlan::collect (src/vec.rs:222-303) with its
// dot_product / cosine_similarity / euclidean_distance_squared calls (src/vec_compute.rs:9-54)
// and the TopKCollector (src/vec_compute.rs:76-294).
//
// Arithmetic contract: scores are BIT-IDENTICAL to the reference's order of operations —
// 8 independent lane accumulators over chunks_exact(8) (separate multiply and add, no FMA),
// wide::f32x8::reduce_add, plus the sequential remainder sum, then (dot*q_inv)*v_inv for
// cosine.  This kernel is HBM-bound (0.5 flop/byte per query), so spending VALU on the exact
// order is free; what it needs is a layout in which ONE lane owns one row's 8 accumulator
// chains.  So: lane = row.  A wave streams a tile of 64 rows; every K-stage it loads
// 64 rows x 128 B with fully coalesced 16-B-per-lane loads (8 lanes cover one row's 128-B
// line), writes them to a wave-private 8 KB LDS tile with an XOR swizzle, and then each lane
// reads back ITS row's 32 B per step with conflict-free ds_read_b128.  Queries are read
// through the scalar cache (wave-uniform addresses -> s_load), so they cost no VGPRs.
// The next stage's global loads are in flight (in registers) while the current stage is
// consumed from LDS; waves are independent (no block barrier in the main loop).
//
// Top-k: each wave keeps a sorted list of k <= 64*E candidates in registers (E per lane),
// gated by the current k-th key; lanes that beat it are inserted with ballot + shuffle.
// Keys are (ord(score) << 32 | ~row, query): a total order (better score, lower row, lower
// query) so results are deterministic; the reference leaves tie order unspecified.
#include <atomic>

#include "ott_internal.h"
#include "ott_prune.h"
#include "ott_i8_check.h"
#include "ott_finish_few.h"
#include "ott_exact_dev.h"  // candidate order, wave list, filter, metric terms, reduce8: shared with ott_gather.hip

namespace ott {

constexpr int KC = 32;  // floats per row per stage: one 128-B line
constexpr int WAVES = 4;
constexpr int STAGE_FLOATS = 64 * KC;  // per wave: 8 KB
constexpr int EXACT_SMEM = WAVES * STAGE_FLOATS * 4;
constexpr int DUMP_QCAP = 128;  // large-k dump: survivors queued per wave between two appends (8 B key + 4 B query each)
constexpr int EXACT_SMEM_DUMP = EXACT_SMEM + WAVES * DUMP_QCAP * 12;
// pruned sweep (PRUNE): a wave's deferred-tail queue, a ring of rows that passed the checkpoint — 8 partial accumulators, the
// inverse norm and the row, one array each.  64 are finished together as one dense tile; the ring holds the 63 that may wait
// plus a whole tile's 64 more
constexpr int PQ_CAP = 128;
constexpr int PQ_WORDS = 10;
// four bits per dim: the digit planes of the quantised query behind the queues — per stage three digits x four words (ott_prune.h)
constexpr int QD_WORDS = (int)(OTT_QEMB_MAX / KC) * 12;
constexpr int EXACT_SMEM_PRUNE = EXACT_SMEM + WAVES * PQ_CAP * PQ_WORDS * 4 + QD_WORDS * 4;  // 53.3 KB: two workgroups per CU
// the int8 check of the head form's survivors (CHK): the query's int8 operand behind the digit planes, one word per four dims of a
// plane row (128-B stages: dim rounded up to 128)
constexpr int Q8_WORDS = (int)((OTT_QEMB_MAX + 127) / 128) * 32;
constexpr int EXACT_SMEM_CHECK = EXACT_SMEM_PRUNE + Q8_WORDS * 4;  // 54.1 KB: two workgroups per CU
// experiment builds only: -DOTT_SK4_DECODE_F32 keeps the four-bit form's former decode (an f32 chain, one fma per dim, and
// prune_score_bound_sketchb) so that both decodes can be alternated in one job
#ifdef OTT_SK4_DECODE_F32
constexpr bool SK4_INT = false;
#else
constexpr bool SK4_INT = true;
#endif
// sketch form of the pruned sweep (SK = 1): the sign words of a row's sketch line a lane keeps in registers — with a and rho at most
// three 16-B loads (OTT_SKETCH1_MAX_WORDS, ott_internal.h)
constexpr int SK_MAXW = (int)OTT_SKETCH1_MAX_WORDS;
// three-bit form (SK = 3): the stages a line can hold codes for (three words each), and its 16-B pieces beyond the eight that
// arrive in the row staging registers (OTT_SKETCH_MAX_WORDS)
constexpr int SK3_MAXST = (int)OTT_SKETCH_MAX_WORDS / 3;
constexpr int SK3_XP = ((int)OTT_SKETCH_MAX_WORDS + 2 + 3) / 4 - 8;
// Workgroups per CU of the persistent grid.  TWO since round 6 (8 waves per CU, 64 KB of row stages in flight per CU, 512 block lists for
// the merge): measured against 3, 4 (rounds 2-5), 5 and 8 on every instantiation — 1M x 128 dot top-10 89.4 + 11.8 -> 86.3 + 9.7 us
// (scoring + merge), 2M / 4M x 128 5 % / 3 % faster, 3M x 768 2 %, the 10M x 768 headline 4403 -> 4374 us, four queries per pass 4799
// -> 4552, top-500 on 1M x 128 294 -> 247, the single-query int8 sweep 1161 -> 1134 (profiles/round6/c1_latency.md).  The pruned
// launch with the three-bit sketch was measured on its own later, three against two for k <= 128 where registers and LDS allow
// it: 2.815 against 2.753 ms on the 10M x 768 headline (profiles/exact_overlap/README.md), so it keeps two as well.  Experiment
// builds override it: variants/build_exact.sh name "-DOTT_X_BLOCKS_PER_CU=4".
#ifndef OTT_X_BLOCKS_PER_CU
#define OTT_X_BLOCKS_PER_CU 2
#endif
constexpr int BLOCKS_PER_CU = OTT_X_BLOCKS_PER_CU;
// The head form's kernels with one list entry per lane finish at most sixteen queued rows as rounds of several stages (pq_finish_few,
// ott_finish_few.h).  Experiment builds give the wide finish back: "-DOTT_X_FINISH_FEW=0".
#ifndef OTT_X_FINISH_FEW
#define OTT_X_FINISH_FEW 1
#endif
static_assert(KC == (int)FF_KC, "ott_finish_few.h walks stages of KC floats");
// small-grid variant (a handful of tiles per CU: the launch is latency-bound, not bandwidth-bound): ONE wave per
// workgroup with a deep LDS-DMA ring
constexpr int SMALL_RING = 8;         // ring slots: 7 K stages in flight per wave (vmcnt counts to 63 = 7 x 8 + 7)
constexpr uint32_t SMALL_QMAX = 2048; // query floats kept in LDS
[[maybe_unused]] constexpr int EXACT_SMEM_SMALL = SMALL_RING * STAGE_FLOATS * 4 + SMALL_QMAX * 4;  // 72 KB: two workgroups per CU

// LDS-DMA piece: a wave instruction moves 8 rows x 128 B from global memory straight into a 1 KB block of LDS (lane i ->
// block base + 16*i); uniform 64-bit base in SGPRs + 32-bit lane byte offset; M0 carries the LDS byte address.  No
// "memory" clobber and no registers written: hipcc does not see a memory operation, so it inserts no wait for it — the
// kernel waits with counted `s_waitcnt vmcnt` itself (the loads retire in order).
__device__ __forceinline__ void exact_glds16(const char* sbase, uint32_t voff, uint32_t lds_addr) {
    uint32_t keep;
    lds_addr = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr);
    asm volatile(
        "s_nop 4\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_addr)
        : "memory");
}


// SMALL = the small-grid variant (single query, merged): with a tile or two per CU a launch is a chain of dependent
// latencies — per K stage the scalar-cache misses of the query loads (nothing is warm) and a ~2 us memory latency behind
// a single prefetched stage; the 24 stages of dim 768 came to 48 us whatever the corpus size.  Here a workgroup is ONE
// wave (launched with 64 threads, one tile each), the query is copied to LDS once and read back by broadcast, and the
// rows arrive by LDS-DMA through a ring of eight stages (seven in flight, no staging registers, counted waits).
// BLK: candidates enter the lists as sorted blocks where a tile brings many (wl_offer_block) — always at k > 64, at k <= 64 only
// from k = 17: the block code costs the k <= 16 instantiation registers for nothing (10M x 768 top-10: 4.45 -> 4.52-4.67 ms
// with it; 1M x 128 top-64: 119 -> 95 us), so the headline runs the kernel without it.
// I8 (round 5): the same sweep over the store's INT8 plane for ONE query — rows of 128-B stages hold 128 int8, the query's int8
// copy rides in the kernel arguments, a lane accumulates its row with v_dot4 (exact i32), and the "score" offered to the wave
// list is the APPROXIMATE (float)(q~ . v~) x row factor: the list's T best go to the exact re-score (run_i8_single).  Rows
// outside the pass's error model (flag bits 0 / 2) are always listed, ranked first.
// PRUNE: the pruned sweep of ONE query, cosine / dot, merged.  A tile runs stages 0 .. c-1 (c = p.prune_stage),
// summing each row's prefix squares beside the eight chains; then every row whose score bound (ott_prune.h) ranks strictly below
// the gate — the seed launch's k-th best, or the wave's own k-th once that is higher — is dropped, and the others (the
// accumulators, the inverse norm, the row) go to the wave's deferred-tail queue in LDS.  The next tile starts at once; whenever
// 64 rows wait they are finished as one dense tile — stages c .. n-1, the same loads and the same additions in the same order,
// so the same bits — and offered to the list (the list orders by key: when a row is offered changes nothing).
// SK (with PRUNE): the store keeps a tail sign sketch (ott_prune.h), so the checkpoint moves from 7/8 to 3/4 of the stages.  Each lane
// fetches its row's line (lane = row: 64 contiguous lines) with the inverse norm, at the checkpoint forms q_t . s from the sign
// words and the query's tail (scalar loads; one shift, one and-or and one fma per dim) and asks prune_score_bound_sketch; no prefix
// sum of squares is kept.  The queue and the finishing of survivors are the same code.
// SK = 3: the three-bit sketch of the last 5/8 of the stages, so the checkpoint is at 3/8 of them.  A line is up to fourteen 16-B
// pieces, too many to hold across the stages: the lane fetches them while the LAST prefix stage is consumed — no row stage is in
// flight then, so the first eight pieces land in the row staging registers, the others are asked for behind the loop and arrive
// while the first are decoded (lane = row: the 64 lines of a tile are one contiguous block).  Per dim: a signed field extract,
// kappa = 2 code + 1, a convert and one fma into D; then prune_score_bound_sketchb with kmax = 7.
// SK = 4: the four-bit sketch of every stage but the first, so the checkpoint is behind stage 0.  A line is a header piece and one
// 16-B piece per sketched stage, up to 28.  The 64 lines of a tile are fetched as the row stages are: eight pieces of every line per
// round, coalesced, through the staging registers into the stage buffer, the next round in flight while the lane decodes its own
// line's pieces out of LDS.  The decode is integer: the workgroup quantises the query once (ott_prune.h: prune_quant_word) and keeps
// its three base-16 digit planes in LDS; a piece's four code words meet the stage's digit words in twelve v_dot8_i32_i4, three
// independent i32 sums, and prune_score_bound_sketchq takes K = sum qhat kappa, exact.
// SEED (with the head form, SK = 5, E = 1): the seed as an estimate pass (ott_exact_plan.h: prune_plan_seed_est).  The launch has no
// gate.  A tile is read as a gated tile is — lines, heads, inverse norms, the same clamps and masks, the same twelve dot products
// per piece — and in place of the bound test every eligible lane offers (ord(estimate), ~row) to the wave's list, which keeps the
// p.seed_keep best (ott_prune.h: prune_score_est_sketchq; a NaN estimate is not offered).  Behind the wave's last tile those rows go
// to the deferred-tail queue with zero accumulators, the list is emptied, and one pq_finish scores them in the full sweep's loads
// and additions and offers the exact scores: the block list holds exact scores of eligible rows only.
// CHK (the gated launch of the head form, E = 1): survivors are checked on the store's int8 plane before their f32 finish
// (ott_exact_plan.h: prune_plan_i8_check; ott_i8_check.h).  The workgroup quantises the query once into its int8 operand in LDS, as
// it does for the digit planes.  When 64 rows wait in the queue, pq_refine scores them as one dense tile — the plane's 128-B stages
// through the same eight-rows-per-instruction loads as pq_finish, lane = row, eight v_dot4 per 32 bytes into two exact i32 sums —
// forms the approximate score with run_i8_single's operand and row factor, and drops every row whose score plus the certified
// error ranks strictly below the gate (i8_check_drops; rows outside the plane's error model and NaNs stay).  The rows that stay
// move to the front of the 64 and pq_finish, untouched, finishes them AT ONCE: the wave's list then sees every row that can
// enter it at the very tile it would without the check, so the gate, and with it the rows that pass the line gate (`rescored`),
// are the same with the check on and off.  At the headline's rates more than half of the tiles of 64 keep no row and skip the
// finish altogether.  The launch counts the rows that passed the line gate in p.prune_tails[0] and the finished ones in [1].
template <int MK, int NQ, int E, bool PERQ, bool DUMP = false, bool SMALL = false, bool BLK = (E > 1), bool I8 = false, bool PRUNE = false, int SK = 0, bool SEED = false,
          bool CHK = false>
__global__ __launch_bounds__(SMALL ? 64 : 256) void exact_kernel(ExactParams p) {
    static_assert(!CHK || (SK == 5 && !SEED && E == 1), "the int8 check is the gated head launch's, one list entry per lane");
    static_assert(!I8 || (NQ == 1 && MK == MK_DOT && !PERQ && !DUMP && !SMALL), "the int8 sweep takes one query, cosine / dot, merged");
    static_assert(!PRUNE || (NQ == 1 && MK == MK_DOT && !PERQ && !DUMP && !SMALL && !I8), "the pruned sweep takes one query, cosine / dot, merged");
    static_assert((SK == 0 || PRUNE) && (SK == 0 || SK == 1 || SK == 3 || SK == 4 || SK == 5), "the sketch is the pruned sweep's: none, one, three or four bits per dim (5: four with a head)");
    constexpr bool HD = SK == 5;               // the head form of the four-bit sketch: the checkpoint in front of stage 0
    constexpr bool SK4 = SK == 4 || SK == 5;   // either four-bit form
    static_assert(!HD || SK4_INT, "the head form decodes by integer dot products only");
    static_assert(!SEED || (HD && E == 1), "the estimate pass is the head form's, one list entry per lane");
    constexpr bool FEW = OTT_X_FINISH_FEW != 0 && HD && E == 1;  // a finish of at most FF_MAX_ROWS rows takes pq_finish_few
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int BW = SMALL ? 1 : WAVES;  // waves per workgroup
    float* st = SMALL ? smem : smem + wave * STAGE_FLOATS;
    float* sQ = smem + SMALL_RING * STAGE_FLOATS;  // SMALL only
    constexpr int NL = PERQ ? NQ : 1;
    constexpr int KS = 64 * E;

    WaveList<E> L[NL];
    uint64_t tk[NL];
    uint32_t tq[NL];
    bool fresh[NL];  // the list has not been offered anything yet (wave-uniform)
#pragma unroll
    for (int i = 0; i < NL; i++) {
        wl_init(L[i]);
        tk[i] = 0;
        tq[i] = 0xFFFFFFFFu;
        fresh[i] = true;
    }

    const bool take_max = p.take_max != 0;
    const uint32_t nq_here = (p.nq_total - p.q0) < (uint32_t)NQ ? (p.nq_total - p.q0) : (uint32_t)NQ;
    // wave-uniform, read-only inputs are addressed through the CONSTANT address space: such loads are always scalar
    // (s_load), whereas for global pointers hipcc only selects s_load while it can prove nothing in the kernel may write
    // the memory (an inline-asm statement anywhere in the kernel ends that proof: every query value then becomes a
    // vector load + readfirstlane)
    typedef __attribute__((address_space(4))) const float* CF32;
    typedef __attribute__((address_space(4))) const uint32_t* CU32;
    typedef __attribute__((address_space(4))) const ott_run* CRUN;
    // embedded inputs live in the kernel-argument segment (constant address space), ExactParams being the only argument
    typedef __attribute__((address_space(4))) const char* CCH;
    const CCH karg = (CCH)__builtin_amdgcn_kernarg_segment_ptr();
    const CF32 Q = p.embedded ? (CF32)(karg + __builtin_offsetof(ExactParams, qemb)) : (CF32)(p.queries + (size_t)p.q0 * p.dimq);
    const CU32 tile_prefix = p.embedded ? (CU32)(karg + __builtin_offsetof(ExactParams, eprefix)) : (CU32)p.tile_prefix;
    const CRUN runs = p.embedded ? (CRUN)(karg + __builtin_offsetof(ExactParams, eruns)) : (CRUN)p.runs;
    float qinv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) qinv[q] = (uint32_t)q < nq_here ? (p.embedded ? p.eqinv : p.qinv[p.q0 + q]) : 0.0f;
    // large-k path, second phase: a pair whose score ordinal is below its query's gate — the k-th best of the rows scored in
    // the first phase, a lower bound of the final k-th — cannot be in the result and is not listed (0 = open)
    uint32_t dgate[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) dgate[q] = (DUMP && p.dump_gate != nullptr && (uint32_t)q < nq_here) ? p.dump_gate[p.q0 + q] : 0u;
    // DUMP: a wave queues its survivors in LDS and appends them with ONE returning atomic on the list's cursor per flush (queue
    // full, or the wave is done).  One atomic per tile that holds a survivor — 70-150k of them on ONE address at 10M rows, each
    // with its wave waiting for the answer — cost the sweep 0.5-0.9 ms of 4.4 (kernel trace: 4.44 ms with nothing listed, 5.37
    // with 100k pairs listed from half of the tiles).
    uint64_t* dq_key = reinterpret_cast<uint64_t*>(smem + WAVES * STAGE_FLOATS) + wave * DUMP_QCAP;
    uint32_t* dq_q = reinterpret_cast<uint32_t*>(smem + WAVES * STAGE_FLOATS + WAVES * DUMP_QCAP * 2) + wave * DUMP_QCAP;
    uint32_t dqn = 0;  // wave-uniform
    auto dq_flush = [&]() {
        if (dqn == 0) return;
        wave_sync();
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(p.dump_cursor, (unsigned long long)dqn);
        base = rl64(base, 0);
        for (uint32_t i = lane; i < dqn; i += 64) {
            const uint64_t at = base + i;
            if (at < p.dump_cap) {
                p.dump_keys[at] = dq_key[i];
                p.dump_q[at] = dq_q[i];
            }
        }
        wave_sync();
        dqn = 0;
    };

    if constexpr (SMALL) {
        for (uint32_t i = threadIdx.x; i < p.dimq; i += 64 * BW) sQ[i] = Q[i];
        __syncthreads();
    }
    const uint32_t gw = blockIdx.x * BW + wave, nw = gridDim.x * BW;
    const int sw = (lane >> 1) & 7;
    const uint32_t nstages = (p.ld + KC - 1) / KC;
    // SK = 4: the digit planes of the quantised query, [stage][digit][word]; one thread per word of eight dims (zeros past dim)
    [[maybe_unused]] uint32_t* qd = reinterpret_cast<uint32_t*>(smem + WAVES * STAGE_FLOATS + WAVES * PQ_CAP * PQ_WORDS);
    // CHK: the query's int8 operand behind them, one thread per word of four dims (zeros past dim): i8_quant_word with the pre-scale
    // and the scale the host measured the query's loss with (ott_i8_check.h: i8_query_quant)
    [[maybe_unused]] uint32_t* q8w = qd + QD_WORDS;
    [[maybe_unused]] const uint32_t ld8w = ((p.dim + 127u) & ~127u) >> 2;  // words of a plane row
    if constexpr (CHK) {
        const float pf8 = p.metric == OTT_METRIC_COSINE ? qinv[0] : 1.0f;
        const float inv_sq = __fdiv_rn(1.0f, p.i8_qscale);
        const uint32_t nw8 = ld8w < (uint32_t)Q8_WORDS ? ld8w : (uint32_t)Q8_WORDS;
        for (uint32_t i = threadIdx.x; i < nw8; i += 64 * BW) {
            float q4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) q4[j] = (4 * i + j < p.dim) ? Q[4 * i + j] : 0.0f;
            q8w[i] = i8_quant_word(q4, pf8, inv_sq);
        }
        // (the barrier behind the digit planes covers these words too: CHK runs in the head form only)
    }
    if constexpr (SK4 && SK4_INT) {
        const uint32_t nqs = nstages < (uint32_t)(QD_WORDS / 12) ? nstages : (uint32_t)(QD_WORDS / 12);
        for (uint32_t i = threadIdx.x; i < nqs * 4; i += 64 * BW) {
            float q8[8];
#pragma unroll
            for (int j = 0; j < 8; j++) q8[j] = (8 * i + j < p.dim) ? Q[8 * i + j] : 0.0f;
            uint32_t d3[3];
            prune_quant_word(q8, p.prune_qinv_scale, d3);
#pragma unroll
            for (int d = 0; d < 3; d++) qd[(i >> 2) * 12 + d * 4 + (i & 3)] = d3[d];
        }
        __syncthreads();
    }
    const int lrow = lane >> 3;          // row within an 8-row load group
    const int lslot = lane & 7;          // 16-B slot within the 128-B line
    // its float offset, kept inside a short row (dim < 29): the staging loads are unconditional, so a slot past the row's
    // end must not make the LAST row of the store read past the allocation
    const uint32_t lsl4 = ((uint32_t)lslot * 4 < p.ld) ? (uint32_t)lslot * 4 : 0u;

    // PRUNE: the gate (the seed's k-th best score ordinal, 0 = open while the seed listed fewer than k rows), the stages a tile
    // runs in the sweep, the wave's queue, and how queued rows are finished
    const uint32_t pstage = HD ? 0u : p.prune_stage;  // the checkpoint
    const uint32_t s_end = PRUNE ? pstage : nstages;
    uint32_t theta = 0;
    if constexpr (PRUNE && !SEED) {
        if (p.prune_seed[0] >= p.k) theta = ord_of(reinterpret_cast<const ott_hit*>(p.prune_seed + 8)[p.k - 1].score, take_max);
    }
    float* pq = smem + WAVES * STAGE_FLOATS + wave * (PQ_CAP * PQ_WORDS);  // [acc 0..7 | vinv | row] x PQ_CAP
    uint32_t* pq_row = reinterpret_cast<uint32_t*>(pq + 9 * PQ_CAP);
    uint32_t pq_head = 0, pq_n = 0;  // wave-uniform
    uint32_t tails_done = 0;         // rows this wave finished (wave-uniform; added to p.prune_tails at the end)
    [[maybe_unused]] auto pq_finish = [&](uint32_t n) {  // the first n <= 64 queued rows: stages c .. n-1 as one tile, then the list
        wave_sync();
        const bool valid = (uint32_t)lane < n;
        const uint32_t e = (pq_head + (valid ? (uint32_t)lane : 0u)) & (PQ_CAP - 1);
        float acc[8];
#pragma unroll
        for (int l = 0; l < 8; l++) acc[l] = pq[l * PQ_CAP + e];
        const float vinv = pq[8 * PQ_CAP + e];
        const uint32_t my_row = pq_row[e];
        float tail = 0.0f;
        const float* rp[8];
        bool rok[8];
#pragma unroll
        for (int m = 0; m < 8; m++) {  // rows past n re-read the first queued row (never offered)
            const uint32_t i = 8 * m + lrow;
            rok[m] = i < n;
            rp[m] = p.rows + (uint64_t)pq_row[(pq_head + (rok[m] ? i : 0u)) & (PQ_CAP - 1)] * p.ld + lsl4;
        }
        v4f R[8];
        auto load_stage = [&](uint32_t s) {
            const uint32_t soff = (s * KC + lslot * 4 < p.ld) ? s * KC : 0u;
#pragma unroll
            for (int m = 0; m < 8; m++) R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rp[m] + soff));
        };
        load_stage(pstage);
        for (uint32_t s = pstage; s < nstages; s++) {
            const bool cok = s * KC + lslot * 4 < p.ld;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int row = 8 * m + lrow;
                const bool ok = rok[m] & cok;
                const v4f v = R[m];
                *reinterpret_cast<float4*>(st + row * KC + ((lslot ^ ((row >> 1) & 7)) << 2)) =
                    make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
            }
            wave_sync();
            if (s + 1 < nstages) load_stage(s + 1);
            {  // the lane's row of this stage into its chains
                const uint32_t cs_stage = s;
                const float* cs_row = st + lane * KC;
                const int cs_swz = sw;
#include "ott_exact_finish_stage.inc"
            }
            wave_sync();
        }
#include "ott_exact_finish_offer.inc"
    };
    // FEW: the first n <= FF_MAX_ROWS queued rows as rounds (ott_finish_few.h): the eight instructions of a round ask for S = 8 / G
    // stages of the n rows (G = 1 row group of eight, or 2), so a row of 24 stages is 3 or 6 round trips instead of 24.  The same
    // bytes by the same clamps — a slot past a short row, a piece past ld, a row past n re-reading the first — and one more: a stage
    // past the last reads the last one and is not consumed.  The round lands where pq_finish puts its eight instructions, which
    // makes the stage buffer S slabs of 8 G rows; a lane walks its row's slabs in stage order through the same stage code
    // (ott_exact_finish_stage.inc), so every chain sees the same terms in the same order
    [[maybe_unused]] auto pq_finish_few = [&](uint32_t n) __attribute__((always_inline)) {
        wave_sync();
        const bool valid = (uint32_t)lane < n;
        const uint32_t e = (pq_head + (valid ? (uint32_t)lane : 0u)) & (PQ_CAP - 1);
        float acc[8];
#pragma unroll
        for (int l = 0; l < 8; l++) acc[l] = pq[l * PQ_CAP + e];
        const float vinv = pq[8 * PQ_CAP + e];
        const uint32_t my_row = pq_row[e];
        float tail = 0.0f;
        const uint32_t S = ff_stages(n);
        const float* rp[2];
        bool rok[2];
#pragma unroll
        for (int g = 0; g < 2; g++) {  // rows past n re-read the first queued row (never offered)
            const uint32_t i = 8 * g + lrow;
            rok[g] = i < n;
            rp[g] = p.rows + (uint64_t)pq_row[(pq_head + (rok[g] ? i : 0u)) & (PQ_CAP - 1)] * p.ld + ff_slot_off((uint32_t)lslot, p.ld);
        }
        v4f R[8];
        auto load_round = [&](uint32_t s0) __attribute__((always_inline)) {
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t sc = ff_stage_clamp(s0 + ff_load_slab(m, n), nstages);
                R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>((ff_load_group(m, n) ? rp[1] : rp[0]) + ff_col_off(sc, (uint32_t)lslot, p.ld)));
            }
        };
        load_round(pstage);
        const uint32_t li = (uint32_t)lane & (8u * ff_groups(n) - 1u);  // (a lane past the slab's rows walks one of them: never offered)
        for (uint32_t s0 = pstage; s0 < nstages; s0 += S) {
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const bool cok = ff_col_ok(s0 + ff_load_slab(m, n), (uint32_t)lslot, p.ld);
                const bool ok = (ff_load_group(m, n) ? rok[1] : rok[0]) & cok;
                const v4f v = R[m];
                *reinterpret_cast<float4*>(st + ff_store_off(m, (uint32_t)lrow, (uint32_t)lslot)) =
                    make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
            }
            wave_sync();
            if (s0 + S < nstages) load_round(s0 + S);
            for (uint32_t sl = 0; sl < S && s0 + sl < nstages; sl++) {  // slab sl: stage s0 + sl
                const uint32_t brow = ff_read_off(li, n, sl, 0u) / KC;  // (slot 0 of a row: the row's base, its swizzle from the row)
                const uint32_t cs_stage = s0 + sl;
                const float* cs_row = st + brow * KC;
                const int cs_swz = (int)((brow >> 1) & 7u);
#include "ott_exact_finish_stage.inc"
            }
            wave_sync();
        }
#include "ott_exact_finish_offer.inc"
    };
    // n queued rows by the finish that fits them; the estimate pass queues at most p.seed_keep <= FF_MAX_ROWS and has no other
    [[maybe_unused]] auto pq_finish_any = [&](uint32_t n) __attribute__((always_inline)) {
        if constexpr (FEW && SEED) {
            pq_finish_few(n);
        } else if constexpr (FEW) {
            if (n <= FF_MAX_ROWS) pq_finish_few(n);
            else pq_finish(n);
        } else {
            pq_finish(n);
        }
    };
    // CHK: the first n <= 64 queued rows on the int8 plane, as one tile.  The rows that stay are moved to the front of the n (their
    // accumulators are zero like everyone's in the head form: only the inverse norm and the row move); returns how many stay
    [[maybe_unused]] uint32_t queued = 0;  // rows that passed the line gate (wave-uniform; added to p.prune_tails[0] at the end)
    [[maybe_unused]] auto pq_refine = [&](uint32_t n, uint32_t gate) __attribute__((always_inline)) -> uint32_t {
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        wave_sync();
        const bool valid = (uint32_t)lane < n;
        const uint32_t e = (pq_head + (valid ? (uint32_t)lane : 0u)) & (PQ_CAP - 1);
        const float vinv = pq[8 * PQ_CAP + e];
        const uint32_t my_row = pq_row[e];
        // the row's scale and flag: scattered 4-B and 1-B reads, in flight behind the stages
        const float sv = p.i8_scale[my_row];
        const uint32_t fl = p.flag[my_row];
        const uint32_t* rp[8];
#pragma unroll
        for (int m = 0; m < 8; m++) {  // rows past n re-read the first queued row (never judged)
            const uint32_t i = 8 * m + lrow;
            rp[m] = reinterpret_cast<const uint32_t*>(p.chk_plane) + (uint64_t)pq_row[(pq_head + (i < n ? i : 0u)) & (PQ_CAP - 1)] * ld8w + (uint32_t)lslot * 4;
        }
        v4f R[8];
        auto load_stage = [&](uint32_t s) {  // (a plane row is whole 128-B stages: no column to clamp)
#pragma unroll
            for (int m = 0; m < 8; m++) R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rp[m] + s * KC));
        };
        const uint32_t nst8 = ld8w / KC;
        int iacc[2] = {0, 0};  // two independent v_dot4 chains, exact
        load_stage(0);
        for (uint32_t s = 0; s < nst8; s++) {
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int row = 8 * m + lrow;
                const v4f v = R[m];
                *reinterpret_cast<float4*>(st + row * KC + ((lslot ^ ((row >> 1) & 7)) << 2)) = make_float4(v.x, v.y, v.z, v.w);
            }
            wave_sync();
            if (s + 1 < nst8) load_stage(s + 1);
#pragma unroll
            for (int j = 0; j < KC / 8; j++) {
                const float4 a = *reinterpret_cast<const float4*>(st + lane * KC + (((2 * j) ^ sw) << 2));
                const float4 b = *reinterpret_cast<const float4*>(st + lane * KC + (((2 * j + 1) ^ sw) << 2));
                const int x[8] = {__float_as_int(a.x), __float_as_int(a.y), __float_as_int(a.z), __float_as_int(a.w),
                                  __float_as_int(b.x), __float_as_int(b.y), __float_as_int(b.z), __float_as_int(b.w)};
                // the operand's eight words of these 32 dims: two broadcast reads (a wave-uniform address)
                const v4u* qp = reinterpret_cast<const v4u*>(q8w + s * KC + 8 * j);
                const v4u q0 = qp[0], q1 = qp[1];
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    iacc[0] = __builtin_amdgcn_sdot4(x[l], (int)q0[l], iacc[0], false);
                    iacc[1] = __builtin_amdgcn_sdot4(x[4 + l], (int)q1[l], iacc[1], false);
                }
            }
            wave_sync();
        }
        const float approx = i8_approx_score(iacc[0] + iacc[1], i8_row_factor(p.metric == OTT_METRIC_COSINE, vinv, sv, p.i8_qscale));
        const bool stay = valid && !i8_check_drops(approx, p.chk_eps, take_max, gate, (fl & 5u) != 0);
        const uint64_t km = __ballot(stay);
        if (stay) {  // (every lane holds its own entry in registers, and a row only moves towards the front)
            const uint32_t at = (pq_head + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))) & (PQ_CAP - 1);
            pq[8 * PQ_CAP + at] = vinv;
            pq_row[at] = my_row;
        }
        return (uint32_t)__popcll(km);
    };
    // the first n queued rows: checked, and what stays finished at once; the gate is the one the last tile was judged with (the
    // list changes in pq_finish only).  While it is open nothing can be dropped and the rows are finished as without the check
    [[maybe_unused]] auto pq_drain = [&](uint32_t n, uint32_t gate) __attribute__((always_inline)) {
        const uint32_t stay = gate != 0 ? pq_refine(n, gate) : n;
        if (stay) pq_finish_any(stay);
        pq_head = (pq_head + (n - stay)) & (PQ_CAP - 1);
        pq_n -= n - stay;
    };

    if constexpr (HD) {
        // The head form (ott_prune.h: prune_sketch4_head_row).  A gated tile reads no row stage: its 64 lines as in the SK = 4 form,
        // eight pieces of every line per round through R into the stage buffer, and lane = row the 64 heads (16 B of stage 0's codes
        // and rho_all, two plain arrays) and inverse norms.  Nothing of a tile hides its first round any more, so the loop is
        // pipelined ACROSS tiles: while the last round of a tile is decoded, round 0 of the next tile that has a row to score, its
        // heads and its inverse norms are in flight (`pf`).  The bound is prune_score_bound_sketchq at m = 0: an all-zero acc,
        // rho_all, K over every stage.  A survivor is queued with zero accumulators and pq_finish runs all of its stages: the loads
        // and additions of the full sweep in its order, so the same bits.  While the gate is open no line and no head is fetched
        // and every row is queued.
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        const uint32_t np = p.sk_pitch >> 2;  // [a | rho | 0 | 0], then one piece per stage from stage 1
        auto locate = [&](uint32_t t, uint64_t& row0, uint32_t& cnt, uint64_t& vm) {  // tile -> rows and the lanes that score one
            uint32_t lo = 0, hi = p.n_runs;
            while (hi - lo > 1) {
                uint32_t mid = (lo + hi) >> 1;
                if (tile_prefix[mid] <= t) lo = mid;
                else hi = mid;
            }
            const uint64_t rs = runs[lo].start, rc = runs[lo].count;
            const uint64_t off = (uint64_t)(t - tile_prefix[lo]) * 64;
            row0 = rs + off;
            cnt = (rc - off) < 64 ? (uint32_t)(rc - off) : 64u;
            const uint64_t r = row0 + lane;
            bool valid = (uint32_t)lane < cnt;
            if (p.row_mask != nullptr && valid && r < p.row_mask_bits) valid = (p.row_mask[r >> 6] >> (r & 63)) & 1;  // src/vec.rs:231-237
            vm = __ballot(valid);
        };
        auto next_tile = [&](uint32_t t, uint64_t& row0, uint32_t& cnt, uint64_t& vm) -> uint32_t {  // (a whole tile masked: its rows are never read)
            for (; t < p.n_tiles; t += nw) {
                locate(t, row0, cnt, vm);
                if (vm != 0) break;
            }
            return t;
        };
        v4f R[8];
        v4u hc = {0u, 0u, 0u, 0u};
        float hrho = __builtin_inff(), hinv = 0.0f;
        // a piece index is clamped to the line's last piece, a row past the tile's end to its last row: nothing outside the tile's
        // own lines, heads and inverse norms is read
        auto load_line = [&](uint64_t row0, uint32_t cnt, uint32_t f) {
            const uint32_t pc = (8 * f + (uint32_t)lslot < np) ? 8 * f + (uint32_t)lslot : np - 1;
            const uint32_t* lb = p.prune_sketch + row0 * (uint64_t)p.sk_pitch + 4 * pc;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t row = 8 * m + lrow;
                R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(lb + (row < cnt ? row : cnt - 1) * p.sk_pitch));
            }
        };
        auto load_head = [&](uint64_t row0, uint32_t cnt) {
            const uint64_t r = row0 + ((uint32_t)lane < cnt ? (uint32_t)lane : cnt - 1);
            hc = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p.prune_head_codes) + r);
            hrho = __builtin_nontemporal_load(p.prune_head_rho + r);
            hinv = __builtin_nontemporal_load(p.inv + r);
        };
        uint64_t row0 = 0, vm = 0;
        uint32_t cnt = 0;
        uint32_t t = next_tile(gw, row0, cnt, vm);
        bool pf = false;  // round 0 of tile t's lines is in R, its heads and inverse norms in hc / hrho / hinv, or on their way (wave-uniform)
        while (t < p.n_tiles) {
            // the gate: the seed's k-th best or, once higher, the wave's own (0 while its list holds fewer than k).  It only rises, so
            // a tile that was fetched for is gated
            uint32_t gate = theta;
            const uint32_t own = (uint32_t)(tk[0] >> 32);
            if (own > gate) gate = own;
            const uint64_t my_row = row0 + lane;
            const bool valid = (vm >> lane) & 1;
            uint64_t row0n = 0, vmn = 0;
            uint32_t cntn = 0;
            const uint32_t tn = next_tile(t + nw, row0n, cntn, vmn);
            bool keep = valid;
            float vinv = 0.0f;
            if (SEED || gate != 0) {
                if (!pf) {
                    load_line(row0, cnt, 0);
                    load_head(row0, cnt);
                }
                const v4u c0 = hc;
                const float rho_all = hrho;
                vinv = hinv;
                pf = false;
                int K0 = 0, K1 = 0, K2 = 0;
                float sk_a = 0.0f;
                for (uint32_t f = 0; 8 * f < np; f++) {
#pragma unroll
                    for (int m = 0; m < 8; m++) {
                        const int row = 8 * m + lrow;
                        const v4f v = R[m];
                        *reinterpret_cast<float4*>(st + row * KC + ((lslot ^ ((row >> 1) & 7)) << 2)) = make_float4(v.x, v.y, v.z, v.w);
                    }
                    wave_sync();
                    if (8 * (f + 1) < np) {
                        load_line(row0, cnt, f + 1);
                    } else if (tn < p.n_tiles) {  // the last round: the next tile's first
                        load_line(row0n, cntn, 0);
                        load_head(row0n, cntn);
                        pf = true;
                    }
                    for (uint32_t j = 0; j < 8 && 8 * f + j < np; j++) {  // piece 8 f + j of the lane's own line
                        const float4 w4 = *reinterpret_cast<const float4*>(st + lane * KC + (((int)j ^ sw) << 2));
                        const uint32_t piece = 8 * f + j;
                        if (piece == 0) {
                            sk_a = w4.x;
                            continue;
                        }
                        const uint32_t sj = p.sk_stage0 + piece - 1u;
                        if (sj < nstages) {
                            const uint32_t w[4] = {__float_as_uint(w4.x), __float_as_uint(w4.y), __float_as_uint(w4.z), __float_as_uint(w4.w)};
                            const v4u* dp = reinterpret_cast<const v4u*>(qd + sj * 12);
                            const v4u d0 = dp[0], d1 = dp[1], d2 = dp[2];
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                K0 = __builtin_amdgcn_sdot8((int)w[i], (int)d0[i], K0, false);
                                K1 = __builtin_amdgcn_sdot8((int)w[i], (int)d1[i], K1, false);
                                K2 = __builtin_amdgcn_sdot8((int)w[i], (int)d2[i], K2, false);
                            }
                        }
                    }
                    wave_sync();
                }
                {  // stage 0: the head's codes against the stage's digit words
                    const v4u* dp = reinterpret_cast<const v4u*>(qd);
                    const v4u d0 = dp[0], d1 = dp[1], d2 = dp[2];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        K0 = __builtin_amdgcn_sdot8((int)c0[i], (int)d0[i], K0, false);
                        K1 = __builtin_amdgcn_sdot8((int)c0[i], (int)d1[i], K1, false);
                        K2 = __builtin_amdgcn_sdot8((int)c0[i], (int)d2[i], K2, false);
                    }
                }
                if constexpr (SEED) {
                    const int K = 2 * (256 * K2 + 16 * K1 + K0) + p.prune_qsum;
                    const float est = prune_score_est_sketchq(vinv, sk_a, rho_all, K, p.prune_qscale, qinv[0], p.metric == OTT_METRIC_COSINE);
                    const bool offer = valid && est - est == 0.0f;  // (NaN or infinite: not offered)
                    const uint64_t key = ((uint64_t)ord_of(est, take_max) << 32) | (uint32_t)(~(uint32_t)my_row);
                    if (fresh[0]) {
                        wl_fill_sorted(L[0], tk[0], tq[0], p.seed_keep, offer, key, p.q0, lane, 0u);
                        fresh[0] = false;
                    } else {
                        wl_offer(L[0], tk[0], tq[0], p.seed_keep, offer, key, p.q0, lane, 0u);
                    }
                    keep = false;
                } else if (valid) {
                    const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    const int K = 2 * (256 * K2 + 16 * K1 + K0) + p.prune_qsum;
                    const float b = prune_score_bound_sketchq(zero, vinv, sk_a, rho_all, K, p.prune_qscale, p.dim, p.prune_qt, p.prune_qe1, p.prune_qn, qinv[0],
                                                              p.metric == OTT_METRIC_COSINE, take_max);
                    keep = !(b == b && ord_of(b, take_max) < gate);  // (NaN: no bound, the row is finished)
                }
            } else if (valid) {
                vinv = p.inv[my_row];
            }
            const uint64_t km = SEED ? 0ull : __ballot(keep);
            if (!SEED && keep) {
                const uint32_t at = (pq_head + pq_n + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))) & (PQ_CAP - 1);
#pragma unroll
                for (int l = 0; l < 8; l++) pq[l * PQ_CAP + at] = 0.0f;
                pq[8 * PQ_CAP + at] = vinv;
                pq_row[at] = (uint32_t)my_row;
            }
            pq_n += (uint32_t)__popcll(km);
            if constexpr (CHK) queued += (uint32_t)__popcll(km);
            if (!SEED && pq_n >= 64) {
                // (64 survivors: about one tile in seventy at the headline's rate.  What was asked for ahead is asked for again behind
                // the finish instead of being kept across it: its 38 registers would sit on top of the finish's own staging registers)
                if constexpr (CHK) pq_drain(64, gate);
                else if constexpr (!SEED) pq_finish(64);
                if (pf) {
                    load_line(row0n, cntn, 0);
                    load_head(row0n, cntn);
                }
            }
            t = tn;
            row0 = row0n;
            cnt = cntn;
            vm = vmn;
        }
        if constexpr (SEED) {
            // the wave's best rows by estimate (positions 0 .. seed_keep - 1 of the list, sentinels behind the real ones) are queued
            // like survivors, and the list starts again: what it ends up with are their exact scores
            const bool have = (uint32_t)lane < p.seed_keep && L[0].key[0] != 0ull;
            const uint64_t hm = __ballot(have);
            if (have) {
                const uint32_t r = ~(uint32_t)L[0].key[0];
                const uint32_t at = (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
#pragma unroll
                for (int l = 0; l < 8; l++) pq[l * PQ_CAP + at] = 0.0f;
                pq[8 * PQ_CAP + at] = p.inv[r];
                pq_row[at] = r;
            }
            pq_n = (uint32_t)__popcll(hm);
            wl_init(L[0]);
            tk[0] = 0;
            tq[0] = 0xFFFFFFFFu;
            fresh[0] = true;
        }
    } else
    for (uint32_t t = gw; t < p.n_tiles; t += nw) {
        // tile -> run of surviving chunks (wave-uniform scalar search)
        uint32_t lo = 0, hi = p.n_runs;
        while (hi - lo > 1) {
            uint32_t mid = (lo + hi) >> 1;
            if (tile_prefix[mid] <= t) lo = mid;
            else hi = mid;
        }
        ott_run run;
        run.start = runs[lo].start;
        run.count = runs[lo].count;
        const uint64_t off = (uint64_t)(t - tile_prefix[lo]) * 64;
        const uint64_t row0 = run.start + off;
        const uint32_t cnt = (run.count - off) < 64 ? (uint32_t)(run.count - off) : 64u;
        const uint64_t my_row = row0 + lane;
        bool valid = (uint32_t)lane < cnt;
        if (p.row_mask != nullptr && valid && my_row < p.row_mask_bits)
            valid = (p.row_mask[my_row >> 6] >> (my_row & 63)) & 1;  // src/vec.rs:231-237
        if (__ballot(valid) == 0) continue;  // whole tile masked: its rows are never read

        // the row's inverse norm is fetched now and used after the K loop: its latency hides behind the stages (after the
        // loop it was a ~2 us bubble per tile, which shows at small dims where a tile is only a few stages long)
        float vinv = 0.0f;
        if ((PRUNE || p.metric == OTT_METRIC_COSINE) && valid) vinv = p.inv[my_row];  // (PRUNE: the bound needs ||v||, dot too)
        float vsq = 0.0f;  // PRUNE without a sketch: the prefix's sum of squares
        // SK: the row's sketch line [a | rho | sign words], fetched now like the inverse norm (non-temporal: read once per sweep)
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        [[maybe_unused]] uint32_t skl[2 + SK_MAXW];
        // SK >= 3: the gate is known before the stages (the wave's list changes only when queued rows are finished): no line is fetched
        // while it is open
        [[maybe_unused]] uint32_t gate3 = 0;
        if constexpr (SK >= 3) {
            gate3 = theta;
            const uint32_t own = (uint32_t)(tk[0] >> 32);
            if (own > gate3) gate3 = own;
        }
        if constexpr (SK == 1) {
#pragma unroll
            for (int i = 0; i < 2 + SK_MAXW; i++) skl[i] = 0u;
            skl[1] = 0x7F800000u;  // (rho = +inf: no bound)
            if (valid) {
                const v4u* sp = reinterpret_cast<const v4u*>(p.prune_sketch + my_row * (uint64_t)p.sk_pitch);
                // (a line is sk_pitch words, 4, 8 or 12: a load past it would leave the buffer behind the store's last row)
                const v4u l0 = __builtin_nontemporal_load(sp);
                v4u l1 = {0u, 0u, 0u, 0u}, l2 = {0u, 0u, 0u, 0u};
                if (p.sk_pitch > 4) l1 = __builtin_nontemporal_load(sp + 1);
                if (p.sk_pitch > 8) l2 = __builtin_nontemporal_load(sp + 2);
                skl[0] = l0.x; skl[1] = l0.y; skl[2] = l0.z; skl[3] = l0.w;
                skl[4] = l1.x; skl[5] = l1.y; skl[6] = l1.z; skl[7] = l1.w;
                skl[8] = l2.x; skl[9] = l2.y; skl[10] = l2.z; skl[11] = l2.w;
            }
        }
        float i8_rf = 0.0f;     // I8: the row factor s_v [x 1/||v||] x s_Q
        bool i8_forced = false; // I8: a row outside the error model
        if constexpr (I8) {
            if (valid) {
                i8_rf = ((p.metric == OTT_METRIC_COSINE ? vinv : 1.0f) * p.i8_scale[my_row]) * p.i8_qscale;
                i8_forced = (p.flag[my_row] & 5u) != 0;
            }
        }
        int iacc[2] = {0, 0};   // I8: two independent v_dot4 chains
        float acc[NQ][8];
        float tail[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            tail[q] = 0.0f;
#pragma unroll
            for (int l = 0; l < 8; l++) acc[q][l] = 0.0f;
        }

        v4f R[8];
        const float* rp[8];
        bool rok[8];
        // SMALL: LDS-DMA.  The XOR swizzle is applied on the SOURCE side (the lane that owns physical slot `lslot` of
        // row `lrow` fetches logical slot lslot ^ f(row)), rows past a short tile's end are clamped to its last row and
        // a column group past `ld` to column 0: what lands there is never read (invalid lanes are never offered, and
        // the arithmetic stops at `dim`).
        const uint32_t lds_ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)st;
        const char* dma_base = reinterpret_cast<const char*>(p.rows + row0 * (uint64_t)p.ld);
        uint32_t dma_row[8];
        if constexpr (SMALL) {
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t row = 8 * m + lrow;
                dma_row[m] = (row < cnt ? row : cnt - 1) * p.ld;
            }
        } else {
            // Branch-free staging: every load is always issued (rows past a short tile's end are clamped to its last row,
            // a column group past `ld` in the last stage re-reads stage 0) and the out-of-range values are zeroed when they
            // are written to LDS.  With the loads under `if`s the compiler split them into basic blocks, one per load.
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t row = 8 * m + lrow;
                rok[m] = row < cnt;
                rp[m] = p.rows + (row0 + (rok[m] ? row : cnt - 1)) * (uint64_t)p.ld + lsl4;
            }
        }
        auto dma_stage = [&](uint32_t s) {
            const uint32_t slot_e = lslot ^ (lrow >> 1);
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t col = s * KC + ((m & 1) ? (slot_e ^ 4) : slot_e) * 4;
                exact_glds16(dma_base, (dma_row[m] + (col < p.ld ? col : 0u)) * 4u,
                             lds_ring + (uint32_t)((s % SMALL_RING) * STAGE_FLOATS * 4 + m * 1024));
            }
        };
        auto load_stage = [&](uint32_t s) {
            const uint32_t soff = (s * KC + lslot * 4 < p.ld) ? s * KC : 0u;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                // non-temporal: the corpus is streamed once per pass; keeping it out of the way of L2 / Infinity Cache
                // replacement is worth +11 % on MI355X (6.17 -> 6.86 TB/s at 10M x 768)
                R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rp[m] + soff));
            }
        };

        // SK = 4: the tile's 64 sketch lines are one contiguous block, fetched like a row stage — round f is pieces 8 f .. 8 f + 7 of
        // every line, 8 lines x 128 B per wave instruction, through the staging registers and the stage buffer to lane = row.  (A lane
        // that fetches its own line piece by piece asks L2 for 64 different lines per instruction, and for each line eight times: that
        // pattern alone took as long as the whole launch, benchmarks/cpp/prefix_stream.hip.)  A piece index is clamped to the line's
        // last piece and a row past the tile's end to its last row: nothing outside the tile's own lines is read
        auto load_line = [&](uint32_t f) {
            const uint32_t np = p.sk_pitch >> 2;
            const uint32_t pc = (8 * f + (uint32_t)lslot < np) ? 8 * f + (uint32_t)lslot : np - 1;
            const uint32_t* lb = p.prune_sketch + row0 * (uint64_t)p.sk_pitch + 4 * pc;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t row = 8 * m + lrow;
                R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(lb + (row < cnt ? row : cnt - 1) * p.sk_pitch));
            }
        };

        if constexpr (SMALL) {
            for (uint32_t s = 0; s < (uint32_t)(SMALL_RING - 1) && s < nstages; s++) dma_stage(s);
        } else {
            load_stage(0);
        }
        for (uint32_t s = 0; s < s_end; s++) {
            const float* sst = st;
            if constexpr (SMALL) {
                // issued so far: stages 0 .. s+RING-2.  Stage s has landed when at most the later stages' pieces (8 each,
                // retiring in order) are outstanding; then stage s+RING-1 goes into the slot stage s-1 was read from
                const uint32_t later = (nstages - 1 - s) < (uint32_t)(SMALL_RING - 2) ? (nstages - 1 - s) : (uint32_t)(SMALL_RING - 2);
                switch (later) {
                    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
                    case 1: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
                    case 2: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
                    case 3: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
                    case 4: asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); break;
                    case 5: asm volatile("s_waitcnt vmcnt(40)" ::: "memory"); break;
                    default: asm volatile("s_waitcnt vmcnt(48)" ::: "memory"); break;
                }
                if (s + SMALL_RING - 1 < nstages) dma_stage(s + SMALL_RING - 1);
                sst = st + (s % SMALL_RING) * STAGE_FLOATS;
            } else {
                const bool cok = s * KC + lslot * 4 < p.ld;
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const int row = 8 * m + lrow;
                    const bool ok = rok[m] & cok;
                    const v4f v = R[m];
                    *reinterpret_cast<float4*>(st + row * KC + ((lslot ^ ((row >> 1) & 7)) << 2)) =
                        make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
                }
                wave_sync();
                if (s + 1 < s_end) {
                    load_stage(s + 1);
                } else if constexpr (SK == 4) {
                    if (gate3 != 0) load_line(0);  // the first round of the tile's lines into the idle staging registers
                } else if constexpr (SK == 3) {
                    // the row's sketch line into the idle staging registers: pieces 0 .. 7, clamped to the line's last piece (a load
                    // past it would leave the buffer behind the store's last row); lanes past the tile's end read its last row's
                    if (gate3 != 0) {
                        const uint64_t lr = row0 + ((uint32_t)lane < cnt ? (uint32_t)lane : cnt - 1);
                        const v4f* sp = reinterpret_cast<const v4f*>(p.prune_sketch + lr * (uint64_t)p.sk_pitch);
                        const uint32_t np = p.sk_pitch >> 2;
#pragma unroll
                        for (int m = 0; m < 8; m++) R[m] = __builtin_nontemporal_load(sp + ((uint32_t)m < np ? (uint32_t)m : np - 1));
                    }
                }
            }

            if constexpr (I8) {
                // 128 int8 of the row per stage: eight dwords per step against eight query dwords (scalar loads), exact i32 sums
                typedef __attribute__((address_space(4))) const int* CI32;
                const CI32 qi = (CI32)Q;
#pragma unroll
                for (int j = 0; j < KC / 8; j++) {
                    const uint32_t col = s * KC + 8 * j;
                    const float4 a = *reinterpret_cast<const float4*>(sst + lane * KC + (((2 * j) ^ sw) << 2));
                    const float4 b = *reinterpret_cast<const float4*>(sst + lane * KC + (((2 * j + 1) ^ sw) << 2));
                    const int x[8] = {__float_as_int(a.x), __float_as_int(a.y), __float_as_int(a.z), __float_as_int(a.w),
                                      __float_as_int(b.x), __float_as_int(b.y), __float_as_int(b.z), __float_as_int(b.w)};
#pragma unroll
                    for (int l = 0; l < 8; l++) iacc[l & 1] = __builtin_amdgcn_sdot4(x[l], qi[col + l], iacc[l & 1], false);
                }
            } else {
#pragma unroll
            for (int j = 0; j < KC / 8; j++) {
                const uint32_t col = s * KC + 8 * j;
                if (col < p.dim) {
                    const float4 a = *reinterpret_cast<const float4*>(sst + lane * KC + (((2 * j) ^ sw) << 2));
                    const float4 b = *reinterpret_cast<const float4*>(sst + lane * KC + (((2 * j + 1) ^ sw) << 2));
                    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    if (col + 8 <= p.dim) {
                        // one chunks_exact(8) step: acc = acc + (q * v)   (vec_compute.rs:12-13, 39-42)
                        // every slot of the NQ-wide pass is computed (the query block is zero padded to a multiple of
                        // 8 rows): no per-query branch, so the scalar query loads of a step are issued together
#pragma unroll
                        for (int q = 0; q < NQ; q++) {
                            const CF32 qp = Q + (size_t)q * p.dimq + col;
#pragma unroll
                            for (int l = 0; l < 8; l++) {
                                float qv;
                                if constexpr (SMALL) qv = sQ[col + l];  // NQ == 1: broadcast LDS read
                                else qv = qp[l];
                                acc[q][l] = __fadd_rn(acc[q][l], exact_term<MK>(qv, x[l]));
                            }
                        }
                        if constexpr (PRUNE && SK == 0) {
#pragma unroll
                            for (int l = 0; l < 8; l++) vsq = fmaf(x[l], x[l], vsq);
                        }
                    } else {
                        // remainder: sequential sum of the last dim%8 products (vec_compute.rs:15-21, 44-53)
                        const uint32_t nt = p.dim - col;
#pragma unroll
                        for (int q = 0; q < NQ; q++) {
                            const CF32 qp = Q + (size_t)q * p.dimq + col;
#pragma unroll
                            for (int l = 0; l < 7; l++) {
                                if ((uint32_t)l < nt) {
                                    float qv;
                                    if constexpr (SMALL) qv = sQ[col + l];  // NQ == 1: broadcast LDS read
                                    else qv = qp[l];
                                    tail[q] = __fadd_rn(tail[q], exact_term<MK>(qv, x[l]));
                                }
                            }
                        }
                    }
                }
            }
            }
            wave_sync();
        }

        if constexpr (PRUNE) {
            // the checkpoint: a row whose bound ranks strictly below the gate is done; the others wait in the queue for stages c ..
            // n-1.  The gate is the seed's k-th best or, once higher, the wave's own (0 while its list holds fewer than k)
            uint32_t gate = theta;
            const uint32_t own = (uint32_t)(tk[0] >> 32);
            if (own > gate) gate = own;
            if constexpr (SK >= 3) gate = gate3;  // the gate the line was fetched for: the staging registers hold a line only then
            bool keep = valid;
            if constexpr (SK == 4) {
                if (gate != 0) {  // (wave-uniform; round 0 of the lines is in R, or on its way)
                    const uint32_t np = p.sk_pitch >> 2;  // [a | rho | 0 | 0], then one piece per sketched stage
                    [[maybe_unused]] float D = 0.0f;
                    [[maybe_unused]] int K0 = 0, K1 = 0, K2 = 0;
                    float sk_a = 0.0f, sk_rho = __builtin_inff();
                    for (uint32_t f = 0; 8 * f < np; f++) {
                        // round f to the stage buffer (the row stages' swizzle); the next round is in flight while this one is decoded
#pragma unroll
                        for (int m = 0; m < 8; m++) {
                            const int row = 8 * m + lrow;
                            const v4f v = R[m];
                            *reinterpret_cast<float4*>(st + row * KC + ((lslot ^ ((row >> 1) & 7)) << 2)) = make_float4(v.x, v.y, v.z, v.w);
                        }
                        wave_sync();
                        if (8 * (f + 1) < np) load_line(f + 1);
                        for (uint32_t j = 0; j < 8 && 8 * f + j < np; j++) {  // piece 8 f + j of the lane's own line
                            const float4 w4 = *reinterpret_cast<const float4*>(st + lane * KC + (((int)j ^ sw) << 2));
                            const uint32_t piece = 8 * f + j;
                            if (piece == 0) {
                                sk_a = w4.x;
                                sk_rho = w4.y;
                                continue;
                            }
                            const uint32_t sj = p.sk_stage0 + piece - 1u;  // piece i >= 1 holds sketched stage i - 1: eight fields per word
                            if (sj >= p.prune_stage && sj < nstages) {
                                const uint32_t w[4] = {__float_as_uint(w4.x), __float_as_uint(w4.y), __float_as_uint(w4.z), __float_as_uint(w4.w)};
                                if constexpr (SK4_INT) {
                                    // the stage's digit words: three broadcast reads (a wave-uniform address)
                                    const v4u* dp = reinterpret_cast<const v4u*>(qd + sj * 12);
                                    const v4u d0 = dp[0], d1 = dp[1], d2 = dp[2];
#pragma unroll
                                    for (int i = 0; i < 4; i++) {
                                        K0 = __builtin_amdgcn_sdot8((int)w[i], (int)d0[i], K0, false);
                                        K1 = __builtin_amdgcn_sdot8((int)w[i], (int)d1[i], K1, false);
                                        K2 = __builtin_amdgcn_sdot8((int)w[i], (int)d2[i], K2, false);
                                    }
                                } else {
#pragma unroll
                                    for (int b = 0; b < 32; b++) {
                                        const int code = (int)(w[b >> 3] << (28 - 4 * (b & 7))) >> 28;
                                        D = fmaf((float)(2 * code + 1), Q[sj * KC + b], D);
                                    }
                                }
                            }
                        }
                        wave_sync();
                    }
                    if (valid) {
                        float b;
                        if constexpr (SK4_INT) {
                            // kappa = 2 code + 1: K = sum qhat kappa = 2 sum qhat code + sum qhat
                            const int K = 2 * (256 * K2 + 16 * K1 + K0) + p.prune_qsum;
                            b = prune_score_bound_sketchq(acc[0], vinv, sk_a, sk_rho, K, p.prune_qscale, p.dim, p.prune_qt, p.prune_qe1, p.prune_qn, qinv[0],
                                                          p.metric == OTT_METRIC_COSINE, take_max);
                        } else {
                            b = prune_score_bound_sketchb(acc[0], vinv, sk_a, sk_rho, D, 15.0, p.prune_stage * KC, p.dim, p.prune_qt, p.prune_q1,
                                                          p.prune_qn, qinv[0], p.metric == OTT_METRIC_COSINE, take_max);
                        }
                        keep = !(b == b && ord_of(b, take_max) < gate);  // (NaN: no bound, the row is finished)
                    }
                }
            } else if constexpr (SK == 3) {
                if (gate != 0) {  // (wave-uniform; the line is in R)
                    v4f X[SK3_XP];
#pragma unroll
                    for (int i = 0; i < SK3_XP; i++) X[i] = R[7];
                    const uint32_t np = p.sk_pitch >> 2;
                    if (np > 8) {  // the pieces beyond the eight: they arrive while the first stages are decoded
                        const uint64_t lr = row0 + ((uint32_t)lane < cnt ? (uint32_t)lane : cnt - 1);
                        const v4f* sp = reinterpret_cast<const v4f*>(p.prune_sketch + lr * (uint64_t)p.sk_pitch);
#pragma unroll
                        for (int i = 0; i < SK3_XP; i++) X[i] = __builtin_nontemporal_load(sp + ((uint32_t)(8 + i) < np ? (uint32_t)(8 + i) : np - 1));
                    }
                    auto word = [&](int k) -> uint32_t {  // line word k (a constant once unrolled)
                        const v4f v = (k >> 2) < 8 ? R[(k >> 2) & 7] : X[((k >> 2) - 8) % SK3_XP];
                        return __float_as_uint(v[k & 3]);
                    };
                    float D = 0.0f;
#pragma unroll
                    for (int j = 0; j < SK3_MAXST; j++) {
                        const uint32_t sj = p.sk_stage0 + (uint32_t)j;
                        if (sj >= p.prune_stage && sj < nstages) {
                            const uint32_t w[3] = {word(2 + 3 * j), word(3 + 3 * j), word(4 + 3 * j)};
#pragma unroll
                            for (int b = 0; b < 32; b++) {
                                const int pos = 3 * b, lo = pos & 31;
                                uint32_t x = w[pos >> 5] >> lo;
                                if (lo + 3 > 32) x |= w[(pos >> 5) + 1] << (32 - lo);
                                const int code = (int)(x << 29) >> 29;
                                D = fmaf((float)(2 * code + 1), Q[sj * KC + b], D);
                            }
                        }
                    }
                    if (valid) {
                        const float b = prune_score_bound_sketchb(acc[0], vinv, __uint_as_float(word(0)), __uint_as_float(word(1)), D, 7.0, p.prune_stage * KC,
                                                                  p.dim, p.prune_qt, p.prune_q1, p.prune_qn, qinv[0], p.metric == OTT_METRIC_COSINE, take_max);
                        keep = !(b == b && ord_of(b, take_max) < gate);  // (NaN: no bound, the row is finished)
                    }
                }
            } else if constexpr (SK == 1) {
                if (gate != 0) {  // (wave-uniform)
                    // D = q_t . s in f32: the sign bit of dim 32 s + b moves to bit 31 and makes +-1.0, one fma per dim (exact product)
                    float D = 0.0f;
#pragma unroll
                    for (int j = 0; j < SK_MAXW; j++) {
                        const uint32_t sj = p.sk_stage0 + (uint32_t)j;
                        if (sj >= p.prune_stage && sj < nstages) {
                            const uint32_t w = skl[2 + j];
#pragma unroll
                            for (int b = 0; b < 32; b++) {
                                const float sg = __uint_as_float(((w << (31 - b)) & 0x80000000u) | 0x3F800000u);
                                D = fmaf(sg, Q[sj * KC + b], D);
                            }
                        }
                    }
                    if (valid) {
                        const float b = prune_score_bound_sketch(acc[0], vinv, __uint_as_float(skl[0]), __uint_as_float(skl[1]), D, p.prune_stage * KC,
                                                                 p.dim, p.prune_qt, p.prune_q1, p.prune_qn, qinv[0], p.metric == OTT_METRIC_COSINE, take_max);
                        keep = !(b == b && ord_of(b, take_max) < gate);  // (NaN: no bound, the row is finished)
                    }
                }
            } else if (valid && gate != 0) {
                const float b = prune_score_bound(acc[0], vsq, vinv, p.prune_stage * KC, p.dim, p.prune_qt, p.prune_qn, qinv[0],
                                                  p.metric == OTT_METRIC_COSINE, take_max);
                keep = !(b == b && ord_of(b, take_max) < gate);  // (NaN: no bound, the row is finished)
            }
            const uint64_t km = __ballot(keep);
            if (keep) {
                const uint32_t at = (pq_head + pq_n + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))) & (PQ_CAP - 1);
#pragma unroll
                for (int l = 0; l < 8; l++) pq[l * PQ_CAP + at] = acc[0][l];
                pq[8 * PQ_CAP + at] = vinv;
                pq_row[at] = (uint32_t)my_row;
            }
            pq_n += (uint32_t)__popcll(km);
            if (pq_n >= 64) pq_finish(64);
            continue;
        }

        // scores -> filter -> top-k gate
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            if ((uint32_t)q < nq_here) {
                float s = __fadd_rn(reduce8(acc[q], p.reduce), tail[q]);
                if (p.metric == OTT_METRIC_COSINE) s = __fmul_rn(__fmul_rn(s, qinv[q]), vinv);  // vec_compute.rs:31
                bool pass = valid && !(s != s) && cmp_holds(s, p.cmp, p.thr);  // NaN dropped: vec_compute.rs:237
                if constexpr (I8) {
                    // the APPROXIMATE score (the host relaxed the filter by the pass's error bound); a row outside the error
                    // model is listed whatever it scores, ahead of everything
                    s = (float)(iacc[0] + iacc[1]) * i8_rf;
                    pass = valid && !(s != s) && cmp_holds(s, p.cmp, p.thr);
                    if (i8_forced) {
                        s = take_max ? __builtin_inff() : -__builtin_inff();
                        pass = valid;
                    }
                }
                // (flat: every passing score ranks the same — as 0.0, a value the hit lists can carry — so the list keeps the FIRST k
                // passing pairs in visit order: the fill phase of the reference's collector, src/vec_compute.rs:257-266; used by
                // the reference tie order only)
                const uint64_t key = ((uint64_t)ord_of(p.flat ? 0.0f : s, take_max) << 32) | (uint32_t)(~((uint32_t)my_row + p.tie_off));
                if (DUMP) {
                    // large k: append every passing (key, query); the device radix sort orders them afterwards
                    const bool keep = pass && (uint32_t)(key >> 32) >= dgate[q];
                    const uint64_t m = __ballot(keep);
                    if (m) {
                        const uint32_t c = (uint32_t)__popcll(m);
                        if (dqn + c > DUMP_QCAP) dq_flush();
                        if (keep) {
                            const uint32_t at = dqn + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                            dq_key[at] = key;
                            dq_q[at] = p.q0 + q;
                        }
                        dqn += c;
                    }
                } else {
                    constexpr int li_max = NL - 1;
                    const int li = PERQ ? q : 0;
                    const int lx = li <= li_max ? li : 0;
                    if (fresh[lx]) {  // (wave-uniform) nothing in this list yet
                        wl_fill_sorted(L[lx], tk[lx], tq[lx], p.k, pass, key, p.q0 + q, lane, p.tie_sh);
                        fresh[lx] = false;
                        continue;
                    }
                    if constexpr (!BLK) wl_offer(L[lx], tk[lx], tq[lx], p.k, pass, key, p.q0 + q, lane, p.tie_sh);
                    else wl_offer_block(L[lx], tk[lx], tq[lx], p.k, pass, key, p.q0 + q, lane, p.tie_sh);
                }
            }
        }
    }

    if constexpr (CHK) {
        if (pq_n) {  // (< 64 left)
            const uint32_t own = (uint32_t)(tk[0] >> 32);
            pq_drain(pq_n, own > theta ? own : theta);
        }
        if (p.prune_tails != nullptr && lane == 0) {
            if (queued != 0) atomicAdd(p.prune_tails, (unsigned long long)queued);
            if (tails_done != 0) atomicAdd(p.prune_tails + 1, (unsigned long long)tails_done);
        }
    } else if constexpr (PRUNE) {
        if (pq_n) {  // (< 64 left; without the narrow finish the wide one is called directly, not through pq_finish_any: the wrapper
                     // moved a few registers in the head form's E = 2 and E = 4 kernels, this way they compile to the code they had)
            if constexpr (FEW) pq_finish_any(pq_n);
            else pq_finish(pq_n);
        }
        if (p.prune_tails != nullptr && tails_done != 0 && lane == 0) atomicAdd(p.prune_tails, (unsigned long long)tails_done);
    }
    if (DUMP) {
        dq_flush();
        return;
    }
    // block merge: waves 1..3 publish a list to LDS, wave 0 folds it in, then writes the block list
    Cand* sl = reinterpret_cast<Cand*>(smem);
#pragma unroll
    for (int i = 0; i < NL; i++) {
        __syncthreads();
        if (wave > 0) {
#pragma unroll
            for (int e = 0; e < E; e++) {
                Cand c;
                c.key = L[i].key[e];
                c.q = L[i].q[e];
                c.pad = 0;
                sl[(wave - 1) * KS + e * 64 + lane] = c;
            }
        }
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < BW - 1; w++) {
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const uint32_t ppos = e * 64 + lane;
                    const Cand c = sl[w * KS + ppos];
                    // (a register of another wave's list is already sorted: entries past k or empty become sentinels, which sort last)
                    const bool real = ppos < p.k && c.key != 0;
                    if constexpr (!BLK) {
                        wl_offer(L[i], tk[i], tq[i], p.k, real, c.key, c.q, lane, p.tie_sh);
                    } else {
                        const bool pass = real && before(c.key, c.q, tk[i], tq[i], p.tie_sh);
                        if (__popcll(__ballot(pass)) < WL_BLOCK_MIN) {
                            wl_offer(L[i], tk[i], tq[i], p.k, pass, c.key, c.q, lane, p.tie_sh);
                        } else {
                            wl_merge_sorted(L[i], real ? c.key : 0ull, real ? c.q : 0xFFFFFFFFu, lane, p.tie_sh);
                            wl_tau(L[i], p.k, tk[i], tq[i]);
                        }
                    }
                }
            }
            Cand* dst;
            if (PERQ) dst = p.lists + ((size_t)(p.q0 + i) * gridDim.x + blockIdx.x) * p.list_stride;
            else dst = p.lists + (size_t)blockIdx.x * p.list_stride;
            if (!PERQ || (uint32_t)i < nq_here) {
#pragma unroll
                for (int e = 0; e < E; e++) {
                    Cand c;
                    c.key = L[i].key[e];
                    c.q = L[i].q[e];
                    c.pad = 0;
                    dst[e * 64 + lane] = c;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// rows8: the small-store kernel, EIGHT LANES PER ROW (single query, merged, k <= 128).
//
// A store of a few thousand rows is one launch of latencies, not a stream: with lane = row a 64-row tile is ONE wave that
// issues all of the tile's 768 multiply-adds per lane on one SIMD (a 10k-row store is 157 such waves on 256 CUs: three
// SIMDs in four idle, 37-48 us whatever was tried on the memory side).  Here lane l of an 8-lane group owns accumulator
// chain l of the reference's f32x8 (src/vec_compute.rs:9-22: acc[l] += q[8j + l] * v[8j + l], strictly in j order), so
// a wave scores 8 rows with an eighth of the dependent work per lane, a 64-row tile is a WORKGROUP of 8 waves spread
// over the CU's four SIMDs, and the horizontal sum is three cross-lane adds in exactly wide's AVX order
// ((l0+l4)+(l2+l6))+((l1+l5)+(l3+l7)) — each lane computes the same tree up to operand order, and IEEE addition
// commutes bit for bit.  Same bits as exact_kernel by construction; the tests hold all three variants to the oracle.
// Rows are read straight from global memory, one float per lane and step (a wave instruction touches 8 rows x 32 B; the
// four steps that share a 128-B line hit in the vector L1), the query sits in LDS and is read by broadcast.
// Epilogue: the 64 scores of the tile go through LDS to wave 0, which builds the block list exactly like the other variants.
// ---------------------------------------------------------------------------------------------
constexpr int R8_WAVES = 8;
constexpr int R8_UNROLL = 12;
constexpr int R8_SMEM_MAX = (8 * (int)SMALL_QMAX + 8 * 64 + 64) * 4;  // 8 queries of 2048 floats + scores: 67.8 KB

// NQ queries share a pass (1, 2, 4 or 8: small batches on small stores; each lane then carries NQ accumulators for its chain),
// PERQ = one list per query instead of one merged list.  Dynamic LDS: [NQ x dimq query floats | NQ x 64 scores | 64 validity words].
template <int MK, int E, int NQ, bool PERQ>
__global__ __launch_bounds__(64 * R8_WAVES) void exact_rows8_kernel(ExactParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sQ = smem;                                 // [NQ][dimq]
    float* sS = smem + (size_t)NQ * p.dimq;           // [NQ][64]
    uint32_t* sV = reinterpret_cast<uint32_t*>(sS + NQ * 64);  // [64]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane >> 3, c = lane & 7;
    typedef __attribute__((address_space(4))) const float* CF32;
    typedef __attribute__((address_space(4))) const uint32_t* CU32;
    typedef __attribute__((address_space(4))) const ott_run* CRUN;
    typedef __attribute__((address_space(4))) const char* CCH;
    const CCH karg = (CCH)__builtin_amdgcn_kernarg_segment_ptr();
    const CF32 Q = p.embedded ? (CF32)(karg + __builtin_offsetof(ExactParams, qemb)) : (CF32)(p.queries + (size_t)p.q0 * p.dimq);
    const CU32 tile_prefix = p.embedded ? (CU32)(karg + __builtin_offsetof(ExactParams, eprefix)) : (CU32)p.tile_prefix;
    const CRUN runs = p.embedded ? (CRUN)(karg + __builtin_offsetof(ExactParams, eruns)) : (CRUN)p.runs;
    const uint32_t nq_here = (p.nq_total - p.q0) < (uint32_t)NQ ? (p.nq_total - p.q0) : (uint32_t)NQ;
    float qinv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) qinv[q] = (uint32_t)q < nq_here ? (p.embedded ? p.eqinv : p.qinv[p.q0 + q]) : 0.0f;
    // (the uploaded query block is zero padded to a multiple of 8 queries: rows past nq_here read as zeros)
    for (uint32_t i = threadIdx.x; i < (uint32_t)NQ * p.dimq; i += 64 * R8_WAVES) sQ[i] = Q[i];

    // tile -> run of surviving chunks (wave-uniform scalar search), as in exact_kernel
    const uint32_t t = blockIdx.x;
    uint32_t lo = 0, hi = p.n_runs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_prefix[mid] <= t) lo = mid;
        else hi = mid;
    }
    const uint64_t rstart = runs[lo].start, rcount = runs[lo].count;
    const uint64_t off = (uint64_t)(t - tile_prefix[lo]) * 64;
    const uint64_t row0 = rstart + off;
    const uint32_t cnt = (rcount - off) < 64 ? (uint32_t)(rcount - off) : 64u;
    const uint32_t lrow = 8u * (uint32_t)wave + (uint32_t)grp;  // this lane group's row within the tile
    bool valid = lrow < cnt;
    const uint64_t my_row = row0 + (valid ? lrow : cnt - 1);     // loads of a row past the tile's end are clamped, never skipped
    if (p.row_mask != nullptr && valid && my_row < p.row_mask_bits) valid = (p.row_mask[my_row >> 6] >> (my_row & 63)) & 1;  // src/vec.rs:231-237
    const float* rp = p.rows + my_row * (uint64_t)p.ld;
    float vinv = 0.0f;
    if (p.metric == OTT_METRIC_COSINE) vinv = p.inv[my_row];
    __syncthreads();  // the queries are in LDS

    // chain c of the row, for every query of the pass: acc = acc + q[8j + c] * v[8j + c], j ascending (vec_compute.rs:12-13, 39-42)
    const uint32_t full = p.dim >> 3;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = 0.0f;
    auto step = [&](uint32_t jj, float xv) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float qv = sQ[(uint32_t)q * p.dimq + 8 * jj + c];
            acc[q] = __fadd_rn(acc[q], exact_term<MK>(qv, xv));
        }
    };
    uint32_t j = 0;
    for (; j + R8_UNROLL <= full; j += R8_UNROLL) {
        float x[R8_UNROLL];
#pragma unroll
        for (int u = 0; u < R8_UNROLL; u++) x[u] = rp[8 * (j + u) + c];
#pragma unroll
        for (int u = 0; u < R8_UNROLL; u++) step(j + u, x[u]);
    }
    for (; j < full; j++) step(j, rp[8 * j + c]);
    // remainder: sequential sum of the last dim % 8 products (vec_compute.rs:15-21, 44-53); every lane of the group computes it
    float tail[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) tail[q] = 0.0f;
    const uint32_t nt = p.dim & 7u;
    for (uint32_t l = 0; l < nt; l++) {
        const float xv = rp[8 * full + l];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float qv = sQ[(uint32_t)q * p.dimq + 8 * full + l];
            tail[q] = __fadd_rn(tail[q], exact_term<MK>(qv, xv));
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        // wide::f32x8::reduce_add across the group's eight lanes
        float sum;
        if (p.reduce == OTT_REDUCE_SEQ4) {
            const int b = lane & ~7;
            float l8[8];
#pragma unroll
            for (int i = 0; i < 8; i++) l8[i] = __shfl(acc[q], b + i);
            sum = reduce8(l8, OTT_REDUCE_SEQ4);
        } else {
            const float s1 = __fadd_rn(acc[q], __shfl_xor(acc[q], 4));  // l_c + l_{c^4}
            const float s2 = __fadd_rn(s1, __shfl_xor(s1, 2));          // (l0+l4)+(l2+l6) on even-pair lanes, (l1+l5)+(l3+l7) on the others
            sum = __fadd_rn(s2, __shfl_xor(s2, 1));
            // lanes with c odd hold ((l1+l5)+(l3+l7)) + ((l0+l4)+(l2+l6)): the same value (a + b == b + a bit for bit)
        }
        float sc = __fadd_rn(sum, tail[q]);
        if (p.metric == OTT_METRIC_COSINE) sc = __fmul_rn(__fmul_rn(sc, qinv[q]), vinv);  // vec_compute.rs:31
        if (c == 0) sS[q * 64 + lrow] = sc;
    }
    if (c == 0) sV[lrow] = valid ? 1u : 0u;
    __syncthreads();

    // lane = row of the tile: filter, key, block list(s) (as exact_kernel's epilogue for a wave's first tile).  Merged: wave 0
    // folds the NQ x 64 candidates into one list; per query: wave q builds query q's list
    const bool take_max = p.take_max != 0;
    const bool ok = sV[lane] != 0;
    const uint64_t row = row0 + lane;
    auto cand_of = [&](int q, bool& pass, uint64_t& key) {
        const float s = sS[q * 64 + lane];
        pass = ok && !(s != s) && cmp_holds(s, p.cmp, p.thr);  // NaN dropped: vec_compute.rs:237
        key = ((uint64_t)ord_of(p.flat ? 0.0f : s, take_max) << 32) | (uint32_t)(~((uint32_t)row + p.tie_off));
    };
    if (p.dump_keys != nullptr) {
        // large-k / default-take path on small stores (ott_sort.hip): every passing (key, query) pair of the tile is appended
        // behind the cursor instead of entering a top-k list — wave q lists query q's 64 rows (NQ <= 8 waves), and the WORKGROUP
        // takes its place in the list with ONE atomic for all its queries (one per (tile, query) queued 628 atomics on one
        // address behind a 10k-row sweep of four queries: 44 us of a 54-us kernel)
        static_assert(NQ <= R8_WAVES, "one wave per query of the pass");
        __shared__ uint32_t sDC[R8_WAVES];
        __shared__ unsigned long long sDB;
        bool pass = false;
        uint64_t key = 0;
        if (wave < NQ && (uint32_t)wave < nq_here) {
            cand_of(wave, pass, key);
            // second phase of the two-phase large-k path: pairs below their query's gate cannot be in the result (see exact_kernel)
            if (p.dump_gate != nullptr) pass = pass && (uint32_t)(key >> 32) >= p.dump_gate[p.q0 + (uint32_t)wave];
        }
        const unsigned long long m = __ballot(pass);
        const uint32_t cnt_q = (uint32_t)__popcll(m);
        if (lane == 0) sDC[wave] = cnt_q;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
#pragma unroll
            for (int w = 0; w < R8_WAVES; w++) total += sDC[w];
            sDB = total ? atomicAdd(p.dump_cursor, (unsigned long long)total) : 0ull;
        }
        __syncthreads();
        if (pass) {
            unsigned long long at = sDB + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; w++) at += sDC[w];
            if (at < p.dump_cap) {
                p.dump_keys[at] = key;
                p.dump_q[at] = p.q0 + (uint32_t)wave;
            }
        }
        return;
    }
    if constexpr (PERQ) {
        if (wave >= NQ || (uint32_t)wave >= nq_here) return;
        bool pass;
        uint64_t key;
        cand_of(wave, pass, key);
        WaveList<E> L;
        wl_init(L);
        uint64_t tk = 0;
        uint32_t tq = 0xFFFFFFFFu;
        wl_fill_sorted(L, tk, tq, p.k, pass, key, p.q0 + wave, lane, p.tie_sh);
        Cand* dst = p.lists + ((size_t)(p.q0 + wave) * gridDim.x + blockIdx.x) * p.list_stride;
#pragma unroll
        for (int e = 0; e < E; e++) {
            Cand cd;
            cd.key = L.key[e];
            cd.q = L.q[e];
            cd.pad = 0;
            dst[e * 64 + lane] = cd;
        }
    } else {
        if (wave != 0) return;
        WaveList<E> L;
        wl_init(L);
        uint64_t tk = 0;
        uint32_t tq = 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            if ((uint32_t)q >= nq_here) break;
            bool pass;
            uint64_t key;
            cand_of(q, pass, key);
            if (q == 0) {
                wl_fill_sorted(L, tk, tq, p.k, pass, key, p.q0 + q, lane, p.tie_sh);
            } else {
                wl_offer_block(L, tk, tq, p.k, pass, key, p.q0 + q, lane, p.tie_sh);  // (the next query's 64 scores against a list of 64: as a block)
            }
        }
        Cand* dst = p.lists + (size_t)blockIdx.x * p.list_stride;
#pragma unroll
        for (int e = 0; e < E; e++) {
            Cand cd;
            cd.key = L.key[e];
            cd.q = L.q[e];
            cd.pad = 0;
            dst[e * 64 + lane] = cd;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// final merge of partial lists -> k hits   (src/meta.rs:699-709: concat, sort, truncate)
// ---------------------------------------------------------------------------------------------
constexpr int MERGE_WAVES = 16;

// PARTIAL: first of two stages (k > 64, a thousand block lists, a few queries: one workgroup walking them all took 0.18 ms at
// k = 100 and 0.69 ms at k = 256) — workgroup (group, part) merges the lists [part * per, (part + 1) * per) of its group into
// ONE list of KS entries (same Cand format, sentinel keys behind the real ones) in `out_lists`; the second stage is this
// kernel again, not PARTIAL, over the `parts` lists of each group.
template <int E, bool PARTIAL>
__device__ __forceinline__ void merge_walk(float* smem, const Cand* lists, uint32_t n_lists, uint32_t list_stride, uint64_t group_stride, uint32_t k,
                                           uint32_t take_max, uint64_t base, ott_hit* out, uint64_t out_stride, uint64_t* counts, Cand* out_lists,
                                           uint32_t parts, uint32_t tie_sh) {
    constexpr int KS = 64 * E;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t group = PARTIAL ? blockIdx.x / parts : blockIdx.x, part = PARTIAL ? blockIdx.x % parts : 0u;
    const uint32_t per = PARTIAL ? (n_lists + parts - 1) / parts : n_lists;
    const uint32_t l_begin = part * per, l_end = (l_begin + per) < n_lists ? (l_begin + per) : n_lists;
    const Cand* gl = lists + (size_t)group * group_stride;

    WaveList<E> L;
    wl_init(L);
    uint64_t tk = 0;
    uint32_t tq = 0xFFFFFFFFu;
    // Column-wise walk: each lane owns one sorted partial list and offers its elements in order.
    // A list dies as soon as one of its elements no longer beats the running k-th key (everything
    // deeper in it is worse), so the number of dependent load rounds is the depth of the deepest
    // contributing list (a few), not the number of lists.
    for (uint32_t l0 = l_begin + (uint32_t)wave * 64; l0 < l_end; l0 += MERGE_WAVES * 64) {
        const uint32_t li = l0 + lane;
        const Cand* src = gl + (size_t)(li < l_end ? li : l_begin) * list_stride;
        bool alive = li < l_end;
        bool any = true;
        for (uint32_t depth = 0; depth < k && any; depth += 4) {
            // four consecutive entries (one 64-B line) per lane per round trip
            Cand c4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c4[j].key = 0;
                c4[j].q = 0xFFFFFFFFu;
                if (alive && depth + j < k) c4[j] = src[depth + j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const Cand c = c4[j];
                const bool pass = alive && c.key != 0 && before(c.key, c.q, tk, tq, tie_sh);
                if (__ballot(pass) == 0) {
                    any = false;
                    break;
                }
                wl_offer(L, tk, tq, k, pass, c.key, c.q, lane, tie_sh);
                alive = pass && !before(tk, tq, c.key, c.q, tie_sh);  // still in the list (it is at least the k-th)
            }
        }
    }
    Cand* sl = reinterpret_cast<Cand*>(smem);
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            Cand c;
            c.key = L.key[e];
            c.q = L.q[e];
            c.pad = 0;
            sl[(wave - 1) * KS + e * 64 + lane] = c;
        }
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 0; w < MERGE_WAVES - 1; w++) {
#pragma unroll
            for (int e = 0; e < E; e++) {
                const uint32_t ppos = e * 64 + lane;
                const Cand c = sl[w * KS + ppos];
                wl_offer(L, tk, tq, k, ppos < k && c.key != 0, c.key, c.q, lane, tie_sh);
            }
        }
        if constexpr (PARTIAL) {
#pragma unroll
            for (int e = 0; e < E; e++) {
                const uint32_t ppos = e * 64 + lane;
                Cand c;
                c.key = ppos < k ? L.key[e] : 0ull;
                c.q = L.q[e];
                c.pad = 0;
                out_lists[(size_t)blockIdx.x * KS + ppos] = c;
            }
            return;
        }
        uint32_t total = 0;
        ott_hit* o = out + (size_t)blockIdx.x * out_stride;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t ppos = e * 64 + lane;
            const bool real = ppos < k && L.key[e] != 0;
            ott_hit h;  // every slot of the KS-wide output is written: real hits first, then sentinels
            h.index = ~0ull;
            h.score = __uint_as_float(0xFFFFFFFFu);
            h.query = 0xFFFFFFFFu;
            if (real) {
                h.index = base + (uint32_t)(~(uint32_t)(L.key[e] & 0xFFFFFFFFull));
                h.score = score_of((uint32_t)(L.key[e] >> 32), take_max != 0);
                h.query = L.q[e];
            }
            o[ppos] = h;
            total += __popcll(__ballot(real));
        }
        if (lane == 0) counts[blockIdx.x] = total;
    }
}

template <int E, bool PARTIAL = false>
__global__ __launch_bounds__(1024) void merge_kernel(const Cand* lists, uint32_t n_lists, uint32_t list_stride,
                                                      uint64_t group_stride, uint32_t k, uint32_t take_max, uint64_t base,
                                                      ott_hit* out, uint64_t out_stride, uint64_t* counts, Cand* out_lists,
                                                      uint32_t parts, uint32_t tie_sh) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    merge_walk<E, PARTIAL>(smem, lists, n_lists, list_stride, group_stride, k, take_max, base, out, out_stride, counts, out_lists, parts, tie_sh);
}

// The want-th largest of n u32 values in LDS (1 <= want <= n), by the whole 1024-thread workgroup: four 8-bit radix-select
// passes from the top.  s_hist: 256 words, s_ctl: 2 words.  Ends with a barrier.
__device__ __forceinline__ uint32_t block_select_kth_largest(const uint32_t* s_vals, uint32_t n, uint32_t want, uint32_t* s_hist, uint32_t* s_ctl, uint32_t tid) {
    uint32_t prefix = 0;
    for (int pass = 3; pass >= 0; pass--) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        const uint32_t shift = (uint32_t)pass * 8;
        const uint32_t himask = pass == 3 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (uint32_t l = tid; l < n; l += 1024) {
            const uint32_t v = s_vals[l];
            if ((v & himask) == prefix) atomicAdd(&s_hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: the digit holding the want-th largest value, from 255 down (4 digits per lane)
            const uint32_t d0 = 255u - 4u * tid;
            const uint32_t c0 = s_hist[d0], c1 = s_hist[d0 - 1], c2 = s_hist[d0 - 2], c3 = s_hist[d0 - 3];
            uint32_t incl = c0 + c1 + c2 + c3;  // inclusive scan over the lanes
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
                if ((int)tid >= off) incl += o;
            }
            const uint32_t excl = incl - (c0 + c1 + c2 + c3);
            if (excl < want && incl >= want) {  // exactly one lane
                uint32_t acc = excl, d = d0;
                if (acc + c0 < want) { acc += c0; d = d0 - 1;
                    if (acc + c1 < want) { acc += c1; d = d0 - 2;
                        if (acc + c2 < want) { acc += c2; d = d0 - 3; } } }
                s_ctl[0] = prefix | (d << shift);
                s_ctl[1] = want - acc;
            }
        }
        __syncthreads();
        prefix = s_ctl[0];
        want = s_ctl[1];
    }
    __syncthreads();
    return prefix;
}

// merge_rank_kernel (round 3): the merge of up to MS_VMAX sorted block lists per result group WITHOUT inserting candidates one
// at a time (merge_walk's wl_offer: 55-120 us for a top-100 over 16-500 lists — more than the scoring of a small store).
//  (1) a bound: the k-th largest score ordinal among the lists' first j = ceil(2 k / n_lists) entries — the exact k-th best of
//      a subset of about 2 k candidates, so the result's k-th best is no worse (one 4-pass radix select in LDS).  (First
//      version: the ceil(k / j)-th largest of the lists' j-th entries alone — with few lists that is the WORST list's j-th
//      entry, and a top-512 over 40 lists overflowed the survivor buffer: 0.87 ms on a 10k-row store);
//  (2) every list is walked from its head while its entries reach the bound (lists are sorted: typically one to three 64-B
//      lines) and the survivors — about k plus one per list — are appended to an LDS buffer;
//  (3) a survivor's rank is the number of survivors in front of it in the result order (`before`: a total order on (key,
//      query) pairs), counted against the LDS buffer; rank < k writes the hit to its slot.
// Ties at the bound are all kept, so any tie rule (`tie_sh`) is decided by (3) alone.  More than MS_CAP survivors (a plateau
// of equal scores across many lists) or more than MS_VMAX lists: merge_walk, in the same launch.
constexpr uint32_t MS_VMAX = 4096;   // lists per result group
constexpr uint32_t MS_NVAL = 8192;   // ordinals the bound is selected from (n_lists x j <= n_lists + k)
constexpr uint32_t MS_CAP = 2048;
constexpr size_t MS_SMEM = (size_t)(MS_NVAL + 256 + 8) * 4 + (size_t)MS_CAP * sizeof(Cand);

// (the merge itself: one copy of its text for the two kernels below)
template <int E>
__device__ __forceinline__ void merge_rank(float* smem, const Cand* lists, uint32_t n_lists, uint32_t list_stride, uint64_t group_stride, uint32_t k,
                                           uint32_t take_max, uint64_t base, ott_hit* out, uint64_t out_stride, uint64_t* counts, uint32_t tie_sh) {
    constexpr uint32_t KS = 64 * E;
    uint32_t* s_vals = reinterpret_cast<uint32_t*>(smem);  // [MS_NVAL] the score ordinals of the lists' first j entries
    uint32_t* s_hist = s_vals + MS_NVAL;                   // [256]
    uint32_t* s_ctl = s_hist + 256;                        // [8] 0 = selected prefix, 1 = rank still wanted, 2 = survivors
    Cand* s_buf = reinterpret_cast<Cand*>(s_ctl + 8);      // [MS_CAP]
    const uint32_t tid = threadIdx.x;
    const Cand* gl = lists + (size_t)blockIdx.x * group_stride;
    const uint32_t kk = k < KS ? k : KS;  // entries of a list that can matter
    bool slow = n_lists > MS_VMAX || n_lists == 0 || kk == 0;
    if (!slow) {
        // twice the k candidates the bound needs: the k-th largest of EXACTLY k values is their minimum — the worst list's
        // j-th entry again (k = 200 over 40 lists: j = 5, 200 values, every list walked to its end, 213 us for this kernel)
        const uint32_t j2 = (2 * kk + n_lists - 1) / n_lists;
        const uint32_t j = j2 < kk ? j2 : kk;  // 1 .. kk; n_lists j < n_lists + 2 kk <= MS_NVAL
        const uint32_t n_vals = n_lists * j;
        for (uint32_t v = tid; v < n_vals; v += 1024) {
            const uint64_t key = gl[(size_t)(v / j) * list_stride + (v % j)].key;
            s_vals[v] = key != 0 ? (uint32_t)(key >> 32) : 0u;  // (a list shorter than j: ordinal 0, below every real one)
        }
        __syncthreads();
        const uint32_t prefix = block_select_kth_largest(s_vals, n_vals, kk, s_hist, s_ctl, tid);  // 0: fewer than k real entries there — no bound
        const uint32_t bound = prefix;
        if (tid == 0) s_ctl[2] = 0;
        __syncthreads();
        for (uint32_t l = tid; l < n_lists; l += 1024) {
            const Cand* src = gl + (size_t)l * list_stride;
            bool more = true;
            for (uint32_t depth = 0; depth < kk && more; depth += 4) {
                Cand c4[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    c4[i].key = 0;
                    c4[i].q = 0xFFFFFFFFu;
                    if (depth + i < kk) c4[i] = src[depth + i];
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (!more) break;
                    if (c4[i].key == 0 || (uint32_t)(c4[i].key >> 32) < bound) {
                        more = false;
                        break;
                    }
                    const uint32_t pos = atomicAdd(&s_ctl[2], 1u);
                    if (pos < MS_CAP) s_buf[pos] = c4[i];
                }
            }
        }
        __syncthreads();
        const uint32_t C = s_ctl[2];
        if (C <= MS_CAP) {
            ott_hit* o = out + (size_t)blockIdx.x * out_stride;
            for (uint32_t i = tid; i < C; i += 1024) {
                const Cand me = s_buf[i];
                uint32_t r = 0;
#pragma unroll 8
                for (uint32_t x = 0; x < C; x++) {
                    const Cand c = s_buf[x];
                    r += before(c.key, c.q, me.key, me.q, tie_sh) ? 1u : 0u;
                }
                if (r < kk) {
                    ott_hit h;
                    h.index = base + (uint32_t)(~(uint32_t)(me.key & 0xFFFFFFFFull));
                    h.score = score_of((uint32_t)(me.key >> 32), take_max != 0);
                    h.query = me.q;
                    o[r] = h;
                }
            }
            const uint32_t total = C < kk ? C : kk;
            for (uint32_t i = total + tid; i < KS; i += 1024) {  // every slot of the KS-wide output is written: sentinels behind the hits
                ott_hit h;
                h.index = ~0ull;
                h.score = __uint_as_float(0xFFFFFFFFu);
                h.query = 0xFFFFFFFFu;
                o[i] = h;
            }
            if (tid == 0) counts[blockIdx.x] = total;
            return;
        }
        slow = true;
        __syncthreads();  // the LDS is about to be reused
    }
    merge_walk<E, false>(smem, lists, n_lists, list_stride, group_stride, k, take_max, base, out, out_stride, counts, (Cand*)nullptr, 1u, tie_sh);
}

template <int E>
__global__ __launch_bounds__(1024) void merge_rank_kernel(const Cand* lists, uint32_t n_lists, uint32_t list_stride, uint64_t group_stride, uint32_t k,
                                                           uint32_t take_max, uint64_t base, ott_hit* out, uint64_t out_stride, uint64_t* counts,
                                                           uint32_t tie_sh) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    merge_rank<E>(smem, lists, n_lists, list_stride, group_stride, k, take_max, base, out, out_stride, counts, tie_sh);
}

// The same launch for k <= 64 as the pruned sweep's final merge on host output (ott_exact_plan.h: prune_plan_ride): it also leaves
// the sweep's two counter totals (`tails`: final when this kernel starts, it is stream-ordered behind the gated launch) at
// `totals`, behind the result block in pinned host memory, so no copy is queued behind the merge
__global__ __launch_bounds__(1024) void merge_rank_totals_kernel(const Cand* lists, uint32_t n_lists, uint32_t list_stride, uint64_t group_stride, uint32_t k,
                                                                  uint32_t take_max, uint64_t base, ott_hit* out, uint64_t out_stride, uint64_t* counts,
                                                                  uint32_t tie_sh, unsigned long long* tails, unsigned long long* totals) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals[0] = __hip_atomic_load(tails, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        totals[1] = __hip_atomic_load(tails + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    merge_rank<1>(smem, lists, n_lists, list_stride, group_stride, k, take_max, base, out, out_stride, counts, tie_sh);
}

// merge_small_kernel: the same merge for k <= 64 (one list entry per lane), i.e. every top-10 call.  What cost merge_kernel<1> its
// 24-28 us was not memory but `wl_offer`'s one-candidate-at-a-time insertion: 64 list heads per wave offered serially, then
// wave 0 folding fifteen other waves' lists the same way.  Here (1) a wave SORTS the 64 heads it fetched with a bitonic
// network over the lanes (21 shuffle steps) — that IS its initial list, and its k-th key gates everything deeper; (2) only
// lists whose head made the wave's top k are walked further (a few serial offers); (3) the sixteen wave lists are folded as a
// binary tree (four levels of k offers in parallel instead of fifteen in a row).
__global__ __launch_bounds__(64 * MERGE_WAVES) void merge_small_kernel(const Cand* lists, uint32_t n_lists, uint32_t list_stride,
                                                                        uint64_t group_stride, uint32_t k, uint32_t take_max, uint64_t base,
                                                                        ott_hit* out, uint64_t out_stride, uint64_t* counts, uint32_t tie_sh) {
    __shared__ Cand sl[MERGE_WAVES * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Cand* gl = lists + (size_t)blockIdx.x * group_stride;
    WaveList<1> L;
    wl_init(L);
    uint64_t tk = 0;
    uint32_t tq = 0xFFFFFFFFu;
    for (uint32_t base_l = (uint32_t)wave * 64; base_l < n_lists; base_l += MERGE_WAVES * 64) {
        const uint32_t li = base_l + lane;
        const Cand* src = gl + (size_t)(li < n_lists ? li : 0) * list_stride;
        Cand head;
        head.key = 0;
        head.q = 0xFFFFFFFFu;
        if (li < n_lists) head = src[0];
        bool alive;
        if (base_l == (uint32_t)wave * 64) {
            // first round: the wave's list is empty, so the sorted heads ARE the list.  Bitonic sort, best first
            uint64_t sk = head.key;
            uint32_t sq = head.q;
            wave_sort_desc(sk, sq, lane, tie_sh);
            L.key[0] = (uint32_t)lane < k ? sk : 0ull;
            L.q[0] = (uint32_t)lane < k ? sq : 0xFFFFFFFFu;
            wl_tau(L, k, tk, tq);
            alive = head.key != 0 && !before(tk, tq, head.key, head.q, tie_sh);  // the head made the list (it is at least the k-th)
        } else {
            const bool pass = head.key != 0 && before(head.key, head.q, tk, tq, tie_sh);
            wl_offer(L, tk, tq, k, pass, head.key, head.q, lane, tie_sh);
            alive = pass && !before(tk, tq, head.key, head.q, tie_sh);
        }
        // deeper entries of the lists still alive, four (one 64-B line) per round trip
        bool any = __ballot(alive) != 0;
        for (uint32_t depth = 1; depth < k && any; depth += 4) {
            Cand c4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c4[j].key = 0;
                c4[j].q = 0xFFFFFFFFu;
                if (alive && depth + j < k) c4[j] = src[depth + j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const Cand c = c4[j];
                const bool pass = alive && c.key != 0 && before(c.key, c.q, tk, tq, tie_sh);
                if (__ballot(pass) == 0) {
                    any = false;
                    break;
                }
                wl_offer(L, tk, tq, k, pass, c.key, c.q, lane, tie_sh);
                alive = pass && !before(tk, tq, c.key, c.q, tie_sh);
            }
        }
    }
    // binary-tree fold of the wave lists
#pragma unroll
    for (int step = 1; step < MERGE_WAVES; step <<= 1) {
        if ((wave & (2 * step - 1)) == step) {
            Cand c;
            c.key = L.key[0];
            c.q = L.q[0];
            c.pad = 0;
            sl[wave * 64 + lane] = c;
        }
        __syncthreads();
        if ((wave & (2 * step - 1)) == 0) {
            const Cand c = sl[(wave + step) * 64 + lane];
            wl_offer(L, tk, tq, k, (uint32_t)lane < k && c.key != 0, c.key, c.q, lane, tie_sh);
        }
        __syncthreads();
    }
    if (wave == 0) {
        const bool real = (uint32_t)lane < k && L.key[0] != 0;
        ott_hit h;  // every slot of the 64-wide output is written: real hits first, then sentinels
        h.index = ~0ull;
        h.score = __uint_as_float(0xFFFFFFFFu);
        h.query = 0xFFFFFFFFu;
        if (real) {
            h.index = base + (uint32_t)(~(uint32_t)(L.key[0] & 0xFFFFFFFFull));
            h.score = score_of((uint32_t)(L.key[0] >> 32), take_max != 0);
            h.query = L.q[0];
        }
        out[(size_t)blockIdx.x * out_stride + lane] = h;
        const uint32_t total = (uint32_t)__popcll(__ballot(real));
        if (lane == 0) counts[blockIdx.x] = total;
    }
}

// ---------------------------------------------------------------------------------------------
// cross-GPU merge: n_lists candidate lists of ott_hit (each best-first, sentinel padded, in
// shard order) -> k best.  Candidate id = list*list_len + pos breaks ties, which equals the
// canonical (row, query) order because shard g holds lower global rows than shard g+1.
// ---------------------------------------------------------------------------------------------
template <int E>
__device__ __forceinline__ void merge_hits_walk(float* smem, const ott_hit* lists_all, uint32_t n_lists, uint32_t n_groups, uint32_t list_len, uint32_t k,
                                                uint32_t take_max, ott_hit* out_all, uint64_t* count, size_t rank_stride) {
    // one workgroup per group (= query in PER_QUERY mode): list `li` of group g starts at ((li * n_groups) + g) * list_len,
    // the layout an all-gather of per-GPU [n_groups][list_len] blocks produces
    const uint32_t grp = blockIdx.x;
    const size_t gstride = rank_stride;  // hits between consecutive ranks' blocks (n_groups * list_len, plus any header slots)
    const ott_hit* lists = lists_all + (size_t)grp * list_len;
    constexpr int KS = 64 * E;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WaveList<E> L;
    wl_init(L);
    uint64_t tk = 0;
    uint32_t tq = 0xFFFFFFFFu;
    for (uint32_t li = wave; li < n_lists; li += MERGE_WAVES) {
        for (uint32_t c0 = 0; c0 < list_len; c0 += 64) {
            const uint32_t pos = c0 + lane;
            bool pass = false;
            uint64_t key = 0;
            if (pos < list_len) {
                const ott_hit h = lists[(size_t)li * gstride + pos];
                pass = h.index != ~0ull && !(h.score != h.score);
                key = ((uint64_t)ord_of(h.score, take_max != 0) << 32) | (uint32_t)(~(li * list_len + pos));
            }
            if (__ballot(pass && before(key, 0, tk, tq, 0u)) == 0) break;
            wl_offer(L, tk, tq, k, pass, key, 0u, lane, 0u);
        }
    }
    Cand* sl = reinterpret_cast<Cand*>(smem);
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            Cand c;
            c.key = L.key[e];
            c.q = L.q[e];
            c.pad = 0;
            sl[(wave - 1) * KS + e * 64 + lane] = c;
        }
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 0; w < MERGE_WAVES - 1; w++) {
#pragma unroll
            for (int e = 0; e < E; e++) {
                const uint32_t ppos = e * 64 + lane;
                const Cand c = sl[w * KS + ppos];
                wl_offer(L, tk, tq, k, ppos < k && c.key != 0, c.key, c.q, lane, 0u);
            }
        }
        uint32_t total = 0;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t ppos = e * 64 + lane;
            const bool real = ppos < k && L.key[e] != 0;
            ott_hit h;
            h.index = ~0ull;
            h.score = __uint_as_float(0xFFFFFFFFu);
            h.query = 0xFFFFFFFFu;
            if (real) {
                const uint32_t id = ~(uint32_t)(L.key[e] & 0xFFFFFFFFull);
                h = lists[(size_t)(id / list_len) * gstride + id % list_len];
            }
            out_all[(size_t)grp * KS + ppos] = h;
            total += __popcll(__ballot(real));
        }
        if (lane == 0) count[grp] = total;
    }
}

// merge_hits_kernel (round 3): the same merge by bound + gather + rank (see merge_rank_kernel): every real hit of the group's
// lists whose score ordinal reaches the bound goes to an LDS buffer as (ordinal << 32 | ~candidate id), its rank is the number
// of larger keys there, rank < k writes the hit.  A world of 8 x top-100 is 800 candidates: no insertion chain on the path
// between the all-gather and the host.  Overflow of the buffer (plateaus over many shards): merge_hits_walk, same launch.
template <int E>
__global__ __launch_bounds__(1024) void merge_hits_kernel(const ott_hit* lists_all, uint32_t n_lists, uint32_t n_groups, uint32_t list_len,
                                                           uint32_t k, uint32_t take_max, ott_hit* out_all, uint64_t* count, uint32_t walk,
                                                           uint32_t rank_stride, uint32_t hdr_slots, ott_hit* hdr_out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr uint32_t KS = 64 * E;
    uint32_t* s_vals = reinterpret_cast<uint32_t*>(smem);      // [MS_NVAL] the score ordinals of the lists' first j hits
    uint32_t* s_hist = s_vals + MS_NVAL;                       // [256]
    uint32_t* s_ctl = s_hist + 256;                            // [8] 0, 1 = the select's, 2 = survivors, 3 = a NaN was met
    uint64_t* s_key = reinterpret_cast<uint64_t*>(s_ctl + 8);  // [MS_CAP]
    const uint32_t tid = threadIdx.x;
    const uint32_t grp = blockIdx.x;
    const size_t gstride = rank_stride;  // hits between consecutive ranks' blocks
    const ott_hit* lists = lists_all + (size_t)grp * list_len;
    // the ranks' block headers (status of every shard's scoring, ott_comm.hip) travel behind their hits: handed to the host here
    if (grp == 0 && hdr_out != nullptr)
        for (uint32_t i = tid; i < n_lists * hdr_slots; i += 1024)
            hdr_out[i] = lists_all[(size_t)(i / hdr_slots) * gstride + (size_t)n_groups * list_len + (i % hdr_slots)];
    const uint32_t kk = k < KS ? k : KS;
    const uint32_t depth_max = list_len < kk ? list_len : kk;  // entries of a list that can matter
    if (!walk && n_lists > 0 && n_lists <= MS_VMAX && depth_max > 0 && (uint64_t)n_lists * list_len < 0xFFFFFFFFull) {
        const uint32_t j0 = (2 * kk + n_lists - 1) / n_lists;  // twice the k candidates the bound needs (see merge_rank_kernel)
        const uint32_t j = j0 < depth_max ? j0 : depth_max;
        const uint32_t n_vals = n_lists * j;  // < n_lists + 2 kk <= MS_NVAL
        for (uint32_t v = tid; v < n_vals; v += 1024) {
            const ott_hit h = lists[(size_t)(v / j) * gstride + (v % j)];
            s_vals[v] = (h.index != ~0ull && !(h.score != h.score)) ? ord_of(h.score, take_max != 0) : 0u;
        }
        if (tid == 0) {
            s_ctl[2] = 0;
            s_ctl[3] = 0;  // a NaN score inside a list (never produced by ott_query_device; the walk below would count it among a list's first j): merge_hits_walk
        }
        __syncthreads();
        // the k-th largest of those ordinals (0 = fewer than k real hits there: no bound)
        const uint32_t sel = n_vals >= kk ? block_select_kth_largest(s_vals, n_vals, kk, s_hist, s_ctl, tid) : 0u;
        if (tid == 0) s_ctl[0] = sel;
        __syncthreads();
        const uint32_t bound = s_ctl[0];
        for (uint32_t l = tid; l < n_lists; l += 1024) {
            for (uint32_t pos = 0; pos < depth_max; pos++) {
                const ott_hit h = lists[(size_t)l * gstride + pos];
                if (h.index == ~0ull) break;  // sentinels behind the real hits
                if (h.score != h.score) {
                    s_ctl[3] = 1u;
                    break;
                }
                const uint32_t o = ord_of(h.score, take_max != 0);
                if (o < bound) break;
                const uint32_t at = atomicAdd(&s_ctl[2], 1u);
                if (at < MS_CAP) s_key[at] = ((uint64_t)o << 32) | (uint32_t)(~(l * list_len + pos));
            }
        }
        __syncthreads();
        const uint32_t C = s_ctl[2];
        if (C <= MS_CAP && s_ctl[3] == 0) {
            for (uint32_t i = tid; i < C; i += 1024) {
                const uint64_t me = s_key[i];
                uint32_t r = 0;
#pragma unroll 8
                for (uint32_t x = 0; x < C; x++) r += s_key[x] > me ? 1u : 0u;
                if (r < kk) {
                    const uint32_t id = ~(uint32_t)(me & 0xFFFFFFFFull);
                    out_all[(size_t)grp * KS + r] = lists[(size_t)(id / list_len) * gstride + id % list_len];
                }
            }
            const uint32_t total = C < kk ? C : kk;
            for (uint32_t i = total + tid; i < KS; i += 1024) {
                ott_hit h;
                h.index = ~0ull;
                h.score = __uint_as_float(0xFFFFFFFFu);
                h.query = 0xFFFFFFFFu;
                out_all[(size_t)grp * KS + i] = h;
            }
            if (tid == 0) count[grp] = total;
            return;
        }
        __syncthreads();  // the LDS is about to be reused
    }
    merge_hits_walk<E>(smem, lists_all, n_lists, n_groups, list_len, k, take_max, out_all, count, gstride);
}

int launch_merge_hits(ott_store* s, const ott_hit* lists, uint32_t n_lists, uint32_t n_groups, uint32_t list_len, uint32_t k, int E,
                      bool take_max, ott_hit* out, uint64_t* count, uint32_t hdr_slots, ott_hit* hdr_out) {
    const uint32_t rank_stride = n_groups * list_len + hdr_slots;
    const size_t smem_w = (size_t)(MERGE_WAVES - 1) * 64 * E * sizeof(Cand);
    const size_t smem_r = (size_t)(MS_NVAL + 256 + 8) * 4 + (size_t)MS_CAP * 8;
    const size_t smem = smem_w > smem_r ? smem_w : smem_r;
    const uint32_t walk = s->opt.merge_walk ? 1u : 0u;
#define OTT_MH(Ev)                                                                                                   \
    if (E == Ev) {                                                                                                   \
        if (smem > 64 * 1024) {                                                                                      \
            static std::atomic<uint64_t> attr_set{0};                                                                \
            if (ott::attr_needed(attr_set, s->device)) {                                                         \
                OTT_HIP(hipFuncSetAttribute((const void*)merge_hits_kernel<Ev>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); \
                ott::attr_done(attr_set, s->device);                                                     \
            }                                                                                                        \
        }                                                                                                            \
        hipLaunchKernelGGL((merge_hits_kernel<Ev>), dim3(n_groups), dim3(64 * MERGE_WAVES), smem, s->stream, lists, n_lists, \
                           n_groups, list_len, k, take_max ? 1u : 0u, out, count, walk, rank_stride, hdr_slots, hdr_out); \
        OTT_HIP(hipGetLastError());                                                                                  \
        return OTT_OK;                                                                                               \
    }
    OTT_MH(1) OTT_MH(2) OTT_MH(4) OTT_MH(8)
#undef OTT_MH
    return fail(OTT_ERR_INVALID, "launch_merge_hits: bad E");
}

// ---------------------------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------------------------
int exact_grid(const ott_store* s, uint32_t n_tiles) {
    uint32_t want = (n_tiles + WAVES - 1) / WAVES;
    uint32_t cap = (uint32_t)s->n_cu * BLOCKS_PER_CU;
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

// the pruned sweep (p.prune_stage != 0): its queue takes the dynamic LDS past 48 KB
template <int E, bool BLK, int SK, bool SEED = false, bool CHK = false>
static int launch_prune(ott_store* s, const ExactParams& p, int grid) {
    auto kern = exact_kernel<MK_DOT, 1, E, false, false, false, BLK, false, true, SK, SEED, CHK>;
    constexpr int smem = CHK ? EXACT_SMEM_CHECK : EXACT_SMEM_PRUNE;  // (the check's int8 operand sits behind the digit planes)
    static std::atomic<uint64_t> attr_set{0};
    if (ott::attr_needed(attr_set, s->device)) {
        OTT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        ott::attr_done(attr_set, s->device);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// (the head form exists with the integer decode only: an -DOTT_SK4_DECODE_F32 experiment build never plans it; and for lists of
// up to four entries per lane only, k <= 256: with eight the kernel needs 256 VGPRs + 8 AGPRs, runs one wave per SIMD and measured
// slower than the c = 1 form, so prune_plan_head never asks for it and it is not instantiated)
template <int E, bool BLK>
static int launch_prune_head(ott_store* s, const ExactParams& p, int grid) {
    if constexpr (SK4_INT && E == 1) {  // (the estimate pass of the seed: k <= 64 only, prune_plan_seed_est)
        if (p.seed_est != 0) return launch_prune<E, BLK, 5, true>(s, p, grid);
    }
    if (p.seed_est != 0) return fail(OTT_ERR_INVALID, "launch_exact: the estimate pass needs the integer decode and a list of k <= 64");
    // (the int8 check of the survivors, p.chk_plane != nullptr: instantiated for k <= 64, which is all prune_plan_i8_check asks for)
    if constexpr (SK4_INT && E == 1) {
        if (p.chk_plane != nullptr) {
            if (p.i8_scale == nullptr || p.flag == nullptr || p.dim > OTT_QEMB_MAX) return fail(OTT_ERR_INVALID, "launch_exact: the int8 check needs the plane's scales and flags and a query of up to 896 dims");
            return launch_prune<E, BLK, 5, false, true>(s, p, grid);
        }
    }
    if (p.chk_plane != nullptr) return fail(OTT_ERR_INVALID, "launch_exact: the int8 check needs the integer decode and a list of k <= 64");
    if constexpr (SK4_INT && E <= 4) return launch_prune<E, BLK, 5>(s, p, grid);
    else return fail(OTT_ERR_INVALID, "launch_exact: the head form needs the integer decode and a list of k <= 256");
}

template <int MK, int NQ, int E, bool PERQ>
static int launch_one(ott_store* s, const ExactParams& p, int grid) {
    if constexpr (MK == MK_DOT && NQ == 1 && !PERQ) {
        if (p.prune_stage != 0) {
            uint32_t sk = p.prune_sketch != nullptr ? p.sk_bits : 0u;  // the sketch form: the store keeps a tail sketch of 1, 3 or 4 bits per dim
            if (p.prune_head_codes != nullptr) {  // the head form: four bits per dim, no f32 stage in front (instantiated as SK = 5)
                if (sk != 4 || p.prune_head_rho == nullptr || !SK4_INT) return fail(OTT_ERR_INVALID, "launch_exact: the head belongs to the four-bit sketch and its integer decode");
                sk = 5;
            }
            if (sk != 0 && sk != 1 && sk != 3 && sk != 4 && sk != 5) return fail(OTT_ERR_INVALID, "launch_exact: a tail sketch has one, three or four bits per dim");
            if constexpr (E == 1) {
                if (p.k > 16)  // (see BLK)
                    return sk == 5 ? launch_prune_head<1, true>(s, p, grid) : sk == 4 ? launch_prune<1, true, 4>(s, p, grid) : sk == 3 ? launch_prune<1, true, 3>(s, p, grid) : sk == 1 ? launch_prune<1, true, 1>(s, p, grid) : launch_prune<1, true, 0>(s, p, grid);
            }
            return sk == 5 ? launch_prune_head<E, (E > 1)>(s, p, grid) : sk == 4 ? launch_prune<E, (E > 1), 4>(s, p, grid) : sk == 3 ? launch_prune<E, (E > 1), 3>(s, p, grid) : sk == 1 ? launch_prune<E, (E > 1), 1>(s, p, grid) : launch_prune<E, (E > 1), 0>(s, p, grid);
        }
    }
    if (p.prune_stage != 0) return fail(OTT_ERR_INVALID, "launch_exact: the pruned sweep takes one query, cosine / dot, merged");
#ifdef OTT_MFMA_DEBUG_BUILD  // round 2's one-wave LDS-DMA variant (SMALL): retired in round 5 (31 us against rows8's 10 on 10k x 768), instantiated in the diagnostic build only
    if constexpr (NQ == 1 && E <= 2 && !PERQ) {
        if (p.small == 1) {
            static std::atomic<uint64_t> attr_set{0};  // > 64 KB of dynamic LDS needs the opt-in, once per DEVICE (idempotent: a race only repeats it)
            auto kern = exact_kernel<MK, NQ, E, PERQ, false, true>;
            if (ott::attr_needed(attr_set, s->device)) {
                OTT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, EXACT_SMEM_SMALL));
                ott::attr_done(attr_set, s->device);
            }
            hipLaunchKernelGGL(kern, dim3(grid), dim3(64), EXACT_SMEM_SMALL, s->stream, p);
            OTT_HIP(hipGetLastError());
            return OTT_OK;
        }
    }
#else
    if (p.small == 1) return fail(OTT_ERR_UNSUPPORTED, "exact_small = 1 (the one-wave LDS-DMA variant) exists in the diagnostic build only");
#endif
    if constexpr (E == 1) {
        if (p.k > 16) {  // (see BLK)
            hipLaunchKernelGGL((exact_kernel<MK, NQ, E, PERQ, false, false, true>), dim3(grid), dim3(256), EXACT_SMEM, s->stream, p);
            OTT_HIP(hipGetLastError());
            return OTT_OK;
        }
    }
    hipLaunchKernelGGL((exact_kernel<MK, NQ, E, PERQ>), dim3(grid), dim3(256), EXACT_SMEM, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

template <int MK>
static int launch_pass(ott_store* s, const ExactParams& p, int nq_tile, int E, int grid) {
    const bool perq = p.perq != 0 && nq_tile > 1;
#define OTT_CASE(NQv, Ev, PQ) \
    if (nq_tile == NQv && E == Ev && perq == PQ) return launch_one<MK, NQv, Ev, PQ>(s, p, grid);
    OTT_CASE(1, 1, false) OTT_CASE(2, 1, false) OTT_CASE(4, 1, false)
    OTT_CASE(1, 2, false) OTT_CASE(2, 2, false) OTT_CASE(4, 2, false)
    OTT_CASE(1, 4, false) OTT_CASE(1, 8, false)
    OTT_CASE(2, 1, true) OTT_CASE(4, 1, true)
    OTT_CASE(2, 2, true) OTT_CASE(4, 2, true)
#undef OTT_CASE
    return fail(OTT_ERR_INVALID, "launch_exact: no kernel for this (nq_tile, E, mode)");
}

int launch_exact_dump(ott_store* s, const ExactParams& p, int nq_tile, int grid) {
#define OTT_DUMP(MKv)                                                                                                                     \
    if (nq_tile == 1) hipLaunchKernelGGL((exact_kernel<MKv, 1, 1, false, true>), dim3(grid), dim3(256), EXACT_SMEM_DUMP, s->stream, p); \
    else hipLaunchKernelGGL((exact_kernel<MKv, 4, 1, false, true>), dim3(grid), dim3(256), EXACT_SMEM_DUMP, s->stream, p);
    switch (metric_kind(p.metric)) {
        case MK_L2: OTT_DUMP(MK_L2) break;
        case MK_L1: OTT_DUMP(MK_L1) break;
        default: OTT_DUMP(MK_DOT) break;
    }
#undef OTT_DUMP
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// rows8 (p.small == 2): eight lanes per row, one 8-wave workgroup per 64-row tile, 1 / 2 / 4 / 8 queries per pass
template <int MK>
static int launch_rows8(ott_store* s, const ExactParams& p, int nq_tile, int E, int grid) {
    const bool perq = p.perq != 0 && nq_tile > 1;
    const size_t smem = ((size_t)nq_tile * p.dimq + (size_t)nq_tile * 64 + 64) * 4;
#define OTT_R8(NQv, Ev, PQ)                                                                                           \
    if (nq_tile == NQv && E == Ev && perq == PQ) {                                                                    \
        auto kern = exact_rows8_kernel<MK, Ev, NQv, PQ>;                                                              \
        if (smem > 48 * 1024) {                                                                                       \
            static std::atomic<uint64_t> attr_set{0};                                                                 \
            if (ott::attr_needed(attr_set, s->device)) {                                                          \
                OTT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, R8_SMEM_MAX)); \
                ott::attr_done(attr_set, s->device);                                                      \
            }                                                                                                         \
        }                                                                                                             \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * R8_WAVES), smem, s->stream, p);                                \
        OTT_HIP(hipGetLastError());                                                                                   \
        return OTT_OK;                                                                                                \
    }
    OTT_R8(1, 1, false) OTT_R8(2, 1, false) OTT_R8(4, 1, false) OTT_R8(8, 1, false)
    OTT_R8(1, 2, false) OTT_R8(2, 2, false) OTT_R8(4, 2, false) OTT_R8(8, 2, false)
    OTT_R8(2, 1, true) OTT_R8(4, 1, true) OTT_R8(8, 1, true)
    OTT_R8(2, 2, true) OTT_R8(4, 2, true) OTT_R8(8, 2, true)
#undef OTT_R8
    return fail(OTT_ERR_INVALID, "launch_exact: no rows8 kernel for this (nq_tile, E, mode)");
}

int launch_exact_i8(ott_store* s, const ExactParams& p, int E, int grid) {
    switch (E) {
        case 2: hipLaunchKernelGGL((exact_kernel<MK_DOT, 1, 2, false, false, false, true, true>), dim3(grid), dim3(256), EXACT_SMEM, s->stream, p); break;
        case 4: hipLaunchKernelGGL((exact_kernel<MK_DOT, 1, 4, false, false, false, true, true>), dim3(grid), dim3(256), EXACT_SMEM, s->stream, p); break;
        case 8: hipLaunchKernelGGL((exact_kernel<MK_DOT, 1, 8, false, false, false, true, true>), dim3(grid), dim3(256), EXACT_SMEM, s->stream, p); break;
        default: return fail(OTT_ERR_INVALID, "launch_exact_i8: the candidate list holds 128, 256 or 512 entries");
    }
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

int launch_exact(ott_store* s, const ExactParams& p, int nq_tile, int E, int grid) {
    switch (metric_kind(p.metric)) {
        case MK_L2: return p.small == 2 ? launch_rows8<MK_L2>(s, p, nq_tile, E, grid) : launch_pass<MK_L2>(s, p, nq_tile, E, grid);
        case MK_L1: return p.small == 2 ? launch_rows8<MK_L1>(s, p, nq_tile, E, grid) : launch_pass<MK_L1>(s, p, nq_tile, E, grid);
        default: return p.small == 2 ? launch_rows8<MK_DOT>(s, p, nq_tile, E, grid) : launch_pass<MK_DOT>(s, p, nq_tile, E, grid);
    }
}

int launch_merge(ott_store* s, const Cand* lists, uint32_t n_lists, uint32_t list_stride, uint64_t group_stride,
                 uint32_t groups, uint32_t k, int E, bool take_max, uint64_t base_offset, ott_hit* out_hits,
                 uint64_t out_stride, uint64_t* out_counts, uint32_t tie_sh, unsigned long long* tails, unsigned long long* totals) {
    if (totals != nullptr) {  // (ott_exact_plan.h: prune_plan_ride — k <= 64 and the merge options at their defaults)
        if (E != 1 || tails == nullptr || s->opt.merge_rank1 == 0 || s->opt.merge_walk || n_lists > MS_VMAX)
            return fail(OTT_ERR_INVALID, "launch_merge: the counters ride with the rank merge of k <= 64 only");
        hipLaunchKernelGGL(merge_rank_totals_kernel, dim3(groups), dim3(1024), MS_SMEM, s->stream, lists, n_lists, list_stride, group_stride, k, take_max ? 1u : 0u,
                           base_offset, out_hits, out_stride, out_counts, tie_sh, tails, totals);
        OTT_HIP(hipGetLastError());
        return OTT_OK;
    }
    if (E == 1 && !(s->opt.merge_rank1 != 0 && !s->opt.merge_walk && n_lists <= MS_VMAX)) {  // option merge_rank1 = 0: k <= 64 through sorted heads + tree fold (round 2's merge)
        hipLaunchKernelGGL(merge_small_kernel, dim3(groups), dim3(64 * MERGE_WAVES), 0, s->stream, lists, n_lists, list_stride, group_stride, k,
                           take_max ? 1u : 0u, base_offset, out_hits, out_stride, out_counts, tie_sh);
        OTT_HIP(hipGetLastError());
        return OTT_OK;
    }
    const size_t smem = (size_t)(MERGE_WAVES - 1) * 64 * E * sizeof(Cand);
    if (n_lists <= MS_VMAX && !s->opt.merge_walk) {  // bound, gather, rank (merge_rank_kernel); merge_walk inside it when a plateau overflows the LDS buffer
        const size_t smem_r = smem > MS_SMEM ? smem : MS_SMEM;
#define OTT_MR(Ev)                                                                                                   \
    if (E == Ev) {                                                                                                   \
        auto kern = merge_rank_kernel<Ev>;                                                                           \
        if (smem_r > 64 * 1024) {                                                                                    \
            static std::atomic<uint64_t> attr_set{0};                                                                \
            if (ott::attr_needed(attr_set, s->device)) {                                                         \
                OTT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_r)); \
                ott::attr_done(attr_set, s->device);                                                     \
            }                                                                                                        \
        }                                                                                                            \
        hipLaunchKernelGGL(kern, dim3(groups), dim3(1024), smem_r, s->stream, lists, n_lists, list_stride, group_stride, k, take_max ? 1u : 0u, \
                           base_offset, out_hits, out_stride, out_counts, tie_sh);                                   \
        OTT_HIP(hipGetLastError());                                                                                  \
        return OTT_OK;                                                                                               \
    }
        OTT_MR(1) OTT_MR(2) OTT_MR(4) OTT_MR(8)
#undef OTT_MR
    }
    // two stages when one workgroup per query would walk hundreds of long lists on its own: 32 parts first, then their merge
    const uint32_t parts = (n_lists >= 256 && groups <= 8) ? 32u : 1u;
    Cand* mid = nullptr;
    if (parts > 1) {
        int rc = s->d_lists2.ensure((size_t)groups * parts * 64 * E * sizeof(Cand));
        if (rc) return rc;
        mid = (Cand*)s->d_lists2.p;
    }
#define OTT_M(Ev)                                                                                                     \
    if (E == Ev) {                                                                                                    \
        if (parts > 1) {                                                                                              \
            hipLaunchKernelGGL((merge_kernel<Ev, true>), dim3(groups * parts), dim3(64 * MERGE_WAVES), smem, s->stream, lists, n_lists, \
                               list_stride, group_stride, k, take_max ? 1u : 0u, base_offset, (ott_hit*)nullptr, (uint64_t)0, \
                               (uint64_t*)nullptr, mid, parts, tie_sh);                                               \
            OTT_HIP(hipGetLastError());                                                                               \
            hipLaunchKernelGGL((merge_kernel<Ev, false>), dim3(groups), dim3(64 * MERGE_WAVES), smem, s->stream, (const Cand*)mid, parts, \
                               (uint32_t)(64 * Ev), (uint64_t)parts * 64 * Ev, k, take_max ? 1u : 0u, base_offset, out_hits, \
                               out_stride, out_counts, (Cand*)nullptr, 1u, tie_sh);                                   \
        } else {                                                                                                      \
            hipLaunchKernelGGL((merge_kernel<Ev, false>), dim3(groups), dim3(64 * MERGE_WAVES), smem, s->stream, lists, n_lists, \
                               list_stride, group_stride, k, take_max ? 1u : 0u, base_offset, out_hits, out_stride,   \
                               out_counts, (Cand*)nullptr, 1u, tie_sh);                                               \
        }                                                                                                             \
        OTT_HIP(hipGetLastError());                                                                                   \
        return OTT_OK;                                                                                                \
    }
    OTT_M(1) OTT_M(2) OTT_M(4) OTT_M(8)
#undef OTT_M
    return fail(OTT_ERR_INVALID, "launch_merge: bad E");
}

}  // namespace ott
