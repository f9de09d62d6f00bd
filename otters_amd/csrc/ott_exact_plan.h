// ott_exact_plan.h — what the exact path's host side (run_exact, ott_api.hip: the fused register top-k of k <= 512) decides before
// it launches anything, free of HIP and of ott_store: plain C++17 over plain values, like ott_sort_plan.h, so that the CPU suite
// compiles the very code libotters_hip.so ships on its own (tests/test_exact_plan_cpu.py).  Each of these is written here once:
//   * lists or sort path, the list width E and the list stride;
//   * which kernel variant sweeps (streaming, one-wave, rows8), and the one predicate "a small variant fits" that the sort path
//     (ott_sort_plan.h: sweep_shape) and the path choice (ott_policy.h: choose_path) share with it;
//   * queries per pass, passes and the number of block lists (the streaming kernel's grid comes in: exact_grid, ott_exact.hip);
//   * whether a call is "lean" (its inputs ride in the kernel arguments);
//   * the pruned sweep: eligibility, form, checkpoint and seed;
//   * the layout of the result block, and what a call reports as bytes scanned.
#pragma once
#include <stddef.h>

#include "../../include/otters_hip.h"  // (and through it stdint.h)

namespace ott {

// ---- limits of the kernel arguments ------------------------------------------------------------------------------------------------
constexpr uint32_t OTT_QEMB_MAX = 896;  // floats of the query embedded in ExactParams (kernel arguments are limited to 4 KB)
// Code words of a sketch line that the sketch form's kernel decodes.  The embedded query holds at most 28 stages, so a three-bit
// sketch of the last 5/8 has at most 18 stages of three words (with a and rho fourteen 16-B pieces), a sign sketch of the last
// quarter at most 7 words; a store with more takes the 7/8 form.
constexpr uint32_t OTT_SKETCH_MAX_WORDS = 54;
constexpr uint32_t OTT_SKETCH1_MAX_WORDS = 10;  // the sign form keeps its words in registers across the stages: three 16-B loads
// the four-bit form: up to 27 of the 28 stages sketched, four words each (a line of up to 28 16-B pieces, streamed eight at a time)
constexpr uint32_t OTT_SKETCH4_MAX_WORDS = 108;

// ---- lists or sort -----------------------------------------------------------------------------------------------------------------
inline int list_E(uint64_t k) { return k <= 64 ? 1 : k <= 128 ? 2 : k <= 256 ? 4 : 8; }  // register list entries per lane for k <= 512
inline uint32_t list_stride(int E) { return 64u * (uint32_t)E; }                           // KS: slots of one list, a wave's lanes x E

enum ExactRoute {
    EXACT_LISTS,    // the fused register top-k
    EXACT_SORT,     // score dump + device radix sort (run_large_k)
    EXACT_REFUSED,  // k > 512 with device output: the sort path is host-output only
};
// k > 512 is beyond the fused register top-k.  Below that:
// 128 < k <= 512 — four and eight list entries per lane — against the sort path (profiles/round3/large_k_from.md).  Round 2:
// the lists lost from 256 up (9.7 against 6.0 ms at 10M x 768, k = 512), and once the sort path's second phase listed only
// what can still make the result they lost from 128 up.  With candidates merged into the lists as sorted blocks
// (wl_merge_sorted) and the block lists merged by rank (merge_rank_kernel) a SINGLE query is faster on the lists at every k
// they hold and every store size measured (10k rows: 0.16 against 0.23 ms at k = 512; 10M rows: 4.81 against 4.93).  Several
// queries still go to the sort path from 128 up — its sweep carries four of them, a sweep of the long lists one: 1M rows, 4
// queries, k = 300: 1.0 against 2.5 ms — unless the store is small (100k rows x 4 queries: lists 0.45 against 0.58 ms).
// `large_k_from` > 0 (store option) replaces the rule's threshold; `fetch`: host output.
inline ExactRoute lists_or_sort(uint64_t k_eff, uint32_t nq, uint64_t rows_scored, int large_k_from, bool fetch) {
    if (k_eff > 512) return fetch ? EXACT_SORT : EXACT_REFUSED;
    const uint64_t pairs = rows_scored * nq;
    const uint64_t from = large_k_from > 0 ? (uint64_t)large_k_from : ((nq == 1 || pairs <= (1ull << 19)) ? 512u : 128u);
    return k_eff > from && fetch && pairs <= (1ull << 28) ? EXACT_SORT : EXACT_LISTS;
}

// ---- the sweep's kernel variant ----------------------------------------------------------------------------------------------------
// A small variant (a workgroup per 64-row tile) fits stores of up to 1024 tiles ~ 65k rows whose padded query fits the LDS.  The
// lists (exact_variant), the sort path's sweep (sweep_shape) and the path choice (choose_path, with its own estimate of the tiles)
// each add their own conditions to this one.
inline bool small_variant_fits(uint32_t dimq, uint64_t tiles) { return dimq <= 2048 && tiles <= 1024; }
// 0 = the streaming kernel, 1 = the one-wave small-grid variant (LDS-DMA ring; single query), 2 = rows8: eight lanes per
// row, one 8-wave workgroup per tile, up to 8 queries per pass (round 3: 10k x 768 in 25-30 us instead of 64; the
// default wherever a small variant fits: batches of up to 16 queries).  `exact_small`: the store option, 0 / 1 / 2 forces the
// choice (a forced variant that does not fit falls back to streaming), negative = rows8 wherever it fits.
inline uint32_t exact_variant(int exact_small, uint32_t nq, bool perq, int E, uint32_t dimq, uint32_t n_tiles) {
    const bool fits = E <= 2 && small_variant_fits(dimq, n_tiles);
    if (exact_small == 1) return fits && nq == 1 && !perq ? 1u : 0u;
    if (exact_small == 2 || exact_small < 0) return fits && nq <= 16 ? 2u : 0u;
    return 0u;
}

// ---- passes, grid, block lists -----------------------------------------------------------------------------------------------------
inline uint32_t pow2_at_least(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
// queries per corpus pass: 4 is the measured sweet spot of the streaming kernel (1-2 queries 4.95 ms, 4 queries 5.3 ms per
// pass at 10M x 768; an 8-wide pass needs 233 VGPRs and ran 14 ms, slower than two 4-wide passes); rows8 takes up to 8
// (one accumulator per query and lane); the long lists (E >= 4) one
inline uint32_t queries_per_pass(uint32_t nq, int E, uint32_t variant) {
    if (E >= 4) return 1;
    const uint32_t most = variant == 2 ? 8u : 4u, p2 = pow2_at_least(nq);
    return p2 < most ? p2 : most;
}
// single query, at most two runs: everything the kernel needs rides in its arguments (no H2D copy, no staging)
inline bool exact_lean(uint32_t nq, uint32_t dimq, size_t n_runs) { return nq == 1 && dimq <= OTT_QEMB_MAX && n_runs <= 2; }

// what one call over the lists looks like
struct ExactPlan {
    int E;             // list entries per lane
    uint32_t KS;       // list stride
    uint32_t variant;  // exact_variant
    uint32_t tile;     // queries per pass
    uint32_t passes;   // launches, = corpus passes (stats)
    int grid;          // workgroups per launch: a tile each under a small variant, else the streaming kernel's persistent grid
    bool lean;
};
// `stream_grid`: the persistent grid of the streaming kernel over n_tiles (exact_grid, ott_exact.hip: it follows from the kernel's
// own constants, which experiment builds override in that file alone)
inline ExactPlan exact_plan(uint64_t k_eff, uint32_t nq, bool perq, uint32_t dimq, uint32_t n_tiles, size_t n_runs, int exact_small, int stream_grid) {
    ExactPlan x;
    x.E = list_E(k_eff);
    x.KS = list_stride(x.E);
    x.variant = exact_variant(exact_small, nq, perq, x.E, dimq, n_tiles);
    x.tile = queries_per_pass(nq, x.E, x.variant);
    x.passes = (nq + x.tile - 1) / x.tile;
    x.grid = x.variant ? (int)n_tiles : stream_grid;
    x.lean = exact_lean(nq, dimq, n_runs);
    return x;
}
// block lists the sweep leaves for the merge: the pruned sweep's two launches; per query: every query's own blocks; merged: one
// list group per pass
inline size_t exact_n_lists(const ExactPlan& x, uint32_t nq, bool perq, bool pruned, int gridA, int gridB) {
    return pruned ? (size_t)(gridA + gridB) : perq ? (size_t)nq * x.grid : (size_t)x.passes * x.grid;
}

// ---- the pruned sweep --------------------------------------------------------------------------------------------------------------
// the large-store seed of the pruned sweep's wide sketch forms: rows / 32.  Experiment builds: -DOTT_X_SEED_DIV=64
#ifndef OTT_X_SEED_DIV
#define OTT_X_SEED_DIV 32
#endif
// the store's tail sketch as the plan sees it
struct SketchState {
    bool present;  // the store holds sketch lines
    bool covers;   // ... for every row (sk_n >= n)
    uint32_t bits, words, stage0;  // bits per dim (1, 3, 4), code words per row, first sketched stage
};
struct PruneIn {
    uint32_t dim, ld, metric;
    bool perq, lean, flat;
    uint32_t variant;
    int exact_prune, exact_sketch;  // store options
    SketchState sk;
    uint64_t rows_scored;
    int E;
};
struct PrunePlan {
    uint32_t c;     // the checkpoint stage; 0 = no pruned sweep
    bool sketch;    // the sketch form, in the store's own width
    uint64_t seed;  // rows of the seed launch
};
// Pruned sweep (store option exact_prune): one query, merged, cosine / dot, the streaming kernel.  A seed of the
// first rows is scored in full and merged; its k-th best gates the second launch over the rest, which skips the last stages (from
// c, 7/8 of them) of every row whose score bound misses it.  Automatic from 2^20 rows and 8 stages (dim >= 225).
// A store that keeps a tail sketch for every row (option exact_sketch) takes the sketch form in the store's own width (option
// exact_sketch_bits): the checkpoint is the sketch's first stage, stage 1 at four bits per dim, 3/8 of the stages at three, 3/4 at one.
// The caller adds two conditions of its own (run_exact: the seed and the rest have at most two runs each and the rest is not
// empty; prune_query_bounds accepts the query).
inline PrunePlan prune_plan(const PruneIn& in) {
    const PrunePlan off{0, false, 0};
    if (!(in.lean && !in.perq && in.variant == 0 && !in.flat && in.exact_prune != 0 && (in.metric == OTT_METRIC_COSINE || in.metric == OTT_METRIC_DOT)))
        return off;
    const uint32_t nst = (in.ld + 31) / 32;
    uint32_t c = nst * 7 / 8;
    while (c > 0 && c * 32 > in.dim - in.dim % 8) c--;  // the prefix holds whole chunks of eight only (no remainder term yet)
    bool sketch = false;
    if (in.exact_sketch != 0 && in.sk.present && in.sk.covers &&
        in.sk.words <= (in.sk.bits == 4 ? OTT_SKETCH4_MAX_WORDS : in.sk.bits == 3 ? OTT_SKETCH_MAX_WORDS : OTT_SKETCH1_MAX_WORDS)) {
        const uint32_t cs = in.sk.stage0;
        if (cs >= 1 && cs < nst && cs * 32 <= in.dim - in.dim % 8) {
            c = cs;
            sketch = true;
        }
    }
    const bool worth = in.exact_prune == 1 || (nst >= 8 && in.rows_scored >= (1ull << 20));
    if (!(worth && c >= 1 && c < nst)) return off;
    // The seed: a tenth of the rows.  With the three- or four-bit sketch and k <= 64, once that is more than 131072 rows: a
    // thirty-second of them, never fewer than 131072 (continuous at 1.31M rows; 10M rows: 312 512 rows read in full instead of
    // 1M, 10M x 768 top-10 2.862 -> 2.753 ms).  A smaller seed gives a lower gate; the wide sketch loses few rows to that, but a
    // longer list's k-th best sits deeper in the seed (k = 500 at 10M x 768: 3.54 -> 3.78 ms with the small seed), and the
    // other forms save less per seed row (their checkpoint is at 3/4 or 7/8 of the row): those keep the tenth
    uint64_t seed = in.rows_scored / 10;
    if (sketch && in.sk.bits >= 3 && in.E == 1 && seed > 131072) seed = in.rows_scored / OTT_X_SEED_DIV > 131072 ? in.rows_scored / OTT_X_SEED_DIV : 131072;
    seed = (seed + 63) & ~63ull;
    if (seed < 64) seed = 64;
    return PrunePlan{c, sketch, seed};
}
// The four-bit form decodes a line against the quantised query (ott_prune.h: prune_query_quant), so a plan in that form needs the
// quantiser to accept the query.  Where it refuses, the call takes the plan it would take had the store no sketch: the 7/8 form
// with its own checkpoint and seed (or none, when prune_query_bounds refuses the query too) — never a slower four-bit decode.
inline bool prune_plan_needs_quant(const PruneIn& in, const PrunePlan& pp) { return pp.c != 0 && pp.sketch && in.sk.bits == 4; }
// The head form of the four-bit sketch (ott_prune.h: prune_sketch4_head_row): the launch runs with its checkpoint in front of stage
// 0 — a gated row reads its line and its head and no f32 stage — when the plan is the four-bit sketch form, the quantiser accepted
// the query, the store's head covers every row and the option (exact_sketch_head) allows it.  The plan itself, its checkpoint and
// its seed stay what prune_plan says; the query-side values are then taken with m = 0.  Lists of up to four entries per lane
// (k <= 256) only: with eight the head kernel needs 256 VGPRs and runs one wave per SIMD, and measured slower than the c = 1 form
// (10M x 768, k = 500: 1.95 against 1.86 ms, profiles/exact_head/README.md).
struct HeadState {
    bool present;  // the store holds a head
    bool covers;   // ... for every row (head_n >= n)
    int option;    // exact_sketch_head: -1 / 1 use it, 0 never
};
inline bool prune_plan_head(const PruneIn& in, const PrunePlan& pp, bool quant_ok, const HeadState& hd) {
    return prune_plan_needs_quant(in, pp) && quant_ok && hd.present && hd.covers && hd.option != 0 && in.E <= 4;
}
// The int8 check of the head form's survivors ("survivors on the int8 plane"; ott_i8_check.h).  A row that passes
// the four-bit bound is scored on the store's int8 plane — 768 B and a scale at dim 768 — and goes on to its 3072-B f32 finish
// only unless that approximate score plus the int8 level's certified error ranks strictly below the gate.  It runs when
//   * the head form runs, with one list entry per lane (k <= 64: the only widths the kernel is instantiated for);
//   * the int8 plane exists and covers every row right now (i8_plane_peek, ott_planes.hip: asking builds nothing, so a store whose background
//     builder has not finished, or that keeps no int8 plane, takes the sweep without the check);
//   * the query is inside the int8 level's error model and its bound is finite (ott_i8_check.h: i8_check_eps);
//   * the option (exact_i8_check: -1 / 1 use it, 0 never) allows it.
// Otherwise the sweep is the one without the check, to the bit and to the launch.  Hits and `rescored` are the same either way.
// Experiment builds: -DOTT_X_I8_CHECK=0 never plans it.
#ifndef OTT_X_I8_CHECK
#define OTT_X_I8_CHECK 1
#endif
struct I8CheckState {
    bool plane_ready;  // i8_plane_peek found the plane covering every row
    int option;        // exact_i8_check
    bool eps_ok;       // the query is query_regular and i8_check_eps gave a finite bound
};
inline bool prune_plan_i8_check(const PruneIn& in, const PrunePlan& pp, bool head, const I8CheckState& ck) {
    return OTT_X_I8_CHECK != 0 && pp.c != 0 && head && in.E == 1 && ck.plane_ready && ck.option != 0 && ck.eps_ok;
}
// The seed as an estimate pass ("the seed by estimate").  The gate only needs k exactly scored rows that score
// well, so in the head form the seed launch need not read its rows in full: it streams their lines, heads and inverse norms,
// ranks them by the decode's estimate (ott_prune.h: prune_score_est_sketchq), and each wave finishes its `keep` best exactly.
// The gated launch then runs over ALL rows and the final merge takes its lists alone.  Returns the rows the estimate pass
// covers, 0 = the full seed launch of prune_plan.  Non-zero only
//   * in the head form with one list entry per lane (k <= 64);
//   * without a score filter: the best rows by estimate might all fail one, the gate would stay open and the gated launch would
//     finish every row, where the full seed finds k passing rows;
//   * from a seed of 131 072 rows (stores from 1 310 720 rows): below, nothing changes.
// Experiment builds: -DOTT_X_SEED_EST=0 keeps the full seed, -DOTT_X_SEED_EST_DIV=16 covers rows / 16 (0 = the plan's seed),
// -DOTT_X_SEED_KEEP=4 finishes four rows per wave (0 = min(k, 16)).
#ifndef OTT_X_SEED_EST
#define OTT_X_SEED_EST 1
#endif
#ifndef OTT_X_SEED_EST_DIV
#define OTT_X_SEED_EST_DIV 0
#endif
#ifndef OTT_X_SEED_KEEP
#define OTT_X_SEED_KEEP 0
#endif
constexpr uint64_t SEED_EST_MIN_ROWS = 131072;
constexpr uint32_t SEED_EST_KEEP_MAX = 16;
// (the estimate pass has the narrow finish only, which takes at most sixteen rows: ott_exact.hip pq_finish_few, ott_finish_few.h FF_MAX_ROWS)
static_assert(OTT_X_SEED_KEEP <= 16, "the estimate pass finishes at most sixteen rows per wave");
inline uint64_t prune_plan_seed_est(const PruneIn& in, const PrunePlan& pp, bool head, bool filtered) {
    // (the seed before prune_plan rounds it up to whole tiles: a tenth of 1 310 656 rows is not yet 131 072)
    if (!OTT_X_SEED_EST || !head || in.E != 1 || filtered || pp.c == 0 || in.rows_scored / 10 < SEED_EST_MIN_ROWS) return 0;
    uint64_t rows = pp.seed;
    if (OTT_X_SEED_EST_DIV > 0) {
        rows = (in.rows_scored / (uint64_t)(OTT_X_SEED_EST_DIV > 0 ? OTT_X_SEED_EST_DIV : 1) + 63) & ~63ull;
        if (rows < SEED_EST_MIN_ROWS) rows = SEED_EST_MIN_ROWS;
    }
    return rows;
}
// rows a wave of the estimate pass finishes exactly
inline uint32_t prune_seed_keep(uint64_t k) {
    if (OTT_X_SEED_KEEP > 0) return OTT_X_SEED_KEEP < 64 ? (uint32_t)OTT_X_SEED_KEEP : 64u;
    return k < SEED_EST_KEEP_MAX ? (uint32_t)k : SEED_EST_KEEP_MAX;
}
// The counters ride in the result block ("the counters ride").  On host output the sweep's two counter totals
// are wanted beside the hits.  Behind an estimate pass — head form, k <= 64, no score filter, a store from 1 310 720 rows — and with
// the rank merge (the merge options at their defaults) the final merge launch writes the totals behind the hits it writes into the
// pinned block: no copy is queued behind the merge, and no timing marker stands between the gated launch and its merge
// (ott_stats.score_ns then spans the chain, the merges included, and merge_ns is 0).  Otherwise the call is the one with the copy
// and the marker, to the launch.  Experiment builds: -DOTT_X_RIDE=0 never plans it.
#ifndef OTT_X_RIDE
#define OTT_X_RIDE 1
#endif
struct MergeOptions {
    int merge_rank1;  // store option merge_rank1 (-1 / 1: the rank merge, 0: round 2's merge)
    bool merge_walk;  // store option merge_walk
};
inline bool prune_plan_ride(uint64_t est_rows, int E, bool fetch, const MergeOptions& mo) {
    return OTT_X_RIDE != 0 && est_rows != 0 && E == 1 && fetch && mo.merge_rank1 != 0 && !mo.merge_walk;
}
inline PrunePlan prune_plan_quant_refused(PruneIn in) {
    in.exact_sketch = 0;
    return prune_plan(in);
}

// ---- the result block --------------------------------------------------------------------------------------------------------------
// [counts (groups x u64, padded to 64 B) | hits (groups x KS)], and on the host 8 bytes more behind it: the pruned sweep's tail counter
struct ExactResult {
    size_t cnt_pad;     // = the hits' offset
    size_t bytes;       // counts and hits
    size_t host_bytes;  // bytes + the tail counter, which sits at `bytes`
};
inline ExactResult exact_result_layout(uint32_t groups, uint32_t KS) {
    const size_t cnt_pad = (((size_t)groups * sizeof(uint64_t)) + 63) & ~(size_t)63;
    const size_t bytes = cnt_pad + (size_t)groups * KS * sizeof(ott_hit);
    return ExactResult{cnt_pad, bytes, bytes + 8};
}

// ---- stats -------------------------------------------------------------------------------------------------------------------------
// every pass reads each scored row once, and its inverse norm where the metric wants one
inline uint64_t exact_bytes_scanned(uint32_t passes, uint64_t rows_scored, uint32_t dim, uint32_t metric) {
    return (uint64_t)passes * rows_scored * ((uint64_t)dim * 4 + (metric == OTT_METRIC_COSINE ? 4 : 0));
}

}  // namespace ott
