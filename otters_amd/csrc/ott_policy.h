// ott_policy.h — which path a query takes and how a store's batch cascade backs off, free of HIP and of ott_store: plain
// C++17 over the public header's enums, so that the CPU suite compiles the very code libotters_hip.so ships on its own
// (tests/test_query_policy_cpu.py), as it does ott_host.h and ott_prune.h.  query_core (ott_api.hip) is the one user.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "../../include/otters_hip.h"
#include "ott_exact_plan.h"  // small_variant_fits: whether rows8 would take the query on the exact path
#include "ott_mfma_plan.h"  // how many candidates each level of the batch path re-scores (mfma_hi_k_ok, t_want_*): the cost model and the back-off read it

namespace ott {

// the options ask for the int8 level in front of the hi pass
inline bool i8_wanted(int hi_fmt, bool mfma_f32, bool no_hi_pass, bool no_batch_image) {
    return (hi_fmt == -1 || hi_fmt == 2) && !mfma_f32 && !no_hi_pass && !no_batch_image;
}
// ONE query at the int8 level may run as a streaming sweep with the top-128 in its epilogue (run_i8_single) instead of the
// cascade's rounds: the sweep kernel scores cosine / dot, has no equality filter, and keeps a list of 128 entries (SWEEP_T, k <= SWEEP_K_MAX = 24: the
// wave lists of 256 / 512 entries cost the sweep more than the rounds cost the cascade: top-100 at 10M x 768 1.97 ms against
// 1.46).  `last`: the caller's own condition — the cost model's "the level is not widened", the cascade's "t_min <= 128".
inline bool i8_single_sweep(uint32_t nq, uint64_t k_q, uint32_t filter_cmp, uint32_t metric, uint32_t dim, bool last) {
    return nq == 1 && k_q <= SWEEP_K_MAX && filter_cmp != OTT_CMP_EQ && metric != OTT_METRIC_EUCLIDEAN && dim <= 3584 && last;
}

// ---- path choice ---------------------------------------------------------------------------------------------------------------
struct PathIn {
    uint64_t rows_scored, n_runs;  // of the run plan
    uint32_t dim, dimq, nq;
    uint64_t k;
    uint32_t metric, filter_cmp, path;  // ott_metric, ott_cmp, ott_path (the requested one)
    bool flat;                          // CoreOpts::flat
    // the options the choice reads
    bool mfma_f32, no_hi_pass, no_batch_image;
    int hi_fmt, exact_small;
};
// what the planes look like right now (PlaneSnapshot, read under the planes' mutex) and whether the int8 level is widened (i8_t512 > 0)
struct PathPlanes {
    bool have_hi, hi_f16, i8_off, i8_widened;
};
enum PathChoice { PATH_CHOICE_EXACT = 0, PATH_CHOICE_MFMA = 1, PATH_CHOICE_REFUSED = 2 };
constexpr const char* kMfmaRefusal = "ott_query: the MFMA path needs dim >= 8 and k <= 484";

// `planes()` -> PathPlanes is called on the AUTO branch only, `first_plane_ready()` -> bool only for ONE query that the hi pass
// could serve: both take the mutex of the store's planes, and a Manhattan, flat or explicit-path query touches no plane state
template <class Planes, class Ready>
inline PathChoice choose_path(const PathIn& in, Planes&& planes, Ready&& first_plane_ready) {
    const uint32_t nq = in.nq;
    // per-query k for the batch path: the merged top-k is contained in the union of per-query top-k
    const uint64_t k_q = in.k < in.rows_scored ? in.k : in.rows_scored;
    const bool mfma_ok = t_want_split(k_q) <= MFMA_T_MAX && in.dim >= 8;
    if (in.flat) return PATH_CHOICE_EXACT;  // (the flat pass exists on the exact-order kernel only)
    if (in.metric == OTT_METRIC_MANHATTAN) return PATH_CHOICE_EXACT;  // EXACT only, decided before the cost model looks at the planes (their mutex)
    if (in.path == OTT_PATH_MFMA) return mfma_ok ? PATH_CHOICE_MFMA : PATH_CHOICE_REFUSED;
    if (in.path == OTT_PATH_EXACT) return PATH_CHOICE_EXACT;
    // AUTO: cost model fitted to MI355X measurements (benchmarks/small_corpus.py, nq_sweep.py), in milliseconds.
    // exact: up to 4 queries share one pass; a pass of m queries costs 0.05 / 0.06 / 0.085 / 0.115 ms of launches + latency and
    //        streams at ~6.5 TB/s, 2.7 % slower per extra query (round 4, benchmarks/auto_choice.py on 300k .. 10M x 768:
    //        one query 0.187 / 0.517 / 1.40 / 4.54 ms, four 0.257 / 0.590 / 1.59 / 4.90; the 0.11 ms per pass this model
    //        carried since round 1 sent single queries on 262k-480k-row stores through the cascade, 20 % slower).
    // mfma:  ~0.16 ms of rounds / select / finalize / transfer, ~4.5 us per query of re-scoring and host merge, then the
    //        slower of the corpus stream (~6 TB/s per 256-query block) and the matrix pipe.
    const double bytes = (double)in.rows_scored * (4.0 * in.dim + 4.0);
    const uint32_t full_passes = nq / 4, last_m = nq % 4;
    static const double pass_fixed[5] = {0.0, 0.05, 0.06, 0.085, 0.115};
    auto t_pass = [&](uint32_t m) { return pass_fixed[m] + bytes / 6.5e9 * (1.0 + 0.027 * (m - 1)); };
    const double t_exact = full_passes * t_pass(4) + (last_m ? t_pass(last_m) : 0.0);
    const uint32_t bn = nq <= 16 ? 16u : nq <= 32 ? 32u : nq <= 64 ? 64u : nq <= 128 ? 128u : 256u;
    const double nq_pad = (double)((nq + bn - 1) / bn * bn);
    const bool f32pipe = in.mfma_f32;
    // (the plane's actual format once it exists — it may have fallen back to bf16 — else what the option asks for)
    const PathPlanes ps = planes();  // (under the planes' mutex: another context may be building or dropping a plane right now)
    const bool plane_half = ps.have_hi ? ps.hi_f16 : in.hi_fmt != 0;
    const bool hi_ok = !f32pipe && mfma_hi_k_ok(k_q, plane_half) && !in.no_hi_pass;
    // round 5: the int8 plane in front (cosine / dot, k <= 128): a quarter of the bytes, twice the matrix rate, 512 candidates
    const bool i8_ok = hi_ok && i8_wanted(in.hi_fmt, in.mfma_f32, in.no_hi_pass, in.no_batch_image) && !ps.i8_off && k_q <= I8_K_MAX;
    // the hi pass streams the 16-bit hi plane: half the bytes
    const double t_stream = (i8_ok ? 0.25 : hi_ok ? 0.5 : 1.0) * bytes * (double)((nq + 255) / 256) / (i8_ok ? 6.0e9 : hi_ok ? (nq <= 32 ? 6.5e9 : 6.2e9) : 5.9e9);  // (non-temporal row pieces, round 2: 6.6-6.8 TB/s up to 32 queries, ~6 at 64-128)
    // matrix pipe: ~125 TFLOP/s on the f32 pipe, ~330 TFLOP/s (f32-equivalent) with the split-bf16 operands, ~800 for the hi pass, ~1500 int8
    const double t_pipe = 2.0 * in.dim * (double)in.rows_scored * nq_pad / (i8_ok ? 1500e9 : hi_ok ? 800e9 : (bn >= 32 && !f32pipe) ? 330e9 : 125e9);
    // (the candidates re-scored per query grow with k — ott_mfma_plan.h: t_want_hi on the hi pass, in steps of 64; MFMA_T_MAX on the int8 pass — and finalize /
    //  select with them: top-100 costs the cascade 0.03-0.05 ms more than top-10 at one query, benchmarks/auto_choice.py)
    const uint64_t t_hi64 = (t_want_hi(k_q) + 63) / 64 * 64;  // (above 128 from k = 37 on)
    const double t_cand = i8_ok ? 0.0003 * (double)(MFMA_T_MAX - 128) : hi_ok && t_hi64 > 128 ? 0.0003 * (double)(t_hi64 - 128) : 0.0;
    double t_mfma = 0.16 + 0.0045 * nq + t_cand + (t_stream > t_pipe ? t_stream : t_pipe);
    // ONE query at the int8 level, k <= 24: a streaming sweep with the top-128 in its epilogue (run_i8_single): ~0.11 ms of
    // launches, merge and re-score around a quarter of the bytes at 6.5 TB/s (profiles/round5/auto_choice.md: 150k x 768 rows
    // 0.13 ms, 1M 0.24, 10M 1.29; the exact kernel 0.12 / 0.54 / 4.7)
    if (i8_ok && i8_single_sweep(nq, k_q, in.filter_cmp, in.metric, in.dim, !ps.i8_widened)) t_mfma = 0.11 + 0.25 * bytes / 6.5e9;
    // a SINGLE query takes the exact-order kernel (no second copy of the corpus is built for the most common call) — unless
    // the bf16 hi plane is ALREADY resident (a batch query or ott_store_prepare_batch built it) and covers every row: then
    // the cascade streams half the bytes (10M x 768: 2.5 ms against 4.5) and returns the same bits;
    // 2-4 queries share one exact pass unless the hi pass (half the bytes) is cheaper; without it the batch path needs > 4
    const bool batch_worthy = nq > (hi_ok ? 1u : 4u) || (nq == 1 && hi_ok && first_plane_ready());
    bool use_mfma = mfma_ok && batch_worthy && in.rows_scored >= 2048 && t_mfma < t_exact;
    // small stores, small batches (round 3): rows8 scores up to 8 queries per pass in ~(40 us + 0.7 us per thousand rows) behind
    // ~35 us of launches and merge, against the batch path's ~(120 us + 3.5 us per query) of rounds, select and finalize
    // (benchmarks/small_corpus.py: 10k x 768, 8 queries: 84 us against 150)
    const uint64_t k_e = in.k < in.rows_scored * nq ? in.k : in.rows_scored * nq;
    if (use_mfma && nq <= 16 && k_e <= 128 && in.exact_small != 0 && in.exact_small != 1 &&
        small_variant_fits(in.dimq, in.rows_scored / 64 + in.n_runs)) {  // (the tiles: an estimate from above, no prefix is built yet)
        const double t_rows8 = 0.035 + (double)((nq + 7) / 8) * (0.040 + 0.7e-6 * (double)in.rows_scored);
        if (t_rows8 < 0.9 * (0.12 + 0.0035 * nq)) use_mfma = false;
    }
    return use_mfma ? PATH_CHOICE_MFMA : PATH_CHOICE_EXACT;
}

// ---- the batch cascade's back-off state of one store ---------------------------------------------------------------------------
// Shared by every query context of a store (read through the owner) while the store is only held shared: each field is an atomic,
// each rule below a short sequence of single loads and stores — two contexts may interleave between them (the averages are
// load-then-store on purpose: a lost update shifts a heuristic by one batch, never a result).
struct CascadeState {
    // hi-pass back-off: a batch in which ANY query falls through pays for both passes (the split pass streams the whole corpus
    // again for the few), so the hi pass only pays while fewer than ~half the batches need the second one.  When more than 1/8
    // of a batch falls through, or more than half of the recent batches needed the split pass, the next `hi_skip` batches go
    // straight to it; the skip doubles (4 .. 64) while re-probes keep failing
    std::atomic<int> hi_skip{0}, hi_backoff{0};
    std::atomic<int> i8_skip{0}, i8_backoff{0};  // the same back-off for the int8 level in front of it
    std::atomic<int> i8_t512{0};                 // calls left for which the int8 level re-scores 512 candidates per query (it failed queries at fewer)
    std::atomic<int> i8_fail_ema{0};             // share (x1024, exponential average) of recent int8-level batches that needed a second pass at all
    std::atomic<int> spec_skip{0};    // batches left that run with conservative gates (a speculative gate failed a query recently)
    std::atomic<int> spec_backoff{0};
    std::atomic<int> wide_first{0};   // batches left that start at the 4096-candidate level (the 512-candidate one kept failing)
    std::atomic<int> hi_t512{0};      // the hi pass re-scores 512 candidates per query on this store (it failed queries at 2k + 56: dense neighbourhoods)
    std::atomic<int> hi_fail_ema{0};  // share (x1024, exponential average) of recent hi-pass batches that needed the split pass at all

    // one batch off a countdown: true while it was still running.  The skip counters (hi_skip, i8_skip, spec_skip) and i8_t512
    // (true = this call re-scores 512 per query: 64 calls after a failure at less, counted down by the calls that follow — one
    // query in a dense neighbourhood does not widen the store's every later call for good)
    static bool consume(std::atomic<int>& left) {
        if (left.load() <= 0) return false;
        left.fetch_sub(1);
        return true;
    }
    bool i8_widened() const { return i8_t512.load() > 0; }
    bool hi_wide() const { return hi_t512.load() != 0; }

    // The int8 level ran on a batch of nq queries and left `open` of them open, `gate_failed` of those through a speculative gate
    // alone.  A batch in which ANY query stays open pays a second pass — the hi pass over the half plane, ~2.4 ms at 10M x 768
    // however few the queries — so the int8 level only pays while most batches certify whole: measured on near-duplicate
    // clusters (7-17 of 256 queries open in EVERY batch) int8 first took 5.65 ms per batch where the hi pass alone takes
    // 4.8.  Batches of more than 512 queries are the exception: their int8 pass saves more than the second pass costs
    // (1024 queries: 9.4 + 2.4 ms against 15.4).  Back-off as for the hi pass: more than 1/8 of a batch open, or more than
    // ~half (small batches: ~40 %) of the recent batches needing the second pass at all.
    void after_i8(uint32_t nq, size_t open, uint32_t gate_failed, bool wide_now, uint64_t k_q) {
        const size_t genuine = open > gate_failed ? open - gate_failed : 0;
        const int ema = (3 * i8_fail_ema.load() + (genuine == 0 ? 0 : 1024)) / 4;
        i8_fail_ema.store(ema);
        if (genuine * 8 > nq && !wide_now && t_want_i8(k_q) < MFMA_T_MAX) {
            i8_t512.store(64);  // first answer to dense neighbourhoods: re-score 512 per query for the next 64 calls
            i8_fail_ema.store(0);
        } else if (genuine * 8 > nq || (nq <= 512 && ema > (nq <= 128 ? 400 : 512))) back_off(i8_backoff, i8_skip, 4, 64);
        else if (genuine == 0) i8_backoff.store(0);
    }
    // The hi pass ran with hi_t candidates per query (0 = its own 2k + 56).  Queries that failed only through their speculative
    // gate say nothing about the hi pass's error bound
    void after_hi(uint32_t nq, size_t open, uint32_t gate_failed, bool wide_now, uint32_t hi_t) {
        const size_t genuine = open > gate_failed ? open - gate_failed : 0;
        if (genuine * 8 > nq && !wide_now && hi_t < MFMA_T_MAX) {
            // first answer to a store whose queries sit in dense neighbourhoods: keep the hi pass, re-score 512 per query
            // from the next batch on (this batch's open queries go to the split pass); only if THAT keeps failing does
            // the store back off from the hi pass
            hi_t512.store(1);
            hi_fail_ema.store(0);
        } else {
            const int ema = (3 * hi_fail_ema.load() + (genuine == 0 ? 0 : 1024)) / 4;
            hi_fail_ema.store(ema);
            if (genuine * 8 > nq || ema > 512) back_off(hi_backoff, hi_skip, 4, 64);
            else if (genuine == 0) hi_backoff.store(0);
        }
    }
    // gate back-off: conservative for 8, 16, .. 256 batches after a failure, forgotten after a clean batch
    void after_spec(bool gate_failed) {
        if (gate_failed) back_off(spec_backoff, spec_skip, 8, 256);
        else spec_backoff.store(0);
    }
    // the 512-candidate level left `open` of nq queries for the 4096-candidate one: most of the batch -> skip the 512 level the
    // next 16 times; batches of up to 8 queries never start wide
    void arm_wide_first(size_t open, uint32_t nq) {
        if (open * 2 > nq) wide_first.store(16);
    }
    bool take_wide_first(uint32_t nq) { return nq > 8 && consume(wide_first); }

private:
    static void back_off(std::atomic<int>& backoff, std::atomic<int>& skip, int lo, int hi) {
        int b = backoff.load() * 2;
        b = b < lo ? lo : b > hi ? hi : b;
        backoff.store(b);
        skip.store(b);
    }
};

}  // namespace ott
