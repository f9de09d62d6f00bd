// ott_maxsim.hip — late-interaction (MaxSim) search over grouped rows: the nq query vectors are the TOKENS of one
// query, a group's score is the sum over the tokens of the best score among the group's surviving rows, the top-k is over groups.
//
//   maxsim_sweep_kernel   sweep_tiles (ott_sweep_dev.h: the streaming tile loop this sweep shares with group_sweep_kernel, tokens in
//                         the place of queries: the bits are the oracle's) and this epilogue per (row, token of the pass):
//                         composed row mask, NaN drop, o = ord_of(score, take) — 32 bits, never 0 for a non-NaN —
//                         and table[token][gid[row]] = max(itself, o): a relaxed agent-scope load, then atomicMax on the 32-bit slot
//                         only when o is larger.  0 = empty slot.  No score filter here: the filter is on the SUM.
//                         FOLD (diagnostic build only until it is measured, option maxsim_fold): rows of a document are normally
//                         appended together, so most lanes of a wave share their neighbour's group and the first tiles of a
//                         group would issue up to 64 same-address atomics per token.  Before the
//                         atomic every token's ordinal is folded over runs of adjacent lanes with equal gid (a segmented max in six
//                         ds_bpermute steps, the gid shuffles shared by the tokens) and only the head lane of a run touches memory.
//                         Max is order-free and only lanes of one group are ever joined, so the table cannot differ.  A wave
//                         without two equal neighbours (a shuffled layout) skips the fold after one shuffle and a ballot.
//   maxsim_reduce_kernel  one lane per group: the group's nq slots in token order, sum = best[0]; sum = sum + best[t] (f32, round to
//                         nearest, this order); dropped on an empty slot (a token without a score: the group has no surviving row,
//                         or every one of them scored NaN for it), a NaN sum (+inf + -inf) or a failed filter; else
//                         key = ord_of(sum) << 32 | ~gid into the [n_groups] table of 8-byte keys (0 = dropped).  Zeroes the slots it
//                         read: the next query's sweep needs no memset.
//
// The key table has exactly the shape grouped search takes its top-k from, so the rest is ott_group.hip's GroupTopK (a hit's index
// is the group), as the host prologue of the sweep is its sweep_prologue.  Tokens per pass: ott_sweep_dev.h; the epilogue adds an
// ordinal per token and the fold's two shuffle temporaries (profiles/maxsim/resource_usage.txt: no scratch).
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_sweep_dev.h"

namespace ott {

constexpr bool MS_FOLD = false;                // the product's epilogue: the plain one until the A/B of profiles/maxsim/README.md is measured
constexpr uint64_t MS_TABLE_MAX = 1ull << 31;  // bytes of the (token, group) table: all tokens are held at once

struct MaxsimParams : SweepParams {
    uint32_t* table;  // [nq_total][n_groups] best ordinal per (token, group); 0 = empty
    uint32_t n_groups;
};

template <int MK, int NQ, bool FOLD>
__global__ __launch_bounds__(64 * SW_WAVES) void maxsim_sweep_kernel(MaxsimParams p) {
    const int lane = threadIdx.x & 63;
    const bool take_max = p.take_max != 0;
    sweep_tiles<MK, NQ>(p, [&](uint64_t, bool valid, uint32_t g, const float (&sc)[NQ], uint32_t nq_here) {
        // score -> ordinal (0 = nothing to offer: no row, a token past the query's last, a NaN score)
        uint32_t o[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float s = sc[q];
            o[q] = (valid && (uint32_t)q < nq_here && !(s != s)) ? ord_of(s, take_max) : 0u;  // NaN dropped: vec_compute.rs:237
        }
        bool head = true;
        if constexpr (FOLD) {
            // runs of adjacent lanes with one gid (a lane without a row has no group's id and joins no run): after the step of
            // distance d a lane holds the max over the lanes of its run among [lane, lane + 2d) (a lane d further on with the same
            // gid outside the run may join too: it is the same slot's)
            const uint32_t gprev = __shfl_up(g, 1);
            head = lane == 0 || gprev != g;
            if (__ballot(!head) != 0) {
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t og = __shfl_down(g, d);
                    const bool join = lane + d < 64 && og == g;
#pragma unroll
                    for (int q = 0; q < NQ; q++) {
                        const uint32_t oo = __shfl_down(o[q], d);
                        if (join && oo > o[q]) o[q] = oo;
                    }
                }
            }
        }
        if (head && valid) {
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                if (o[q] != 0) {
                    uint32_t* slot = p.table + (size_t)(p.q0 + q) * p.n_groups + g;
                    // the load goes past this CU's vector L1 (agent scope), so it sees what other CUs' atomics left; a value that
                    // is stale all the same is a smaller one (slots only rise) and costs an atomic, never a result
                    if (o[q] > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, o[q]);
                }
            }
        }
    });
}

// One lane per group.  keys: [n_groups] 8-byte keys, zero when the kernel starts (d_gtable's protocol): only kept groups are written.
// gid_of: the table's slots are a LIST of groups (ott_maxsim_gather.hip), slot g is group gid_of[g]; nullptr = slot g is group g.
__global__ __launch_bounds__(256) void maxsim_reduce_kernel(uint32_t* table, uint32_t n_groups, uint32_t nq, uint32_t take_max, uint32_t cmp, float thr,
                                                            unsigned long long* keys, const uint32_t* __restrict__ gid_of) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const bool tmax = take_max != 0;
    bool complete = true;
    float acc = 0.0f;
    for (uint32_t t = 0; t < nq; t++) {
        uint32_t* slot = table + (size_t)t * n_groups + g;
        const uint32_t o = *slot;
        if (o == 0) {
            complete = false;
        } else {
            *slot = 0u;
            const float b = score_of(o, tmax);
            acc = t == 0 ? b : __fadd_rn(acc, b);  // starts from best[0], not from 0.0: a -0.0 stays -0.0
        }
    }
    const uint32_t id = gid_of ? gid_of[g] : (uint32_t)g;
    if (complete && !(acc != acc) && cmp_holds(acc, cmp, thr)) keys[g] = ((unsigned long long)ord_of(acc, tmax) << 32) | (uint32_t)(~id);
}

int launch_maxsim_reduce(ott_store* s, uint32_t* table, uint32_t n_slots, uint32_t nq, uint32_t take_max, uint32_t cmp, float thr, unsigned long long* keys,
                         const uint32_t* gid_of) {
    hipLaunchKernelGGL(maxsim_reduce_kernel, dim3((uint32_t)(((uint64_t)n_slots + 255) / 256)), dim3(256), 0, s->stream, table, n_slots, nq, take_max, cmp, thr, keys, gid_of);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

namespace {

int launch_maxsim_sweep(ott_store* s, const MaxsimParams& p, uint32_t nq_tile, uint32_t grid) {
#ifdef OTT_MFMA_DEBUG_BUILD
    // the diagnostic build carries both epilogues (option maxsim_fold: the A/B of benchmarks/maxsim.py)
    if (s->opt.maxsim_fold >= 0 && (s->opt.maxsim_fold != 0) != MS_FOLD) return launch_sweep(s->stream, p, nq_tile, grid, OTT_SWEEP_KERNEL(maxsim_sweep_kernel, !MS_FOLD));
#endif
    return launch_sweep(s->stream, p, nq_tile, grid, OTT_SWEEP_KERNEL(maxsim_sweep_kernel, MS_FOLD));
}

}  // namespace

// The query on a context whose `mu` the caller holds (and the owner's `rw`, shared).  k_eff = min(k, n_groups) >= 1.
// (ott_maxsim_gather.hip runs it too: a listed query on the mask route IS this query with one more mask.)
int run_maxsim(ott_store* s, const ott_query_desc* d, uint64_t k_eff, ott_hit* out, uint64_t* n_out, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    const uint32_t nq = d->nq, ng = s->n_groups;
    MaxsimParams p{};
    uint32_t grid = 0;
    if ((rc = sweep_prologue(s, d, &st, &p, &grid))) return rc;
    if (grid != 0) {
        // the ordinals are left zeroed by the reduce kernel, the keys by the select / compact kernel
        if ((rc = ensure_zeroed(s, s->d_mstable, s->mstable_clean, (size_t)nq * ng * 4))) return rc;
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)ng * 8))) return rc;
        unsigned long long* keys = (unsigned long long*)s->d_gtable.p;
        p.table = (uint32_t*)s->d_mstable.p;
        p.n_groups = ng;

        GroupTopK tk;
        tk.n_groups = ng;
        tk.nq = 1;
        tk.k = k_eff;
        tk.take_max = p.take_max != 0;
        tk.index_is_group = true;
        tk.also_clean = &s->mstable_clean;
        if ((rc = tk.prepare(s, nullptr))) return rc;
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        const uint32_t tile = nq == 1 ? 1u : SW_NQ;
        for (uint32_t ps = 0; ps < st.passes; ps++) {
            p.q0 = ps * tile;
            if ((rc = launch_maxsim_sweep(s, p, tile, grid))) return rc;
        }
        if ((rc = launch_maxsim_reduce(s, p.table, ng, nq, p.take_max, (uint32_t)d->filter_cmp, d->filter_thr, keys, nullptr))) return rc;
        if ((rc = tk.pass(s, keys, 0, 1))) return rc;
        if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
        if ((rc = tk.finish(s, timing, out, n_out, nullptr))) return rc;
        if (timing) read_exact_events(s, &st);
    }
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_maxsim(ott_store* s, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, ott_stats* stats) {
    // what the descriptor alone decides comes first: these refusals need no store
    if (d && d->mode == OTT_MODE_PER_QUERY)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim: the query vectors are the tokens of ONE query; PER_QUERY (a batch of token sets) is not served");
    if (d && d->path == OTT_PATH_MFMA) return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim: the MFMA path does not serve late-interaction queries; use path AUTO or EXACT");
    if (!s) return fail(OTT_ERR_INVALID, "ott_query_maxsim: store is NULL");
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (s->multi)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim: a multi-GPU store is not served (a group may span shards: the maxima would have to be joined before the sum)");
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if ((rc = check_group_ids(s, "ott_query_maxsim", false))) return rc;
    const auto table_fits = [&](uint32_t n_groups) { return (uint64_t)d->nq * n_groups * 4 <= MS_TABLE_MAX; };
    const char* too_big = "ott_query_maxsim: tokens x groups x 4 bytes is above 2 GiB (the table holds every token's maxima at once); use fewer tokens or groups";
    if (!table_fits(s->n_groups)) return fail(OTT_ERR_UNSUPPORTED, too_big);
    ott::host::SharedLock rd;  // the corpus and the group ids cannot change while this query runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    // what the checks above read without the lock is read again, and k_eff only here: a set_groups may have come in between
    if ((rc = check_group_ids(s, "ott_query_maxsim", true))) return rc;
    if (!table_fits(s->n_groups)) return fail(OTT_ERR_UNSUPPORTED, too_big);
    const uint64_t k_eff = d->k < s->n_groups ? d->k : s->n_groups;
    if (cap < k_eff) return fail(OTT_ERR_INVALID, "ott_query_maxsim: output capacity is smaller than min(k, n_groups)");
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_maxsim: out is NULL");
    if (k_eff == 0) return OTT_OK;
    CtxLease ctx(s);
    return run_maxsim(ctx.c, d, k_eff, out, n_out, stats);
}

}  // extern "C"
