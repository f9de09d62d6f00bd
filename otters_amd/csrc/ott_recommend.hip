// ott_recommend.hip — recommend by example rows (Qdrant's recommend with the best_score strategy):
// ott_query_recommend ranks the store's rows by their best score against the POSITIVE example rows, and keeps the rows that are
// closer to a NEGATIVE example than to every positive one for the end of the list, or out of it.  The examples are rows of the
// store, named by id: nothing of them crosses the host.
//
//   example_gather_kernel    the examples' stored rows into the context's query block (upload_exact_inputs' layout: zero padded to
//                            dimq, the slots past the last example zero) and their STORED inverse norms into the qinv slots: the
//                            pair score P[e][r] is ott_query_mmr's, the example's row plays the query.
//   recommend_sweep_kernel   sweep_tiles (ott_sweep_dev.h: the streaming tile loop of the grouped sweeps, examples in the place of
//                            queries: the bits are the oracle's) and this epilogue per row: the pass's up to four ordinals
//                            o = ord_of(score, take) — 0 for a NaN score, a padding slot or a masked row — are reduced in registers
//                            into a positive and a negative maximum (slot q0 + q is positive iff it lies below first_neg) and folded
//                            into the row's 8-byte state {bp, bn}: a plain load, max and a streaming vector store.  A row belongs to one lane of a pass
//                            and the passes are launches on one stream, so nothing is atomic; the first pass finds the table zero
//                            and does not load.  A row no lane ever wrote (masked, deleted, pruned chunk) keeps {0, 0}.
//   example_clear_kernel     the examples' own slots back to {0, 0}: an example is never a candidate.
//   recommend_keys_kernel    one lane per row, side 1 or 0: candidate (bp != 0, the filter holds for BP) on that side ->
//                            key = ordinal << 32 | ~row in the context's key table, else nothing (the table is zero when found).
//                            Side 1 (bn == 0 or bp > bn): ordinal bp.  Side 0 (bp <= bn): ord_of(BN, !take) = ~bn, so that the
//                            top-k with the FLIPPED take ranks ascending bn and decodes BN.  The kernel that reads the state last
//                            zeroes it (`last`).
//
// The key table has the shape grouped search takes its top-k from with one "group" per row: the rest is ott_group.hip's GroupTopK
// (index_is_group = false: a hit's index is base_offset + row).  Side 0 is a second keys kernel and a second GroupTopK, run only
// when OTT_RECOMMEND_FILL is set, negatives exist and side 1 returned fewer than k_eff: one more host wait in that case alone.
// When that round can run but does not, the state table is cleared by a memset behind the first round.
// Examples per pass: ott_sweep_dev.h; the epilogue adds two ordinals (profiles/recommend/resource_usage.txt: no scratch).
// ott_query_recommend_strategy adds Qdrant's other two strategies below: sum_scores, the same sweep with a running
// f32 sum in the state, and average_vector, one ordinary query with a vector built from the examples' rows; strategy 0 is the call above.
// The gather and clear kernels and the host frame around a sweep over example rows (ExampleFrame, ott_internal.h) are here once:
// best_score, sum_scores and discovery search (ott_discover.hip, whose slots are the pairs' rows and a target row) run through them.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_sweep_dev.h"

namespace ott {

static_assert(REC_NQ == SW_NQ, "ott_recommend_plan.h counts the passes of ott_sweep_dev.h's sweep");

struct RecommendParams : SweepParams {
    uint2* state;        // [n] {bp, bn}; 0 = none
    uint32_t first_neg;  // slots below it are positives
};

constexpr uint32_t EX_MAX_ROWS = DISC_MAX_SLOTS;  // the rows a call gathers ride in the kernel arguments
constexpr uint32_t EX_CLEAR_LANES = 128;          // example_clear_kernel's one workgroup: a lane per gathered row
static_assert(EX_MAX_ROWS >= REC_MAX_EXAMPLES && EX_MAX_ROWS >= DISC_MAX_SLOTS && EX_MAX_ROWS <= EX_CLEAR_LANES,
              "the gather array holds recommend's examples and discovery's slots, the clear kernel has a lane for each");

struct ExampleGatherParams {
    const float* rows;
    const float* inv;
    float* queries;  // [slots * dimq]
    float* qinv;     // [slots]
    uint2* state;    // example_clear_kernel
    uint32_t ld, dim, dimq, n;
    uint32_t ex[EX_MAX_ROWS];  // the gathered rows (slot e is row ex[e]), every one below the store's length (checked on the host)
};

// blockIdx.x = slot.  Every float of the slot's dimq is written: the row's dim, then zeros.
__global__ __launch_bounds__(256) void example_gather_kernel(ExampleGatherParams p) {
    const uint32_t e = blockIdx.x;
    if (e >= p.n) return;
    const float* src = p.rows + (uint64_t)p.ex[e] * p.ld;
    float* dst = p.queries + (size_t)e * p.dimq;
    for (uint32_t i = threadIdx.x; i < p.dimq; i += blockDim.x) dst[i] = i < p.dim ? src[i] : 0.0f;
    if (threadIdx.x == 0) p.qinv[e] = p.inv[p.ex[e]];
}

__global__ __launch_bounds__(EX_CLEAR_LANES) void example_clear_kernel(ExampleGatherParams p) {
    if (threadIdx.x < p.n) p.state[p.ex[threadIdx.x]] = make_uint2(0u, 0u);
}

template <int MK, int NQ>
__global__ __launch_bounds__(64 * SW_WAVES) void recommend_sweep_kernel(RecommendParams p) {
    const bool take_max = p.take_max != 0;
    sweep_tiles<MK, NQ>(p, [&](uint64_t my_row, bool valid, uint32_t, const float (&sc)[NQ], uint32_t nq_here) {
        uint32_t bp = 0, bn = 0;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float s = sc[q];
            const uint32_t o = (valid && (uint32_t)q < nq_here && !(s != s)) ? ord_of(s, take_max) : 0u;  // NaN dropped: vec_compute.rs:237
            if (p.q0 + (uint32_t)q < p.first_neg) bp = o > bp ? o : bp;
            else bn = o > bn ? o : bn;
        }
        if (valid && (bp | bn) != 0) {
            uint2* slot = p.state + my_row;
            if (p.q0 != 0) {  // (wave-uniform: the first pass finds the table zero)
                const uint2 cur = *slot;
                bp = cur.x > bp ? cur.x : bp;
                bn = cur.y > bn ? cur.y : bn;
            }
            // streamed like the rows: nothing reads the slot again before the next launch (a plain store was measurably slower:
            // profiles/recommend/README.md)
            typedef unsigned int v2u __attribute__((ext_vector_type(2)));
            v2u v;
            v.x = bp;
            v.y = bn;
            __builtin_nontemporal_store(v, reinterpret_cast<v2u*>(slot));
        }
    });
}

// One lane per row.  keys: [n] 8-byte keys, zero when the kernel starts (d_gtable's protocol): only candidates of `side` are written.
__global__ __launch_bounds__(256) void recommend_keys_kernel(uint2* state, uint32_t n, uint32_t side, uint32_t take_max, uint32_t cmp, float thr, uint32_t last,
                                                             unsigned long long* keys) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint2 st = state[r];
    if ((st.x | st.y) == 0) return;
    if (last) state[r] = make_uint2(0u, 0u);
    const uint32_t bp = st.x, bn = st.y;
    if (bp == 0 || !cmp_holds(score_of(bp, take_max != 0), cmp, thr)) return;  // the filter acts on BP, on both sides
    const bool positive = bn == 0 || bp > bn;
    if (positive != (side != 0)) return;
    const uint32_t o = positive ? bp : ~bn;  // ~bn == ord_of(BN, !take): never 0, bn is the ordinal of a non-NaN
    keys[r] = ((unsigned long long)o << 32) | (uint32_t)(~(uint32_t)r);
}

// ---- the sum_scores and average_vector strategies (ott_query_recommend_strategy) ---------------------------------------
//   recommend_sum_sweep_kernel  sweep_tiles and this epilogue per row: the running sum S of the row's pair scores, slot by slot — the
//                               first slot's score itself, then one __fadd_rn per positive slot and one __fsub_rn per negative one —
//                               kept as {bits of S, REC_SUM_MARK} in the row's 8-byte state.  The first pass does not load it; a later
//                               pass loads S, continues the chain over its up to four slots and streams the state back.
//   recommend_sum_keys_kernel   one lane per row: marked, S not NaN, the filter holds for S -> key = ord_of(S) << 32 | ~row.  It reads
//                               the state last and leaves it zeroed.
//   recommend_average_kernel    one thread per dim: the examples' stored values summed in slot order, one division per side, and
//                               (mp + mp) - mn with negatives, into the context's id-mask scratch behind the mask; the first threads
//                               clear the examples' bits of that mask (filled with ones on the stream before).
template <int MK, int NQ>
__global__ __launch_bounds__(64 * SW_WAVES) void recommend_sum_sweep_kernel(RecommendParams p) {
    sweep_tiles<MK, NQ>(p, [&](uint64_t my_row, bool valid, uint32_t, const float (&sc)[NQ], uint32_t nq_here) {
        if (!valid) return;
        uint2* slot = p.state + my_row;
        float S = sc[0];  // slot 0 is a positive: the chain starts as its score itself (a -0.0 stays -0.0)
        if (p.q0 != 0) {  // (wave-uniform: only the first pass starts the chain)
            const float cur = __uint_as_float(slot->x);
            S = rec_slot_positive(p.q0, p.first_neg) ? __fadd_rn(cur, sc[0]) : __fsub_rn(cur, sc[0]);
        }
#pragma unroll
        for (int q = 1; q < NQ; q++)
            if ((uint32_t)q < nq_here) S = rec_slot_positive(p.q0 + (uint32_t)q, p.first_neg) ? __fadd_rn(S, sc[q]) : __fsub_rn(S, sc[q]);  // (wave-uniform)
        typedef unsigned int v2u __attribute__((ext_vector_type(2)));
        v2u v;
        v.x = __float_as_uint(S);
        v.y = REC_SUM_MARK;
        __builtin_nontemporal_store(v, reinterpret_cast<v2u*>(slot));  // streamed, as recommend_sweep_kernel's
    });
}

// One lane per row.  keys: [n] 8-byte keys, zero when the kernel starts (d_gtable's protocol): only candidates are written.
__global__ __launch_bounds__(256) void recommend_sum_keys_kernel(uint2* state, uint32_t n, uint32_t take_max, uint32_t cmp, float thr, unsigned long long* keys) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint2 st = state[r];
    if (st.y == 0) return;  // never written, or an example's cleared slot: {0, 0}
    state[r] = make_uint2(0u, 0u);
    const float S = __uint_as_float(st.x);
    if (S != S || !cmp_holds(S, cmp, thr)) return;
    keys[r] = ((unsigned long long)ord_of(S, take_max != 0) << 32) | (uint32_t)(~(uint32_t)r);
}

struct RecommendAverageParams {
    const float* rows;
    float* q;                  // [dim]
    unsigned long long* mask;  // [ceil(rows / 64)] words of ones
    uint32_t ld, dim, n, first_neg;
    uint32_t ex[REC_MAX_EXAMPLES];  // the examples' rows, every one below the store's length (checked on the host)
};

__global__ __launch_bounds__(256) void recommend_average_kernel(RecommendAverageParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < p.n) atomicAnd(p.mask + (p.ex[i] >> 6), ~(1ull << (p.ex[i] & 63)));  // (at most 64: all in the first workgroup)
    if (i >= p.dim) return;
    float sp = p.rows[(uint64_t)p.ex[0] * p.ld + i];
    for (uint32_t e = 1; e < p.first_neg; e++) sp = __fadd_rn(sp, p.rows[(uint64_t)p.ex[e] * p.ld + i]);
    float q = __fdiv_rn(sp, (float)p.first_neg);  // correctly rounded, not a multiply by a reciprocal
    if (p.first_neg < p.n) {
        float sn = p.rows[(uint64_t)p.ex[p.first_neg] * p.ld + i];
        for (uint32_t e = p.first_neg + 1; e < p.n; e++) sn = __fadd_rn(sn, p.rows[(uint64_t)p.ex[e] * p.ld + i]);
        q = __fsub_rn(__fadd_rn(q, q), __fdiv_rn(sn, (float)(p.n - p.first_neg)));
    }
    p.q[i] = q;
}

// ---- the frame of a sweep over example rows (ExampleFrame, ott_internal.h) --------------------------------------------------------------
int ExampleFrame::begin(SweepParams* p, const float* host_block, uint32_t n_slots) {
    int rc;
    OTT_HIP(use_device(s));
    n = (uint32_t)s->n;
    if ((rc = sweep_prologue(s, d, host_block, n_slots, &st, p, &grid))) return rc;
    if (grid == 0) return OTT_OK;
    st.bytes_scanned = (uint64_t)st.passes * (st.vectors_compared / n_slots) * ((uint64_t)s->dim * 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));  // (no group id is read)
    // the states are left zeroed by the run's kernel that reads them last (or its memset), the keys by the top-k's select / compact kernel
    if ((rc = ensure_zeroed(s, s->d_rectable, s->rectable_clean, rec_state_bytes(n)))) return rc;  // (== disc_state_bytes, disc_key_bytes)
    if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, rec_key_bytes(n)))) return rc;
    state = (uint2*)s->d_rectable.p;
    keys = (unsigned long long*)s->d_gtable.p;
    p->gid = nullptr;  // (a store with groups has ids: this sweep does not read them)
    return OTT_OK;
}

int ExampleFrame::prepare(const uint32_t* gather_rows, uint32_t n_gather, bool tk_take_max, bool* also_clean) {
    rows = gather_rows;
    n_rows = n_gather;
    tk.n_groups = n;
    tk.nq = 1;
    tk.k = k_eff;
    tk.take_max = tk_take_max;
    tk.also_clean = also_clean;
    return tk.prepare(s, nullptr);
}

int ExampleFrame::sweep(uint32_t tile, const std::function<int(uint32_t q0)>& launch_pass) {
    int rc;
    ExampleGatherParams gp;
    memset(&gp, 0, sizeof(gp));
    gp.rows = s->d_rows;
    gp.inv = s->d_inv;
    gp.queries = (float*)s->d_queries.p;
    gp.qinv = (float*)((char*)s->d_queries.p + s->in_off_qinv);
    gp.state = state;
    gp.ld = s->ld;
    gp.dim = s->dim;
    gp.dimq = s->dimq;
    gp.n = n_rows;
    memcpy(gp.ex, rows, sizeof(uint32_t) * n_rows);
    hipLaunchKernelGGL(example_gather_kernel, dim3(n_rows), dim3(256), 0, s->stream, gp);
    OTT_HIP(hipGetLastError());
    if (timing()) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
    for (uint32_t ps = 0; ps < st.passes; ps++)
        if ((rc = launch_pass(ps * tile))) return rc;
    hipLaunchKernelGGL(example_clear_kernel, dim3(1), dim3(EX_CLEAR_LANES), 0, s->stream, gp);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

int ExampleFrame::rank() {
    int rc;
    if ((rc = tk.pass(s, keys, 0, 1))) return rc;
    if (timing()) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
    return OTT_OK;
}

int ExampleFrame::finish(ott_hit* out, uint64_t* n_hits) {
    int rc;
    if ((rc = tk.finish(s, timing(), out, n_hits, nullptr))) return rc;
    if (timing()) read_exact_events(s, &st);
    if (*n_hits > k_eff) return fail(OTT_ERR_HIP, std::string(who) + ": the top-k returned more hits than k");
    return OTT_OK;
}

void ExampleFrame::end() {
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
}

namespace {

int launch_keys(ott_store* s, uint2* state, uint32_t n, uint32_t side, bool take_max, const ott_query_desc* d, bool last, unsigned long long* keys) {
    hipLaunchKernelGGL(recommend_keys_kernel, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, s->stream, state, n, side, take_max ? 1u : 0u, (uint32_t)d->filter_cmp, d->filter_thr,
                       last ? 1u : 0u, keys);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

const char* refusal_text(RecRefusal r) {
    switch (r) {
        case REC_NO_POSITIVE: return "ott_query_recommend: at least one positive example is needed";
        case REC_NULL_LIST: return "ott_query_recommend: an example list is NULL";
        case REC_BAD_FLAGS: return "ott_query_recommend: unknown flag bits";
        case REC_HAS_QUERIES: return "ott_query_recommend: the examples are the queries; d->queries must be NULL and d->nq 0";
        case REC_PER_QUERY: return "ott_query_recommend: the examples make ONE query; PER_QUERY is not served";
        case REC_MFMA: return "ott_query_recommend: the MFMA path does not serve recommend queries; use path AUTO or EXACT";
        case REC_MULTI_GPU: return "ott_query_recommend: a multi-GPU store is not served (the examples' rows lie on different shards)";
        case REC_TOO_MANY_ROWS: return "ott_query_recommend: a store of more than 2^32 - 16 rows is not served";
        case REC_TOO_MANY: return "ott_query_recommend: more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples";
        case REC_SMALL_CAP: return "ott_query_recommend: output capacity is smaller than min(k, rows)";
        case REC_NULL_OUT: return "ott_query_recommend: out is NULL";
        default: return "";
    }
}

// strategy 0 is ott_query_recommend under its own name and texts; the other two are ott_query_recommend_strategy's
const char* entry_name(uint32_t strategy) { return strategy == REC_BEST_SCORE ? "ott_query_recommend" : "ott_query_recommend_strategy"; }

int refuse(uint32_t strategy, RecRefusal r, uint64_t id = 0, uint64_t len = 0) {
    const int code = rec_refusal_is_invalid(r) ? OTT_ERR_INVALID : OTT_ERR_UNSUPPORTED;
    const std::string who = entry_name(strategy);
    if (r == REC_BAD_ID) return fail(code, who + ": example id " + std::to_string(id) + " is not below the store's length " + std::to_string(len));
    if (r == REC_BOTH_SIDES) return fail(code, who + ": row " + std::to_string(id) + " is listed as both a positive and a negative example");
    return fail(code, strategy == REC_BEST_SCORE ? refusal_text(r) : rec_strategy_text(r));
}

// best_score (`sum` false) and sum_scores on a context whose `mu` the caller holds (and the owner's `rw`, shared): the frame with
// this strategy's sweep and keys kernels; best_score alone has a second round.  k_eff = min(k, rows) >= 1; every example < s->n.
int run_recommend(ott_store* s, const ott_query_desc* d, const RecExamples& ex, bool sum, uint32_t flags, uint64_t k_eff, ott_hit* out, uint64_t* n_out,
                  uint32_t* side_of_hit, ott_stats* stats_out) {
    int rc;
    ExampleFrame fr{s, d, entry_name(sum ? REC_SUM_SCORES : REC_BEST_SCORE), k_eff, stats_out};
    RecommendParams p{};
    if ((rc = fr.begin(&p, nullptr, ex.n))) return rc;
    uint64_t n1 = 0, n0 = 0;
    if (fr.grid != 0) {
        const uint32_t n = fr.n;
        p.state = fr.state;
        p.first_neg = ex.first_neg;
        const bool take_max = p.take_max != 0;
        const bool fill = !sum && rec_fill_possible(flags, ex);
        // (with a second round to come the first keys kernel does not read the states last: they are not clean behind the first top-k)
        if ((rc = fr.prepare(ex.rows, ex.n, take_max, fill ? nullptr : &s->rectable_clean))) return rc;
        const uint32_t tile = rec_tile(ex.n);
        rc = fr.sweep(tile, [&](uint32_t q0) {
            p.q0 = q0;
            return sum ? launch_sweep(s->stream, p, tile, fr.grid, OTT_SWEEP_KERNEL(recommend_sum_sweep_kernel))
                       : launch_sweep(s->stream, p, tile, fr.grid, OTT_SWEEP_KERNEL(recommend_sweep_kernel));
        });
        if (rc) return rc;
        if (sum) {
            hipLaunchKernelGGL(recommend_sum_keys_kernel, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, s->stream, p.state, n, take_max ? 1u : 0u, (uint32_t)d->filter_cmp, d->filter_thr,
                               fr.keys);
            OTT_HIP(hipGetLastError());
        } else if ((rc = launch_keys(s, p.state, n, 1u, take_max, d, !fill, fr.keys))) {
            return rc;
        }
        if ((rc = fr.rank())) return rc;
        if ((rc = fr.finish(out, &n1))) return rc;
        if (fill) {
            const uint64_t k2 = rec_second_k(fill, k_eff, n1);
            if (k2 != 0) {
                // the negative side: ascending bn through the flipped take; this keys kernel reads the states last
                if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, rec_key_bytes(n)))) return rc;
                GroupTopK t2;
                t2.n_groups = n;
                t2.nq = 1;
                t2.k = k2;
                t2.take_max = !take_max;
                t2.also_clean = &s->rectable_clean;
                if ((rc = t2.prepare(s, nullptr))) return rc;
                if ((rc = launch_keys(s, p.state, n, 0u, take_max, d, true, fr.keys))) return rc;
                if ((rc = t2.pass(s, fr.keys, 0, 1))) return rc;
                if ((rc = t2.finish(s, false, out + n1, &n0, nullptr))) return rc;
                if (n0 > k2) return fail(OTT_ERR_HIP, "ott_query_recommend: the second top-k returned more hits than it was asked for");
            } else {
                // no second round after all: nothing reads the states again
                OTT_HIP(hipMemsetAsync(s->d_rectable.p, 0, rec_state_bytes(n), s->stream));
                s->rectable_clean = true;  // (the stream orders the memset before the next query's sweep)
            }
        }
    }
    if (side_of_hit) {
        for (uint64_t i = 0; i < n1; i++) side_of_hit[i] = 1u;
        for (uint64_t i = 0; i < n0; i++) side_of_hit[n1 + i] = 0u;
    }
    if (n_out) *n_out = n1 + n0;
    fr.end();
    return OTT_OK;
}

// average_vector on a context whose `mu` the caller holds: the vector and the mask of every row but the examples are made on the
// device, the vector comes back (ott_query's host side computes its norm), and the query is ott_query's with that mask joined where
// every row mask reaches the kernels (run_ids_as_mask's route, ott_gather.hip).  Every example < s->n; s->n >= 1.
int run_recommend_average(ott_store* s, const ott_query_desc* d, const RecExamples& ex, ott_hit* out, uint64_t cap, uint64_t* n_out, uint32_t* side_of_hit,
                          ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t words = rec_mask_words(s->n);
    if ((rc = s->d_idmask.ensure(rec_mask_bytes(s->n, s->dim)))) return rc;
    uint64_t* d_words = (uint64_t*)s->d_idmask.p;
    RecommendAverageParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.rows = s->d_rows;
    ap.q = (float*)(d_words + 2 * words);
    ap.mask = (unsigned long long*)d_words;
    ap.ld = s->ld;
    ap.dim = s->dim;
    ap.n = ex.n;
    ap.first_neg = ex.first_neg;
    memcpy(ap.ex, ex.rows, sizeof(uint32_t) * ex.n);
    OTT_HIP(hipMemsetAsync(d_words, 0xFF, (size_t)words * 8, s->stream));
    hipLaunchKernelGGL(recommend_average_kernel, dim3((std::max(s->dim, ex.n) + 255) / 256), dim3(256), 0, s->stream, ap);
    OTT_HIP(hipGetLastError());
    std::vector<float> q(s->dim);
    OTT_HIP(hipMemcpyAsync(q.data(), ap.q, (size_t)s->dim * 4, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    ott_query_desc d2 = *d;
    d2.queries = q.data();
    d2.nq = 1;
    IdMaskGuard guard{s};
    s->cur_idmask = d_words;
    uint64_t n1 = 0;
    if ((rc = query_on(s, &d2, out, nullptr, cap, &n1, nullptr, nullptr, stats_out))) return rc;
    if (side_of_hit)
        for (uint64_t i = 0; i < n1; i++) side_of_hit[i] = 1u;
    if (n_out) *n_out = n1;
    return OTT_OK;
}

// The body of both entry points: `strategy` is known, and names the entry point (entry_name).
int recommend_entry(uint32_t strategy, ott_store* s, const ott_query_desc* d, const uint64_t* positive, uint64_t n_positive, const uint64_t* negative, uint64_t n_negative,
                    uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out, uint32_t* side_of_hit, ott_stats* stats) {
    const char* who = entry_name(strategy);
    int rc;
    // what the arguments and the descriptor alone decide comes first: these refusals need no store
    if (!d) return fail(OTT_ERR_INVALID, std::string(who) + ": desc is NULL");
    const bool has_queries = d->nq != 0 || d->queries != nullptr, per_query = d->mode == OTT_MODE_PER_QUERY, mfma = d->path == OTT_PATH_MFMA;
    RecRefusal why = strategy == REC_BEST_SCORE
                         ? rec_check_args(positive == nullptr, n_positive, negative == nullptr, n_negative, flags, has_queries, per_query, mfma)
                         : rec_strategy_check_args(strategy, positive == nullptr, n_positive, negative == nullptr, n_negative, flags, has_queries, per_query, mfma,
                                                   d->metric == OTT_METRIC_MANHATTAN);
    if (why != REC_OK) return refuse(strategy, why);
    if ((rc = check_desc_enums(who, d))) return rc;
    if (!s) return fail(OTT_ERR_INVALID, std::string(who) + ": store is NULL");
    const uint64_t len = ott_store_len(s);
    if ((why = rec_check_store(s->multi != nullptr, len)) != REC_OK) return refuse(strategy, why);
    if ((rc = check_device_row_mask(who, s, d))) return rc;
    RecExamples ex;
    uint64_t bad = 0;
    if ((why = rec_examples(positive, n_positive, negative, n_negative, len, &ex, &bad)) != REC_OK) return refuse(strategy, why, bad, len);
    if ((why = rec_check_out(rec_k_eff(d->k, len), cap, out == nullptr)) != REC_OK) return refuse(strategy, why);
    ott::host::SharedLock rd;  // the corpus cannot change while this query runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    // what the checks above read without the lock is read again, and k_eff only here: appends (this call's own flush of rows another
    // thread staged after `len` was read) or a compact may have come in between, so the store may be longer or shorter than `len`
    if ((why = rec_check_store(false, s->n)) != REC_OK) return refuse(strategy, why);
    for (uint32_t e = 0; e < ex.n; e++)
        if (ex.rows[e] >= s->n) return refuse(strategy, REC_BAD_ID, ex.rows[e], s->n);
    const uint64_t k_eff = rec_k_eff(d->k, s->n);
    if ((why = rec_check_out(k_eff, cap, out == nullptr)) != REC_OK) return refuse(strategy, why);
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (k_eff == 0) return OTT_OK;
    CtxLease ctx(s);
    if (strategy == REC_AVERAGE_VECTOR) return run_recommend_average(ctx.c, d, ex, out, cap, n_out, side_of_hit, stats);
    return run_recommend(ctx.c, d, ex, strategy == REC_SUM_SCORES, flags, k_eff, out, n_out, side_of_hit, stats);
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_recommend(ott_store* s, const ott_query_desc* d, const uint64_t* positive, uint64_t n_positive, const uint64_t* negative, uint64_t n_negative,
                        uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out, uint32_t* side_of_hit, ott_stats* stats) {
    return recommend_entry(REC_BEST_SCORE, s, d, positive, n_positive, negative, n_negative, flags, out, cap, n_out, side_of_hit, stats);
}

// strategy 0 is ott_query_recommend whole, with that name in its messages; an unknown strategy is refused before anything else is looked at
int ott_query_recommend_strategy(ott_store* s, const ott_query_desc* d, uint32_t strategy, const uint64_t* positive, uint64_t n_positive, const uint64_t* negative,
                                 uint64_t n_negative, uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out, uint32_t* side_of_hit, ott_stats* stats) {
    if (!rec_strategy_known(strategy)) return refuse(strategy, REC_BAD_STRATEGY);
    return recommend_entry(strategy, s, d, positive, n_positive, negative, n_negative, flags, out, cap, n_out, side_of_hit, stats);
}

}  // extern "C"
