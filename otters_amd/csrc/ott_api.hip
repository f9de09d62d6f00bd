// ott_api.hip — ott_query: the body of VecQueryPlan::collect (src/vec.rs:206-311) and the
// score + merge block of MetaQueryPlan::collect (src/meta.rs:671-709) on one MI355X.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ott_internal.h"
#include "ott_prune.h"
#include "ott_i8_check.h"

using namespace ott;

namespace ott {

// query-side inverse norm, src/vec.rs:390-396 (sequential f32 sum, sqrt, reciprocal; the file
// is built with -ffp-contract=off, `volatile` keeps the compiler from widening or reordering)
float host_inv_norm_exact(const float* v, uint32_t dim) {
    volatile float s = 0.0f;
    for (uint32_t i = 0; i < dim; i++) {
        volatile float sq = v[i] * v[i];
        s = s + sq;
    }
    float norm = sqrtf(s);
    return norm != 0.0f ? 1.0f / norm : 0.0f;
}

std::vector<uint32_t> tile_prefix(const RunPlan& pl, uint32_t tile_rows) {
    std::vector<uint32_t> pre;
    pre.push_back(0);
    uint64_t tiles = 0;
    for (const auto& r : pl.runs) {
        tiles += (r.count + tile_rows - 1) / tile_rows;
        pre.push_back((uint32_t)tiles);
    }
    return pre;
}

}  // namespace ott


namespace ott {

int upload_exact_inputs(ott_store* s, const float* queries, uint32_t nq, const RunPlan& pl, const std::vector<uint32_t>& prefix) {
    const uint32_t nq_pad = (nq + 7u) & ~7u;  // the kernels read whole NQ-wide query blocks: pad with zero rows
    const size_t q_bytes = (size_t)nq_pad * s->dimq * 4, qi_bytes = (size_t)nq_pad * 4;
    const size_t run_bytes = pl.runs.size() * sizeof(ott_run), pre_bytes = prefix.size() * 4;
    size_t off_q = 0, off_qi = off_q + q_bytes, off_run = (off_qi + qi_bytes + 15) & ~(size_t)15;
    size_t off_pre = off_run + run_bytes, total = off_pre + pre_bytes;
    int rc = s->h_stage.ensure(total);
    if (rc) return rc;
    char* hs = (char*)s->h_stage.p;
    float* hq = (float*)(hs + off_q);
    memset(hq, 0, q_bytes + qi_bytes);
    // (queries == nullptr: the block goes up zeroed and a kernel fills it from stored rows, ott_recommend.hip)
    for (uint32_t i = 0; queries != nullptr && i < nq; i++) {
        memcpy(hq + (size_t)i * s->dimq, queries + (size_t)i * s->dim, (size_t)s->dim * 4);
        ((float*)(hs + off_qi))[i] = host_inv_norm_exact(queries + (size_t)i * s->dim, s->dim);
    }
    memcpy(hs + off_run, pl.runs.data(), run_bytes);
    memcpy(hs + off_pre, prefix.data(), pre_bytes);
    // one device block, one copy: [queries | qinv | runs | tile prefix]
    if ((rc = s->d_queries.ensure(total))) return rc;
    OTT_HIP(hipMemcpyAsync(s->d_queries.p, hs, total, hipMemcpyHostToDevice, s->stream));
    s->in_off_qinv = off_qi;
    s->in_off_runs = off_run;
    s->in_off_prefix = off_pre;
    return OTT_OK;
}

void fill_exact_params(ott_store* s, const ott_query_desc* d, const RunPlan& pl, uint32_t nq, const uint64_t* d_mask, uint64_t mask_bits,
                       uint32_t n_tiles, ExactParams& p) {
    memset(&p, 0, sizeof(p));
    p.rows = s->d_rows;
    p.inv = s->d_inv;
    p.queries = (const float*)s->d_queries.p;
    p.qinv = (const float*)((const char*)s->d_queries.p + s->in_off_qinv);
    p.row_mask = d_mask;
    p.row_mask_bits = mask_bits;
    p.runs = (const ott_run*)((const char*)s->d_queries.p + s->in_off_runs);
    p.tile_prefix = (const uint32_t*)((const char*)s->d_queries.p + s->in_off_prefix);
    p.ld = s->ld;
    p.dim = s->dim;
    p.dimq = s->dimq;
    p.n_runs = (uint32_t)pl.runs.size();
    p.n_tiles = n_tiles;
    p.nq_total = nq;
    p.metric = d->metric;
    p.take_max = d->take == OTT_TAKE_MAX;
    p.cmp = d->filter_cmp;
    p.thr = d->filter_thr;
    p.reduce = s->reduce;
    p.tie_sh = s->cur_tie_sh;
    p.tie_off = s->cur_tie_off;
    p.flat = s->cur_flat ? 1u : 0u;
}

void embed_exact_inputs(ExactParams& p, const void* query, size_t query_bytes, float inv_norm, const RunPlan& pl, const std::vector<uint32_t>& prefix) {
    p.embedded = 1;
    p.queries = nullptr;
    p.qinv = nullptr;
    p.runs = nullptr;
    p.tile_prefix = nullptr;
    memcpy(p.qemb, query, query_bytes);  // the tail up to dimq stays zero (fill_exact_params cleared the struct)
    p.eqinv = inv_norm;
    memset(p.eruns, 0, sizeof(p.eruns));  // (a copy of another launch's parameters may hold that launch's runs)
    memset(p.eprefix, 0, sizeof(p.eprefix));
    for (size_t i = 0; i < pl.runs.size(); i++) p.eruns[i] = pl.runs[i];
    for (size_t i = 0; i < prefix.size(); i++) p.eprefix[i] = prefix[i];
}

}  // namespace ott

namespace {

// chunk mask -> runs of consecutive surviving chunks (candidate_chunks, src/meta.rs:648-659)
void build_plan(const ott_store* s, const uint64_t* chunk_mask, RunPlan& pl) {
    const uint64_t n = s->n, cs = s->chunk_size;
    pl.total_chunks = n ? (n + cs - 1) / cs : 0;
    if (!n) return;
    if (!chunk_mask) {
        pl.runs.push_back({0, n});
        pl.evaluated = pl.total_chunks;
        pl.rows_scored = n;
        return;
    }
    bool open = false;
    for (uint64_t c = 0; c < pl.total_chunks; c++) {
        const bool keep = (chunk_mask[c >> 6] >> (c & 63)) & 1;
        if (keep) {
            const uint64_t start = c * cs;
            const uint64_t len = (n - start) < cs ? (n - start) : cs;
            if (open) pl.runs.back().count += len;
            else pl.runs.push_back({start, len});
            open = true;
            pl.evaluated++;
            pl.rows_scored += len;
        } else {
            open = false;
        }
    }
}

}  // namespace

namespace ott {
void make_run_plan(const ott_store* s, const uint64_t* chunk_mask, RunPlan& pl) { build_plan(s, chunk_mask, pl); }

int check_desc_enums(const char* who, const ott_query_desc* d) {
    const auto unknown = [who](const char* what) { return fail(OTT_ERR_INVALID, std::string(who) + ": unknown " + what); };
    if (d->metric > OTT_METRIC_MANHATTAN) return unknown("metric");
    if (d->take > OTT_TAKE_MAX) return unknown("take type");
    if (d->filter_cmp > OTT_CMP_EQ) return unknown("filter comparator");
    if (d->mode > OTT_MODE_PER_QUERY) return unknown("mode");
    if (d->path > OTT_PATH_MFMA) return unknown("path");
    return OTT_OK;
}

int check_device_row_mask(const char* who, const ott_store* s, const ott_query_desc* d) {
    if (d->use_device_row_mask && s->evalmask_bits == 0 && s->n)
        return fail(OTT_ERR_INVALID, std::string(who) + ": use_device_row_mask set but ott_store_eval_row_mask was not called");
    return OTT_OK;
}

int validate_query(const ott_store* s, const ott_query_desc* d) {
    int rc;
    if (!s) return fail(OTT_ERR_INVALID, "ott_query: store is NULL");
    if (!d) return fail(OTT_ERR_INVALID, "ott_query: desc is NULL");
    if (d->nq == 0) return fail(OTT_ERR_INVALID, "No queries provided");  // src/vec.rs:188-190
    if (!d->queries) return fail(OTT_ERR_INVALID, "ott_query: queries is NULL");
    if ((rc = check_desc_enums("ott_query", d))) return rc;
    if (d->path == OTT_PATH_MFMA && d->metric == OTT_METRIC_MANHATTAN)  // |q - v| is not a dot product: no candidate pass bounds it
        return fail(OTT_ERR_UNSUPPORTED, "ott_query: the MFMA path does not score the Manhattan metric; use path AUTO or EXACT");
    return check_device_row_mask("ott_query", s, d);
}

void read_exact_events(ott_store* s, ott_stats* st) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->ev[3], s->ev[4]) == hipSuccess) st->score_ns = (uint64_t)(ms * 1e6);
    if (hipEventElapsedTime(&ms, s->ev[4], s->ev[5]) == hipSuccess) st->merge_ns = (uint64_t)(ms * 1e6);
}
}  // namespace ott

namespace {

// total of the per-group counts a merge launch left in device memory (PER_QUERY device output)
__global__ void sum_counts_kernel(const uint64_t* counts, uint32_t n, uint64_t* out) {
    uint64_t t = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 64) t += counts[i];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (threadIdx.x == 0) *out = t;
}

// One call over the lists (k <= 512): what run_exact's stages share
struct ExactCtx {
    ott_store* s;
    const float* queries;
    uint32_t nq;
    const ott_query_desc* d;
    bool perq;
    const RunPlan& pl;
    uint64_t k_eff;
    bool fetch, timing;
    const std::vector<uint32_t>& prefix;  // the 64-row tiles of pl
    ExactPlan x;                          // ott_exact_plan.h
    uint32_t groups;                      // result groups: 1 merged, nq per query
    // the pruned sweep (prune.c != 0): the seed's rows and the rest with their tiles and grids, the query's bounds
    PrunePlan prune{0, false, 0};
    RunPlan plA, plB;
    std::vector<uint32_t> preA, preB;
    int gridA = 0, gridB = 0;
    double qt = 0.0, qn = 0.0, q1 = 0.0;
    PruneQuant qq{0, 0.0f, 0.0f, 0.0, 0};  // four bits per dim: the quantised query (ott_prune.h)
    bool head = false;                     // ... in the head form: no f32 stage in front, the query-side values over the whole query
    bool seed_est = false;                 // the seed is an estimate pass over plA; plB is then the WHOLE plan and the final merge takes its lists alone
    bool ride = false;                     // ... and the final merge writes the counters' totals behind the hits (prune_plan_ride): no copy, no ev[4]
    // the int8 check of the gated launch's survivors (ott_exact_plan.h: prune_plan_i8_check): the plane and its scales as they were
    // when the call was planned, the query's scale and the certified error
    bool i8_check = false;
    const int8_t* chk_plane = nullptr;
    const float* chk_scale = nullptr;
    float chk_qscale = 0.0f, chk_eps = 0.0f;
    // the query's reference-order inverse norm (one dependent float chain over the dims): taken once, by whoever asks first — the
    // check's plan or the embedded call
    bool have_q_inv = false;
    float q_inv = 0.0f;
    float query_inv_norm() {
        if (!have_q_inv) {
            q_inv = host_inv_norm_exact(queries, s->dim);
            have_q_inv = true;
        }
        return q_inv;
    }
    // the result block, as the merge kernel sees it
    ExactResult res{0, 0, 0};
    uint64_t* d_counts = nullptr;
    ott_hit* d_hits = nullptr;
    ExactParams p;
};

// Whether the pruned sweep runs, and over which rows: the header's plan, and the two conditions that need the runs and the query
// themselves — the seed and the rest have at most two runs each (they ride in the kernel arguments) and the rest is not empty;
// prune_query_bounds accepts the query
void plan_pruned_sweep(ExactCtx& c) {
    ott_store* s = c.s;
    const PruneIn in{s->dim, s->ld, c.d->metric, c.perq, c.x.lean, s->cur_flat, c.x.variant, s->opt.exact_prune, s->opt.exact_sketch,
                     SketchState{s->d_sketch != nullptr, s->sk_n >= s->n, s->sk_bits, s->sk_words, s->sk_stage0}, c.pl.rows_scored, c.x.E};
    PrunePlan pp = prune_plan(in);
    // (the four-bit form needs the quantised query; a query the quantiser refuses takes the plan of a store without a sketch.  The
    // head form — the same plan, the checkpoint in front of stage 0 — takes the query-side sums over the whole query, m = 0, the
    // other forms from the checkpoint on.  Whether the quantiser accepts the query does not depend on m and the head form runs
    // exactly when it accepts and everything else allows it, so m is known before the one call: the query is walked once)
    const HeadState hs{s->d_head != nullptr, s->head_n >= s->n, s->opt.exact_sketch_head};
#ifdef OTT_SK4_DECODE_F32  // (experiment builds with the former f32 decode have no head kernel)
    const bool head_if_ok = false;
#else
    const bool head_if_ok = prune_plan_head(in, pp, true, hs);
#endif
    bool quant_ok = false;
    if (prune_plan_needs_quant(in, pp) && !(quant_ok = prune_query_quant(c.queries, s->dim, head_if_ok ? 0u : pp.c * 32, &c.qq))) pp = prune_plan_quant_refused(in);
    if (!pp.c) return;
    const bool head = head_if_ok && quant_ok;
    const uint32_t m = head ? 0u : pp.c * 32;
    // (the seed as an estimate pass: over the first rows, the plan's seed unless an experiment build says otherwise; the gated launch
    // then takes every row, the seed's included)
    const uint64_t est_rows = prune_plan_seed_est(in, pp, head, c.d->filter_cmp != OTT_CMP_NONE);
    split_plan(c.pl, est_rows ? est_rows : pp.seed, c.plA, c.plB);
    const bool two_runs_each = c.plA.runs.size() <= 2 && c.plB.runs.size() <= 2 && c.plB.rows_scored > 0;
    if (!two_runs_each || !prune_query_bounds(c.queries, s->dim, m, &c.qt, &c.qn)) return;
    c.prune = pp;
    c.head = head;
    c.seed_est = est_rows != 0;
    c.ride = prune_plan_ride(est_rows, c.x.E, c.fetch, MergeOptions{s->opt.merge_rank1, s->opt.merge_walk});
    if (c.seed_est) c.plB = c.pl;  // (a lean call: at most two runs)
    c.q1 = prune_query_l1(c.queries, s->dim, m);
    c.preA = tile_prefix(c.plA, 64);
    c.preB = tile_prefix(c.plB, 64);
    c.gridA = exact_grid(s, c.preA.back());
    c.gridB = exact_grid(s, c.preB.back());
    // (the int8 check: asked only where everything else allows it — the plane is looked at under its lock, never built; the query is
    // quantised as run_i8_single quantises it, and the kernel makes the same operand from the scale)
    if (head && c.x.E == 1 && s->opt.exact_i8_check != 0) {
        I8CheckState ck{false, s->opt.exact_i8_check, false};
        float rel = 0.0f;
        if ((ck.plane_ready = i8_plane_peek(s, &c.chk_plane, &c.chk_scale, &rel))) {
            const I8Query iq = i8_query_quant(c.queries, s->dim, c.d->metric == OTT_METRIC_COSINE, c.query_inv_norm(), nullptr);
            const I8CheckEps e = i8_check_eps(s->dim, c.d->metric, s->opt.eps_scale_ppm, rel, iq, max_norm(s->min_pos_inv));
            ck.eps_ok = e.ok;
            c.chk_qscale = iq.s_q;
            c.chk_eps = e.eps;
        }
        c.i8_check = prune_plan_i8_check(in, pp, head, ck);
    }
}

// the inputs on the device (unless they ride in the arguments), room for the block lists, and the result block
int ensure_exact_result(ExactCtx& c) {
    ott_store* s = c.s;
    int rc;
    if (!c.x.lean && (rc = upload_exact_inputs(s, c.queries, c.nq, c.pl, c.prefix))) return rc;
    const size_t n_lists_total = exact_n_lists(c.x, c.nq, c.perq, c.prune.c != 0, c.gridA, c.gridB);
    if ((rc = s->d_lists.ensure(n_lists_total * c.x.KS * sizeof(Cand)))) return rc;
    // results block: [counts (groups x u64, padded to 64 B) | hits (groups x KS)].  Host output: the merge kernel
    // writes it straight into pinned host memory (no D2H copy behind the launch); device output: into d_hits
    c.res = exact_result_layout(c.groups, c.x.KS);
    char* res_dev = nullptr;
    if (c.fetch) {
        if ((rc = s->h_hits.ensure(c.res.host_bytes + 8))) return rc;  // (+ 8 and 8: the pruned sweep's two counters)
        void* mapped = nullptr;
        OTT_HIP(hipHostGetDevicePointer(&mapped, s->h_hits.p, 0));
        res_dev = (char*)mapped;
    } else {
        if ((rc = s->d_hits.ensure(c.res.bytes))) return rc;
        res_dev = (char*)s->d_hits.p;
    }
    c.d_counts = (uint64_t*)res_dev;
    c.d_hits = (ott_hit*)(res_dev + c.res.cnt_pad);
    return OTT_OK;
}

void fill_exact_call(ExactCtx& c, const uint64_t* d_mask, uint64_t mask_bits) {
    ott_store* s = c.s;
    fill_exact_params(s, c.d, c.pl, c.nq, d_mask, mask_bits, c.prefix.back(), c.p);
    c.p.k = (uint32_t)c.k_eff;
    c.p.perq = c.perq;
    c.p.list_stride = c.x.KS;
    c.p.small = c.x.variant;
    if (c.x.lean) embed_exact_inputs(c.p, c.queries, (size_t)s->dim * 4, c.query_inv_norm(), c.pl, c.prefix);
}

// the call's parameters over a part of its rows (the pruned sweep's seed, or the rest), its block lists at dst
ExactParams part_params(const ExactCtx& c, const RunPlan& sub, const std::vector<uint32_t>& pre, Cand* dst) {
    ExactParams q = c.p;
    q.n_runs = (uint32_t)sub.runs.size();
    q.n_tiles = pre.back();
    embed_exact_inputs(q, c.queries, (size_t)c.s->dim * 4, c.p.eqinv, sub, pre);
    q.lists = dst;
    return q;
}

// The pruned sweep: the seed launch, its merge, and the gated launch over the rest
int pruned_sweep(ExactCtx& c) {
    ott_store* s = c.s;
    const uint32_t KS = c.x.KS;
    int rc;
    // [count (u64, 64 B) | KS hits]: the seed's merged result, read by the second launch
    if ((rc = s->d_prune.ensure(64 + (size_t)KS * sizeof(ott_hit)))) return rc;
    uint64_t* seed_res = (uint64_t*)s->d_prune.p;
    // the kernel's counts of the rows that passed the gate and of the rows it finished in f32 (one and the same count without the
    // int8 check): running totals in device memory, read back with the result (host output only)
    unsigned long long* tails_dev = nullptr;
    if (c.fetch) {
        if (!s->d_tails.p) {
            if ((rc = s->d_tails.ensure(16))) return rc;
            OTT_HIP(hipMemsetAsync(s->d_tails.p, 0, 16, s->stream));
            s->tails_seen = 0;
            s->fin_seen = 0;
        }
        tails_dev = (unsigned long long*)s->d_tails.p;
    }
    ExactParams pa = part_params(c, c.plA, c.preA, (Cand*)s->d_lists.p);
    // what both launches of the sketch forms read: the lines, the quantised query's values, the head
    auto sketch_inputs = [&](ExactParams& q) {
        q.prune_stage = c.prune.c;
        q.prune_qt = c.qt;
        q.prune_qn = c.qn;
        if (!c.prune.sketch) return;
        q.prune_sketch = s->d_sketch;
        q.sk_pitch = s->sk_pitch;
        q.sk_stage0 = s->sk_stage0;
        q.sk_bits = s->sk_bits;
        q.prune_q1 = c.q1;
        q.prune_qe1 = c.qq.qe1;
        q.prune_qscale = c.qq.scale;
        q.prune_qinv_scale = c.qq.inv_scale;
        q.prune_qsum = c.qq.qsum;
        if (c.head) {
            q.prune_head_codes = reinterpret_cast<const uint32_t*>(s->d_head);
            q.prune_head_rho = reinterpret_cast<const float*>(s->d_head + s->cap * (size_t)16);
        }
    };
    if (c.seed_est) {  // the estimate pass: no gate and no tail counter
        sketch_inputs(pa);
        pa.seed_est = 1;
        pa.seed_keep = prune_seed_keep(c.k_eff);
    }
    if ((rc = launch_exact(s, pa, 1, c.x.E, c.gridA))) return rc;
    if ((rc = launch_merge(s, (const Cand*)s->d_lists.p, (uint32_t)c.gridA, KS, 0, 1, (uint32_t)c.k_eff, c.x.E, c.p.take_max != 0, tie_base(s),
                           (ott_hit*)(seed_res + 8), KS, seed_res, s->cur_tie_sh)))
        return rc;
    ExactParams pb = part_params(c, c.plB, c.preB, (Cand*)s->d_lists.p + (size_t)c.gridA * KS);
    sketch_inputs(pb);
    pb.prune_seed = seed_res;
    pb.prune_tails = tails_dev;
    if (c.i8_check) {
        pb.chk_plane = c.chk_plane;
        pb.i8_scale = c.chk_scale;
        pb.flag = s->d_flag;
        pb.i8_qscale = c.chk_qscale;
        pb.chk_eps = c.chk_eps;
    }
    return launch_exact(s, pb, 1, c.x.E, c.gridB);
}

int plain_passes(ExactCtx& c) {
    ott_store* s = c.s;
    const uint32_t tile = c.x.tile;
    int rc;
    for (uint32_t ps = 0; ps < c.x.passes; ps++) {
        c.p.q0 = ps * tile;
        // merged: one list group per pass.  per-query: list (query, block) lives at (query*grid + block)*KS; a
        // 1-query pass runs the single-list kernel, so it is pointed at its query's slot (q0 == ps there)
        c.p.lists = (Cand*)s->d_lists.p + ((c.perq && tile > 1) ? 0 : (size_t)ps * c.x.grid * c.x.KS);
        if ((rc = launch_exact(s, c.p, (int)tile, c.x.E, c.x.grid))) return rc;
    }
    return OTT_OK;
}

// the block lists into the result block: per query every query's own `grid` lists, else all of them (the pruned sweep: of both
// launches — behind an estimate pass of the gated launch alone, which saw every row: a seed row would appear twice)
int merge_exact(ExactCtx& c) {
    ott_store* s = c.s;
    const uint32_t KS = c.x.KS, grid = (uint32_t)c.x.grid;
    if (c.seed_est)  // (the counters riding: this launch also writes their totals behind the result block)
        return launch_merge(s, (const Cand*)s->d_lists.p + (size_t)c.gridA * KS, (uint32_t)c.gridB, KS, 0, c.groups, (uint32_t)c.k_eff, c.x.E,
                            c.p.take_max != 0, tie_base(s), c.d_hits, KS, c.d_counts, s->cur_tie_sh,
                            c.ride ? (unsigned long long*)s->d_tails.p : nullptr, c.ride ? (unsigned long long*)((char*)c.d_counts + c.res.bytes) : nullptr);
    const uint32_t n_lists = c.perq ? grid : (uint32_t)exact_n_lists(c.x, c.nq, false, c.prune.c != 0, c.gridA, c.gridB);
    return launch_merge(s, (const Cand*)s->d_lists.p, n_lists, KS, c.perq ? (uint64_t)grid * KS : 0, c.groups, (uint32_t)c.k_eff, c.x.E,
                        c.p.take_max != 0, tie_base(s), c.d_hits, KS, c.d_counts, s->cur_tie_sh);
}

// host output: the one wait, then the lists out of the pinned block
int fetch_exact(ExactCtx& c, std::vector<std::vector<ott_hit>>& lists, ott_stats& st) {
    ott_store* s = c.s;
    const uint32_t KS = c.x.KS;
    char* hh = (char*)s->h_hits.p;
    // (the counters riding: the final merge has written the two totals there itself)
    if (c.prune.c && !c.ride) OTT_HIP(hipMemcpyAsync(hh + c.res.bytes, s->d_tails.p, 16, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    // rows whose last stages were read after the checkpoint (the seed's rows are not counted: they have no checkpoint; behind an
    // estimate pass the gated launch covers every row, the few rows that pass finished are not counted)
    if (c.prune.c) {
        uint64_t total[2];
        memcpy(total, hh + c.res.bytes, 16);
        const uint64_t passed = total[0] - s->tails_seen;
        // (with the int8 check the rows finished in f32 are counted apart; without it they are the rows that passed)
        (s->owner ? s->owner : s)->exact_finished.fetch_add(c.i8_check ? total[1] - s->fin_seen : passed, std::memory_order_relaxed);
        st.rescored += passed;
        s->tails_seen = total[0];
        s->fin_seen = total[1];
    }
    const uint64_t* counts = (const uint64_t*)hh;
    const ott_hit* hits = (const ott_hit*)(hh + c.res.cnt_pad);
    lists.assign(c.groups, {});
    for (uint32_t g = 0; g < c.groups; g++) lists[g].assign(hits + (size_t)g * KS, hits + (size_t)g * KS + counts[g]);
    float ms = 0.f;
    if (c.ride) {  // one span over the chain, the merges inside it: no marker was recorded between the gated launch and its merge
        if (c.timing && hipEventElapsedTime(&ms, s->ev[3], s->ev[5]) == hipSuccess) st.score_ns += (uint64_t)(ms * 1e6);
        return OTT_OK;
    }
    if (c.timing && hipEventElapsedTime(&ms, s->ev[3], s->ev[4]) == hipSuccess) st.score_ns += (uint64_t)(ms * 1e6);
    if (c.timing && hipEventElapsedTime(&ms, s->ev[4], s->ev[5]) == hipSuccess) st.merge_ns += (uint64_t)(ms * 1e6);
    return OTT_OK;
}

// EXACT path.  queries: host [nq*dim].  Results: per group (1 for merged, nq for per-query) on the
// host in `lists`.  `perq` selects the grouping.  Device output (!fetch, merged or per query): the merge kernel leaves its
// [groups][KS] sentinel-padded hits in d_hits for ott_query_device — or, with hits_dev_direct, writes them straight there
// (direct_stride must be the KS this call derives from k_eff).
// What the call looks like — lists or sort path, list width, kernel variant, passes, grid, lean, the pruned sweep, the result
// block — is decided in ott_exact_plan.h; the stages above run it.
int run_exact(ott_store* s, const float* queries, uint32_t nq, const ott_query_desc* d, bool perq, const RunPlan& pl, uint64_t k_eff,
              const uint64_t* d_mask, uint64_t mask_bits, bool fetch, std::vector<std::vector<ott_hit>>& lists, ott_stats& st,
              bool timing = true, ott_hit* hits_dev_direct = nullptr, uint32_t direct_stride = 0) {
    switch (lists_or_sort(k_eff, nq, pl.rows_scored, s->opt.large_k_from, fetch)) {
        case EXACT_REFUSED: return fail(OTT_ERR_UNSUPPORTED, "ott_query_device: k > 512 is host-output only");
        case EXACT_SORT: return run_large_k(s, queries, nq, d, perq, pl, k_eff, d_mask, mask_bits, lists, st);  // score dump + device radix sort
        case EXACT_LISTS: break;
    }
    const std::vector<uint32_t> prefix = tile_prefix(pl, 64);
    ExactCtx c{s, queries, nq, d, perq, pl, k_eff, fetch, timing, prefix,
               exact_plan(k_eff, nq, perq, s->dimq, prefix.back(), pl.runs.size(), s->opt.exact_small, exact_grid(s, prefix.back())), perq ? nq : 1u};
    plan_pruned_sweep(c);
    int rc;
    if ((rc = ensure_exact_result(c))) return rc;
    if (!fetch && hits_dev_direct != nullptr && direct_stride == c.x.KS) c.d_hits = hits_dev_direct;
    fill_exact_call(c, d_mask, mask_bits);

    if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
    if ((rc = c.prune.c ? pruned_sweep(c) : plain_passes(c))) return rc;
    if (timing && !c.ride) OTT_HIP(hipEventRecord(s->ev[4], s->stream));  // (no marker inside a chain whose counters ride: it kept the merge 6 us behind the gated launch)
    if ((rc = merge_exact(c))) return rc;
    if (timing) OTT_HIP(hipEventRecord(s->ev[5], s->stream));
    st.passes += c.x.passes;
    st.bytes_scanned += exact_bytes_scanned(c.x.passes, pl.rows_scored, s->dim, d->metric);
    return fetch ? fetch_exact(c, lists, st) : OTT_OK;
}

}  // namespace

// The row mask a query's kernels get, on the context's stream: the caller's host mask (uploaded) or the evaluated device mask,
// ANDed with the mask of an id list that takes the mask route (ott_gather.hip: cur_idmask) and with the live mask of deleted
// rows (ott_tomb.hip).  A query that brings none of them gets nullptr and takes neither branch.
int ott::compose_row_mask(ott_store* s, const ott_query_desc* d, const uint64_t** d_mask_out, uint64_t* mask_bits_out) {
    int rc;
    const uint64_t* d_mask = nullptr;
    uint64_t mask_bits = 0;
    if (d->use_device_row_mask) {
        d_mask = (const uint64_t*)s->d_evalmask.p;
        mask_bits = s->evalmask_bits;
    } else if (d->row_mask && d->row_mask_bits) {
        const size_t words = (size_t)((d->row_mask_bits + 63) / 64);
        if ((rc = s->d_rowmask.ensure(words * 8))) return rc;
        OTT_HIP(hipMemcpyAsync(s->d_rowmask.p, d->row_mask, words * 8, hipMemcpyHostToDevice, s->stream));
        d_mask = (const uint64_t*)s->d_rowmask.p;
        mask_bits = d->row_mask_bits;
    }
    // an id list on the mask route: its bits over the store's rows, ANDed with the caller's mask into the words behind them
    if (s->cur_idmask) {
        if (d_mask) {
            uint64_t* both = s->cur_idmask + (s->n + 63) / 64;
            if ((rc = mask_and(s, s->cur_idmask, d_mask, mask_bits, s->n, both))) return rc;
            d_mask = both;
        } else {
            d_mask = s->cur_idmask;
        }
        mask_bits = s->n;
    }
    // a by-mask-group run of ott_query_masks (ott_masks.hip): the queries' own mask joins the same way, in that call's scratch
    if (s->cur_qmask && (rc = masks_join(s, &d_mask, &mask_bits))) return rc;
    // deleted rows (ott_tomb.hip): the store's live mask joins here — as the mask itself when the query brought none, else ANDed
    // with it into this context's scratch.  A store without deletions has no live mask and takes neither branch.
    if (s->n_dead && (rc = live_compose(s, &d_mask, &mask_bits))) return rc;
    *d_mask_out = d_mask;
    *mask_bits_out = mask_bits;
    return OTT_OK;
}

// runs on a query context `s` (the store itself or one of its workers) whose `mu` the caller holds
int ott::query_on(ott_store* s, const ott_query_desc* d, ott_hit* out_host, void* out_dev, uint64_t cap, uint64_t* n_out,
                  uint64_t* n_per_query, void* n_out_dev, ott_stats* stats_out, bool nosync, bool* events_pending) {
    CoreOpts co;
    if (s->opt.tie_order != 0) {
        // host output: the reference's literal outcome (ott_ties.hip).  Device output (ott_query_device, the shard blocks of
        // ott_query_sharded): candidates ranked in the reference's visit order, without the collector's anchor rule
        if (out_host && !out_dev) {
            if (events_pending) *events_pending = false;
            return query_ref_ties(s, d, out_host, cap, n_out, n_per_query, stats_out);
        }
        co.tie_sh = 3;
    }
    return query_core(s, d, out_host, out_dev, cap, n_out, n_per_query, n_out_dev, stats_out, nosync, events_pending, co);
}

namespace {

// where one query's result goes: the caller's host buffer or device block and the counts beside it
struct QueryOut {
    ott_hit* host;
    void* dev;
    uint64_t cap;
    uint64_t* n_out;
    uint64_t* n_per_query;
    void* n_dev;
    bool nosync;
    bool* events_pending;
};

// the one way out of a query that went well
int finish(ott_stats& st, uint64_t t0, ott_stats* stats_out) {
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

// device output: every slot the scoring path does not write must hold a sentinel.  The fill is queued lazily: the exact path
// writing a block of exactly its own geometry, and the staged host lists, cover every slot themselves
int fill_sentinels(ott_store* s, const QueryOut& o) {
    OTT_HIP(hipMemsetAsync(o.dev, 0xFF, o.cap * sizeof(ott_hit), s->stream));
    return OTT_OK;
}

// the rows `which` of a batch's queries, packed (a cascade level or the exact redo over the queries still open)
std::vector<float> gather_queries(const float* queries, uint32_t dim, const std::vector<uint32_t>& which) {
    std::vector<float> sub((size_t)which.size() * dim);
    for (size_t i = 0; i < which.size(); i++) memcpy(&sub[i * dim], queries + (size_t)which[i] * dim, (size_t)dim * 4);
    return sub;
}

// The exact route.  *emitted: the result is with the caller already (the host "direct" sorted result, device output of
// k <= 512); else it is in `lists` (groups: 1 merged, nq per query)
int exact_route(ott_store* s, const ott_query_desc* d, const RunPlan& pl, uint64_t k_eff, const uint64_t* d_mask, uint64_t mask_bits,
                const QueryOut& o, bool timing, std::vector<std::vector<ott_hit>>& lists, ott_stats& st, bool* emitted) {
    int rc;
    const bool perq = d->mode == OTT_MODE_PER_QUERY;
    st.path_used = OTT_PATH_EXACT;
    // device output of k <= 512: the merge kernel leaves [groups][KS] sentinel-padded hits in d_hits, copied to the caller's
    // block on the stream — nothing comes back to the host
    const bool dev_direct = o.dev != nullptr && k_eff <= 512;
    const uint32_t groups = perq ? d->nq : 1u;
    const uint64_t KS = list_stride(list_E(k_eff)), gstride = o.dev ? o.cap / groups : 0;  // (the KS and the result block run_exact derives: ott_exact_plan.h)
    // when the caller's block has exactly the merge kernel's geometry ([groups][KS]: what ott_query_sharded asks for), the
    // merge writes into it directly: no sentinel fill in front, no copy behind
    const bool in_place = dev_direct && gstride == KS;
    // host output in the canonical order: the sort path may write a large result straight into the caller's buffer
    struct DirectGuard {
        ott_store* c;
        ~DirectGuard() {
            c->direct_out = nullptr;
            c->direct_cap = 0;
            c->direct_done = false;
        }
    } direct_guard{s};
    if (o.host && !o.dev && s->cur_tie_sh == 0 && !s->cur_flat) {
        s->direct_out = o.host;
        s->direct_cap = o.cap;
    }
    s->direct_done = false;
    rc = run_exact(s, d->queries, d->nq, d, perq, pl, k_eff, d_mask, mask_bits, !dev_direct, lists, st, timing, in_place ? (ott_hit*)o.dev : nullptr,
                   (uint32_t)KS);
    if (rc) return rc;
    *emitted = s->direct_done || dev_direct;
    if (s->direct_done) {
        uint64_t total = 0;
        for (size_t gq = 0; gq < s->direct_counts.size(); gq++) {
            if (o.n_per_query && perq) o.n_per_query[gq] = s->direct_counts[gq];
            total += s->direct_counts[gq];
        }
        if (o.n_out) *o.n_out = total;
    } else if (dev_direct) {
        if (!in_place) {
            if ((rc = fill_sentinels(s, o))) return rc;
            const uint64_t width = (KS < gstride ? KS : gstride) * sizeof(ott_hit);  // k_eff <= gstride: no hit is cut
            const char* src = (const char*)s->d_hits.p + exact_result_layout(groups, (uint32_t)KS).cnt_pad;  // the hits behind the counts
            if (groups == 1) OTT_HIP(hipMemcpyAsync(o.dev, src, width, hipMemcpyDeviceToDevice, s->stream));
            else OTT_HIP(hipMemcpy2DAsync(o.dev, gstride * sizeof(ott_hit), src, KS * sizeof(ott_hit), width, groups, hipMemcpyDeviceToDevice, s->stream));
        }
        if (o.n_dev) {
            hipLaunchKernelGGL(sum_counts_kernel, dim3(1), dim3(64), 0, s->stream, (const uint64_t*)s->d_hits.p, groups, (uint64_t*)o.n_dev);
            OTT_HIP(hipGetLastError());
        }
        if (o.nosync) {
            if (o.events_pending) *o.events_pending = timing;
        } else {
            OTT_HIP(hipStreamSynchronize(s->stream));  // the caller's collective runs on another stream
            if (timing) read_exact_events(s, &st);
        }
    }
    return OTT_OK;
}

// what one cascade level adds to the call's stats.  A level starts from a copy of them, so the counters it only ever raises
// come back accumulated; the level a query meets FIRST sets the rest (and the path), a later one adds to them
void add_level_stats(ott_stats& st, const ott_stats& lv, bool first) {
    st.gate_failed = lv.gate_failed;
    st.bound_violations = lv.bound_violations;
    if (first) {
        st.score_ns = lv.score_ns; st.merge_ns = lv.merge_ns; st.rescored = lv.rescored; st.passes = lv.passes;
        st.bytes_scanned = lv.bytes_scanned; st.path_used = lv.path_used;
    } else {
        st.score_ns += lv.score_ns; st.merge_ns += lv.merge_ns; st.rescored += lv.rescored; st.passes += lv.passes;
        st.bytes_scanned += lv.bytes_scanned;
    }
    if (lv.err_ratio_max > st.err_ratio_max) st.err_ratio_max = lv.err_ratio_max;
}

// The batch route.  Cascade of candidate passes, each certified against the exact re-score: int8 level (a quarter of the f32
// bytes) -> hi pass (bf16 hi plane: half the bytes, a third of the MFMAs, bound ~2^-8) -> split pass (bound ~2^-16) for the
// queries it could not certify -> the same re-scoring 4096 per query -> exact path.  Which levels a batch meets is the store's
// back-off state (ott_policy.h: CascadeState, read through the owner).
struct Cascade {
    ott_store* s;
    const ott_query_desc* d;
    const RunPlan& pl;
    uint64_t k_q;
    const uint64_t* d_mask;
    uint64_t mask_bits;
    ott_stats& st;     // the call's stats: every level adds to them (add_level_stats)
    CascadeState& cs;  // the store's
    std::vector<std::vector<ott_hit>> pq;  // per query: its list, best first
    std::vector<uint32_t> unc;             // per query: != 0 while no level has certified it
    bool hi_pass = false;
    // the hi plane is looked at (built, extended) only when a level is about to stream it: with the int8 level in front most
    // stores never need it
    bool hi_checked = false;
    bool hi_backing_off = false;  // the hi pass would run but is sitting out: the corpus is dense, the split pass keeps its 512 candidates
    bool spec_now = false;        // speculative gates for the level a query meets first

    int check_hi() {
        if (hi_checked || !hi_pass) return OTT_OK;
        hi_checked = true;
        const uint16_t* himg = nullptr;
        float hrel = 0.f;
        bool is_half = false;
        const int rc = ensure_hi_plane(s, &himg, &hrel, &is_half);
        if (rc) return rc;
        // the format the plane ACTUALLY has decides (a store whose norms spread over many binades falls back to bf16 by itself:
        // k in 229..363 would then re-score fewer candidates than the bf16 bound needs and every batch would pay a hi pass
        // that certifies nothing)
        hi_pass = himg != nullptr && mfma_hi_k_ok(k_q, is_half);
        if (hi_pass && CascadeState::consume(cs.hi_skip)) {  // backing off: recent batches mostly needed the split pass anyway
            hi_pass = false;
            hi_backing_off = true;
        }
        return OTT_OK;
    }

    // one level over the queries `which` (indices into the batch; empty = all of it)
    int run_level(const std::vector<uint32_t>& which, int level, uint32_t t_min, bool first) {
        std::vector<float> sub;
        ott_query_desc d2 = *d;
        if (!which.empty()) {
            sub = gather_queries(d->queries, s->dim, which);
            d2.queries = sub.data();
            d2.nq = (uint32_t)which.size();
        }
        std::vector<std::vector<ott_hit>> pq2;
        std::vector<uint32_t> unc2;
        ott_stats st2 = st;
        // speculative emission thresholds: only where a query meets the cascade FIRST (a level that re-runs the queries
        // another level could not certify uses conservative gates, whatever the reason they failed), and not while
        // backing off after a gate failed on this store
        const bool spec = first && spec_now;
        // (round 5: ONE query at the int8 level is a streaming sweep with the top-T in its epilogue — three launches instead of
        //  the cascade's five rounds)
        const bool single_sweep = level == 2 && i8_single_sweep(d2.nq, k_q, d2.filter_cmp, d2.metric, s->dim, t_min <= 128);
        const int rc = single_sweep ? run_i8_single(s, &d2, pl, k_q, d_mask, mask_bits, pq2, unc2, st2, t_min)
                                    : run_mfma(s, &d2, pl, k_q, d_mask, mask_bits, pq2, unc2, st2, level, t_min, spec);
        if (rc) return rc;
        add_level_stats(st, st2, first);
        if (which.empty()) {
            pq = std::move(pq2);
            unc = std::move(unc2);
        } else {
            for (size_t i = 0; i < which.size(); i++) {
                for (auto& h : pq2[i]) h.query = which[i];
                pq[which[i]] = std::move(pq2[i]);
                unc[which[i]] = unc2[i];
            }
        }
        return OTT_OK;
    }

    std::vector<uint32_t> open_queries() const {
        std::vector<uint32_t> v;
        for (uint32_t q = 0; q < d->nq; q++)
            if (unc[q]) v.push_back(q);
        return v;
    }

    // uncertified queries: recompute on the exact path (per-query lists)
    int redo_exact() {
        const std::vector<uint32_t> redo = open_queries();
        st.retries = (uint32_t)redo.size();
        if (redo.empty()) return OTT_OK;
        const std::vector<float> sub = gather_queries(d->queries, s->dim, redo);
        std::vector<std::vector<ott_hit>> fix;
        const int rc = run_exact(s, sub.data(), (uint32_t)redo.size(), d, true, pl, k_q, d_mask, mask_bits, true, fix, st);
        if (rc) return rc;
        for (size_t i = 0; i < redo.size(); i++) {
            for (auto& h : fix[i]) h.query = redo[i];
            pq[redo[i]] = std::move(fix[i]);
        }
        return OTT_OK;
    }

    int run() {
        int rc;
        const uint32_t nq = d->nq;
        hi_pass = mfma_hi_k_ok(k_q, s->opt.hi_fmt != 0) && !s->opt.mfma_f32 && !s->opt.no_hi_pass;
        // Round 5 (default; option hi_fmt = -1 / 2): an INT8 level in front of the hi pass (cosine / dot, k <= 128): a quarter of the
        // f32 bytes, one v_mfma_i32_32x32x32_i8 per 32 k, exact integer accumulation — its bound is the measured quantisation loss
        // alone (~8e-3 relative on uniform 768-d rows), so it re-scores 512 candidates per query and certifies where fewer than
        // 512 - k rows lie that close to the k-th score; what it leaves open goes to the hi pass.  Same back-off as the hi pass.
        bool i8_pass = hi_pass && i8_wanted(s->opt) && k_q <= I8_K_MAX;
        if (i8_pass) {
            const int8_t* i8 = nullptr;
            const float* i8s = nullptr;
            float i8rel = 0.f;
            if ((rc = ensure_i8_plane(s, &i8, &i8s, &i8rel))) return rc;
            i8_pass = i8 != nullptr;
        }
        if (i8_pass && CascadeState::consume(cs.i8_skip)) i8_pass = false;
        if (!i8_pass && (rc = check_hi())) return rc;
        // the split pass is then a later level: it re-scores 512 candidates per query — also while the hi pass backs off (it backs off
        // on dense or clustered corpora, exactly where k + 28 candidates certify nothing)
        const bool cascade = hi_pass || i8_pass || hi_backing_off;
        // the 4096-candidate level is there for every bf16 batch (also k > 228 or no hi plane: split pass, wide split pass, exact)
        const bool escalate = !s->opt.mfma_f32;
        // (not while backing off: a speculative gate failed a query on this store recently)
        spec_now = s->opt.mfma_spec != 0 && !CascadeState::consume(cs.spec_skip);
        const std::vector<uint32_t> all;
        std::vector<uint32_t> after_i8;  // the queries the int8 level left open (it ran and certified the rest)
        if (i8_pass) {
            const bool i8_wide_now = CascadeState::consume(cs.i8_t512);
            if ((rc = run_level(all, 2, i8_wide_now ? 512u : 0u, true))) return rc;
            after_i8 = open_queries();
            st.i8_refined = (uint32_t)after_i8.size();
            cs.after_i8(nq, after_i8.size(), st.gate_failed, i8_wide_now, k_q);
            if (!after_i8.empty() && (rc = check_hi())) return rc;  // what the int8 level left open needs the hi plane now
        }
        const std::vector<uint32_t>& rest = i8_pass ? after_i8 : all;  // what the next level runs on; it is a query's first unless the int8 level ran
        if (i8_pass && after_i8.empty()) {
            // every query certified by the int8 level: nothing left for the others
        } else if (hi_pass) {
            // candidates re-scored per query by the hi pass: 2k + 56, or 512 once this store's queries have failed at that
            // (dense neighbourhoods: clustered corpora), or what the hi_tmin option says
            const bool hi_wide_now = cs.hi_wide();
            const uint32_t hi_t = s->opt.hi_tmin ? (uint32_t)s->opt.hi_tmin : (hi_wide_now ? 512u : 0u);
            if ((rc = run_level(rest, 0, hi_t, !i8_pass))) return rc;
            const std::vector<uint32_t> refine = open_queries();
            st.refined = (uint32_t)refine.size();
            cs.after_hi(nq, refine.size(), st.gate_failed, hi_wide_now, hi_t);
            if (!refine.empty() && (rc = run_level(refine, 1, 512, false))) return rc;
        } else if (escalate && cs.take_wide_first(nq)) {
            // the 512-candidate level has been failing on this store: start at the 4096-candidate one for a while
            if ((rc = run_level(rest, 1, 4096, !i8_pass))) return rc;
        } else {
            if ((rc = run_level(rest, 1, cascade ? 512u : 0u, !i8_pass))) return rc;
        }
        if (spec_now) cs.after_spec(st.gate_failed != 0);
        if (escalate) {
            // third level: still more than a couple of exact passes' worth of open queries (near-duplicate clusters: hundreds of
            // rows within the split pass's bound of the k-th score) — the split pass once more, re-scoring 4096 per query
            const std::vector<uint32_t> wide = open_queries();
            if (wide.size() > 8 && st.rescored < (uint64_t)nq * 4096) {
                cs.arm_wide_first(wide.size(), nq);
                if ((rc = run_level(wide, 1, 4096, false))) return rc;
            }
        }
        return redo_exact();
    }
};

// reference semantics of a merged batch: one list over all (query, row) pairs (src/vec.rs:217-219).  The per-query lists are
// sorted best first, so the merged top-k is a k-way merge over their heads: k pops of a heap of nq cursors (a partial_sort
// over all nq x k hits was ~0.1 ms of a 256-query batch)
std::vector<ott_hit> merge_lists(const std::vector<std::vector<ott_hit>>& pq, const CanonLess& less, size_t k) {
    std::vector<std::pair<uint32_t, uint32_t>> heap;  // (list, position); the heap's top is the best head
    auto worse = [&](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) {
        return less(pq[b.first][b.second], pq[a.first][a.second]);
    };
    for (uint32_t q = 0; q < pq.size(); q++)
        if (!pq[q].empty()) heap.emplace_back(q, 0u);
    std::make_heap(heap.begin(), heap.end(), worse);
    std::vector<ott_hit> all;
    all.reserve(k);
    while (!heap.empty() && all.size() < k) {
        std::pop_heap(heap.begin(), heap.end(), worse);
        const std::pair<uint32_t, uint32_t> cur = heap.back();
        heap.pop_back();
        all.push_back(pq[cur.first][cur.second]);
        if (cur.second + 1 < pq[cur.first].size()) {
            heap.emplace_back(cur.first, cur.second + 1);
            std::push_heap(heap.begin(), heap.end(), worse);
        }
    }
    return all;
}

// device output of host-side lists (batch path, k > 512): [groups][cap / groups] slots, each list best first, the rest
// sentinels.  ONE copy of the whole block from pinned staging (a copy per query was ~5 us of enqueue each: 5 ms for the 1024
// queries of a C4 shard)
int emit_device_staged(ott_store* s, const std::vector<std::vector<ott_hit>>& lists, uint32_t groups, const QueryOut& o) {
    int rc;
    const uint64_t gstride = o.cap / groups;
    const size_t blk = (size_t)groups * gstride * sizeof(ott_hit);
    if ((rc = s->h_stage.ensure(blk + sizeof(uint64_t)))) return rc;
    char* hs = (char*)s->h_stage.p;
    memset(hs, 0xFF, blk);  // sentinels: this block covers every slot of out_dev
    uint64_t tot = 0;
    for (uint32_t q = 0; q < groups; q++) {
        const size_t c = lists[q].size() < gstride ? lists[q].size() : (size_t)gstride;
        if (c) memcpy(hs + (size_t)q * gstride * sizeof(ott_hit), lists[q].data(), c * sizeof(ott_hit));
        tot += c;
    }
    memcpy(hs + blk, &tot, sizeof(uint64_t));
    OTT_HIP(hipMemcpyAsync(o.dev, hs, blk, hipMemcpyHostToDevice, s->stream));
    if (o.n_dev) OTT_HIP(hipMemcpyAsync(o.n_dev, hs + blk, sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
    if (!o.nosync) OTT_HIP(hipStreamSynchronize(s->stream));  // (nosync: h_stage stays untouched until the caller's own wait)
    return OTT_OK;
}

void emit_host(const std::vector<std::vector<ott_hit>>& lists, bool perq, const QueryOut& o) {
    uint64_t total = 0;
    for (size_t gq = 0; gq < lists.size(); gq++) {
        const size_t c = lists[gq].size();
        if (c) memcpy(o.host + total, lists[gq].data(), c * sizeof(ott_hit));
        if (o.n_per_query && perq) o.n_per_query[gq] = c;
        total += c;
    }
    if (o.n_out) *o.n_out = total;
}

}  // namespace

// One plain query on a context: plan, checks, path choice (ott_policy.h: choose_path), one of the two routes above, emit.
int ott::query_core(ott_store* s, const ott_query_desc* d, ott_hit* out_host, void* out_dev, uint64_t cap, uint64_t* n_out,
                    uint64_t* n_per_query, void* n_out_dev, ott_stats* stats_out, bool nosync, bool* events_pending, const CoreOpts& co) {
    int rc;
    if (events_pending) *events_pending = false;
    struct CurOrder {  // the candidate order of THIS call, for the launch wrappers (the context is ours until the caller releases it)
        ott_store* s;
        CurOrder(ott_store* st, const CoreOpts& c) : s(st) { s->cur_tie_sh = c.tie_sh; s->cur_tie_off = c.tie_sh ? (c.tie_off & 7u) : 0u; s->cur_flat = c.flat; }
        ~CurOrder() { s->cur_tie_sh = 0; s->cur_tie_off = 0; s->cur_flat = false; }
    } cur_order(s, co);
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    memset(&st, 0, sizeof(st));

    RunPlan pl;
    build_plan(s, d->chunk_mask, pl);
    st.prune_ns = now_ns() - t0;
    st.total_chunks = pl.total_chunks;
    st.evaluated_chunks = pl.evaluated;
    st.pruned_chunks = pl.total_chunks - pl.evaluated;
    st.vectors_compared = pl.rows_scored * d->nq;  // sum chunk.len * nq, src/meta_compute.rs:166

    const bool perq = d->mode == OTT_MODE_PER_QUERY;
    const uint32_t nq = d->nq;
    const uint64_t pool = perq ? pl.rows_scored : pl.rows_scored * nq;
    const uint64_t k_eff = d->k < pool ? d->k : pool;  // take_count, src/vec.rs:213; a list never outgrows the pool
    const uint64_t need = perq ? k_eff * nq : k_eff;
    if (cap < need) return fail(OTT_ERR_INVALID, "ott_query: output capacity is smaller than min(k, rows*nq)");
    if (out_dev && perq && cap % nq != 0) return fail(OTT_ERR_INVALID, "ott_query_device: PER_QUERY capacity must be a multiple of nq");

    const QueryOut o{out_host, out_dev, cap, n_out, n_per_query, n_out_dev, nosync, events_pending};
    if (out_dev && n_out_dev) OTT_HIP(hipMemsetAsync(n_out_dev, 0, sizeof(uint64_t), s->stream));
    if (n_out) *n_out = 0;
    if (n_per_query)
        for (uint32_t i = 0; i < nq; i++) n_per_query[i] = 0;
    if (k_eff == 0 || pl.rows_scored == 0) {  // k == 0 (src/vec_compute.rs:174) or nothing to score
        if (out_dev && (rc = fill_sentinels(s, o))) return rc;
        if (out_dev && !nosync) OTT_HIP(hipStreamSynchronize(s->stream));
        return finish(st, t0, stats_out);
    }

    // row mask -> device: the ONE place every mask joins (the caller's or the evaluated one, an id list's, the live mask)
    const uint64_t* d_mask = nullptr;
    uint64_t mask_bits = 0;
    if ((rc = compose_row_mask(s, d, &d_mask, &mask_bits))) return rc;

    ott_store* own = s->owner ? s->owner : s;
    const Options& op = s->opt;
    const PathIn in{pl.rows_scored, pl.runs.size(), s->dim, s->dimq, nq, d->k, d->metric, d->filter_cmp, d->path, co.flat,
                    op.mfma_f32, op.no_hi_pass, op.no_batch_image, op.hi_fmt, op.exact_small};
    const PathChoice path = choose_path(
        in,
        [&] {
            const PlaneSnapshot ps = plane_snapshot(s);
            return PathPlanes{ps.have_hi, ps.hi_f16, ps.i8_off, own->cascade.i8_widened()};
        },
        [&] { return first_plane_ready(s); });
    if (path == PATH_CHOICE_REFUSED) return fail(OTT_ERR_UNSUPPORTED, kMfmaRefusal);

    std::vector<std::vector<ott_hit>> lists;  // groups: 1 (merged) or nq
    if (path == PATH_CHOICE_EXACT) {
        // kernel timing (three event records, each a barrier packet between the launches) only when the caller asked for stats
        bool emitted = false;
        if ((rc = exact_route(s, d, pl, k_eff, d_mask, mask_bits, o, stats_out != nullptr, lists, st, &emitted))) return rc;
        if (emitted) return finish(st, t0, stats_out);
    } else {
        // per-query k for the batch path: the merged top-k is contained in the union of per-query top-k
        const uint64_t k_q = d->k < pl.rows_scored ? d->k : pl.rows_scored;
        Cascade c{s, d, pl, k_q, d_mask, mask_bits, st, own->cascade};
        if ((rc = c.run())) return rc;
        if (perq) lists = std::move(c.pq);
        else {
            const size_t most = (size_t)k_eff < (size_t)nq * k_q ? (size_t)k_eff : (size_t)nq * k_q;
            lists.assign(1, merge_lists(c.pq, CanonLess{d->take == OTT_TAKE_MAX, co.tie_sh, tie_base(s)}, most));
        }
    }
    if (out_dev) {
        if ((rc = emit_device_staged(s, lists, perq ? nq : 1u, o))) return rc;
    } else emit_host(lists, perq, o);
    return finish(st, t0, stats_out);
}

namespace {

int query_common(ott_store* s, const ott_query_desc* d, ott_hit* out_host, void* out_dev, uint64_t cap, uint64_t* n_out,
                 uint64_t* n_per_query, void* n_out_dev, ott_stats* stats_out) {
    int rc = validate_query(s, d);
    if (rc) return rc;
    ott::host::SharedLock rd;  // the corpus cannot change while this query runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    CtxLease ctx(s);
    return query_on(ctx.c, d, out_host, out_dev, cap, n_out, n_per_query, n_out_dev, stats_out);
}

}  // namespace

extern "C" {

int ott_query(ott_store* s, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
              ott_stats* stats) {
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query: out is NULL");
    if (s && s->multi) return multi_query(s, d, out, cap, n_out, n_per_query, stats);
    return query_common(s, d, out, nullptr, cap, n_out, n_per_query, nullptr, stats);
}

int ott_query_device(ott_store* s, const ott_query_desc* d, void* out_dev, uint64_t cap, void* n_out_dev, ott_stats* stats) {
    if (!out_dev) return fail(OTT_ERR_INVALID, "ott_query_device: out_dev is NULL");
    if (s && s->multi) return fail(OTT_ERR_UNSUPPORTED, "ott_query_device: a multi-GPU store returns its result to the host (ott_query)");
    return query_common(s, d, nullptr, out_dev, cap, nullptr, nullptr, n_out_dev, stats);
}

static int merge_hits_common(ott_store* s, const void* lists_dev, uint64_t n_lists, uint64_t n_groups, uint64_t list_len, uint32_t take,
                             uint64_t k, ott_hit* out_host, uint64_t* n_out, uint64_t* n_per_group) {
    if (!s || !lists_dev || !out_host) return fail(OTT_ERR_INVALID, "ott_merge_hits_device: NULL argument");
    if (s->multi) return fail(OTT_ERR_UNSUPPORTED, "ott_merge_hits_device: not on a multi-GPU store (its own merge runs inside ott_query)");
    if (take > OTT_TAKE_MAX) return fail(OTT_ERR_INVALID, "ott_merge_hits_device: unknown take type");
    if (n_lists * list_len > 0xFFFFFFF0ull || n_groups > 0xFFFFull * 16) return fail(OTT_ERR_INVALID, "ott_merge_hits_device: too many candidates");
    ott::host::SharedLock rd(s->rw);
    CtxLease ctx(s);
    s = ctx.c;
    OTT_HIP(use_device(s));
    const uint64_t pool = n_lists * list_len;
    const uint64_t k_eff = k < pool ? k : pool;
    if (n_out) *n_out = 0;
    if (n_per_group)
        for (uint64_t i = 0; i < n_groups; i++) n_per_group[i] = 0;
    if (k_eff == 0 || n_groups == 0) return OTT_OK;
    if (k_eff > 512) {
        // beyond the register lists: the candidates come to the host and are merged there in the same order the kernel uses
        // (better score, then lower list, then lower position: shard order = global row order)
        std::vector<ott_hit> all((size_t)n_lists * n_groups * list_len);
        OTT_HIP(hipMemcpyAsync(all.data(), lists_dev, all.size() * sizeof(ott_hit), hipMemcpyDeviceToHost, s->stream));
        OTT_HIP(hipStreamSynchronize(s->stream));
        const bool tmax = take == OTT_TAKE_MAX;
        uint64_t total = 0;
        std::vector<std::pair<uint64_t, uint64_t>> keys;  // (ord << 32 | ~id ... as two words: ord, id)
        for (uint64_t gq = 0; gq < n_groups; gq++) {
            keys.clear();
            for (uint64_t li = 0; li < n_lists; li++)
                for (uint64_t pos = 0; pos < list_len; pos++) {
                    const ott_hit& h = all[(li * n_groups + gq) * list_len + pos];
                    if (h.index == ~0ull || h.score != h.score) continue;
                    keys.emplace_back((uint64_t)ord_of(h.score, tmax), li * list_len + pos);
                }
            const size_t keep = keys.size() < k_eff ? keys.size() : (size_t)k_eff;
            std::partial_sort(keys.begin(), keys.begin() + keep, keys.end(),
                              [](const std::pair<uint64_t, uint64_t>& a, const std::pair<uint64_t, uint64_t>& b) {
                                  return a.first != b.first ? a.first > b.first : a.second < b.second;
                              });
            for (size_t i = 0; i < keep; i++) {
                const uint64_t li = keys[i].second / list_len, pos = keys[i].second % list_len;
                out_host[total + i] = all[(li * n_groups + gq) * list_len + pos];
            }
            if (n_per_group) n_per_group[gq] = keep;
            total += keep;
        }
        if (n_out) *n_out = total;
        return OTT_OK;
    }
    const int E = list_E(k_eff);
    const uint32_t KS = 64 * E;
    int rc;
    const size_t hits_bytes = (size_t)n_groups * KS * sizeof(ott_hit), cnt_bytes = (size_t)n_groups * 8;
    // the kernel writes counts + hits straight into pinned host memory (no D2H copies behind the launch)
    if ((rc = s->h_hits.ensure(hits_bytes + cnt_bytes))) return rc;
    char* hh = (char*)s->h_hits.p;
    void* mapped = nullptr;
    OTT_HIP(hipHostGetDevicePointer(&mapped, hh, 0));
    rc = launch_merge_hits(s, (const ott_hit*)lists_dev, (uint32_t)n_lists, (uint32_t)n_groups, (uint32_t)list_len, (uint32_t)k_eff, E,
                           take == OTT_TAKE_MAX, (ott_hit*)((char*)mapped + cnt_bytes), (uint64_t*)mapped);
    if (rc) return rc;
    OTT_HIP(hipStreamSynchronize(s->stream));
    const uint64_t* cnt = (const uint64_t*)hh;
    const ott_hit* hits = (const ott_hit*)(hh + cnt_bytes);
    uint64_t total = 0;
    for (uint64_t gq = 0; gq < n_groups; gq++) {
        if (cnt[gq]) memcpy(out_host + total, hits + gq * KS, cnt[gq] * sizeof(ott_hit));
        if (n_per_group) n_per_group[gq] = cnt[gq];
        total += cnt[gq];
    }
    if (n_out) *n_out = total;
    return OTT_OK;
}

int ott_merge_hits_device(ott_store* s, const void* lists_dev, uint64_t n_lists, uint64_t list_len, uint32_t take, uint64_t k,
                          ott_hit* out_host, uint64_t* n_out) {
    return merge_hits_common(s, lists_dev, n_lists, 1, list_len, take, k, out_host, n_out, nullptr);
}

int ott_merge_hits_device_grouped(ott_store* s, const void* lists_dev, uint64_t n_lists, uint64_t n_groups, uint64_t list_len,
                                  uint32_t take, uint64_t k, ott_hit* out_host, uint64_t* n_out, uint64_t* n_per_group) {
    return merge_hits_common(s, lists_dev, n_lists, n_groups, list_len, take, k, out_host, n_out, n_per_group);
}

}  // extern "C"
