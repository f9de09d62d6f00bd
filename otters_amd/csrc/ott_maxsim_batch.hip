// ott_maxsim_batch.hip — MaxSim re-ranking in batches: ott_query_maxsim_groups_batch answers B queries, each with
// its own tokens and its own list of groups, and returns for every one exactly the hits of ott_query_maxsim_groups (query = b).
// What a batch saves is everything a call pays once: one upload, one gather launch, one top-k, one host wait.
//
//   maxsim_gather_batch_kernel  maxsim_gather_kernel's geometry and arithmetic (the per-row step is the same text,
//                               ott_maxsim_gather_step.inc; the join and the sum are ott_maxsim_gather_dev.h's).  New: the slots of
//                               all queries lie back to back in query order and a persistent workgroup walks the contiguous range
//                               mg_batch_split gave it (balanced by listed rows).  Where the slot's query changes it reloads that
//                               query's transposed token block into LDS between two barriers; the sum runs over that query's own
//                               tokens (the block is zero padded to the batch's width NT); the key goes to keys[b * S + pos].
//                               Padded slots of a query with fewer than S distinct groups are never written: they stay zero, the
//                               table's "dropped".  Vector loads and stores and plain C++; no global atomics.
//   the top-k                   ONE GroupTopK over B tables of S keys at stride S: its select / merge (k <= 512) and compact / sort
//                               (above) serve nq tables already, its q is the hit's query.
//   the loop route              whatever the batched gather does not serve (a query with more tokens than one pass holds, a padded
//                               dim above 2048, option group_gather = 0, no index, batches past the launch limits): the queries one
//                               by one through maxsim_groups_locked — what ott_query_maxsim_groups runs — under the one shared lock.
//
// The host-side decisions — stride, token width, route, the split of the slots — are ott_maxsim_gather_plan.h's (MgBatch).
// Resources: profiles/maxsim_rerank_batch/resource_usage.txt.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "ott_internal.h"
#include "ott_exact_dev.h"
#include "ott_maxsim_gather_dev.h"

namespace ott {

struct MgBatchParams {
    const float* rows;
    const float* inv;
    const float* tokens;  // [B][dimq][NT + MG_PAD]: a block per query, transposed, zero padded
    const float* qinv;    // [B][NT]
    const uint64_t* row_mask;  // the composed mask (caller & live), or nullptr
    uint64_t row_mask_bits;
    const uint64_t* chunk_mask;  // one bit per chunk of chunk_rows rows, or nullptr
    const uint32_t* gix;         // the rows ordered by group; every one < the store's length
    const uint32_t* slot_gid;    // [n_slots] per query ascending and duplicate-free, the queries back to back
    const uint32_t* slot_start;  // [n_slots] the group's first place in gix ...
    const uint32_t* slot_count;  // ... and its rows: start + count <= the store's length (the index's own extents)
    const uint32_t* slot_query;  // [n_slots] the slot's query, < B, never decreasing
    const uint32_t* slot_pos;    // [n_slots] the slot's place among its query's slots, < stride
    const uint32_t* q_tokens;    // [B] tokens of the query, 1 .. NT
    const uint32_t* first;       // [gridDim.x + 1] workgroup w walks the slots [first[w], first[w + 1]); first[gridDim.x] == n_slots
    unsigned long long* keys;    // [B][stride] keys, 0 = dropped
    uint32_t n_slots, stride;
    uint32_t ld, dim, dimq;
    uint32_t metric, take_max, reduce, cmp;
    uint32_t chunk_rows;
    float thr;
};

// Dynamic LDS: mg_lds_bytes(dimq, NT), as maxsim_gather_kernel.
template <int MK, int NT>
__global__ __launch_bounds__(64 * MG_WAVES) void maxsim_gather_batch_kernel(MgBatchParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTP = NT + (int)MG_PAD;
    float* sT = smem;                                            // [dimq][NTP]
    float* sQi = sT + (size_t)p.dimq * NTP;                      // [NT]
    uint32_t* sB = reinterpret_cast<uint32_t*>(sQi + NT);        // [MG_WAVES][NT]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 3, c = lane & 7;
    const bool take_max = p.take_max != 0;
    const uint32_t full = p.dim >> 3, nt = p.dim & 7u;
    const uint32_t lo = p.first[blockIdx.x];
    uint32_t hi = p.first[blockIdx.x + 1];
    if (hi > p.n_slots) hi = p.n_slots;
    uint32_t cur = 0xFFFFFFFFu, n_tokens = 0;  // the query whose tokens are in LDS
    for (uint32_t slot = lo; slot < hi; slot++) {
        const uint32_t b = p.slot_query[slot];  // (the same for the whole workgroup)
        if (b != cur) {
            __syncthreads();  // the block of the query before is no longer read
            const float4* src = reinterpret_cast<const float4*>(p.tokens + (size_t)b * p.dimq * NTP);
            float4* dst = reinterpret_cast<float4*>(sT);
            const uint32_t n4 = p.dimq * (uint32_t)NTP / 4;
            for (uint32_t i = tid; i < n4; i += 64 * MG_WAVES) dst[i] = src[i];
            if (tid < NT) sQi[tid] = p.qinv[(size_t)b * NT + tid];
            __syncthreads();
            cur = b;
            n_tokens = p.q_tokens[b];
        }
        const uint32_t start = p.slot_start[slot], count = p.slot_count[slot];
        uint32_t best[NT];  // per token: the best ordinal among this lane group's rows of the group (0 = none yet)
#pragma unroll
        for (int q = 0; q < NT; q++) best[q] = 0u;
        for (uint32_t base = 0; base < count; base += MG_STEP_ROWS) {
#include "ott_maxsim_gather_step.inc"
        }

        mg_join_wave<NT>(best, sB, wave, lane);
        __syncthreads();
        if (tid == 0) {
            // the sum over this query's own tokens (the padded ones scored zeros that nobody reads), and the key
            const unsigned long long key = mg_sum_key<NT>(sB, n_tokens, take_max, p.cmp, p.thr, p.slot_gid[slot]);
            if (key != 0) p.keys[(size_t)b * p.stride + p.slot_pos[slot]] = key;
        }
        __syncthreads();  // sB is the next group's
    }
}

namespace {

template <int MK, int NT>
int launch_mgb(ott_store* s, const MgBatchParams& p, uint32_t grid) {
    const size_t smem = (size_t)mg_lds_bytes(p.dimq, NT);
    auto kern = maxsim_gather_batch_kernel<MK, NT>;
    if (smem > 48 * 1024) {  // more dynamic LDS than the default limit: the opt-in, once per device
        static std::atomic<uint64_t> attr_set{0};
        if (attr_needed(attr_set, s->device)) {
            OTT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MG_LDS_MAX));
            attr_done(attr_set, s->device);
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * MG_WAVES), smem, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

template <int MK>
int launch_mgb_mk(ott_store* s, const MgBatchParams& p, uint32_t nt, uint32_t grid) {
    switch (nt) {
        case 8: return launch_mgb<MK, 8>(s, p, grid);
        case 16: return launch_mgb<MK, 16>(s, p, grid);
        case 32: return launch_mgb<MK, 32>(s, p, grid);
        default: return fail(OTT_ERR_INVALID, "maxsim gather batch: no kernel for this number of tokens per pass");
    }
}

int launch_mgb_any(ott_store* s, const MgBatchParams& p, uint32_t nt, uint32_t grid) {
    switch (metric_kind(p.metric)) {
        case MK_L2: return launch_mgb_mk<MK_L2>(s, p, nt, grid);
        case MK_L1: return launch_mgb_mk<MK_L1>(s, p, nt, grid);
        default: return launch_mgb_mk<MK_DOT>(s, p, nt, grid);
    }
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// The batched gather on a context whose `mu` the caller holds (and the owner's `rw`, shared).  mb: the batch's slots with their
// extents in the index; every query fits one pass of mb.NT tokens; k_top = min(k, mb.S) >= 1.
int run_maxsim_gather_batch(ott_store* s, const ott_query_desc* d, const MgBatch& mb, uint64_t k_top, ott_hit* out, uint64_t* n_out, uint64_t* n_per_query,
                            ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    memset(&st, 0, sizeof(st));
    const uint32_t B = (uint32_t)mb.tokens.size(), T = (uint32_t)mb.gid.size(), nt = mb.NT, ntp = nt + MG_PAD;
    RunPlan pl;
    make_run_plan(s, d->chunk_mask, pl);
    st.path_used = OTT_PATH_EXACT;
    st.total_chunks = pl.total_chunks;
    st.evaluated_chunks = pl.evaluated;
    st.pruned_chunks = pl.total_chunks - pl.evaluated;
    st.passes = 1;
    st.vectors_compared = mb.compared;  // every query's listed rows x its tokens, before the masks
    st.bytes_scanned = mb.rows * ((uint64_t)s->dim * 4 + 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));  // (+ 4: the index's word)
    if (pl.rows_scored != 0 && mb.rows != 0) {
        MgBatchParams p{};
        if ((rc = compose_row_mask(s, d, &p.row_mask, &p.row_mask_bits))) return rc;
        // a workgroup per listed group, at most what the CUs hold at once (ott_query_maxsim_groups' rule); a workgroup walks a range
        const uint64_t lds = mg_lds_bytes(s->dimq, nt);
        uint32_t per_cu = (uint32_t)(160ull * 1024 / lds);
        per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
        const uint32_t grid = std::min<uint32_t>(T, (uint32_t)s->n_cu * per_cu);
        // one block up, one copy: [token blocks | qinv | slot gid, start, count, query, pos | tokens per query | first | chunk mask words]
        const size_t tok_bytes = (size_t)B * s->dimq * ntp * 4, qi_bytes = (size_t)B * nt * 4, slot_bytes = (size_t)T * 4;
        const size_t cm_words = d->chunk_mask ? (size_t)((pl.total_chunks + 63) / 64) : 0;
        const size_t off_qi = tok_bytes, off_slots = align16(off_qi + qi_bytes), off_qt = off_slots + 5 * slot_bytes, off_first = off_qt + (size_t)B * 4;
        const size_t off_cm = align16(off_first + ((size_t)grid + 1) * 4), total = off_cm + cm_words * 8;
        if ((rc = s->h_stage.ensure(total))) return rc;
        char* hs = (char*)s->h_stage.p;
        memset(hs, 0, off_slots);
        const float* q = d->queries;
        for (uint32_t b = 0; b < B; b++) {
            float* blk = (float*)hs + (size_t)b * s->dimq * ntp;
            float* qi = (float*)(hs + off_qi) + (size_t)b * nt;
            for (uint32_t t = 0; t < mb.tokens[b]; t++, q += s->dim) {
                for (uint32_t i = 0; i < s->dim; i++) blk[(size_t)i * ntp + t] = q[i];
                qi[t] = host_inv_norm_exact(q, s->dim);
            }
        }
        const std::vector<uint32_t>* slot_arrays[5] = {&mb.gid, &mb.start, &mb.count, &mb.query, &mb.pos};
        for (int a = 0; a < 5; a++) memcpy(hs + off_slots + (size_t)a * slot_bytes, slot_arrays[a]->data(), slot_bytes);
        memcpy(hs + off_qt, mb.tokens.data(), (size_t)B * 4);
        mg_batch_split(mb.count.data(), T, grid, (uint32_t*)(hs + off_first));
        if (cm_words) memcpy(hs + off_cm, d->chunk_mask, cm_words * 8);
        if ((rc = s->d_queries.ensure(total))) return rc;
        OTT_HIP(hipMemcpyAsync(s->d_queries.p, hs, total, hipMemcpyHostToDevice, s->stream));
        const char* dq = (const char*)s->d_queries.p;
        p.rows = s->d_rows;
        p.inv = s->d_inv;
        p.tokens = (const float*)dq;
        p.qinv = (const float*)(dq + off_qi);
        p.slot_gid = (const uint32_t*)(dq + off_slots);
        p.slot_start = p.slot_gid + T;
        p.slot_count = p.slot_start + T;
        p.slot_query = p.slot_count + T;
        p.slot_pos = p.slot_query + T;
        p.q_tokens = (const uint32_t*)(dq + off_qt);
        p.first = (const uint32_t*)(dq + off_first);
        p.chunk_mask = cm_words ? (const uint64_t*)(dq + off_cm) : nullptr;
        p.chunk_rows = s->chunk_size < 0xFFFFFFFFull ? (uint32_t)s->chunk_size : 0xFFFFFFFFu;  // (rows stay below 2^32 - 16)
        p.gix = s->d_gix;
        p.n_slots = T;
        p.stride = mb.S;
        p.ld = s->ld;
        p.dim = s->dim;
        p.dimq = s->dimq;
        p.metric = d->metric;
        p.take_max = d->take == OTT_TAKE_MAX;
        p.reduce = s->reduce;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;

        // the keys are left zeroed by the select / compact kernel
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)mg_key_bytes((uint64_t)B * mb.S)))) return rc;
        p.keys = (unsigned long long*)s->d_gtable.p;

        GroupTopK tk;
        tk.n_groups = mb.S;
        tk.q_stride = mb.S;
        tk.nq = B;
        tk.k = k_top;
        tk.take_max = p.take_max != 0;
        tk.index_is_group = true;
        tk.id_span = s->n_groups;
        if ((rc = tk.prepare(s, nullptr))) return rc;
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        if ((rc = launch_mgb_any(s, p, nt, grid))) return rc;
        if ((rc = tk.pass(s, p.keys, 0, B))) return rc;
        if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
        if ((rc = tk.finish(s, timing, out, n_out, n_per_query))) return rc;
        if (timing) read_exact_events(s, &st);
    }
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_maxsim_groups_batch(ott_store* s, const ott_query_desc* d, const void* tokens_void, const uint64_t* listed_per_query, uint32_t n_queries,
                                  const void* groups_void, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats) {
    const uint32_t* tokens_per_query = (const uint32_t*)tokens_void;
    const uint32_t* groups = (const uint32_t*)groups_void;
    const char* fn = "ott_query_maxsim_groups_batch";
    const std::string name(fn);
    // what the arguments alone decide comes first: these refusals need no store
    if (d && d->mode == OTT_MODE_PER_QUERY)
        return fail(OTT_ERR_UNSUPPORTED, name + ": tokens_per_query says which query vectors belong to which query; PER_QUERY is not served");
    if (d && d->path == OTT_PATH_MFMA) return fail(OTT_ERR_UNSUPPORTED, name + ": the MFMA path does not serve late-interaction queries; use path AUTO or EXACT");
    if (n_queries == 0) return fail(OTT_ERR_INVALID, name + ": n_queries is 0");
    if (n_queries > OTT_MAXSIM_BATCH_MAX)
        return fail(OTT_ERR_INVALID, name + ": n_queries " + std::to_string(n_queries) + " is above OTT_MAXSIM_BATCH_MAX (" + std::to_string(OTT_MAXSIM_BATCH_MAX) + ")");
    if (!tokens_per_query) return fail(OTT_ERR_INVALID, name + ": tokens_per_query is NULL");
    if (!listed_per_query) return fail(OTT_ERR_INVALID, name + ": listed_per_query is NULL");
    uint64_t n_tokens = 0, n_listed = 0;
    for (uint32_t b = 0; b < n_queries; b++) {
        if (tokens_per_query[b] == 0) return fail(OTT_ERR_INVALID, name + ": query " + std::to_string(b) + " has no tokens");
        n_tokens += tokens_per_query[b];
        n_listed += listed_per_query[b];
    }
    if (n_listed && !groups) return fail(OTT_ERR_INVALID, name + ": groups is NULL");
    if (d && n_tokens != d->nq)
        return fail(OTT_ERR_INVALID, name + ": tokens_per_query sums to " + std::to_string(n_tokens) + ", the descriptor holds " + std::to_string(d->nq) + " query vectors");
    if (!s) return fail(OTT_ERR_INVALID, name + ": store is NULL");
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (s->multi)
        return fail(OTT_ERR_UNSUPPORTED, name + ": a multi-GPU store is not served (a group may span shards: the maxima would have to be joined before the sum)");
    // before any device work: the ids are set and cover the store, the lists name groups that exist
    if ((rc = check_group_ids(s, fn, false))) return rc;
    const auto check_lists = [&](uint32_t n_groups) {
        uint64_t at = 0;
        for (uint32_t b = 0; b < n_queries; at += listed_per_query[b], b++)
            for (uint64_t i = 0; i < listed_per_query[b]; i++)
                if (groups[at + i] >= n_groups)
                    return fail(OTT_ERR_INVALID, name + ": query " + std::to_string(b) + ": group " + std::to_string(groups[at + i]) + " is out of range (the store holds " +
                                                     std::to_string(n_groups) + " groups)");
        return (int)OTT_OK;
    };
    if ((rc = check_lists(ott_store_group_count(s)))) return rc;
    ott::host::SharedLock rd;  // the corpus, the group ids and the index cannot change while the batch runs
    if ((rc = maxsim_groups_lock(s, fn, rd))) return rc;
    // what the checks above read without the lock is read again, and the k_eff only here: a set_groups may have come in between
    if ((rc = check_group_ids(s, fn, true))) return rc;
    if ((rc = check_lists(s->n_groups))) return rc;
    const bool wants_index = mg_wants_index(false, false, s->dimq, s->opt.group_gather);
    const bool have_index = s->d_gix != nullptr && s->gix_start.size() == (size_t)s->n_groups + 1;
    MgBatch mb;
    mg_batch_build(groups, tokens_per_query, listed_per_query, n_queries, s->n_groups, have_index ? s->gix_start.data() : nullptr, s->dimq, mb);
    uint64_t k_sum = 0;
    for (const uint32_t n : mb.distinct) k_sum += d->k < n ? d->k : n;
    if (cap < k_sum) return fail(OTT_ERR_INVALID, name + ": output capacity is smaller than the sum over the queries of min(k, distinct listed groups)");
    if (!out && k_sum) return fail(OTT_ERR_INVALID, name + ": out is NULL");
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_per_query) memset(n_per_query, 0, (size_t)n_queries * sizeof(uint64_t));
    if (k_sum == 0) return OTT_OK;  // empty lists, or k == 0: a valid batch with no hits

    if (mg_batch_takes_gather(wants_index, have_index, s->opt.group_gather, s->dimq, mb)) {
        CtxLease ctx(s);
        return run_maxsim_gather_batch(ctx.c, d, mb, d->k < mb.S ? d->k : mb.S, out, n_out, n_per_query, stats);
    }
    // the loop route: the queries one by one, as ott_query_maxsim_groups answers them, under this lock
    ott_stats sum;
    memset(&sum, 0, sizeof(sum));
    const uint64_t t0 = now_ns();
    uint64_t total = 0, tok_at = 0, list_at = 0;
    for (uint32_t b = 0; b < n_queries; b++) {
        ott_query_desc db = *d;
        db.queries = d->queries + (size_t)tok_at * s->dim;
        db.nq = tokens_per_query[b];
        uint64_t nb = 0;
        ott_stats sb;
        memset(&sb, 0, sizeof(sb));
        if ((rc = maxsim_groups_locked(s, &db, groups + list_at, listed_per_query[b], out ? out + total : nullptr, cap - total, &nb, stats ? &sb : nullptr, fn))) return rc;
        for (uint64_t i = 0; i < nb; i++) out[total + i].query = b;
        if (n_per_query) n_per_query[b] = nb;
        total += nb;
        tok_at += tokens_per_query[b];
        list_at += listed_per_query[b];
        if (sb.path_used != 0 || sb.passes != 0) {  // (a query without hits to give ran nothing)
            sum.total_chunks = sb.total_chunks;
            sum.evaluated_chunks = sb.evaluated_chunks;
            sum.pruned_chunks = sb.pruned_chunks;
        }
        sum.passes += sb.passes;
        sum.vectors_compared += sb.vectors_compared;
        sum.bytes_scanned += sb.bytes_scanned;
        sum.score_ns += sb.score_ns;
        sum.merge_ns += sb.merge_ns;
    }
    sum.path_used = OTT_PATH_EXACT;
    sum.total_ns = now_ns() - t0;
    if (n_out) *n_out = total;
    if (stats) *stats = sum;
    return OTT_OK;
}

}  // extern "C"
