// ott_maxsim_gather.hip — MaxSim re-ranking: ott_query_maxsim_groups scores only a LISTED set of groups.  It returns
// exactly ott_query_maxsim's hits with one more row mask — "the row's group is listed" — so every rule of 3.1f holds; what is new is
// that the work follows the list, not the store, as ott_gather.hip made it for row ids.
//
//   group-to-rows index   the rows ordered by group (d_gix, 4 B per row) and the groups' extents (gix_start, on the host), built on
//                         the device from d_gid by the first listed query that may take the gather: gix_count_kernel (a histogram
//                         by vector atomicAdd), a prefix sum on the host, gix_scatter_kernel (a returning atomicAdd per row hands
//                         out the places inside a group, so their order is not defined: max in the total order does not care).
//                         Built under the store's exclusive lock by lock_shared_clean's clean step (the dirty predicate becomes
//                         "rows are staged, or the index is missing"); dropped with the group ids (group_drop) and by nothing else.
//   maxsim_gather_kernel  gather route.  A workgroup of four waves takes one listed group at a time and walks its rows through the
//                         index, 32 rows per step: an 8-lane group owns a row, lane c carries chain c of the reference's f32x8 for
//                         every token of the pass (exact_term, the cross-lane reduce8 in either order, the sequential remainder and
//                         the cosine scaling of ott_exact_dev.h in exact_gather8_kernel's arrangement: the same additions in the same
//                         order, so the same bits).  The pass's tokens sit in LDS, transposed ([dim][tokens + 4]: one 16-B read
//                         gives a lane four tokens of its dim).  Per row: the composed row mask's bit, the chunk's bit of
//                         chunk_mask, the NaN drop, ord_of; per token a running maximum in registers across the group's rows, joined
//                         over the row groups by shuffles and over the waves in LDS.  No global atomics, no [nq][n_groups] table.
//                         One pass of tokens: lane 0 sums the maxima in token order from best[0] and writes the group's key
//                         ord_of(sum) << 32 | ~gid into the [n_listed] key table.  More passes: the maxima go to a compact
//                         [nq][n_listed] table of ordinals and maxsim_reduce_kernel (ott_maxsim.hip, with the slots' group ids) makes
//                         the keys.  The top-k is GroupTopK over the n_listed slots; both tables keep "zero when found".
//   groups_mask_kernel    mask route (whatever the gather does not serve, and option group_gather = 0): a bitmap over the groups
//                         in, one lane per 64 rows reading d_gid, the row-mask words out; they join compose_row_mask where an id
//                         list's mask joins (cur_idmask) and ott_maxsim.hip's run_maxsim runs unchanged.  Needs no index.
//
// The host-side decisions — tokens per pass, the slot arrays, the tables' sizes, the route — are ott_maxsim_gather_plan.h's.
// The kernel's per-row step is ott_maxsim_gather_step.inc, its join and its sum ott_maxsim_gather_dev.h: ott_maxsim_batch.hip's kernel
// (many queries and their lists in one launch) runs the same; what this call does around and under its lock is
// maxsim_groups_lock / maxsim_groups_locked, which the batch's loop route calls per query.
// Resources (profiles/maxsim_rerank/resource_usage.txt): no scratch at any of the three widths.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "ott_internal.h"
#include "ott_exact_dev.h"
#include "ott_maxsim_gather_dev.h"

namespace ott {

struct MgParams {
    const float* rows;
    const float* inv;
    const float* tokens;  // [passes][dimq][NT + MG_PAD]: transposed, zero padded
    const float* qinv;    // [passes * NT]
    const uint64_t* row_mask;  // the composed mask (caller & live), or nullptr
    uint64_t row_mask_bits;
    const uint64_t* chunk_mask;  // one bit per chunk of chunk_rows rows, or nullptr
    const uint32_t* gix;         // the rows ordered by group; every one < the store's length (they are the indices of d_gid's entries)
    const uint32_t* slot_gid;    // [n_slots] ascending, duplicate-free
    const uint32_t* slot_start;  // [n_slots] the group's first place in gix ...
    const uint32_t* slot_count;  // ... and its rows: start + count <= the store's length (the index's own extents)
    uint32_t* table;             // more than one pass: [nq_total][n_slots] ordinals, 0 = empty
    unsigned long long* keys;    // one pass: [n_slots] keys, 0 = dropped
    uint32_t n_slots;
    uint32_t ld, dim, dimq;
    uint32_t pass, nq_total, single;
    uint32_t metric, take_max, reduce, cmp;
    uint32_t chunk_rows;
    float thr;
};

// NT tokens share a pass (8, 16 or 32).  Dynamic LDS: mg_lds_bytes(dimq, NT) = [dimq][NT + 4] tokens | [NT] inverse norms | [4][NT] maxima.
template <int MK, int NT>
__global__ __launch_bounds__(64 * MG_WAVES) void maxsim_gather_kernel(MgParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTP = NT + (int)MG_PAD;
    float* sT = smem;                                            // [dimq][NTP]
    float* sQi = sT + (size_t)p.dimq * NTP;                      // [NT]
    uint32_t* sB = reinterpret_cast<uint32_t*>(sQi + NT);        // [MG_WAVES][NT]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 3, c = lane & 7;
    const uint32_t q0 = p.pass * NT;
    const uint32_t nq_here = (p.nq_total - q0) < (uint32_t)NT ? (p.nq_total - q0) : (uint32_t)NT;
    const bool take_max = p.take_max != 0;
    {
        // (the uploaded block is transposed and zero padded on the host: a straight copy; tokens past nq_here read as zeros)
        const float4* src = reinterpret_cast<const float4*>(p.tokens + (size_t)p.pass * p.dimq * NTP);
        float4* dst = reinterpret_cast<float4*>(sT);
        const uint32_t n4 = p.dimq * (uint32_t)NTP / 4;
        for (uint32_t i = tid; i < n4; i += 64 * MG_WAVES) dst[i] = src[i];
        if (tid < NT) sQi[tid] = p.qinv[q0 + tid];
    }
    __syncthreads();

    const uint32_t full = p.dim >> 3, nt = p.dim & 7u;
    for (uint32_t slot = blockIdx.x; slot < p.n_slots; slot += gridDim.x) {
        const uint32_t start = p.slot_start[slot], count = p.slot_count[slot];
        uint32_t best[NT];  // per token: the best ordinal among this lane group's rows of the group (0 = none yet)
#pragma unroll
        for (int q = 0; q < NT; q++) best[q] = 0u;
        for (uint32_t base = 0; base < count; base += MG_STEP_ROWS) {
#include "ott_maxsim_gather_step.inc"
        }

        // join: over the wave's eight row groups by shuffles, over the waves in LDS (ott_maxsim_gather_dev.h)
        mg_join_wave<NT>(best, sB, wave, lane);
        __syncthreads();
        if (p.single) {
            // one pass holds every token: the sum in token order, started from best[0], and the key
            if (tid == 0) {
                const unsigned long long key = mg_sum_key<NT>(sB, nq_here, take_max, p.cmp, p.thr, p.slot_gid[slot]);
                if (key != 0) p.keys[slot] = key;
            }
        } else if ((uint32_t)tid < nq_here) {
            const uint32_t o = mg_joined<NT>(sB, (uint32_t)tid);
            if (o != 0) p.table[(size_t)(q0 + (uint32_t)tid) * p.n_slots + slot] = o;  // (the table is zero when found: an empty slot is not written)
        }
        __syncthreads();  // sB is the next group's
    }
}

// counts[gid[i]] += 1 — every id < n_groups (checked on the host when the ids were set)
__global__ __launch_bounds__(256) void gix_count_kernel(const uint32_t* __restrict__ gid, uint64_t n, uint32_t* __restrict__ counts) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) atomicAdd(counts + gid[i], 1u);
}

// cursor[g] starts at the group's first place; a row takes the next one.  The places of a group are exactly its count, so at < n.
__global__ __launch_bounds__(256) void gix_scatter_kernel(const uint32_t* __restrict__ gid, uint64_t n, uint32_t* __restrict__ cursor, uint32_t* __restrict__ rows) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t at = atomicAdd(cursor + gid[i], 1u);
        if (at < n) rows[at] = (uint32_t)i;
    }
}

// One lane per 64 rows: bit b of words[w] = the group of row 64 w + b is in the bitmap (bits of rows at and past n are 0)
__global__ __launch_bounds__(256) void groups_mask_kernel(const uint32_t* __restrict__ gid, uint64_t n, const uint32_t* __restrict__ bitmap, uint64_t* __restrict__ words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= (n + 63) / 64) return;
    const uint64_t r0 = w * 64;
    const uint32_t cnt = (n - r0) < 64 ? (uint32_t)(n - r0) : 64u;
    uint64_t m = 0;
    for (uint32_t b = 0; b < cnt; b++) {
        const uint32_t g = gid[r0 + b];
        m |= (uint64_t)((bitmap[g >> 5] >> (g & 31)) & 1u) << b;
    }
    words[w] = m;
}

void group_index_drop(ott_store* s) {
    if (s->d_gix) (void)hipFree(s->d_gix);
    s->d_gix = nullptr;
    std::vector<uint32_t>().swap(s->gix_start);
    s->gix_ready.store(false, std::memory_order_release);
}

namespace {

// lock_shared_clean's clean step of a listed query that may take the gather: the staged rows go to the GPU and the index is built,
// under the exclusive lock (no query is running on any context).  Whoever comes second finds it there.
int group_index_ensure(ott_store* s, const char* fn) {
    ott::host::ExclusiveLock wr(s->rw);
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    if (s->gix_ready.load(std::memory_order_acquire)) return OTT_OK;
    if ((rc = check_group_ids(s, fn, true))) return rc;
    if (s->n_groups > MG_INDEX_MAX_GROUPS) {  // declined: the query takes the mask route
        s->gix_ready.store(true, std::memory_order_release);
        return OTT_OK;
    }
    OTT_HIP(use_device(s));
    const uint64_t n = s->gid_n;
    const uint32_t ng = s->n_groups;
    struct Tmp {
        uint32_t* p = nullptr;
        ~Tmp() { if (p) (void)hipFree(p); }
    } cnt, rows;
    OTT_HIP(hipMalloc((void**)&cnt.p, (size_t)ng * 4));
    OTT_HIP(hipMalloc((void**)&rows.p, (size_t)n * 4));
    const uint32_t grid = grid_blocks(n, 256, s->n_cu);
    OTT_HIP(hipMemsetAsync(cnt.p, 0, (size_t)ng * 4, s->stream));
    hipLaunchKernelGGL(gix_count_kernel, dim3(grid), dim3(256), 0, s->stream, (const uint32_t*)s->d_gid, n, cnt.p);
    OTT_HIP(hipGetLastError());
    std::vector<uint32_t> start((size_t)ng + 1);
    OTT_HIP(hipMemcpyAsync(start.data() + 1, cnt.p, (size_t)ng * 4, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    start[0] = 0;
    for (uint32_t i = 0; i < ng; i++) start[i + 1] += start[i];  // (n < 2^32 - 16: the sums fit)
    if (start[ng] != n) return fail(OTT_ERR_HIP, std::string(fn) + ": the group index counted " + std::to_string(start[ng]) + " rows of " + std::to_string(n));
    OTT_HIP(hipMemcpyAsync(cnt.p, start.data(), (size_t)ng * 4, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(gix_scatter_kernel, dim3(grid), dim3(256), 0, s->stream, (const uint32_t*)s->d_gid, n, cnt.p, rows.p);
    OTT_HIP(hipGetLastError());
    OTT_HIP(hipStreamSynchronize(s->stream));
    s->d_gix = rows.p;
    rows.p = nullptr;
    s->gix_start.swap(start);
    s->gix_builds.fetch_add(1, std::memory_order_relaxed);
    s->gix_ready.store(true, std::memory_order_release);
    return OTT_OK;
}

template <int MK, int NT>
int launch_mg(ott_store* s, const MgParams& p, uint32_t grid) {
    const size_t smem = (size_t)mg_lds_bytes(p.dimq, NT);
    auto kern = maxsim_gather_kernel<MK, NT>;
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
int launch_mg_mk(ott_store* s, const MgParams& p, uint32_t nt, uint32_t grid) {
    switch (nt) {
        case 8: return launch_mg<MK, 8>(s, p, grid);
        case 16: return launch_mg<MK, 16>(s, p, grid);
        case 32: return launch_mg<MK, 32>(s, p, grid);
        default: return fail(OTT_ERR_INVALID, "maxsim gather: no kernel for this number of tokens per pass");
    }
}

int launch_mg_any(ott_store* s, const MgParams& p, uint32_t nt, uint32_t grid) {
    switch (metric_kind(p.metric)) {
        case MK_L2: return launch_mg_mk<MK_L2>(s, p, nt, grid);
        case MK_L1: return launch_mg_mk<MK_L1>(s, p, nt, grid);
        default: return launch_mg_mk<MK_DOT>(s, p, nt, grid);
    }
}

// The gather route on a context whose `mu` the caller holds (and the owner's `rw`, shared).  sl: the list's slots with their extents
// in the index (at least one, at most MG_MAX_SLOTS); k_eff = min(k, slots) >= 1.
int run_maxsim_gather(ott_store* s, const ott_query_desc* d, const MgSlots& sl, uint64_t k_eff, ott_hit* out, uint64_t* n_out, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    memset(&st, 0, sizeof(st));
    const uint32_t nq = d->nq, n_slots = (uint32_t)sl.gid.size();
    const uint32_t nt = mg_tokens_per_pass(s->dimq, nq), passes = mg_passes(s->dimq, nq), ntp = nt + MG_PAD;
    RunPlan pl;
    make_run_plan(s, d->chunk_mask, pl);
    st.path_used = OTT_PATH_EXACT;
    st.total_chunks = pl.total_chunks;
    st.evaluated_chunks = pl.evaluated;
    st.pruned_chunks = pl.total_chunks - pl.evaluated;
    st.passes = passes;
    st.vectors_compared = sl.rows * nq;  // the listed groups' rows, before the masks
    st.bytes_scanned = (uint64_t)passes * sl.rows * ((uint64_t)s->dim * 4 + 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));  // (+ 4: the index's word)
    if (pl.rows_scored != 0 && sl.rows != 0) {
        MgParams p{};
        if ((rc = compose_row_mask(s, d, &p.row_mask, &p.row_mask_bits))) return rc;
        // one block up, one copy: [tokens, transposed per pass | qinv | slot gid | slot start | slot count | chunk mask words]
        const size_t tok_bytes = (size_t)passes * s->dimq * ntp * 4, qi_bytes = (size_t)passes * nt * 4, slot_bytes = (size_t)n_slots * 4;
        const size_t cm_words = d->chunk_mask ? (size_t)((pl.total_chunks + 63) / 64) : 0;
        const size_t off_qi = tok_bytes, off_gid = (off_qi + qi_bytes + 15) & ~(size_t)15, off_start = off_gid + slot_bytes, off_count = off_start + slot_bytes;
        const size_t off_cm = (off_count + slot_bytes + 15) & ~(size_t)15, total = off_cm + cm_words * 8;
        if ((rc = s->h_stage.ensure(total))) return rc;
        char* hs = (char*)s->h_stage.p;
        memset(hs, 0, off_gid);
        for (uint32_t t = 0; t < nq; t++) {
            const float* q = d->queries + (size_t)t * s->dim;
            float* dst = (float*)hs + (size_t)(t / nt) * s->dimq * ntp + (t % nt);
            for (uint32_t i = 0; i < s->dim; i++) dst[(size_t)i * ntp] = q[i];
            ((float*)(hs + off_qi))[t] = host_inv_norm_exact(q, s->dim);
        }
        memcpy(hs + off_gid, sl.gid.data(), slot_bytes);
        memcpy(hs + off_start, sl.start.data(), slot_bytes);
        memcpy(hs + off_count, sl.count.data(), slot_bytes);
        if (cm_words) memcpy(hs + off_cm, d->chunk_mask, cm_words * 8);
        if ((rc = s->d_queries.ensure(total))) return rc;
        OTT_HIP(hipMemcpyAsync(s->d_queries.p, hs, total, hipMemcpyHostToDevice, s->stream));
        const char* dq = (const char*)s->d_queries.p;
        p.rows = s->d_rows;
        p.inv = s->d_inv;
        p.tokens = (const float*)dq;
        p.qinv = (const float*)(dq + off_qi);
        p.slot_gid = (const uint32_t*)(dq + off_gid);
        p.slot_start = (const uint32_t*)(dq + off_start);
        p.slot_count = (const uint32_t*)(dq + off_count);
        p.chunk_mask = cm_words ? (const uint64_t*)(dq + off_cm) : nullptr;
        p.chunk_rows = s->chunk_size < 0xFFFFFFFFull ? (uint32_t)s->chunk_size : 0xFFFFFFFFu;  // (rows stay below 2^32 - 16)
        p.gix = s->d_gix;
        p.n_slots = n_slots;
        p.ld = s->ld;
        p.dim = s->dim;
        p.dimq = s->dimq;
        p.nq_total = nq;
        p.single = passes == 1;
        p.metric = d->metric;
        p.take_max = d->take == OTT_TAKE_MAX;
        p.reduce = s->reduce;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;

        // the ordinals are left zeroed by the reduce kernel, the keys by the select / compact kernel
        if (passes > 1 && (rc = ensure_zeroed(s, s->d_mstable, s->mstable_clean, (size_t)mg_table_bytes(nq, n_slots, passes)))) return rc;
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)mg_key_bytes(n_slots)))) return rc;
        p.table = passes > 1 ? (uint32_t*)s->d_mstable.p : nullptr;
        p.keys = (unsigned long long*)s->d_gtable.p;

        GroupTopK tk;
        tk.n_groups = n_slots;
        tk.nq = 1;
        tk.k = k_eff;
        tk.take_max = p.take_max != 0;
        tk.index_is_group = true;
        tk.id_span = s->n_groups;
        tk.also_clean = passes > 1 ? &s->mstable_clean : nullptr;
        if ((rc = tk.prepare(s, nullptr))) return rc;
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        // a workgroup per listed group, at most what the CUs hold at once (a workgroup then takes its next group)
        const uint64_t lds = mg_lds_bytes(s->dimq, nt);
        uint32_t per_cu = (uint32_t)(160ull * 1024 / lds);
        per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
        const uint32_t grid = std::min<uint32_t>(n_slots, (uint32_t)s->n_cu * per_cu);
        for (uint32_t ps = 0; ps < passes; ps++) {
            p.pass = ps;
            if ((rc = launch_mg_any(s, p, nt, grid))) return rc;
        }
        if (passes > 1 && (rc = launch_maxsim_reduce(s, p.table, n_slots, nq, p.take_max, (uint32_t)d->filter_cmp, d->filter_thr, p.keys, p.slot_gid))) return rc;
        if ((rc = tk.pass(s, p.keys, 0, 1))) return rc;
        if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
        if ((rc = tk.finish(s, timing, out, n_out, nullptr))) return rc;
        if (timing) read_exact_events(s, &st);
    }
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

// The mask route: the list as a device row mask in the context's scratch — [the mask | the mask & the caller's (compose_row_mask) |
// the bitmap over the groups] — then ott_query_maxsim's own sweep with it.  gids: ascending, duplicate-free, every one < n_groups.
int run_groups_as_mask(ott_store* s, const ott_query_desc* d, const std::vector<uint32_t>& gids, uint64_t k_eff, ott_hit* out, uint64_t* n_out,
                       ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t words = (s->n + 63) / 64;
    const size_t bm_words = ((size_t)s->n_groups + 31) / 32;
    if ((rc = s->d_idmask.ensure((size_t)words * 16 + bm_words * 4))) return rc;
    uint64_t* d_words = (uint64_t*)s->d_idmask.p;
    uint32_t* d_bitmap = (uint32_t*)(d_words + 2 * words);
    if ((rc = s->h_stage.ensure(bm_words * 4))) return rc;
    uint32_t* hb = (uint32_t*)s->h_stage.p;
    memset(hb, 0, bm_words * 4);
    for (const uint32_t g : gids) hb[g >> 5] |= 1u << (g & 31);
    OTT_HIP(hipMemcpyAsync(d_bitmap, hb, bm_words * 4, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(groups_mask_kernel, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, s->stream, (const uint32_t*)s->d_gid, (uint64_t)s->n, (const uint32_t*)d_bitmap,
                       d_words);
    OTT_HIP(hipGetLastError());
    OTT_HIP(hipStreamSynchronize(s->stream));  // (h_stage is the query's own staging next)
    IdMaskGuard guard{s};
    s->cur_idmask = d_words;
    return run_maxsim(s, d, k_eff, out, n_out, stats_out);
}

}  // namespace

int check_listed_groups(const char* fn, const uint32_t* groups, uint64_t n_listed, uint32_t n_groups) {
    if (n_listed && !groups) return fail(OTT_ERR_INVALID, std::string(fn) + ": groups is NULL");
    for (uint64_t i = 0; i < n_listed; i++)
        if (groups[i] >= n_groups)
            return fail(OTT_ERR_INVALID, std::string(fn) + ": group " + std::to_string(groups[i]) + " is out of range (the store holds " + std::to_string(n_groups) + " groups)");
    return OTT_OK;
}

// The store shared, with nothing left to do first: staged rows go to the GPU and — where a listed query of this store may take the
// gather — the group-to-rows index is there.  Both happen under the exclusive lock, in the clean step; no query waits on a mutex
// for them.  (ott_query_maxsim_groups_batch takes it once for all its queries.)
int maxsim_groups_lock(ott_store* s, const char* fn, ott::host::SharedLock& rd) {
    const auto wants_index = [s] { return mg_wants_index(false, false, s->dimq, s->opt.group_gather); };
    return ott::host::lock_shared_clean(
        s->rw, rd, [&] { return s->pend.count() != 0 || (wants_index() && !s->gix_ready.load(std::memory_order_acquire)); },
        [&] { return wants_index() ? group_index_ensure(s, fn) : store_flush(s); });
}

// One listed query under the shared lock (`fn`: the entry point the messages name): the route and the run.
int maxsim_groups_locked(ott_store* s, const ott_query_desc* d, const uint32_t* groups, uint64_t n_groups_listed, ott_hit* out, uint64_t cap, uint64_t* n_out,
                         ott_stats* stats, const char* fn) {
    int rc;
    const std::string name(fn);
    // what the checks in front of the lock read without it is read again, and k_eff only here: a set_groups may have come in between
    if ((rc = check_group_ids(s, fn, true))) return rc;
    if ((rc = check_listed_groups(fn, groups, n_groups_listed, s->n_groups))) return rc;
    const bool wants_index = mg_wants_index(false, false, s->dimq, s->opt.group_gather);
    const bool have_index = s->d_gix != nullptr && s->gix_start.size() == (size_t)s->n_groups + 1;
    MgSlots sl;
    mg_slots(groups, n_groups_listed, s->n_groups, have_index ? s->gix_start.data() : nullptr, sl);
    const uint64_t k_eff = d->k < sl.gid.size() ? d->k : sl.gid.size();
    if (cap < k_eff) return fail(OTT_ERR_INVALID, name + ": output capacity is smaller than min(k, distinct listed groups)");
    if (!out && cap) return fail(OTT_ERR_INVALID, name + ": out is NULL");
    if (k_eff == 0) return OTT_OK;  // an empty list, or k == 0: a valid query with no hits
    const bool gather = mg_takes_gather(wants_index, have_index, s->opt.group_gather, sl.gid.size(), sl.rows);
    if (!gather && !mg_sweep_table_fits(d->nq, s->n_groups))
        return fail(OTT_ERR_UNSUPPORTED,
                    name + ": tokens x groups x 4 bytes is above 2 GiB on the mask route (the sweep's table holds every group of the store); use fewer "
                           "tokens or groups, or a list the gather kernel serves");
    CtxLease ctx(s);
    return gather ? run_maxsim_gather(ctx.c, d, sl, k_eff, out, n_out, stats) : run_groups_as_mask(ctx.c, d, sl.gid, k_eff, out, n_out, stats);
}

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_maxsim_groups(ott_store* s, const ott_query_desc* d, const void* groups_void, uint64_t n_groups_listed, ott_hit* out, uint64_t cap, uint64_t* n_out,
                            ott_stats* stats) {
    const uint32_t* groups = (const uint32_t*)groups_void;
    const char* fn = "ott_query_maxsim_groups";
    // what the descriptor alone decides comes first: these refusals need no store
    if (d && d->mode == OTT_MODE_PER_QUERY)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim_groups: the query vectors are the tokens of ONE query; PER_QUERY (a batch of token sets) is not served");
    if (d && d->path == OTT_PATH_MFMA)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_maxsim_groups: the MFMA path does not serve late-interaction queries; use path AUTO or EXACT");
    if (!s) return fail(OTT_ERR_INVALID, "ott_query_maxsim_groups: store is NULL");
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (s->multi)
        return fail(OTT_ERR_UNSUPPORTED,
                    "ott_query_maxsim_groups: a multi-GPU store is not served (a group may span shards: the maxima would have to be joined before the sum)");
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    // before any device work: the ids are set and cover the store, the list names groups that exist
    if ((rc = check_group_ids(s, fn, false))) return rc;
    if ((rc = check_listed_groups(fn, groups, n_groups_listed, ott_store_group_count(s)))) return rc;
    ott::host::SharedLock rd;  // the corpus, the group ids and the index cannot change while this query runs
    if ((rc = maxsim_groups_lock(s, fn, rd))) return rc;
    return maxsim_groups_locked(s, d, groups, n_groups_listed, out, cap, n_out, stats, fn);
}

uint64_t ott_store_group_index_builds(const ott_store* s) { return s ? s->gix_builds.load(std::memory_order_relaxed) : 0ull; }

}  // extern "C"
