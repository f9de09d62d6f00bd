// ott_group.hip — grouped search: one best hit per group, top-k over the groups.  ott_query_groups returns the
// hits of the same query with the default take (every passing pair in the canonical order) after dropping every hit whose group
// occurred earlier in that list, cut at k — per query.  One sweep and one small table give that answer on the GPU:
//
//   group_sweep_kernel    sweep_tiles (ott_sweep_dev.h: the streaming tile loop this sweep shares with maxsim_sweep_kernel) and this
//                         epilogue per (row, query of the pass): composed row mask, NaN drop, cmp_holds, key = ord(score) << 32 |
//                         ~row; if the key beats a load of table[q][gid[row]], a vector atomicMax on that 64-bit slot.  The load
//                         in front keeps the atomics at the number of IMPROVEMENTS, not the number of rows.  0 = empty slot (no
//                         key is 0: rows stay below 2^32 - 16, so ~row >= 15).  The largest key of a group is its best score and,
//                         among equal scores, its lowest row: the group's first hit in the canonical list.
//   group_select_kernel   k_eff <= 512: one-wave workgroups sweep the table and offer every non-empty slot to a register wave list
//                         (WaveList<E>); block lists in the layout launch_merge takes.  Leaves the slots it read zeroed.
//   group_compact_kernel  k_eff > 512 (what a plan without take() gives): the non-empty slots become (key, query) pairs in the
//                         arrays of ott_sort.hip; its radix sort and hits_from_sorted order them (sort_group_pairs).  Zeroes too.
//
// Tie order: ALWAYS the canonical one (better score, lower row, lower query), whatever option tie_order says — the reference has
// no grouped query whose tie outcome could be reproduced.  MERGED with nq > 1 is refused (one winner per group ACROSS queries is
// left out: use PER_QUERY), Path.Mfma too (AUTO takes this sweep and never builds, extends or waits for a plane, as for Manhattan).
//
// The host half of a sweep over grouped rows is shared with ott_maxsim.hip too (declared in ott_internal.h): sweep_prologue (plan,
// mask, upload, SweepParams, grid), ensure_zeroed (the "zero when found" table protocol), GroupTopK (key table -> host hits) and
// check_group_ids.  Queries per pass: ott_sweep_dev.h; the epilogue here adds a key and a slot address, not a list.
// ott_group_top.hip (up to m hits per group) uses the same host half, run_groups itself for m = 1, and the select /
// compact kernels on the first plane of its [query][level][group] table: that is what their q_stride argument is for.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_sweep_dev.h"

namespace ott {

constexpr uint32_t GS_MAX_LISTS = 1024;  // block lists per query the select kernel writes (merge_rank_kernel takes up to 4096)

struct GroupParams : SweepParams {
    unsigned long long* table;  // [NQ][n_groups] best key per (query of the pass, group); 0 = empty
    uint32_t n_groups;
    uint32_t cmp;
    float thr;
};

template <int MK, int NQ>
__global__ __launch_bounds__(64 * SW_WAVES) void group_sweep_kernel(GroupParams p) {
    const bool take_max = p.take_max != 0;
    // score -> filter -> key -> the group's slot
    sweep_tiles<MK, NQ>(p, [&](uint64_t my_row, bool valid, uint32_t g, const float (&sc)[NQ], uint32_t nq_here) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            if ((uint32_t)q < nq_here) {
                const float s = sc[q];
                const bool pass = valid && !(s != s) && cmp_holds(s, p.cmp, p.thr);  // NaN dropped: vec_compute.rs:237
                if (pass) {
                    const unsigned long long key = ((unsigned long long)ord_of(s, take_max) << 32) | (uint32_t)(~(uint32_t)my_row);
                    unsigned long long* slot = p.table + (size_t)q * p.n_groups + g;
                    // the load goes past this CU's vector L1 (agent scope), so it sees what other CUs' atomics left; a value that
                    // is stale all the same is a smaller one (slots only rise) and costs an atomic, never a result
                    if (key > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, key);
                }
            }
        }
    });
}

// One wave per workgroup; blockIdx.x = list, blockIdx.y = query of the pass.  The wave walks tiles of 64 slots, list by list
// strided, and offers the non-empty ones; the slots it read are left zeroed (the next query's sweep needs no memset).  q_stride:
// slots between the tables of two queries of the pass (n_groups; group_size x n_groups where ott_group_top.hip keeps deeper planes).
template <int E>
__global__ __launch_bounds__(64) void group_select_kernel(unsigned long long* table, uint32_t n_groups, uint64_t q_stride, uint32_t q0, uint32_t k, Cand* lists,
                                                          uint32_t n_lists, uint32_t list_stride) {
    const int lane = threadIdx.x;
    const uint32_t qy = blockIdx.y;
    unsigned long long* tab = table + (size_t)qy * q_stride;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n_groups + 63) / 64);  // (in 64 bits: n_groups + 63 wraps from 2^32 - 63 groups on)
    WaveList<E> L;
    wl_init(L);
    uint64_t tk = 0;
    uint32_t tq = 0xFFFFFFFFu;
    bool fresh = true;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t i = t * 64 + (uint32_t)lane;
        uint64_t key = 0;
        if (i < n_groups) {
            key = tab[i];
            if (key != 0) tab[i] = 0ull;
        }
        const bool pass = key != 0;
        if (__ballot(pass) == 0) continue;
        if (fresh) {
            wl_fill_sorted(L, tk, tq, k, pass, key, q0 + qy, lane, 0u);
            fresh = false;
        } else {
            wl_offer_block(L, tk, tq, k, pass, key, q0 + qy, lane, 0u);
        }
    }
    Cand* dst = lists + ((size_t)(q0 + qy) * n_lists + blockIdx.x) * list_stride;
#pragma unroll
    for (int e = 0; e < E; e++) {
        Cand c;
        c.key = L.key[e];
        c.q = L.q[e];
        c.pad = 0;
        dst[e * 64 + lane] = c;
    }
}

// k_eff > 512: every non-empty slot of the pass's table becomes a (key, query) pair behind the cursor — one returning atomic
// per wave and tile that holds any — and is zeroed.  blockIdx.y = query of the pass.
__global__ __launch_bounds__(256) void group_compact_kernel(unsigned long long* table, uint32_t n_groups, uint64_t q_stride, uint32_t q0, uint64_t* keys, uint32_t* qs,
                                                            unsigned long long* cursor, uint64_t cap) {
    const int lane = threadIdx.x & 63;
    const uint32_t qy = blockIdx.y;
    unsigned long long* tab = table + (size_t)qy * q_stride;
    const uint64_t n_round = ((uint64_t)n_groups + 63) & ~63ull;  // whole waves stay together for the ballot
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t key = 0;
        if (i < n_groups) {
            key = tab[i];
            if (key != 0) tab[i] = 0ull;
        }
        const uint64_t m = __ballot(key != 0);
        if (m == 0) continue;
        unsigned long long base = 0;
        if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
        base = rl64(base, (int)__builtin_ctzll(m));
        if (key != 0) {
            const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (at < cap) {
                keys[at] = key;
                qs[at] = q0 + qy;
            }
        }
    }
}

// out[i] = gid[rows[i]], rows[i] < the rows the ids cover (checked on the host)
__global__ __launch_bounds__(256) void group_gather_kernel(const uint32_t* __restrict__ gid, const uint64_t* __restrict__ rows, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gid[rows[i]];
}

namespace {

int launch_group_select(ott_store* s, unsigned long long* table, uint32_t n_groups, uint64_t q_stride, uint32_t q0, uint32_t nq_here, uint32_t k, int E, Cand* lists,
                        uint32_t n_lists) {
#define OTT_GSEL(Ev)                                                                                                                       \
    if (E == Ev) {                                                                                                                         \
        hipLaunchKernelGGL((group_select_kernel<Ev>), dim3(n_lists, nq_here), dim3(64), 0, s->stream, table, n_groups, q_stride, q0, k, lists, \
                           n_lists, (uint32_t)(64 * Ev));                                                                                  \
        OTT_HIP(hipGetLastError());                                                                                                        \
        return OTT_OK;                                                                                                                     \
    }
    OTT_GSEL(1) OTT_GSEL(2) OTT_GSEL(4) OTT_GSEL(8)
#undef OTT_GSEL
    return fail(OTT_ERR_INVALID, "group select: bad E");
}

int launch_group_compact(ott_store* s, unsigned long long* table, uint32_t n_groups, uint64_t q_stride, uint32_t q0, uint32_t nq_here, uint64_t* keys, uint32_t* qs,
                         unsigned long long* cursor, uint64_t cap) {
    uint32_t blocks = (uint32_t)(((uint64_t)n_groups + 255) / 256);
    if (blocks > (uint32_t)s->n_cu * 8) blocks = (uint32_t)s->n_cu * 8;
    hipLaunchKernelGGL(group_compact_kernel, dim3(blocks, nq_here), dim3(256), 0, s->stream, table, n_groups, q_stride, q0, keys, qs, cursor, cap);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

}  // namespace

// The grouped query on a context whose `mu` the caller holds (and the owner's `rw`, shared).  k_eff = min(k, n_groups) >= 1.
// (ott_group_top.hip runs it too: group_size 1 IS this query.)
int run_groups(ott_store* s, const ott_query_desc* d, uint64_t k_eff, ott_hit* out, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    const uint32_t nq = d->nq, ng = s->n_groups;
    GroupParams p{};
    uint32_t grid = 0;
    if ((rc = sweep_prologue(s, d, &st, &p, &grid))) return rc;
    if (grid != 0) {
        const uint32_t tile = nq == 1 ? 1u : SW_NQ;
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)tile * ng * 8))) return rc;
        p.table = (unsigned long long*)s->d_gtable.p;
        p.n_groups = ng;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;

        GroupTopK tk;
        tk.n_groups = ng;
        tk.nq = nq;
        tk.k = k_eff;
        tk.take_max = p.take_max != 0;
        if ((rc = tk.prepare(s, "ott_query_groups: more than 2^32 - 16 (query, group) pairs; use take(k) with k <= 512 or fewer queries"))) return rc;
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        for (uint32_t ps = 0; ps < st.passes; ps++) {
            p.q0 = ps * tile;
            if ((rc = launch_sweep(s->stream, p, tile, grid, OTT_SWEEP_KERNEL(group_sweep_kernel)))) return rc;
            if ((rc = tk.pass(s, p.table, p.q0, (nq - p.q0) < tile ? (nq - p.q0) : tile))) return rc;
        }
        if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
        if ((rc = tk.finish(s, timing, out, n_out, n_per_query))) return rc;
        if (timing) read_exact_events(s, &st);
    }
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

// Stats, run plan, composed row mask, tile prefix and the upload of a sweep over grouped rows; `p` gets what the store, the
// descriptor and the plan decide (q0 and whatever the kernel's own struct adds are the caller's).  *grid: the persistent grid — a
// workgroup of four waves per four tiles, at most SW_BLOCKS_PER_CU per CU: from 4 x SW_BLOCKS_PER_CU x n_cu tiles (2048 tiles =
// 131072 rows on 256 CUs) a wave takes a second tile — or 0: no row survives the chunk mask, `st` is complete and nothing was uploaded.
int sweep_prologue(ott_store* s, const ott_query_desc* d, ott_stats* st, SweepParams* p, uint32_t* grid) {
    return sweep_prologue(s, d, d->queries, d->nq, st, p, grid);
}

// The stats of `nq` queries, the run plan and — where a row survives the chunk mask — the composed row mask (the descriptor's own,
// caller's or evaluated, an id list's, the live mask): what a sweep needs before it looks at a query block
int sweep_plan(ott_store* s, const ott_query_desc* d, uint32_t nq, ott_stats* st, RunPlan* pl, const uint64_t** row_mask, uint64_t* row_mask_bits) {
    memset(st, 0, sizeof(*st));
    make_run_plan(s, d->chunk_mask, *pl);
    st->path_used = OTT_PATH_EXACT;
    st->total_chunks = pl->total_chunks;
    st->evaluated_chunks = pl->evaluated;
    st->pruned_chunks = pl->total_chunks - pl->evaluated;
    st->vectors_compared = pl->rows_scored * nq;
    if (pl->rows_scored == 0) return OTT_OK;
    return compose_row_mask(s, d, row_mask, row_mask_bits);
}

// ... with the query block named apart from the descriptor: `queries` nullptr = nq zeroed slots that a kernel of the caller's fills
// from stored rows before the sweep reads them (ott_recommend.hip)
int sweep_prologue(ott_store* s, const ott_query_desc* d, const float* queries, uint32_t nq, ott_stats* st, SweepParams* p, uint32_t* grid) {
    int rc;
    RunPlan pl;
    *grid = 0;
    if ((rc = sweep_plan(s, d, nq, st, &pl, &p->row_mask, &p->row_mask_bits))) return rc;
    if (pl.rows_scored == 0) return OTT_OK;
    const std::vector<uint32_t> prefix = tile_prefix(pl, 64);
    if ((rc = upload_exact_inputs(s, queries, nq, pl, prefix))) return rc;
    st->passes = nq == 1 ? 1u : (nq + SW_NQ - 1) / SW_NQ;
    st->bytes_scanned = (uint64_t)st->passes * pl.rows_scored * ((uint64_t)s->dim * 4 + 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));  // (+ 4: the group id)
    p->rows = s->d_rows;
    p->inv = s->d_inv;
    p->queries = (const float*)s->d_queries.p;
    p->qinv = (const float*)((const char*)s->d_queries.p + s->in_off_qinv);
    p->runs = (const ott_run*)((const char*)s->d_queries.p + s->in_off_runs);
    p->tile_prefix = (const uint32_t*)((const char*)s->d_queries.p + s->in_off_prefix);
    p->gid = s->d_gid;
    p->ld = s->ld;
    p->dim = s->dim;
    p->dimq = s->dimq;
    p->n_runs = (uint32_t)pl.runs.size();
    p->n_tiles = prefix.back();
    p->nq_total = nq;
    p->metric = d->metric;
    p->take_max = d->take == OTT_TAKE_MAX;
    p->reduce = s->reduce;
    *grid = std::min((p->n_tiles + SW_WAVES - 1) / SW_WAVES, (uint32_t)s->n_cu * SW_BLOCKS_PER_CU);
    if (*grid < 1) *grid = 1;
    return OTT_OK;
}

// A table that is zero when a query finds it: zeroed here when it is (re)allocated or a query failed half way (`clean` is false),
// left zeroed by the kernel that reads it; the caller sets `clean` again once the stream has drained.
int ensure_zeroed(ott_store* s, DevBuf& b, bool& clean, size_t bytes) {
    int rc;
    if (b.cap < bytes || !clean) {
        if ((rc = b.ensure(bytes))) return rc;
        OTT_HIP(hipMemsetAsync(b.p, 0, b.cap, s->stream));
    }
    clean = false;
    return OTT_OK;
}

int GroupTopK::prepare(ott_store* s, const char* too_many_pairs) {
    int rc;
    lists_path = k <= 512;
    E = lists_path ? list_E(k) : 1;
    KS = 64u * (uint32_t)E;
    n_lists = std::min((uint32_t)(((uint64_t)n_groups + 63) / 64), GS_MAX_LISTS);
    pair_cap = (uint64_t)nq * n_groups;
    if (lists_path) return s->d_lists.ensure((size_t)nq * n_lists * KS * sizeof(Cand));
    if (too_many_pairs && pair_cap > 0xFFFFFFF0ull) return fail(OTT_ERR_UNSUPPORTED, too_many_pairs);
    if ((rc = ensure_group_pairs(s, pair_cap))) return rc;
    if ((rc = s->d_gctl.ensure(64))) return rc;
    OTT_HIP(hipMemsetAsync(s->d_gctl.p, 0, 8, s->stream));
    return OTT_OK;
}

int GroupTopK::pass(ott_store* s, unsigned long long* table, uint32_t q0, uint32_t nq_here) {
    const uint64_t stride = q_stride ? q_stride : n_groups;
    if (lists_path) return launch_group_select(s, table, n_groups, stride, q0, nq_here, (uint32_t)k, E, (Cand*)s->d_lists.p, n_lists);
    return launch_group_compact(s, table, n_groups, stride, q0, nq_here, (uint64_t*)s->l_keysA.p, (uint32_t*)s->l_qA.p, (unsigned long long*)s->d_gctl.p, pair_cap);
}

int GroupTopK::finish(ott_store* s, bool timing, ott_hit* out, uint64_t* n_out, uint64_t* n_per_query) {
    int rc;
    uint64_t total = 0;
    if (lists_path) {
        // results block in pinned host memory, as run_exact lays it out: [counts (nq x u64, padded to 64 B) | hits (nq x KS)]
        const size_t cnt_pad = (((size_t)nq * sizeof(uint64_t)) + 63) & ~(size_t)63;
        if ((rc = s->h_hits.ensure(cnt_pad + (size_t)nq * KS * sizeof(ott_hit)))) return rc;
        void* mapped = nullptr;
        OTT_HIP(hipHostGetDevicePointer(&mapped, s->h_hits.p, 0));
        if ((rc = launch_merge(s, (const Cand*)s->d_lists.p, n_lists, KS, (uint64_t)n_lists * KS, nq, (uint32_t)k, E, take_max, index_is_group ? 0 : s->base_offset,
                               (ott_hit*)((char*)mapped + cnt_pad), KS, (uint64_t*)mapped, 0)))
            return rc;
        if (after_merge && (rc = after_merge(s, after_arg, (const ott_hit*)((const char*)mapped + cnt_pad), (const uint64_t*)mapped))) return rc;
        if (timing) OTT_HIP(hipEventRecord(s->ev[5], s->stream));
        OTT_HIP(hipStreamSynchronize(s->stream));
        s->gtable_clean = true;
        if (also_clean) *also_clean = true;
        const char* hh = (const char*)s->h_hits.p;
        const uint64_t* counts = (const uint64_t*)hh;
        const ott_hit* hits = (const ott_hit*)(hh + cnt_pad);
        for (uint32_t q = 0; q < nq; q++) {
            uint64_t cq = counts[q];
            if (index_is_group && cq > k) cq = k;
            if (cq) memcpy(out + total, hits + (size_t)q * KS, (size_t)cq * sizeof(ott_hit));
            if (n_per_query) n_per_query[q] = cq;
            total += cq;
        }
    } else {
        unsigned long long n_pairs = 0;
        OTT_HIP(hipMemcpyAsync(&n_pairs, s->d_gctl.p, 8, hipMemcpyDeviceToHost, s->stream));
        OTT_HIP(hipStreamSynchronize(s->stream));
        s->gtable_clean = true;
        if (also_clean) *also_clean = true;
        if (n_pairs > pair_cap) n_pairs = pair_cap;
        std::vector<std::vector<ott_hit>> lists;
        if ((rc = sort_group_pairs(s, n_pairs, nq, take_max, k, lists, index_is_group ? (id_span ? id_span : n_groups) : 0))) return rc;
        if (timing) {
            OTT_HIP(hipEventRecord(s->ev[5], s->stream));
            OTT_HIP(hipStreamSynchronize(s->stream));
        }
        for (uint32_t q = 0; q < nq; q++) {
            std::vector<ott_hit>& l = lists[q];
            if (index_is_group)
                for (ott_hit& h : l) h.index -= s->base_offset;  // the sort path's hits are rows of the store; these are groups
            if (!l.empty()) memcpy(out + total, l.data(), l.size() * sizeof(ott_hit));
            if (n_per_query) n_per_query[q] = l.size();
            total += l.size();
        }
    }
    if (n_out) *n_out = total;
    return OTT_OK;
}

// What ott_query_groups and ott_query_maxsim (`fn`) ask of the group ids: they are set and cover the store's rows.  Asked before
// the lock, and again under it (`locked`): a set_groups may have come in between.  A multi-GPU store's ids live on its shards.
int check_group_ids(const ott_store* s, const char* fn, bool locked) {
    const std::string name(fn);
    if (s->n_groups == 0) return fail(OTT_ERR_INVALID, name + ": no group ids are set (ott_store_set_groups)");
    if (locked) {
        if (s->gid_n != s->n) return fail(OTT_ERR_INVALID, name + ": the group ids no longer cover the store's rows (set them again)");
    } else if (!s->multi && s->gid_n != ott_store_len(s)) {  // staged rows count: they were appended
        return fail(OTT_ERR_INVALID, name + ": the group ids cover " + std::to_string(s->gid_n) + " rows, the store holds " + std::to_string(ott_store_len(s)) +
                                         " (rows were appended since ott_store_set_groups: set them again)");
    }
    return OTT_OK;
}

int group_grow(ott_store* s, uint64_t ncap) {
    if (!s->d_gid || ncap <= s->cap) return OTT_OK;
    uint32_t* ng = nullptr;
    OTT_HIP(hipMalloc((void**)&ng, (size_t)ncap * 4));
    OTT_HIP(hipMemcpyAsync(ng, s->d_gid, (size_t)s->gid_n * 4, hipMemcpyDeviceToDevice, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    (void)hipFree(s->d_gid);
    s->d_gid = ng;
    return OTT_OK;
}

// The groups of `n` hits of this store (a shard of a multi-GPU store hands them to the merging host with its hits): a gather of n
// values from the resident ids.  The caller holds the store shared (or the multi-GPU front that owns it).
int group_ids_of_hits(ott_store* s, const ott_hit* hits, uint64_t n, uint32_t* out) {
    if (n == 0) return OTT_OK;
    if (!s->d_gid) return fail(OTT_ERR_INVALID, "group_ids_of_hits: no group ids are set");
    CtxLease lease(s);
    ott_store* ctx = lease.c;
    int r;
    OTT_HIP(use_device(ctx));
    if ((r = ctx->h_stage.ensure((size_t)n * 8))) return r;
    uint64_t* hr = (uint64_t*)ctx->h_stage.p;
    for (uint64_t i = 0; i < n; i++) {
        hr[i] = hits[i].index - ctx->base_offset;
        if (hr[i] >= ctx->gid_n) return fail(OTT_ERR_INVALID, "group_ids_of_hits: a hit outside the store's rows");
    }
    if ((r = ctx->d_gather.ensure(64 + (size_t)n * 12))) return r;
    uint64_t* d_rows = (uint64_t*)((char*)ctx->d_gather.p + 64);
    uint32_t* d_out = (uint32_t*)(d_rows + n);
    OTT_HIP(hipMemcpyAsync(d_rows, hr, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(group_gather_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)ctx->d_gid, (const uint64_t*)d_rows, n, d_out);
    OTT_HIP(hipGetLastError());
    OTT_HIP(hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    OTT_HIP(hipStreamSynchronize(ctx->stream));
    return OTT_OK;
}

void group_drop(ott_store* s) {
    group_index_drop(s);  // the group-to-rows index of listed MaxSim depends on the ids alone: it goes with them
    if (s->d_gid) (void)hipFree(s->d_gid);
    s->d_gid = nullptr;
    s->gid_n = 0;
    s->n_groups = 0;
}

}  // namespace ott

using namespace ott;

extern "C" {

int ott_store_set_groups(ott_store* s, const void* gid_void, uint64_t n, uint32_t n_groups) {
    const uint32_t* gid_host = (const uint32_t*)gid_void;
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_groups: store is NULL");
    if (n && !gid_host) return fail(OTT_ERR_INVALID, "ott_store_set_groups: gid is NULL");
    if (n != ott_store_len(s))
        return fail(OTT_ERR_INVALID, "ott_store_set_groups: " + std::to_string(n) + " group ids for a store of " + std::to_string(ott_store_len(s)) + " rows");
    if (n && n_groups == 0) return fail(OTT_ERR_INVALID, "ott_store_set_groups: n_groups is 0");
    for (uint64_t i = 0; i < n; i++)  // before any device work
        if (gid_host[i] >= n_groups)
            return fail(OTT_ERR_INVALID, "ott_store_set_groups: group id " + std::to_string(gid_host[i]) + " of row " + std::to_string(i) + " is not below n_groups = " +
                                             std::to_string(n_groups));
    if (s->multi) return multi_set_groups(s, gid_host, n, n_groups);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    if (n != s->n) return fail(OTT_ERR_INVALID, "ott_store_set_groups: the store's length changed during the call");
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    group_drop(s);
    if (n == 0) return OTT_OK;
    const uint64_t slots = s->cap > n ? s->cap : n;
    OTT_HIP(hipMalloc((void**)&s->d_gid, (size_t)slots * 4));
    const hipError_t e = hipMemcpy(s->d_gid, gid_host, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        group_drop(s);
        return fail(OTT_ERR_HIP, std::string("ott_store_set_groups: ") + hipGetErrorString(e));
    }
    s->gid_n = n;
    s->n_groups = n_groups;
    return OTT_OK;
}

int ott_store_clear_groups(ott_store* s) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_clear_groups: store is NULL");
    if (s->multi) return multi_clear_groups(s);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    if (!s->d_gid) return OTT_OK;
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    group_drop(s);
    return OTT_OK;
}

uint32_t ott_store_group_count(const ott_store* s) { return s ? s->n_groups : 0u; }

int ott_query_groups(ott_store* s, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats) {
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (d->mode == OTT_MODE_MERGED && d->nq > 1)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_groups: a merged list over several queries is not served (one winner per group across queries); use PER_QUERY");
    if (d->path == OTT_PATH_MFMA) return fail(OTT_ERR_UNSUPPORTED, "ott_query_groups: the MFMA path does not serve grouped queries; use path AUTO or EXACT");
    if (n_out) *n_out = 0;
    if (n_per_query)
        for (uint32_t i = 0; i < d->nq; i++) n_per_query[i] = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if ((rc = check_group_ids(s, "ott_query_groups", false))) return rc;
    if (s->multi) return multi_query_groups(s, d, out, cap, n_out, n_per_query, stats);
    ott::host::SharedLock rd;  // the corpus and the group ids cannot change while this query runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    // what the checks above read without the lock is read again, and k_eff only here: a set_groups may have come in between
    if ((rc = check_group_ids(s, "ott_query_groups", true))) return rc;
    const uint64_t k_eff = d->k < s->n_groups ? d->k : s->n_groups;
    if (cap < k_eff * d->nq) return fail(OTT_ERR_INVALID, "ott_query_groups: output capacity is smaller than nq * min(k, n_groups)");
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_groups: out is NULL");
    if (k_eff == 0) return OTT_OK;
    CtxLease ctx(s);
    return run_groups(ctx.c, d, k_eff, out, n_out, n_per_query, stats);
}

}  // extern "C"
