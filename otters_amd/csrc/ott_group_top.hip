// ott_group_top.hip — grouped search with up to m hits per group: ott_query_groups_top.  The hits of the same
// query with the default take (every passing pair in the canonical order) after dropping every hit that has m earlier hits of its
// group; groups ranked by their first hit, the first k_eff = min(k, n_groups) groups kept, each group's hits contiguous — per query.
// group_size 1 IS ott_query_groups (run_groups of ott_group.hip, untouched).  For m >= 2:
//
//   the table               [query][level][group] 8-byte keys for ALL nq queries at once (the deeper levels must outlive the passes
//                           until the winners are known), key = ord(score) << 32 | ~row as in ott_group.hip, 0 = empty.  Plane 0 of a
//                           query is exactly grouped search's table, so its top-k kernels (group_select_kernel / group_compact_kernel,
//                           GroupTopK) rank the groups on it with one added stride and zero it as they read.
//   group_top_sweep_kernel  sweep_tiles (ott_sweep_dev.h) and group_sweep_kernel's epilogue — composed row mask, NaN drop, cmp_holds,
//                           the key — followed by a CASCADE INSERTION into the group's m slots: for level j = 0 .. m-1, a relaxed
//                           agent-scope load of slot j; if the carried key is larger, old = atomicMax(slot j, key); when old < key
//                           the thread took the slot and goes on with `old` as its carried key (it stops on old == 0: nothing was
//                           there); otherwise it goes to the next level with the same key.  Why slot j ends as the (j+1)-th largest
//                           key of the group under ANY interleaving:
//                             - every key is at any time in exactly one place: a slot, or the register of a thread walking down;
//                             - so level j receives every key except the final occupants of the levels above it;
//                             - atomicMax is order-free: a slot ends as the maximum of what it received, and what a slot gives up
//                               is carried to the next level, so level j's maximum is the (j+1)-th largest key;
//                             - a stale load is a smaller value (slots only rise): it costs an atomic, never a result;
//                             - the keys of one query are distinct, because the rows are: old == key cannot happen.
//                           In front of the cascade the thread loads slot m-1 — the group's current m-th best, never above the
//                           final one — and skips the cascade unless its key beats it: a skipped key is not among the final m
//                           largest.  The atomics number the IMPROVEMENTS, not the rows, as in group_sweep_kernel.  Vector atomics
//                           and plain C++ only.
//   group_emit_kernel       one lane per winner (query, rank): row of the winner's hit -> gid[row] -> the group's slots of levels
//                           1 .. m-1 -> hits (base_offset added as everywhere), the group's id and hit count, in ONE block the host
//                           copies.  The winners come from the host (GroupTopK::finish ends there): one extra round trip, winners up,
//                           hits down, as group_ids_of_hits takes.
//   clearing                plane 0 is zeroed by the top-k kernels; the deeper planes — those of groups that did not win too — by one
//                           async memset of the table behind the emit.  gtable_clean is only set once that has drained: a query that
//                           fails anywhere leaves it false and the next query on the context (grouped, MaxSim or this) zeroes first.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_sweep_dev.h"

namespace ott {

constexpr uint64_t GT_TABLE_MAX = 1ull << 31;  // bytes of the [query][level][group] table: all queries are held at once

struct GroupTopParams : SweepParams {
    unsigned long long* table;  // [nq_total][m][n_groups]; 0 = empty
    uint32_t n_groups;
    uint32_t m;  // group_size, 2 .. OTT_GROUP_SIZE_MAX
    uint32_t cmp;
    float thr;
};

template <int MK, int NQ>
__global__ __launch_bounds__(64 * SW_WAVES) void group_top_sweep_kernel(GroupTopParams p) {
    const bool take_max = p.take_max != 0;
    // score -> filter -> key -> cascade into the group's m slots
    sweep_tiles<MK, NQ>(p, [&](uint64_t my_row, bool valid, uint32_t g, const float (&sc)[NQ], uint32_t nq_here) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            if ((uint32_t)q < nq_here) {
                const float s = sc[q];
                const bool pass = valid && !(s != s) && cmp_holds(s, p.cmp, p.thr);  // NaN dropped: vec_compute.rs:237
                if (pass) {
                    unsigned long long key = ((unsigned long long)ord_of(s, take_max) << 32) | (uint32_t)(~(uint32_t)my_row);
                    unsigned long long* slot = p.table + (size_t)(p.q0 + q) * p.m * p.n_groups + g;  // level 0; level j is j planes on
                    // the loads go past this CU's vector L1 (agent scope); a stale value is a smaller one (slots only rise)
                    if (key > __hip_atomic_load(slot + (size_t)(p.m - 1) * p.n_groups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        for (uint32_t j = 0; j < p.m; j++, slot += p.n_groups) {
                            if (key > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                                const unsigned long long old = atomicMax(slot, key);
                                if (old < key) {  // the slot is this key's now: what it held walks on
                                    if (old == 0) break;
                                    key = old;
                                }
                            }
                        }
                    }
                }
            }
        }
    });
}

// One lane per winner.  winners[w]: a hit of GroupTopK::finish, index - base_offset < the rows the ids cover and query < nq
// (checked on the host).  hits: [n_winners][m] (a group's hits best first, the winner itself first); counts / groups: [n_winners].
__global__ __launch_bounds__(256) void group_emit_kernel(const unsigned long long* __restrict__ table, const uint32_t* __restrict__ gid,
                                                         const ott_hit* __restrict__ winners, uint64_t n_winners, uint32_t m, uint32_t n_groups,
                                                         uint64_t base_offset, uint32_t take_max, ott_hit* __restrict__ hits, uint32_t* __restrict__ counts,
                                                         uint32_t* __restrict__ groups) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_winners) return;
    const ott_hit win = winners[w];
    const uint32_t g = gid[win.index - base_offset];
    const unsigned long long* slot = table + (size_t)win.query * m * n_groups + g;
    ott_hit* dst = hits + w * m;
    dst[0] = win;
    uint32_t c = 1;
    for (uint32_t j = 1; j < m; j++) {
        const unsigned long long key = slot[(size_t)j * n_groups];
        if (key == 0) break;  // the levels fill from the top: nothing lies below an empty slot
        ott_hit h;
        h.index = (uint64_t)(uint32_t)(~(uint32_t)key) + base_offset;
        h.score = score_of((uint32_t)(key >> 32), take_max != 0);
        h.query = win.query;
        dst[c++] = h;
    }
    counts[w] = c;
    groups[w] = g;
}

namespace {

// The winners' groups read back out of the deeper planes, and the table zeroed behind it.  `win`: per query in query order, best
// first, `per[q]` of them.  Hits, counts and group ids go to the caller's buffers.
int emit_groups(ott_store* s, const GroupTopParams& p, const std::vector<ott_hit>& win, const std::vector<uint64_t>& per, size_t table_bytes, ott_hit* out,
                uint64_t* n_out, uint64_t* n_per_query, uint32_t* group_of_hit) {
    int rc;
    const uint64_t W = win.size();
    const uint32_t m = p.m;
    size_t off_hits = 0, off_cnt = 0, off_grp = 0, blk = 0;
    if (W) {
        if ((rc = s->h_stage.ensure((size_t)W * sizeof(ott_hit)))) return rc;
        for (uint64_t i = 0; i < W; i++)
            if (win[i].index - s->base_offset >= s->gid_n || win[i].query >= p.nq_total) return fail(OTT_ERR_INVALID, "ott_query_groups_top: a winner outside the store's rows");
        memcpy(s->h_stage.p, win.data(), (size_t)W * sizeof(ott_hit));
        // device: [winners | hits (W x m) | counts (W) | groups (W)]; the last three are the block the host copies
        off_hits = (size_t)W * sizeof(ott_hit);
        off_cnt = off_hits + (size_t)W * m * sizeof(ott_hit);
        off_grp = off_cnt + (size_t)W * 4;
        blk = off_grp + (size_t)W * 4 - off_hits;
        if ((rc = s->d_gather.ensure(off_hits + blk))) return rc;
        if ((rc = s->h_hits.ensure(blk))) return rc;
        char* dg = (char*)s->d_gather.p;
        OTT_HIP(hipMemcpyAsync(dg, s->h_stage.p, (size_t)W * sizeof(ott_hit), hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(group_emit_kernel, dim3((uint32_t)((W + 255) / 256)), dim3(256), 0, s->stream, (const unsigned long long*)p.table, p.gid, (const ott_hit*)dg, W, m,
                           p.n_groups, s->base_offset, p.take_max, (ott_hit*)(dg + off_hits), (uint32_t*)(dg + off_cnt), (uint32_t*)(dg + off_grp));
        OTT_HIP(hipGetLastError());
        OTT_HIP(hipMemcpyAsync(s->h_hits.p, dg + off_hits, blk, hipMemcpyDeviceToHost, s->stream));
    }
    OTT_HIP(hipMemsetAsync(p.table, 0, table_bytes, s->stream));  // the deeper planes, non-winners' too (plane 0 is zero already)
    OTT_HIP(hipStreamSynchronize(s->stream));
    s->gtable_clean = true;
    const char* hb = (const char*)s->h_hits.p;
    const ott_hit* hits = (const ott_hit*)hb;
    const uint32_t* counts = (const uint32_t*)(hb + (off_cnt - off_hits));
    const uint32_t* groups = (const uint32_t*)(hb + (off_grp - off_hits));
    uint64_t total = 0, w = 0;
    for (uint32_t q = 0; q < p.nq_total; q++) {
        uint64_t nq_hits = 0;
        for (uint64_t r = 0; r < per[q]; r++, w++) {
            const uint32_t c = counts[w] < m ? counts[w] : m;
            memcpy(out + total, hits + w * m, (size_t)c * sizeof(ott_hit));
            if (group_of_hit)
                for (uint32_t i = 0; i < c; i++) group_of_hit[total + i] = groups[w];
            total += c;
            nq_hits += c;
        }
        if (n_per_query) n_per_query[q] = nq_hits;
    }
    if (n_out) *n_out = total;
    return OTT_OK;
}

// The query on a context whose `mu` the caller holds (and the owner's `rw`, shared).  m >= 2, k_eff = min(k, n_groups) >= 1.
int run_groups_top(ott_store* s, const ott_query_desc* d, uint32_t m, uint64_t k_eff, ott_hit* out, uint64_t* n_out, uint64_t* n_per_query, uint32_t* group_of_hit,
                   ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint64_t t0 = now_ns();
    ott_stats st;
    const uint32_t nq = d->nq, ng = s->n_groups;
    GroupTopParams p{};
    uint32_t grid = 0;
    if ((rc = sweep_prologue(s, d, &st, &p, &grid))) return rc;
    if (grid != 0) {
        const size_t table_bytes = (size_t)nq * m * ng * 8;
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, table_bytes))) return rc;
        p.table = (unsigned long long*)s->d_gtable.p;
        p.n_groups = ng;
        p.m = m;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;

        GroupTopK tk;
        tk.n_groups = ng;
        tk.nq = nq;
        tk.k = k_eff;
        tk.take_max = p.take_max != 0;
        tk.q_stride = (uint64_t)m * ng;
        if ((rc = tk.prepare(s, nullptr))) return rc;  // (nq x n_groups pairs stay below 2^27: the table's 2 GiB)
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        const uint32_t tile = nq == 1 ? 1u : SW_NQ;
        for (uint32_t ps = 0; ps < st.passes; ps++) {
            p.q0 = ps * tile;
            if ((rc = launch_sweep(s->stream, p, tile, grid, OTT_SWEEP_KERNEL(group_top_sweep_kernel)))) return rc;
            if ((rc = tk.pass(s, p.table + (size_t)p.q0 * m * ng, p.q0, (nq - p.q0) < tile ? (nq - p.q0) : tile))) return rc;
        }
        if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
        std::vector<ott_hit> win((size_t)nq * k_eff);
        std::vector<uint64_t> per(nq, 0);
        uint64_t n_win = 0;
        rc = tk.finish(s, timing, win.data(), &n_win, per.data());
        s->gtable_clean = false;  // plane 0 is zero, the deeper planes are not yet
        if (rc) return rc;
        if (timing) read_exact_events(s, &st);
        win.resize(n_win);
        if ((rc = emit_groups(s, p, win, per, table_bytes, out, n_out, n_per_query, group_of_hit))) return rc;
    }
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_groups_top(ott_store* s, const ott_query_desc* d, uint32_t group_size, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                         uint32_t* group_of_hit, ott_stats* stats) {
    int rc = validate_query(s, d);
    if (rc) return rc;
    if (group_size == 0 || group_size > OTT_GROUP_SIZE_MAX)
        return fail(OTT_ERR_INVALID, "ott_query_groups_top: group_size is " + std::to_string(group_size) + ", it must be 1 .. " + std::to_string(OTT_GROUP_SIZE_MAX));
    if (d->mode == OTT_MODE_MERGED && d->nq > 1)
        return fail(OTT_ERR_UNSUPPORTED, "ott_query_groups_top: a merged list over several queries is not served (the best hits per group across queries); use PER_QUERY");
    if (d->path == OTT_PATH_MFMA) return fail(OTT_ERR_UNSUPPORTED, "ott_query_groups_top: the MFMA path does not serve grouped queries; use path AUTO or EXACT");
    if (s->multi)
        return fail(OTT_ERR_UNSUPPORTED,
                    "ott_query_groups_top: a multi-GPU store is not served (a group's second-best row may sit in a shard where the group is not among that shard's top-k "
                    "groups: shard lists of k groups do not suffice)");
    if (n_out) *n_out = 0;
    if (n_per_query)
        for (uint32_t i = 0; i < d->nq; i++) n_per_query[i] = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if ((rc = check_group_ids(s, "ott_query_groups_top", false))) return rc;
    const auto table_fits = [&](uint32_t n_groups) { return group_size == 1 || (uint64_t)d->nq * group_size * n_groups * 8 <= GT_TABLE_MAX; };
    const char* too_big = "ott_query_groups_top: queries x group_size x groups x 8 bytes is above 2 GiB (the key table holds every query's slots at once); use fewer queries "
                          "or a smaller group_size";
    if (!table_fits(s->n_groups)) return fail(OTT_ERR_UNSUPPORTED, too_big);
    ott::host::SharedLock rd;  // the corpus and the group ids cannot change while this query runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    // what the checks above read without the lock is read again, and k_eff only here: a set_groups may have come in between
    if ((rc = check_group_ids(s, "ott_query_groups_top", true))) return rc;
    if (!table_fits(s->n_groups)) return fail(OTT_ERR_UNSUPPORTED, too_big);
    const uint64_t k_eff = d->k < s->n_groups ? d->k : s->n_groups;
    if (cap < k_eff * d->nq * group_size) return fail(OTT_ERR_INVALID, "ott_query_groups_top: output capacity is smaller than nq * min(k, n_groups) * group_size");
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_groups_top: out is NULL");
    if (k_eff == 0) return OTT_OK;
    uint64_t total = 0;
    {
        CtxLease ctx(s);
        if (group_size == 1) rc = run_groups(ctx.c, d, k_eff, out, &total, n_per_query, stats);
        else rc = run_groups_top(ctx.c, d, group_size, k_eff, out, &total, n_per_query, group_of_hit, stats);
    }
    if (rc) return rc;
    if (n_out) *n_out = total;
    if (group_size == 1 && group_of_hit) return group_ids_of_hits(s, out, total, group_of_hit);  // the existing gather (the store is still held shared)
    return OTT_OK;
}

}  // extern "C"
