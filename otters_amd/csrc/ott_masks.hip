// ott_masks.hip — batch search with a row mask per query: ott_query_masks answers N requests that each bring their
// own metadata filter.  Query b's hits are exactly ott_query's for that query alone with the descriptor's own mask ANDed with mask
// mask_of_query[b].  Two routes, the same bits (host decisions: ott_masks_plan.h):
//
//   by mask group           the definition, and what serves everything: under the one shared lock, one PER_QUERY run of ott_query's
//                           internals (query_on) per distinct mask id with all of that mask's queries; the mask joins where every
//                           row mask reaches the kernels (compose_row_mask: cur_qmask, the route cur_idmask takes).  Tie orders 1
//                           and 2, Path.Mfma, any k; a multi-GPU store with host masks.
//   the masks sweep         canonical tie order, path AUTO / EXACT, a single-GPU store: the queries ordered stably by mask id, four
//                           per pass.
//     masks_union_kernel    per pass: union[w] = common[w] & (m0[w] | m1[w] | m2[w] | m3[w]) into ONE buffer reused pass after pass
//                           (stream order makes that safe); a query without a mask, and rows at or beyond a mask's bit count,
//                           contribute ones.  It is the row mask sweep_tiles sees: a tile in which no query of the pass has a
//                           surviving row is never read.  The same kernel with one mask is the by-mask-group route's join.
//     masks_sweep_kernel    sweep_tiles (ott_sweep_dev.h) and this epilogue per (row, query of the pass): the query's own mask bit (a
//                           per-lane load), NaN drop, cmp_holds, key = ord(score) << 32 | ~row, a PLAIN store to table[q][row] — a
//                           (query, row) pair has one writer.  The table is d_gtable under its zero-when-found protocol.
//     GroupTopK             grouped search's top-k over the table with n_groups = rows: pass() after every sweep, finish() once —
//                           one host wait for the whole batch.
//
// Device mask slots (ott_store_eval_row_mask_slot, ott_store_write_row_mask_slot, ott_store_clear_row_mask_slots): OTT_MASK_SLOTS
// masks resident beside the single mask of ott_store_eval_row_mask, so a filter the GPU evaluated is used in place.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_sweep_dev.h"

namespace ott {

static_assert(MASKS_NQ == SW_NQ, "the plan's passes are the sweep's");
static_assert(MASKS_NO_MASK == OTT_NO_MASK && MASKS_SLOT_BASE == OTT_MASK_SLOT_BASE && MASKS_SLOTS == OTT_MASK_SLOTS && MASKS_MAX_QUERIES == OTT_MASKS_MAX_QUERIES,
              "ott_masks_plan.h restates the header's constants");

struct MasksParams : SweepParams {
    unsigned long long* table;        // [NQ][n_rows] candidate key per (query of the pass, row); 0 = empty
    uint64_t n_rows;
    const uint64_t* qmask[SW_NQ];     // the own mask of every query of the pass, nullptr = none
    uint64_t qmask_bits[SW_NQ];       // the rows it covers (its words: (bits + 63) / 64); rows at and beyond are kept
    uint32_t cmp;
    float thr;
};

template <int MK, int NQ>
__global__ __launch_bounds__(64 * SW_WAVES) void masks_sweep_kernel(MasksParams p) {
    const bool take_max = p.take_max != 0;
    // `valid`: the row survived the pass's union mask (and the tile's end); my_row < n_rows then
    sweep_tiles<MK, NQ>(p, [&](uint64_t my_row, bool valid, uint32_t, const float (&sc)[NQ], uint32_t nq_here) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            if ((uint32_t)q < nq_here) {
                const uint64_t* m = p.qmask[q];
                bool own = valid;
                if (own && m != nullptr && my_row < p.qmask_bits[q]) own = (m[my_row >> 6] >> (my_row & 63)) & 1;  // src/vec.rs:231-237
                const float s = sc[q];
                if (own && !(s != s) && cmp_holds(s, p.cmp, p.thr))  // NaN dropped: vec_compute.rs:237
                    p.table[(size_t)q * p.n_rows + my_row] = ((unsigned long long)ord_of(s, take_max) << 32) | (uint32_t)(~(uint32_t)my_row);
            }
        }
    });
}

struct UnionParams {
    const uint64_t* common;  // nullptr = all ones
    uint64_t common_bits;
    const uint64_t* m[SW_NQ];
    uint64_t bits[SW_NQ];
    uint32_t n_masks;        // 1 .. SW_NQ, none of them nullptr
    uint64_t n_words;
    uint64_t* out;
};

// word w of a mask of `bits` rows with every bit at and beyond `bits` set (ott_masks_plan.h: masks_word_ext); never reads past
// the mask's (bits + 63) / 64 words
__device__ __forceinline__ uint64_t mask_word_ext(const uint64_t* words, uint64_t bits, uint64_t w) {
    if (words == nullptr || w * 64 >= bits) return ~0ull;
    uint64_t x = words[w];
    if (bits - w * 64 < 64) x |= ~0ull << (bits - w * 64);
    return x;
}

__global__ __launch_bounds__(256) void masks_union_kernel(UnionParams p) {
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < p.n_words; w += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t any = 0;
#pragma unroll
        for (int i = 0; i < (int)SW_NQ; i++)
            if ((uint32_t)i < p.n_masks) any |= mask_word_ext(p.m[i], p.bits[i], w);
        p.out[w] = mask_word_ext(p.common, p.common_bits, w) & any;
    }
}

namespace {

int launch_union(ott_store* s, const UnionParams& u) {
    hipLaunchKernelGGL(masks_union_kernel, dim3(grid_blocks(u.n_words, 256, s->n_cu)), dim3(256), 0, s->stream, u);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// where the masks of one call are once they are on the device: host mask i in the context's scratch, slot masks in place
struct MaskTable {
    const uint64_t* host0 = nullptr;  // the first uploaded host mask
    uint64_t host_words = 0, host_bits = 0;
    const ott_store* own = nullptr;   // whose slots
    void of(uint32_t id, const uint64_t** words, uint64_t* bits) const {
        *words = nullptr;
        *bits = 0;
        if (id == MASKS_NO_MASK) return;
        if (masks_is_slot(id)) {
            *words = (const uint64_t*)own->d_mslot[id - MASKS_SLOT_BASE].p;
            *bits = own->mslot_bits[id - MASKS_SLOT_BASE];
        } else if (host_bits) {  // (a host mask of 0 bits keeps every row: no mask)
            *words = host0 + (size_t)id * host_words;
            *bits = host_bits;
        }
        if (*bits == 0) *words = nullptr;
    }
};

// the context's scratch of one call ([join | union | host masks]) and the ONE upload of the host masks
int upload_masks(ott_store* ctx, const uint64_t* masks, uint32_t n_masks, uint64_t mask_bits, MaskTable& mt) {
    int rc;
    const uint64_t words_n = masks_words(ctx->n);
    if ((rc = ctx->d_qmasks.ensure((size_t)masks_scratch_bytes(ctx->n, n_masks, mask_bits)))) return rc;
    mt.own = ctx->owner ? ctx->owner : ctx;
    mt.host_words = masks_words(mask_bits);
    mt.host_bits = mask_bits;
    mt.host0 = (const uint64_t*)ctx->d_qmasks.p + 2 * words_n;
    if (n_masks && mt.host_words)
        OTT_HIP(hipMemcpyAsync((void*)mt.host0, masks, (size_t)n_masks * mt.host_words * 8, hipMemcpyHostToDevice, ctx->stream));
    return OTT_OK;
}

// The by-mask-group route on a context whose `mu` the caller holds (and the owner's `rw`, shared): one query_on per distinct mask
// id with all of its queries; res[b] = the caller's query b's hits.
int run_by_group(ott_store* ctx, const ott_query_desc* d, const uint32_t* moq, const MasksPlan& pl, const MaskTable& mt, uint64_t k_eff,
                 std::vector<std::vector<ott_hit>>& res, ott_stats* sum) {
    int rc;
    struct QMaskGuard {
        ott_store* c;
        ~QMaskGuard() { c->cur_qmask = nullptr; c->cur_qmask_bits = 0; }
    } guard{ctx};
    const uint32_t dim = ctx->dim;
    std::vector<float> qbuf;
    std::vector<ott_hit> tmp;
    std::vector<uint64_t> per;
    for (uint32_t g = 0; g < pl.n_distinct; g++) {
        const uint32_t lo = pl.group_start[g], ng = pl.group_start[g + 1] - lo;
        qbuf.resize((size_t)ng * dim);
        for (uint32_t i = 0; i < ng; i++) memcpy(qbuf.data() + (size_t)i * dim, d->queries + (size_t)pl.order[lo + i] * dim, (size_t)dim * 4);
        ott_query_desc dg = *d;
        dg.queries = qbuf.data();
        dg.nq = ng;
        mt.of(moq[pl.order[lo]], &ctx->cur_qmask, &ctx->cur_qmask_bits);
        tmp.resize((size_t)ng * k_eff);
        per.assign(ng, 0);
        uint64_t n_g = 0;
        ott_stats sg;
        memset(&sg, 0, sizeof(sg));
        if ((rc = query_on(ctx, &dg, tmp.data(), nullptr, tmp.size(), &n_g, per.data(), nullptr, sum ? &sg : nullptr))) return rc;
        uint64_t at = 0;
        for (uint32_t i = 0; i < ng; i++) {
            const uint32_t b = pl.order[lo + i];
            res[b].assign(tmp.begin() + at, tmp.begin() + at + per[i]);
            for (ott_hit& h : res[b]) h.query = b;
            at += per[i];
        }
        if (sum) {
            sum->total_chunks = sg.total_chunks;
            sum->evaluated_chunks = sg.evaluated_chunks;
            sum->pruned_chunks = sg.pruned_chunks;
            sum->path_used = sg.path_used;
            sum->passes += sg.passes;
            sum->vectors_compared += sg.vectors_compared;
            sum->bytes_scanned += sg.bytes_scanned;
            sum->score_ns += sg.score_ns;
            sum->merge_ns += sg.merge_ns;
            sum->rescored += sg.rescored;
            sum->retries += sg.retries;
        }
    }
    return OTT_OK;
}

// The masks sweep on a context whose `mu` the caller holds.  k_eff = min(k, rows the chunk mask leaves) >= 1.
int run_masks_sweep(ott_store* s, const ott_query_desc* d, const uint32_t* moq, const MasksPlan& pl, const MaskTable& mt, uint64_t k_eff,
                    std::vector<std::vector<ott_hit>>& res, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const uint32_t nq = d->nq, dim = s->dim;
    const uint64_t n = s->n;
    // the queries in the plan's order: position i of the block is the caller's query order[i]
    std::vector<float> qbuf((size_t)nq * dim);
    for (uint32_t i = 0; i < nq; i++) memcpy(qbuf.data() + (size_t)i * dim, d->queries + (size_t)pl.order[i] * dim, (size_t)dim * 4);
    ott_stats st;
    MasksParams p{};
    uint32_t grid = 0;
    // (the descriptor's own mask — caller's or evaluated, live mask — is composed here: the COMMON mask of every pass)
    if ((rc = sweep_prologue(s, d, qbuf.data(), nq, &st, &p, &grid))) return rc;
    if (grid != 0) {
        p.gid = nullptr;  // no group ids are read
        const uint64_t* common = p.row_mask;
        const uint64_t common_bits = p.row_mask_bits;
        const uint32_t tile = nq == 1 ? 1u : SW_NQ;
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)tile * n * 8))) return rc;
        p.table = (unsigned long long*)s->d_gtable.p;
        p.n_rows = n;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;
        uint64_t* d_union = (uint64_t*)s->d_qmasks.p + masks_words(n);

        GroupTopK tk;
        tk.n_groups = (uint32_t)n;  // (n < 2^32 - 16: masks_sweep_eligible)
        tk.nq = nq;
        tk.k = k_eff;
        tk.take_max = p.take_max != 0;
        if ((rc = tk.prepare(s, nullptr))) return rc;
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        for (uint32_t ps = 0; ps < pl.passes; ps++) {
            p.q0 = ps * tile;
            const uint32_t nq_here = (nq - p.q0) < tile ? (nq - p.q0) : tile;
            UnionParams u{};
            bool every_query_masked = true;
            for (uint32_t q = 0; q < SW_NQ; q++) {
                p.qmask[q] = nullptr;
                p.qmask_bits[q] = 0;
                if (q < nq_here) {
                    mt.of(moq[pl.order[p.q0 + q]], &p.qmask[q], &p.qmask_bits[q]);
                    if (p.qmask[q] == nullptr) every_query_masked = false;
                    u.m[u.n_masks] = p.qmask[q];
                    u.bits[u.n_masks] = p.qmask_bits[q];
                    u.n_masks += p.qmask[q] != nullptr;
                }
            }
            if (every_query_masked) {  // the pass's union; a query without a mask makes it the common mask itself
                u.common = common;
                u.common_bits = common_bits;
                u.n_words = masks_words(n);
                u.out = d_union;
                if ((rc = launch_union(s, u))) return rc;
                p.row_mask = d_union;
                p.row_mask_bits = n;
            } else {
                p.row_mask = common;
                p.row_mask_bits = common_bits;
            }
            if ((rc = launch_sweep(s->stream, p, tile, grid, OTT_SWEEP_KERNEL(masks_sweep_kernel)))) return rc;
            if ((rc = tk.pass(s, p.table, p.q0, nq_here))) return rc;
        }
        if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
        std::vector<ott_hit> tmp((size_t)nq * k_eff);
        std::vector<uint64_t> per(nq, 0);
        uint64_t total = 0;
        if ((rc = tk.finish(s, timing, tmp.data(), &total, per.data()))) return rc;
        if (timing) read_exact_events(s, &st);
        uint64_t at = 0;
        for (uint32_t i = 0; i < nq; i++) {  // back to the caller's order
            const uint32_t b = pl.order[i];
            res[b].assign(tmp.begin() + at, tmp.begin() + at + per[i]);
            for (ott_hit& h : res[b]) h.query = b;
            at += per[i];
        }
        st.passes = pl.passes;
        st.bytes_scanned = (uint64_t)pl.passes * (st.vectors_compared / nq) * ((uint64_t)dim * 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));
    }
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

// A multi-GPU store: by mask group with HOST masks — the group's mask ANDed with the caller's host mask over the store's rows,
// then ott_query's own fan-out (the shards slice the mask like any other).
int multi_query_masks(ott_store* ms, const ott_query_desc* d, const uint64_t* masks, uint64_t mask_bits, const uint32_t* moq, const MasksPlan& pl,
                      std::vector<std::vector<ott_hit>>& res, ott_stats* sum) {
    int rc;
    const uint64_t n = ott_store_len(ms), words_n = masks_words(n), host_words = masks_words(mask_bits);
    const uint64_t k_eff = d->k < n ? d->k : n;
    std::vector<float> qbuf;
    std::vector<ott_hit> tmp;
    std::vector<uint64_t> per, joined;
    for (uint32_t g = 0; g < pl.n_distinct; g++) {
        const uint32_t lo = pl.group_start[g], ng = pl.group_start[g + 1] - lo, id = moq[pl.order[lo]];
        qbuf.resize((size_t)ng * ms->dim);
        for (uint32_t i = 0; i < ng; i++) memcpy(qbuf.data() + (size_t)i * ms->dim, d->queries + (size_t)pl.order[lo + i] * ms->dim, (size_t)ms->dim * 4);
        ott_query_desc dg = *d;
        dg.queries = qbuf.data();
        dg.nq = ng;
        if (id != MASKS_NO_MASK && mask_bits) {
            const uint64_t* own = masks + (size_t)id * host_words;
            const uint64_t* common = (d->row_mask && d->row_mask_bits) ? d->row_mask : nullptr;
            joined.resize((size_t)words_n + 1);
            for (uint64_t w = 0; w < words_n; w++) joined[(size_t)w] = masks_word_ext(common, d->row_mask_bits, w) & masks_word_ext(own, mask_bits, w);
            dg.row_mask = joined.data();
            dg.row_mask_bits = n;
        }
        tmp.resize((size_t)ng * k_eff + 1);
        per.assign(ng, 0);
        uint64_t n_g = 0;
        ott_stats sg;
        memset(&sg, 0, sizeof(sg));
        if ((rc = multi_query(ms, &dg, tmp.data(), (uint64_t)ng * k_eff, &n_g, per.data(), sum ? &sg : nullptr))) return rc;
        uint64_t at = 0;
        for (uint32_t i = 0; i < ng; i++) {
            const uint32_t b = pl.order[lo + i];
            res[b].assign(tmp.begin() + at, tmp.begin() + at + per[i]);
            for (ott_hit& h : res[b]) h.query = b;
            at += per[i];
        }
        if (sum) {
            sum->total_chunks = sg.total_chunks;
            sum->evaluated_chunks = sg.evaluated_chunks;
            sum->pruned_chunks = sg.pruned_chunks;
            sum->path_used = sg.path_used;
            sum->passes += sg.passes;
            sum->vectors_compared += sg.vectors_compared;
            sum->bytes_scanned += sg.bytes_scanned;
            sum->score_ns += sg.score_ns;
            sum->merge_ns += sg.merge_ns;
            sum->exchange_ns += sg.exchange_ns;
        }
    }
    return OTT_OK;
}

int refuse(MasksRefusal r, uint32_t nq, const uint32_t* moq, uint32_t n_masks, uint32_t bad) {
    const std::string name = "ott_query_masks: ";
    switch (r) {
        case MASKS_NO_QUERIES: return fail(OTT_ERR_INVALID, "No queries provided");  // src/vec.rs:188-190
        case MASKS_TOO_MANY: return fail(OTT_ERR_INVALID, name + std::to_string(nq) + " queries are above OTT_MASKS_MAX_QUERIES (" + std::to_string(MASKS_MAX_QUERIES) + ")");
        case MASKS_MERGED: return fail(OTT_ERR_INVALID, name + "a row mask per query needs OTT_MODE_PER_QUERY (a merged list over differently masked queries is not served)");
        case MASKS_NULL_MAP: return fail(OTT_ERR_INVALID, name + "mask_of_query is NULL");
        case MASKS_NULL_MASKS: return fail(OTT_ERR_INVALID, name + "masks is NULL");
        case MASKS_BAD_INDEX:
            return fail(OTT_ERR_INVALID, name + "query " + std::to_string(bad) + ": mask " + std::to_string(moq[bad]) + " is out of range (the call brings " + std::to_string(n_masks) +
                                             " masks) and is neither a slot reference nor OTT_NO_MASK");
        case MASKS_BAD_SLOT:
            return fail(OTT_ERR_INVALID, name + "query " + std::to_string(bad) + ": slot " + std::to_string(moq[bad] - MASKS_SLOT_BASE) + " is not below OTT_MASK_SLOTS (" +
                                             std::to_string(MASKS_SLOTS) + ")");
        case MASKS_EMPTY_SLOT:
            return fail(OTT_ERR_INVALID, name + "query " + std::to_string(bad) + ": slot " + std::to_string(moq[bad] - MASKS_SLOT_BASE) +
                                             " was never filled, or was dropped when the rows moved (ott_store_eval_row_mask_slot, ott_store_write_row_mask_slot)");
        default: return OTT_OK;
    }
}

int slot_check(ott_store* s, uint32_t slot, const char* fn) {
    const std::string name(fn);
    if (!s) return fail(OTT_ERR_INVALID, name + ": store is NULL");
    if (slot >= OTT_MASK_SLOTS) return fail(OTT_ERR_INVALID, name + ": slot " + std::to_string(slot) + " is not below OTT_MASK_SLOTS (" + std::to_string(OTT_MASK_SLOTS) + ")");
    if (s->multi) return fail(OTT_ERR_UNSUPPORTED, name + ": device mask slots are not served on a multi-GPU store; send host masks (ott_query_masks)");
    return OTT_OK;
}

}  // namespace

int masks_join(ott_store* s, const uint64_t** d_mask, uint64_t* mask_bits) {
    if (*d_mask == nullptr) {  // the group's mask is the only one
        *d_mask = s->cur_qmask;
        *mask_bits = s->cur_qmask_bits;
        return OTT_OK;
    }
    int rc;
    const uint64_t words_n = masks_words(s->n);
    if (s->d_qmasks.cap < words_n * 8) return fail(OTT_ERR_INVALID, "ott_query_masks: the call's scratch is smaller than a row mask");  // (upload_masks sized it)
    UnionParams u{};
    u.common = *d_mask;
    u.common_bits = *mask_bits;
    u.m[0] = s->cur_qmask;
    u.bits[0] = s->cur_qmask_bits;
    u.n_masks = 1;
    u.n_words = words_n;
    u.out = (uint64_t*)s->d_qmasks.p;
    if ((rc = launch_union(s, u))) return rc;
    *d_mask = u.out;
    *mask_bits = s->n;
    return OTT_OK;
}

void mask_slots_drop(ott_store* s) {
    for (uint32_t i = 0; i < OTT_MASK_SLOTS; i++) {
        s->mslot_bits[i] = 0;
        s->d_mslot[i].release();
    }
}

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_masks(ott_store* s, const ott_query_desc* d, const uint64_t* masks, uint32_t n_masks, uint64_t mask_bits, const void* mask_of_query, ott_hit* out,
                    uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats) {
    const uint32_t* moq = (const uint32_t*)mask_of_query;
    if (!d) return fail(OTT_ERR_INVALID, "ott_query_masks: desc is NULL");
    // what the arguments alone decide comes first: these refusals need no store
    uint32_t bad = 0;
    const MasksRefusal r = masks_check_args(d->nq, d->mode == OTT_MODE_PER_QUERY, moq, masks == nullptr, n_masks, &bad);
    if (r != MASKS_OK) return refuse(r, d->nq, moq, n_masks, bad);
    if (!s) return fail(OTT_ERR_INVALID, "ott_query_masks: store is NULL");
    int rc = validate_query(s, d);
    if (rc) return rc;
    const uint32_t nq = d->nq;
    MasksPlan pl;
    masks_plan_build(moq, nq, pl);
    std::vector<std::vector<ott_hit>> res(nq);
    ott_stats st;
    memset(&st, 0, sizeof(st));
    const uint64_t t0 = now_ns();
    const auto emit = [&]() -> int {  // the lists back to back in the caller's order
        uint64_t total = 0;
        for (uint32_t b = 0; b < nq; b++) {
            if (!res[b].empty()) memcpy(out + total, res[b].data(), res[b].size() * sizeof(ott_hit));
            if (n_per_query) n_per_query[b] = res[b].size();
            total += res[b].size();
        }
        if (n_out) *n_out = total;
        st.total_ns = now_ns() - t0;
        if (stats) *stats = st;
        return OTT_OK;
    };
    const auto zero_outputs = [&] {
        if (n_out) *n_out = 0;
        if (n_per_query) memset(n_per_query, 0, (size_t)nq * sizeof(uint64_t));
        if (stats) memset(stats, 0, sizeof(*stats));
    };

    if (s->multi) {
        for (uint32_t b = 0; b < nq; b++)
            if (masks_is_slot(moq[b])) return refuse(MASKS_EMPTY_SLOT, nq, moq, n_masks, b);  // (a multi-GPU store has no slots: none was ever filled)
        bool any_mask = false;
        for (uint32_t b = 0; b < nq; b++) any_mask |= moq[b] != MASKS_NO_MASK;
        if (d->use_device_row_mask && any_mask && mask_bits)
            return fail(OTT_ERR_UNSUPPORTED, "ott_query_masks: on a multi-GPU store the evaluated device mask cannot be joined with a mask per query; send the common mask as row_mask");
        const uint64_t n = ott_store_len(s), k_eff = d->k < n ? d->k : n;
        if (cap < k_eff * nq) return fail(OTT_ERR_INVALID, "ott_query_masks: output capacity is smaller than nq * min(k, rows)");
        if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_masks: out is NULL");
        zero_outputs();
        if (k_eff == 0) return OTT_OK;
        if ((rc = multi_query_masks(s, d, masks, mask_bits, moq, pl, res, stats ? &st : nullptr))) return rc;
        return emit();
    }

    ott::host::SharedLock rd;  // the corpus and the slots cannot change while the batch runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    const MasksRefusal rs = masks_check_slots(nq, moq, s->mslot_bits, &bad);
    if (rs != MASKS_OK) return refuse(rs, nq, moq, n_masks, bad);
    RunPlan rp;
    make_run_plan(s, d->chunk_mask, rp);
    const uint64_t k_eff = d->k < rp.rows_scored ? d->k : rp.rows_scored;  // ott_query's PER_QUERY rule: a list never outgrows the pool
    if (cap < k_eff * nq) return fail(OTT_ERR_INVALID, "ott_query_masks: output capacity is smaller than nq * min(k, rows)");
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_masks: out is NULL");
    zero_outputs();
    if (k_eff == 0) return OTT_OK;  // k == 0 or nothing to score: a valid batch with no hits

    const bool eligible = masks_sweep_eligible(s->opt.tie_order, d->path, false, s->n, k_eff, nq);
    const bool sweep = masks_takes_sweep(s->opt.masks_sweep, eligible, s->n, s->dim, nq, pl.n_distinct, pl.largest_group);
    {
        CtxLease lease(s);
        ott_store* ctx = lease.c;
        rc = [&]() -> int {
            int r2;
            OTT_HIP(use_device(ctx));
            MaskTable mt;
            if ((r2 = upload_masks(ctx, masks, n_masks, mask_bits, mt))) return r2;
            if (sweep) return run_masks_sweep(ctx, d, moq, pl, mt, k_eff, res, stats ? &st : nullptr);
            return run_by_group(ctx, d, moq, pl, mt, k_eff, res, stats ? &st : nullptr);
        }();
        // (the upload reads the caller's masks: nothing of this call is in flight when it returns, and the context is given back after that)
        if (rc) (void)hipStreamSynchronize(ctx->stream);
    }
    if (rc) return rc;
    return emit();
}

int ott_store_eval_row_mask_slot(ott_store* s, uint32_t slot, const ott_leaf* leaves, uint32_t n_leaves, uint32_t n_clauses, uint64_t* out_host) {
    int rc = slot_check(s, slot, "ott_store_eval_row_mask_slot");
    if (rc) return rc;
    if (n_leaves && !leaves) return fail(OTT_ERR_INVALID, "ott_store_eval_row_mask_slot: leaves is NULL");
    (void)n_clauses;
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    return eval_row_mask_into(s, "ott_store_eval_row_mask_slot", leaves, n_leaves, s->d_mslot[slot], &s->mslot_bits[slot], out_host);
}

int ott_store_write_row_mask_slot(ott_store* s, uint32_t slot, const uint64_t* bits, uint64_t n_bits) {
    int rc = slot_check(s, slot, "ott_store_write_row_mask_slot");
    if (rc) return rc;
    if (n_bits && !bits) return fail(OTT_ERR_INVALID, "ott_store_write_row_mask_slot: bits is NULL");
    ott::host::ExclusiveLock wr(s->rw);
    std::lock_guard<std::mutex> g(s->mu);
    OTT_HIP(use_device(s));
    if ((rc = store_flush_locked(s))) return rc;
    s->mslot_bits[slot] = 0;
    if (!n_bits) return OTT_OK;
    const size_t words = (size_t)masks_words(n_bits);
    if ((rc = s->d_mslot[slot].ensure(words * 8))) return rc;
    OTT_HIP(hipMemcpyAsync(s->d_mslot[slot].p, bits, words * 8, hipMemcpyHostToDevice, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    s->mslot_bits[slot] = n_bits;
    return OTT_OK;
}

int ott_store_clear_row_mask_slots(ott_store* s) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_clear_row_mask_slots: store is NULL");
    if (s->multi) return fail(OTT_ERR_UNSUPPORTED, "ott_store_clear_row_mask_slots: device mask slots are not served on a multi-GPU store");
    ott::host::ExclusiveLock wr(s->rw);
    std::lock_guard<std::mutex> g(s->mu);
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    mask_slots_drop(s);
    return OTT_OK;
}

}  // extern "C"
