// ott_discover.hip — discovery and context search (Qdrant's Discovery API): ott_query_discover ranks the store's rows
// by how many context pairs (positive row, negative row) they WIN — closer to the pair's positive than to its negative — and then by
// their closeness to a target (a vector or a stored row); without a target, by a loss that is zero where every pair is won and
// falls with every violated pair.  The examples are rows of the store, named by id: nothing of them crosses the host.
//
//   example_gather_kernel   (ott_recommend.hip, through ExampleFrame) the pairs' stored rows (slot 2i the positive, 2i + 1 the negative
//                           of pair i) and a target ROW's into the context's query block with their STORED inverse norms; a vector
//                           target went up with the block, with its host-side inverse norm (ott_query's).
//   discover_sweep_kernel   sweep_tiles (ott_sweep_dev.h: the bits are the oracle's) and this epilogue per row: slots (0, 1) and
//                           (2, 3) of a pass are whole pairs, or the target and nothing.  The row's 8-byte state {wins | flags,
//                           y} is loaded (not in the first pass: the table is zero when found), a won pair adds one to wins, and y
//                           is folded: without a target the loss so far (one __fsub_rn, one compare, one __fadd_rn per pair, in pair
//                           order because the passes are launches on one stream), with a target the target score's ordinal.  A NaN
//                           pair or target score sets the INVALID flag for good.  One streaming vector store; nothing is atomic.
//                           A row no lane ever wrote (masked, deleted, pruned chunk) keeps {0, 0}: SEEN tells a written row apart.
//   example_clear_kernel    (the same) the examples' and the target row's states back to {0, 0}: they are never candidates.
//   discover_keys_kernel    no target.  One lane per row: candidate -> key = ord_of(loss, Max) << 32 | ~row in the key table and its
//                           wins in a byte per row; the state is zeroed.  GroupTopK (one "group" per row) does the rest, and
//                           discover_wins_kernel, behind the merge, looks the hits' wins up before the host waits.
//   discover_count_kernel   with a target.  The candidates per wins level: an LDS histogram per workgroup, flushed once.
//   discover_select_kernel  derives the cut level L* from the counters (disc_level_cut: the highest level with
//                           count(wins >= L*) >= k_eff).  A candidate ON the level leaves ord(T) << 32 | ~row in the key table for
//                           GroupTopK asked for k_eff; one ABOVE it — fewer than k_eff by construction — is appended to a list of
//                           {wins, key} through a cursor.  The state is zeroed.  The counters and the list come back behind the
//                           top-k's one host wait; the host sorts the short list and appends the level's best hits.
// Resources: profiles/discover/resource_usage.txt (no scratch; the sweep keeps recommend_sweep_kernel's occupancy).
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_sweep_dev.h"

namespace ott {

static_assert(DISC_NQ == SW_NQ, "ott_discover_plan.h counts the passes of ott_sweep_dev.h's sweep");

constexpr uint32_t DISC_INVALID = 1u << 31;  // a NaN pair or target score was seen
constexpr uint32_t DISC_SEEN = 1u << 30;     // a lane wrote the state: the row passed the masks
constexpr uint32_t DISC_WINS = 0x3Fu;        // 0 .. 32

struct DiscoverParams : SweepParams {
    uint2* state;           // [n] {wins | flags, loss bits or target ordinal}; {0, 0} = never written
    uint32_t n_pair_slots;  // 2 * n_pairs
    uint32_t target_slot;   // 2 * n_pairs, or 0xFFFFFFFF: none
};

// what the kernels behind the sweep ask of a state
struct DiscoverPick {
    uint32_t min_wins, has_target, take_max, cmp;
    float thr;
};

template <int MK, int NQ>
__global__ __launch_bounds__(64 * SW_WAVES) void discover_sweep_kernel(DiscoverParams p) {
    static_assert(NQ % 2 == 0, "a pass holds whole pairs");
    const bool take_max = p.take_max != 0;
    const bool has_target = p.target_slot != 0xFFFFFFFFu;
    sweep_tiles<MK, NQ>(p, [&](uint64_t my_row, bool valid, uint32_t, const float (&sc)[NQ], uint32_t) {
        if (!valid) return;
        uint2* slot = p.state + my_row;
        uint32_t x = DISC_SEEN, y = 0u;  // (y: +0.0f, the loss's start, or no target ordinal yet)
        if (p.q0 != 0) {                 // (wave-uniform: the first pass finds the table zero)
            const uint2 cur = *slot;
            x = cur.x;
            y = cur.y;
        }
#pragma unroll
        for (int j = 0; j < NQ / 2; j++) {
            const uint32_t a = p.q0 + 2u * (uint32_t)j;  // (wave-uniform)
            const float sp = sc[2 * j], sn = sc[2 * j + 1];
            if (a == p.target_slot) {
                if (sp != sp) x |= DISC_INVALID;
                else y = ord_of(sp, take_max);
            } else if (a < p.n_pair_slots) {
                if (sp != sp || sn != sn) {
                    x |= DISC_INVALID;
                } else {
                    if (ord_of(sp, take_max) > ord_of(sn, take_max)) x += 1u;
                    if (!has_target) {
                        const float dlt = take_max ? __fsub_rn(sp, sn) : __fsub_rn(sn, sp);
                        const float t = dlt < 0.0f ? dlt : 0.0f;  // (a NaN from inf - inf counts 0)
                        y = __float_as_uint(__fadd_rn(__uint_as_float(y), t));
                    }
                }
            }
        }
        // streamed like the rows: nothing reads the slot again before the next launch (ott_recommend.hip)
        typedef unsigned int v2u __attribute__((ext_vector_type(2)));
        v2u v;
        v.x = x;
        v.y = y;
        __builtin_nontemporal_store(v, reinterpret_cast<v2u*>(slot));
    });
}

// candidate: written, no NaN, enough wins, the filter holds on the hit's score.  *wins, *o: its wins and its score's ordinal
__device__ __forceinline__ bool discover_candidate(uint2 st, const DiscoverPick& k, uint32_t* wins, uint32_t* o) {
    if ((st.x & DISC_SEEN) == 0 || (st.x & DISC_INVALID) != 0) return false;
    *wins = st.x & DISC_WINS;
    if (*wins < k.min_wins) return false;
    float score;
    if (k.has_target) {
        if (st.y == 0) return false;  // (no pass carried the target: cannot happen for a written row)
        *o = st.y;
        score = score_of(st.y, k.take_max != 0);
    } else {
        score = __uint_as_float(st.y);
        *o = ord_of(score, true);  // the loss ranks descending in the total order, whatever the take
    }
    return cmp_holds(score, k.cmp, k.thr);
}

// One lane per row, no target.  keys: [n] 8-byte keys, zero when the kernel starts (d_gtable's protocol).
__global__ __launch_bounds__(256) void discover_keys_kernel(uint2* state, uint32_t n, DiscoverPick k, unsigned long long* keys, uint8_t* wins8) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint2 st = state[r];
    if ((st.x | st.y) == 0) return;
    state[r] = make_uint2(0u, 0u);
    uint32_t w, o;
    if (!discover_candidate(st, k, &w, &o)) return;
    keys[r] = ((unsigned long long)o << 32) | (uint32_t)(~(uint32_t)r);
    wins8[r] = (uint8_t)w;
}

// Behind the merge kernel: hit i's wins, read through the device's view of the pinned hits.  counts[0] hits, at most k.
__global__ __launch_bounds__(256) void discover_wins_kernel(const ott_hit* hits, const uint64_t* counts, uint64_t k, uint64_t base, uint32_t n, const uint8_t* wins8,
                                                            uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t c = counts[0] < k ? counts[0] : k;
    if (i >= c) return;
    const uint64_t row = hits[i].index - base;
    out[i] = row < n ? wins8[row] : 0u;
}

// With a target: hist[w] += candidates with w wins.
__global__ __launch_bounds__(256) void discover_count_kernel(const uint2* state, uint32_t n, DiscoverPick k, uint32_t* hist) {
    __shared__ uint32_t s_hist[DISC_LEVELS];
    if (threadIdx.x < DISC_LEVELS) s_hist[threadIdx.x] = 0u;
    __syncthreads();
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 st = state[r];
        uint32_t w, o;
        if ((st.x | st.y) != 0 && discover_candidate(st, k, &w, &o) && w < DISC_LEVELS) atomicAdd(&s_hist[w], 1u);
    }
    __syncthreads();
    if (threadIdx.x < DISC_LEVELS && s_hist[threadIdx.x] != 0) atomicAdd(&hist[threadIdx.x], s_hist[threadIdx.x]);
}

// With a target: the level's keys into the table, the candidates above the level behind the cursor (hdr[DISC_HDR_CURSOR]); the
// counters hdr[0 .. n_levels) are complete (the count kernel ran before on the stream) and do not change here.
__global__ __launch_bounds__(256) void discover_select_kernel(uint2* state, uint32_t n, DiscoverPick k, uint32_t* hdr, uint32_t n_levels, uint64_t k_eff,
                                                              unsigned long long* keys, DiscAbove* list) {
    __shared__ uint32_t s_cut;
    if (threadIdx.x == 0) {
        uint64_t n_above;
        s_cut = disc_level_cut(hdr, n_levels, k_eff, &n_above);
    }
    __syncthreads();
    const uint32_t cut = s_cut;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 st = state[r];
        if ((st.x | st.y) == 0) continue;
        state[r] = make_uint2(0u, 0u);
        uint32_t w, o;
        if (!discover_candidate(st, k, &w, &o) || w < cut) continue;
        const unsigned long long key = ((unsigned long long)o << 32) | (uint32_t)(~(uint32_t)r);
        if (w == cut) {
            keys[r] = key;
        } else {
            const uint32_t at = atomicAdd(&hdr[DISC_HDR_CURSOR], 1u);
            if (at < k_eff) {  // (always: fewer than k_eff lie above the level)
                DiscAbove e;
                e.wins = w;
                e.pad = 0u;
                e.key = key;
                list[at] = e;
            }
        }
    }
}

namespace {

uint32_t row_blocks(const ott_store* s, uint32_t n) {
    uint32_t blocks = (uint32_t)(((uint64_t)n + 255) / 256);  // (in 64 bits: n + 255 wraps from 2^32 - 255 rows on, below the limit of 2^32 - 16)
    if (blocks > (uint32_t)s->n_cu * 8) blocks = (uint32_t)s->n_cu * 8;
    return blocks < 1 ? 1 : blocks;
}

struct WinsLookup {
    uint64_t k, base;
    uint32_t n;
    const uint8_t* wins8;
    uint32_t* out;  // the device's view of the pinned block
};

int launch_wins_lookup(ott_store* s, void* arg, const ott_hit* d_hits, const uint64_t* d_counts) {
    const WinsLookup* w = (const WinsLookup*)arg;
    hipLaunchKernelGGL(discover_wins_kernel, dim3((uint32_t)((w->k + 255) / 256)), dim3(256), 0, s->stream, d_hits, d_counts, w->k, w->base, w->n, w->wins8, w->out);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

const char* refusal_text(DiscRefusal r) {
    switch (r) {
        case DISC_BAD_PAIRS: return "ott_query_discover: between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed";
        case DISC_NULL_LIST: return "ott_query_discover: a pair list is NULL";
        case DISC_BAD_FLAGS: return "ott_query_discover: flags must be 0";
        case DISC_MANY_QUERIES: return "ott_query_discover: at most one target vector (d->nq <= 1)";
        case DISC_NULL_QUERY: return "ott_query_discover: d->queries and d->nq disagree (a target vector is d->queries with d->nq 1)";
        case DISC_BOTH_TARGETS: return "ott_query_discover: a target vector and a target row are both given";
        case DISC_BAD_MIN_WINS: return "ott_query_discover: min_wins is above the number of pairs";
        case DISC_PER_QUERY: return "ott_query_discover: the context makes ONE query; PER_QUERY is not served";
        case DISC_MFMA: return "ott_query_discover: the MFMA path does not serve discovery queries; use path AUTO or EXACT";
        case DISC_MULTI_GPU: return "ott_query_discover: a multi-GPU store is not served (the examples' rows lie on different shards)";
        case DISC_TOO_MANY_ROWS: return "ott_query_discover: a store of more than 2^32 - 16 rows is not served";
        case DISC_SMALL_CAP: return "ott_query_discover: output capacity is smaller than min(k, rows)";
        case DISC_NULL_OUT: return "ott_query_discover: out is NULL";
        default: return "";
    }
}

int refuse(DiscRefusal r, uint64_t id = 0, uint64_t len = 0) {
    const int code = disc_refusal_is_invalid(r) ? OTT_ERR_INVALID : OTT_ERR_UNSUPPORTED;
    if (r == DISC_BAD_ID) return fail(code, "ott_query_discover: row id " + std::to_string(id) + " is not below the store's length " + std::to_string(len));
    if (r == DISC_SAME_ROW) return fail(code, "ott_query_discover: row " + std::to_string(id) + " is both the positive and the negative of a pair");
    return fail(code, refusal_text(r));
}

// The query on a context whose `mu` the caller holds (and the owner's `rw`, shared).  k_eff = min(k, rows) >= 1; every slot's row < s->n.
int run_discover(ott_store* s, const ott_query_desc* d, const DiscSlots& sl, uint32_t min_wins, uint64_t k_eff, ott_hit* out, uint64_t* n_out, uint32_t* wins_of_hit,
                 ott_stats* stats_out) {
    int rc;
    const bool has_target = sl.target != DISC_TARGET_NONE;
    ExampleFrame fr{s, d, "ott_query_discover", k_eff, stats_out};
    DiscoverParams p{};
    // a vector target goes up in its slot, the last, with the host-side inverse norm of ott_query; the other slots go up zeroed
    std::vector<float> qblock;
    if (sl.target == DISC_TARGET_VECTOR) {
        qblock.assign((size_t)sl.n_slots * s->dim, 0.0f);
        memcpy(qblock.data() + (size_t)(sl.n_slots - 1) * s->dim, d->queries, (size_t)s->dim * 4);
    }
    if ((rc = fr.begin(&p, qblock.empty() ? nullptr : qblock.data(), sl.n_slots))) return rc;
    uint64_t total = 0;
    if (fr.grid != 0) {
        // (the states are left zeroed by the keys / select kernel)
        const uint32_t n = fr.n;
        GroupTopK& tk = fr.tk;
        if ((rc = s->d_disc.ensure(disc_scratch_bytes(has_target, n, k_eff)))) return rc;
        unsigned long long* keys = fr.keys;
        uint32_t* hdr = (uint32_t*)s->d_disc.p;
        DiscAbove* list = (DiscAbove*)((char*)s->d_disc.p + disc_list_off());
        uint8_t* wins8 = (uint8_t*)s->d_disc.p + disc_wins_off();
        p.state = fr.state;
        p.n_pair_slots = 2 * sl.n_pairs;
        p.target_slot = disc_target_slot(sl);
        const bool take_max = p.take_max != 0;
        DiscoverPick pick;
        pick.min_wins = min_wins;
        pick.has_target = has_target ? 1u : 0u;
        pick.take_max = take_max ? 1u : 0u;
        pick.cmp = (uint32_t)d->filter_cmp;
        pick.thr = d->filter_thr;

        // (the keys of a context search hold the loss's ordinal under Max)
        if ((rc = fr.prepare(sl.rows, sl.n_gather, has_target ? take_max : true, &s->rectable_clean))) return rc;
        // what the host reads behind the one wait
        const size_t list_bytes = disc_list_off() + (size_t)k_eff * sizeof(DiscAbove);
        WinsLookup wl{};
        if (has_target) {
            if ((rc = s->h_disc.ensure(list_bytes))) return rc;
            OTT_HIP(hipMemsetAsync(hdr, 0, disc_hdr_bytes(), s->stream));
        } else if (wins_of_hit) {
            if ((rc = s->h_disc.ensure(tk.lists_path ? (size_t)k_eff * 4 : (size_t)n))) return rc;
            if (tk.lists_path) {
                void* mapped = nullptr;
                OTT_HIP(hipHostGetDevicePointer(&mapped, s->h_disc.p, 0));
                wl.k = k_eff;
                wl.base = s->base_offset;
                wl.n = n;
                wl.wins8 = wins8;
                wl.out = (uint32_t*)mapped;
                tk.after_merge = launch_wins_lookup;
                tk.after_arg = &wl;
            }
        }
        rc = fr.sweep(SW_NQ, [&](uint32_t q0) {  // (NQ = SW_NQ alone: a pass holds whole pairs)
            p.q0 = q0;
            return launch_sweep<false>(s->stream, p, SW_NQ, fr.grid, OTT_SWEEP_KERNEL(discover_sweep_kernel));
        });
        if (rc) return rc;
        uint64_t n1 = 0;
        if (!has_target) {
            hipLaunchKernelGGL(discover_keys_kernel, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, s->stream, p.state, n, pick, keys, wins8);
            OTT_HIP(hipGetLastError());
            if ((rc = fr.rank())) return rc;
            if (wins_of_hit && !tk.lists_path) OTT_HIP(hipMemcpyAsync(s->h_disc.p, wins8, n, hipMemcpyDeviceToHost, s->stream));
            if ((rc = fr.finish(out, &n1))) return rc;
            total = n1;
            if (wins_of_hit) {
                if (tk.lists_path) {
                    memcpy(wins_of_hit, s->h_disc.p, (size_t)n1 * 4);
                } else {
                    const uint8_t* hw = (const uint8_t*)s->h_disc.p;
                    for (uint64_t i = 0; i < n1; i++) wins_of_hit[i] = hw[out[i].index - s->base_offset];
                }
            }
        } else {
            const uint32_t n_levels = sl.n_pairs + 1;
            hipLaunchKernelGGL(discover_count_kernel, dim3(row_blocks(s, n)), dim3(256), 0, s->stream, p.state, n, pick, hdr);
            OTT_HIP(hipGetLastError());
            hipLaunchKernelGGL(discover_select_kernel, dim3(row_blocks(s, n)), dim3(256), 0, s->stream, p.state, n, pick, hdr, n_levels, k_eff, keys, list);
            OTT_HIP(hipGetLastError());
            if ((rc = fr.rank())) return rc;
            OTT_HIP(hipMemcpyAsync(s->h_disc.p, s->d_disc.p, list_bytes, hipMemcpyDeviceToHost, s->stream));
            if ((rc = fr.finish(out, &n1))) return rc;
            const uint32_t* hh = (const uint32_t*)s->h_disc.p;
            uint64_t n_above = 0;
            const uint32_t cut = disc_level_cut(hh, n_levels, k_eff, &n_above);
            if (hh[DISC_HDR_CURSOR] != n_above || n_above >= k_eff) return fail(OTT_ERR_HIP, "ott_query_discover: the list above the cut level disagrees with the counters");
            DiscAbove* above = (DiscAbove*)((char*)s->h_disc.p + disc_list_off());
            std::sort(above, above + n_above, [](const DiscAbove& a, const DiscAbove& b) { return a.wins != b.wins ? a.wins > b.wins : a.key > b.key; });
            const uint64_t n_level = std::min<uint64_t>(n1, k_eff - n_above);
            if (n_above != 0 && n_level != 0) memmove(out + n_above, out, (size_t)n_level * sizeof(ott_hit));
            for (uint64_t i = 0; i < n_above; i++) {
                ott_hit h;
                h.index = s->base_offset + (uint32_t)(~(uint32_t)above[i].key);
                h.score = score_of((uint32_t)(above[i].key >> 32), take_max);
                h.query = 0;
                out[i] = h;
                if (wins_of_hit) wins_of_hit[i] = above[i].wins;
            }
            if (wins_of_hit)
                for (uint64_t i = 0; i < n_level; i++) wins_of_hit[n_above + i] = cut;
            total = n_above + n_level;
        }
    }
    if (n_out) *n_out = total;
    fr.end();
    return OTT_OK;
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_discover(ott_store* s, const ott_query_desc* d, uint64_t target_row, const uint64_t* positive, const uint64_t* negative, uint64_t n_pairs, uint32_t min_wins,
                       uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out, uint32_t* wins_of_hit, ott_stats* stats) {
    // what the arguments and the descriptor alone decide comes first: these refusals need no store
    if (!d) return fail(OTT_ERR_INVALID, "ott_query_discover: desc is NULL");
    DiscRefusal why = disc_check_args(n_pairs, positive == nullptr, negative == nullptr, flags, d->nq, d->queries == nullptr, target_row != DISC_NO_ROW, min_wins,
                                      d->mode == OTT_MODE_PER_QUERY, d->path == OTT_PATH_MFMA);
    if (why != DISC_OK) return refuse(why);
    int rc;
    if ((rc = check_desc_enums("ott_query_discover", d))) return rc;
    if (!s) return fail(OTT_ERR_INVALID, "ott_query_discover: store is NULL");
    const uint64_t len = ott_store_len(s);
    if ((why = disc_check_store(s->multi != nullptr, len)) != DISC_OK) return refuse(why);
    if ((rc = check_device_row_mask("ott_query_discover", s, d))) return rc;
    DiscSlots sl;
    uint64_t bad = 0;
    if ((why = disc_slots(positive, negative, (uint32_t)n_pairs, target_row, d->nq == 1, len, &sl, &bad)) != DISC_OK) return refuse(why, bad, len);
    if ((why = disc_check_out(disc_k_eff(d->k, len), cap, out == nullptr)) != DISC_OK) return refuse(why);
    ott::host::SharedLock rd;  // the corpus cannot change while this query runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    // what the checks above read without the lock is read again, and k_eff only here: appends (this call's own flush of rows another
    // thread staged after `len` was read) or a compact may have come in between, so the store may be longer or shorter than `len`
    if ((why = disc_check_store(false, s->n)) != DISC_OK) return refuse(why);
    for (uint32_t e = 0; e < sl.n_gather; e++)
        if (sl.rows[e] >= s->n) return refuse(DISC_BAD_ID, sl.rows[e], s->n);
    const uint64_t k_eff = disc_k_eff(d->k, s->n);
    if ((why = disc_check_out(k_eff, cap, out == nullptr)) != DISC_OK) return refuse(why);
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (k_eff == 0) return OTT_OK;
    CtxLease ctx(s);
    return run_discover(ctx.c, d, sl, min_wins, k_eff, out, n_out, wins_of_hit, stats);
}

}  // extern "C"
