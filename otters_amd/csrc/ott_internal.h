// ott_internal.h — shared declarations of libotters_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/otters_hip.h"
#include "ott_host.h"  // the host-side concurrency (thread pool, context pool, staged appends, background worker): HIP-free, sanitizer-tested
#include "ott_policy.h"  // path choice and the batch cascade's back-off rules: HIP-free, CPU-tested
#include "ott_plane_policy.h"  // the two format decisions of the cascade's planes: HIP-free, CPU-tested
#include "ott_mfma_plan.h"  // the batch path's host-side plan (tile geometry, candidate budget, error bound, query norms, query block): HIP-free, CPU-tested
#include "ott_maxsim_gather_plan.h"  // listed MaxSim's host-side plan (tokens per pass, slot arrays, table sizes, route, the 2 GiB refusal): HIP-free, CPU-tested
#include "ott_exact_plan.h"  // the exact path's host-side plan (lists or sort, list width, kernel variant, passes and grid, lean, pruned sweep, result block): HIP-free, CPU-tested
#include "ott_discover_plan.h"  // discovery / context search's host-side plan (refusals, slot layout, passes, k_eff, scratch bytes, the level cut): HIP-free, CPU-tested
#include "ott_recommend_plan.h"  // recommend-by-example's host-side plan (refusals, example layout, passes, k_eff, the second round, scratch bytes): HIP-free, CPU-tested
#include "ott_mmr_plan.h"  // MMR re-ranking's host-side plan (refusals, scratch layout, the pair grid, the greedy launch): HIP-free, CPU-tested
#include "ott_masks_plan.h"  // ott_query_masks' host-side plan (refusals, the queries' order by mask id, the route and its auto rule): HIP-free, CPU-tested
#include "ott_binary_plan.h"  // bit rows and ott_query_binary's host-side plan (refusals, the transposed slice layout, the route, the gate's LDS and capacity, Hamming in C): HIP-free, CPU-tested
#include "ott_sparse_plan.h"  // sparse rows and ott_query_sparse's host-side plan (refusals, the sliced-ELL layout, the lookup's form and passes, the score in C): HIP-free, CPU-tested
#include "ott_sort_plan.h"  // the sort path's host-side plan (pass plans, sweep shape, rank or radix, prefix, slices, group extents, copy pieces): HIP-free, CPU-tested
#ifdef OTT_DEVICE_AUDIT
#include "ott_audit.h"  // test build: every HIP call below goes through a device-affinity check (see "which GPU a call is for")
#endif

namespace ott {

// ---- error plumbing ------------------------------------------------------------------------
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define OTT_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            (void)hipGetLastError(); /* reported here: a later launch check must not see it again */ \
            return ::ott::fail(_e == hipErrorOutOfMemory ? OTT_ERR_OOM : OTT_ERR_HIP,              \
                               std::string(#expr) + ": " + hipGetErrorString(_e));                 \
        }                                                                                          \
    } while (0)

// ---- which GPU a call is for ------------------------------------------------------------------------------------------------
// Every store (shard, worker context) lives on one HIP device, and everything done for it — allocations, launches, event and
// stream calls — must happen with that device current on the calling thread.  use_device() is the ONE way the library selects
// a device.  Besides the physical ordinal a store carries a LOGICAL device id: equal to the ordinal normally; with the test
// option "multi_fake_distinct" every shard of a multi-GPU store gets an id of its own although the shards share the box's one
// GPU.  The device-affinity audit build (make audit: -DOTT_DEVICE_AUDIT, ott_audit.hip) records the logical id of the last
// use_device() in a thread-local and checks it at every allocation, launch, copy, event and stream call against the
// id the stream / event / buffer was created under: a missed use_device() on a shard thread, in the background plane builder
// or in drain() then fails on ONE GPU instead of corrupting memory on eight.
#ifndef OTT_DEVICE_AUDIT
#define OTT_AUDIT_PTR(ptr, store) ((void)0)
inline hipError_t use_device_raw(int device, int /*logical*/) { return hipSetDevice(device); }
#endif

// hipFuncSetAttribute applies to the CURRENT device: one bit per device ordinal says where a kernel already has its opt-in
// (a process may hold stores on several GPUs: ott_store_create_multi)
inline bool attr_needed(const std::atomic<uint64_t>& seen, int device) {
    return device > 63 || !((seen.load(std::memory_order_acquire) >> (device & 63)) & 1ull);
}
inline void attr_done(std::atomic<uint64_t>& seen, int device) {
    if (device <= 63) seen.fetch_or(1ull << (device & 63), std::memory_order_release);
}

inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// blocks of a grid-stride launch: one per `per_block` items, at most `per_cu` per compute unit, at least one
inline uint32_t grid_blocks(uint64_t items, uint32_t per_block, int n_cu, uint32_t per_cu = 8) {
    const uint64_t want = (items + per_block - 1) / per_block, most = (uint64_t)n_cu * per_cu;
    return (uint32_t)(want < 1 ? 1 : want < most ? want : most);
}

// ---- device buffers that grow on demand -----------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);  // keeps contents only if no reallocation is needed
    void release();
};
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
};

// Behaviour switches of one store.  Read ONCE from the environment (OTT_* variables of the same names, upper case) when
// the store is created, changed afterwards only through ott_store_set_option: the query path never looks at the
// environment.  TWENTY-NINE of them have a name in the product library (ott_store.hip: kOptNames; round 5 retired the rest):
// tie_order, hi_fmt, hi_prebuild, stage_appends, multi_transport, multi_rebalance, multi_min_shard_rows — behaviour a host may
// want; exact_small, exact_prune, exact_sketch, exact_sketch_bits, exact_sketch_head, exact_i8_check, id_gather, group_gather, masks_sweep, fuse_device, sparse_table, sparse_df_lds, binary_gate, binary_gate_cap, large_k_from, small_sort, mfma_f32, no_hi_pass, no_batch_image — which of several equivalent paths
// runs (tests hold each to the oracle); force_fallback, eps_scale_ppm, multi_fake_distinct — tests only.  The fields marked
// [debug build] can be set by name only in a library built with -DOTT_MFMA_DEBUG_BUILD (kernel tuning / timing ablations);
// the fields marked [fallback] are set through the bits of force_fallback.
struct Options {
    int exact_small = -1;         // single-query small-store kernel: -1 = automatic, 0 = streaming kernel, 2 = rows8 (eight lanes per row)
                                  // (1, round 2's one-wave LDS-DMA variant, is retired: 31 us against rows8's 10)
    int exact_prune = -1;         // single-query exact sweep: score a seed of the rows first, then skip the last stages of rows whose score
                                  // bound misses the seed's k-th best: -1 = automatic (stores of 2^20 rows and more), 0 = off, 1 = forced
    int exact_sketch = -1;        // the pruned sweep's per-row tail sign sketch (one sign bit per dim of the last quarter of the
                                  // stages, a mean magnitude and a remainder norm, ~1 % of the row bytes, made when rows are appended): -1 =
                                  // automatic (stores of 8 stages and more, dim >= 225), 0 = never, 1 = always.  A store that keeps one
                                  // stops rows at 3/4 of the stages instead of 7/8
    int exact_sketch_bits = 4;    // the sketch's form, read when the store makes its first line: 4 = a four-bit code per dim of every stage but
                                  // the first (384 B per row at dim 768, 1/8 of the row bytes; rows stop after their first stage), 3 = a
                                  // three-bit code per dim of the last 5/8 of the stages (192 B per row at dim 768, 1/16 of the row bytes;
                                  // rows stop at 3/8 of the stages), 1 = the sign sketch described above
    int exact_sketch_head = -1;   // the head of the four-bit lines (20 B per row: stage 0's codes and a remainder norm over every stage, made with
                                  // the lines): -1 / 1 = kept and used wherever the store keeps four-bit lines — a gated row then reads no f32
                                  // stage at all — 0 = never: the sweep reads stage 0 of every row, as it does on a store without a head
    int exact_i8_check = -1;      // the head form's survivors are checked on the int8 plane before their f32 finish (ott_exact_plan.h:
                                  // prune_plan_i8_check): -1 / 1 = wherever the plane is ready and the query is inside its error model, 0 = never
    int force_fallback = 0;       // TESTS: bit mask of code paths the library otherwise takes only in rare conditions, forced on so that the
                                  // suite and the option fuzz hold them to the oracle: 1 = block lists merged by insertion (merge_kernel: the
                                  // rank merge's own fallback when a plateau overflows its buffer or there are > 4096 lists), 2 = k <= 64
                                  // through sorted heads + tree fold (merge_small_kernel: > 4096 lists), 4 = the 256-query blocks of a row
                                  // tile one after the other on one workgroup (what three blocks or a short round get anyway), 8 = the
                                  // sort path lists every pair (no prefix gate: what its first phase does anyway), 16 = the open first
                                  // round through the cursor atomics instead of dense stores, 32 = conservative emission thresholds between
                                  // the row rounds (what a store backs off to after a speculative gate failed), 64 = the sort path cuts its
                                  // rows into slices of 2^14 (row, query) pairs instead of 2^29 (what only stores of billions of pairs do)
    bool mfma_f32 = false;        // batch path: ONE candidate pass on the f32 matrix pipe (v_mfma_f32_32x32x2_f32)
    bool no_hi_pass = false;      // batch path starts at the split-bf16 pass (no hi plane is built)
    bool no_batch_image = false;  // no bf16 copies of the corpus at all (the split pass splits the f32 rows in registers)
    int mfma_wg = 0;              // [debug build] workgroups per CU of the candidate pass (0 = the tile's default)
    int mfma_growth = 8;          // [debug build] growth factor of the candidate pass's row rounds
    bool mfma_no_dense = false;   // [fallback 16] open first round through the cursor atomics instead of dense stores
    bool mfma_debug = false;      // [debug build] in-kernel cycle stamps
    int mfma_abl = 0;             // [debug build] timing ablations of the candidate kernel and the radix sort (results are then wrong)
    int mfma_spec = -1;           // [fallback 32] speculative emission thresholds between the row rounds of the first cascade level (-1 = default on, 0 / 1)
    int mfma_coop = -1;           // [fallback 4] > 256 queries: the query blocks of a row tile on sibling workgroups of one XCD at the same time (-1 = default, 0 / 1)
    int tie_order = 0;            // 0 = canonical total order; 1 = the reference's outcome at exact score ties, ONE collector over the store
                                  // (VecStore, src/vec.rs:217-310); 2 = one collector per chunk, then concat-sort-truncate (MetaStore,
                                  // src/meta.rs:678-709).  See ott_ties.hip
    int hi_fmt = -1;              // what the batch path's 16-bit / 8-bit copies of the corpus are: -1 (default) / 2 = an INT8 plane as the cascade's
                                  // first level (k <= 128; a quarter of the f32 bytes) with an IEEE-half hi plane behind it, built only
                                  // once a query needs it (k > 128, or what the int8 level could not certify); 1 = the half plane alone
                                  // (round 3-4's default); 0 = a bf16 plane alone.  Takes effect when a plane is (re)built
    int hi_tmin = 0;              // [debug build] the hi pass re-scores at least this many candidates per query (0 = 2k + 56; at most 512)
    int merge_rank1 = -1;         // [fallback 2] k <= 64: merge_rank_kernel (-1 / 1, default) or round 2's merge_small_kernel (0)
    bool merge_walk = false;      // [fallback 1] k > 64: merge the block lists by insertion (merge_kernel) instead of bound + gather + rank (merge_rank_kernel)
    int large_k_from = 0;         // experiments: k above which host-output queries take the sort path (0 = automatic: 512 for one query or a small store, 128 for several queries; at most 512)
    int large_k_pre = -1;         // [fallback 8] large-k (sort) path: score a prefix of the rows first and list, of the rest, only pairs that reach its k-th best (-1 / 1 = on, 0 = off)
    int hi_prebuild = -1;         // the batch path's 16-bit hi plane is built (extended) in the background right after appends, off the first batch's
                                  // critical path: -1 = automatic (stores of 262144 rows and more, while the plane takes at most a quarter of the free
                                  // HBM), 0 = never (built by the first batch query or ott_store_prepare_batch), 1 = always
    int stage_appends = -1;       // appends below 256 KB are staged in pinned host memory and sent to the GPU 4 MB at a time (-1 / 1 = on, 0 = every append goes at once)
    int small_sort = -1;          // results of up to 16384 (row, query) pairs sorted by rank in two launches (-1 / 1 = on, 0 = the radix sort path)
    int eps_scale_ppm = 1000000;  // TEST ONLY: the batch path's error bound multiplied by this many millionths (a deliberately-too-small bound
                                  // must be noticed by the measured |approximate - exact| / eps and answered by the next cascade level)
    int multi_transport = 0;      // multi-GPU store (ott_store_create_multi): how the shards' candidate blocks reach the merging GPU.
                                  // 0 = automatic (RCCL all-gather when the device ordinals are distinct and librccl loads, peer copies
                                  // otherwise), 1 = peer copies (hipMemcpyPeerAsync + events), 2 = RCCL (ncclCommInitAll + grouped ncclAllGather)
    int multi_rebalance = 1;      // multi-GPU store: 1 = rows are moved between the shards (before a query, after appends) when one shard holds
                                  // more than 1.25x its even share; 0 = never (rows stay where the appends put them)
    bool multi_fake_distinct = false;  // TEST ONLY (OTT_MULTI_FAKE_DISTINCT=1, read when the store is created): every shard of a multi-GPU
                                  // store counts as a device of its own although the ordinals repeat — the exchange, the row moves and
                                  // device appends then take the code paths of distinct GPUs (send buffer + hipMemcpyPeerAsync + event
                                  // wait, or the grouped all-gather) on a one-GPU box.  Results never depend on it.
    int id_gather = -1;           // candidate id lists (ott_query_ids): -1 = automatic, 0 = never (the list becomes a row mask and
                                  // takes the mask's paths), 1 = the gather kernel wherever it is eligible
    int group_gather = -1;        // listed MaxSim (ott_query_maxsim_groups): -1 = automatic, 0 = never (the list becomes a row mask and
                                  // ott_query_maxsim's sweep runs), 1 = the gather kernel wherever it is eligible
    int masks_sweep = 2;          // a row mask per query (ott_query_masks): 2 = automatic (ott_masks_plan.h), 0 = always by mask group
                                  // (one PER_QUERY run per distinct mask), 1 = the masks sweep wherever it is eligible
    int maxsim_fold = -1;         // [debug build] late-interaction sweep (ott_maxsim.hip): -1 = the product's epilogue, 0 = one atomic per lane,
                                  // 1 = folded over runs of adjacent lanes of one group first (the A/B of profiles/maxsim)
    int multi_min_shard_rows = 32768;  // multi-GPU store: a shard is only brought in for this many rows (a store of fewer than twice as many stays
                                  // on its first GPU and is answered by that shard alone: the fan-out over N GPUs costs 50-150 us per query,
                                  // more than a small store's whole query); 0 = always split evenly over all shards
    int fuse_device = -1;         // rank fusion (ott_query_fuse): -1 = automatic (ott_fuse_plan.h: the host route), 0 = always the host route (the legs'
                                  // lists come back to the host and go up in one copy), 1 = the device route wherever it is eligible
    int sparse_df_lds = -1;       // document frequencies (ott_store_sparse_df): -1 = automatic (ott_sparse_plan.h: sparse_df_take_lds), 0 = global atomics always, 1 = a histogram in LDS wherever the vocab fits
    int sparse_table = -1;        // sparse queries (ott_query_sparse): where the weight lookup reads from: -1 = automatic (ott_sparse_plan.h),
                                  // 0 = the LDS form wherever it is eligible (vocab <= 32768), 1 = always the device table form
    int binary_gate = -1;         // binary queries (ott_query_binary): which route answers: -1 = automatic (ott_binary_plan.h: binary_take_gate),
                                  // 0 = always the key table, 1 = the gated sweep wherever it is eligible
    int binary_gate_cap = 0;      // the gated sweep's pair capacity: 0 = the plan's (binary_gate_capacity), otherwise this many pairs (tests reach the overflow
                                  // branch with it at a small shape)
};
void options_from_env(Options& o);                                   // ott_store.hip; called by ott_store_create only
int option_set(Options& o, const char* name, long long value);       // 0, or -1 for an unknown name / bad value

// librccl.so.1, dlopen'ed on first use (ott_comm.hip): the library loads — and every single-GPU entry point works — without it
struct NcclId {
    char internal[OTT_COMM_ID_BYTES];
};
struct Rccl {
    void* handle = nullptr;
    int (*GetUniqueId)(NcclId*) = nullptr;
    int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*GetVersion)(int*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string why;  // load failure
};
constexpr int kNcclUint8 = 1;  // ncclDataType_t::ncclUint8 (rccl.h)
Rccl* rccl();

// ---- the cascade's planes (ott_planes.hip; their life cycle: DESIGN.md 2, "The cascade's planes") ---------------------------
// One compact copy of the corpus for the batch path: built lazily by the first query that needs it (or declined), extended after
// appends, kept in step by write_rows, dropped by whatever moves the rows and built again on demand.
struct Plane {
    void* d = nullptr;          // [cap rows of the plane's pitch]; nullptr = not there
    uint64_t rows = 0;          // rows [0, rows) are converted
    bool off = false;           // declined (no room, an option, the wrong format for the store); survives a drop
    uint32_t* d_rel = nullptr;  // hi, int8: 16 B of device words, survive a drop — [0] running max of the measured loss over the regular
                                // rows (float bits, atomicMax), [1] rows marked irregular, [2] scratch (min_regular_inv_kernel)
    float rel = 0.0f;           // host copy of d_rel[0]: MEASURED, which makes the pass's error bound rigorous and tighter than the worst case
};
struct PlaneSet {
    std::mutex mu;  // guards every field here, for all three planes: held by whoever builds or extends one (also from other query contexts
                    // while the store is only held shared), so a query that needs a plane waits for the builder
    // Split image: every row pre-split into bf16 hi + bf16 lo, per 32-k stage [32 hi | 32 lo] (the same 128 B a stage of f32 takes;
    // row pitch = dim rounded up to 32 floats).  Doubles the store's HBM footprint; without it the kernel splits the f32 rows in
    // registers.  Only built when a query falls through to the split pass.  split.off also switches the other two off.
    Plane split;
    // Hi plane: the 16-bit round-to-nearest value of every element, row pitch = dim rounded up to 64 elements — HALF the corpus
    // bytes; the first candidate pass of a store without an int8 plane streams only this (one 16-bit MFMA per 16 k).
    Plane hi;
    HiFormat hi_format{false, 1.0f};  // IEEE half (11 significant bits, ~8x tighter bound) or bf16; half's one factor (hi_plane_format)
    // Int8 plane (option hi_fmt = -1 / 2): every row as int8 with ONE f32 scale per row (s_v = max|v_i| / 127, element =
    // rint(v_i / s_v)), row pitch = dim rounded up to 128 bytes — a QUARTER of the corpus bytes.  The batch path's cheapest
    // candidate pass streams it (v_mfma_i32_32x32x32_i8: the integer accumulation is exact, so the pass's error bound is pure
    // quantisation).  Rows that measure more than 2^-5 (one huge element among small ones) are marked irregular.
    Plane i8;
    float* d_i8_scale = nullptr;  // [cap] s_v
    // d_flag bytes (bit 1: the half plane's factor does not suit the row; bit 2: int8 loses too much of it): ONE writer at a time —
    // the plane builders, under `mu` — while other contexts' kernels read them.  Readers tolerate either value of a bit that is
    // being set or taken back: a set bit only forces the row into the candidate list and its exact re-score (never changes a result),
    // and a bit is cleared only together with dropping the plane whose passes consult it (ensure_i8_plane's rollback).
};

struct Column {
    uint32_t dtype;
    void* d_vals;
    uint64_t* d_nulls;  // may be null
    uint64_t n;
};

}  // namespace ott

// A run of consecutive surviving chunks: local rows [start, start+count).
struct ott_run {
    uint64_t start;
    uint64_t count;
};

struct ott_multi;  // ott_multi.hip: the shards of a store that spans several GPUs (ott_store_create_multi)

struct ott_store {
    ott_multi* multi = nullptr;  // set: this object is the FRONT of a multi-GPU store — dim / n / chunk_size / base_offset / opt / rw
                                 // are the whole store's, the rows live in multi->shards (every extern "C" entry point dispatches on it)
    int device = 0;
    int logical = 0;             // logical device id (= device, unless the multi-GPU store was created with "multi_fake_distinct"): see use_device
    uint32_t dim = 0;
    uint32_t ld = 0;    // row pitch in floats (dim rounded up to 4: rows are 16-B aligned)
    uint32_t dimq = 0;  // query pitch in floats (dim rounded up to 8)
    uint64_t n = 0, cap = 0;
    uint64_t chunk_size = 1024;
    uint64_t base_offset = 0;
    uint32_t reduce = OTT_REDUCE_AVX;
    int n_cu = 256;
    float min_pos_inv = __builtin_inff();  // smallest non-zero inverse norm appended so far (1/max row norm)
    ott::Options opt;

    float* d_rows = nullptr;  // [cap * ld]
    float* d_inv = nullptr;   // [cap]
    // tail sign sketch of the pruned exact sweep (ott_prune.h: prune_sketch_row): [cap * sk_pitch] words, made beside the inverse
    // norms for the same rows (launch_inv_norms).  sk_n: rows [0, sk_n) hold one — the sweep uses it only when that covers the store
    uint32_t* d_sketch = nullptr;
    uint64_t sk_n = 0;
    uint32_t sk_words = 0, sk_pitch = 0, sk_stage0 = 0;  // code words per row, line pitch in words, first sketched stage
    uint32_t sk_bits = 0;                                // bits per sketched dim of the lines that are there (1, 3 or 4)
    // the head of the four-bit lines (ott_prune.h: prune_sketch4_head_row), two plain arrays in one allocation: [16 cap bytes of stage
    // 0's codes | cap floats rho_all], made by the launch that makes the lines and kept wherever they are kept (option
    // exact_sketch_head).  head_n: rows [0, head_n) hold one — the sweep reads no f32 stage only when that covers the store
    char* d_head = nullptr;
    uint64_t head_n = 0;
    uint8_t* d_flag = nullptr;  // [cap] 1 = row norm is inf / NaN / > 1e18 / tiny but non-zero / underflowed (always re-scored exactly by the MFMA path)
    ott::PlaneSet planes;       // the cascade's compact copies of the corpus (owner store only: contexts reach them through `owner`)
    ott::CascadeState cascade;  // the batch cascade's back-off state (ott_policy.h), shared by the store's contexts: read through the owner

    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {};  // 0-2 batch path timing, 3-5 exact path timing, 6 multi-GPU store: this shard's candidate block is ready

    // per-query scratch
    ott::DevBuf d_queries, d_qinv, d_rowmask, d_runs, d_prefix, d_lists, d_lists2, d_hits, d_count, d_cand, d_misc;  // d_lists2: first stage of the two-stage merge
    ott::DevBuf d_prune;     // pruned exact sweep: the seed's merged result (the gate of the second launch)
    ott::DevBuf d_tails;     // pruned exact sweep: two running counts (u64 each) — [0] the rows that passed the gate (without the int8 check:
                             // the rows whose tails the kernel finished, the same rows), [1] with the int8 check the rows finished in f32
    uint64_t tails_seen = 0; // ... and what of [0] earlier queries have reported
    uint64_t fin_seen = 0;   // ... and of [1]
    std::atomic<uint64_t> exact_finished{0};  // owner store: rows the pruned sweeps of all contexts finished in f32 so far (ott_store_exact_finished)
    ott::DevBuf d_minpos;    // device word behind min_pos_inv
    // MFMA path scratch
    ott::DevBuf m_Q, m_qinv, m_qnorm, m_tau, m_cntA, m_cntB, m_candA, m_candB, m_over, m_out, m_outcnt, m_uncert, m_prefix;
    // sort path (ott_sort.hip): the pairs and the sort's other buffers (ensure_pairs), the radix sort's control block and tile
    // status words (sort_pairs), the dump's cursor (dump_counted), the groups' start words (group_starts), the gates (radix_slice)
    ott::DevBuf l_keysA, l_keysB, l_qA, l_qB, l_tmp, l_cursor, l_hist, l_gate;
    ott::DevBuf l_ctl;         // rank-sort path (small_slice): cursor | tickets | ranks | histogram (small_ctl_layout), kept zeroed between queries
    bool l_ctl_clean = false;  // the last query on this context left l_ctl zeroed
    // sort path, results of a million hits and more: written straight into the caller's host buffer (query_core sets
    // direct_out / direct_cap for the call; fetch_pieces sets direct_done and the groups' counts when it used them; run_large_k
    // withdraws the offer while it merges slices)
    ott_hit* direct_out = nullptr;
    uint64_t direct_cap = 0;
    bool direct_done = false;
    std::vector<uint64_t> direct_counts;  // large-k (sort) path
    ott::DevBuf x_send, x_recv;  // sharded queries: this shard's candidate block, the gathered blocks of all shards
    ott::DevBuf d_evalmask;  // mask built by ott_store_eval_row_mask
    uint64_t evalmask_bits = 0;
    // A row mask per query (ott_masks.hip).  d_mslot / mslot_bits: the device mask slots, filled by
    // ott_store_eval_row_mask_slot / ott_store_write_row_mask_slot under `rw` exclusive; mslot_bits[i] = the rows slot i covers, 0 =
    // empty.  Owned by the store: worker contexts read them through `owner` (the caller holds `rw` shared).  Dropped wherever the
    // rows move (mask_slots_drop).  d_qmasks: THIS context's scratch of one ott_query_masks call (ott_masks_plan.h:
    // masks_scratch_bytes); cur_qmask / cur_qmask_bits: the per-query mask of the by-mask-group run this context is making right
    // now (compose_row_mask joins it, like cur_idmask), nullptr = none
    ott::DevBuf d_mslot[OTT_MASK_SLOTS];
    uint64_t mslot_bits[OTT_MASK_SLOTS] = {};
    ott::DevBuf d_qmasks;
    const uint64_t* cur_qmask = nullptr;
    uint64_t cur_qmask_bits = 0;
    // Deleted rows (ott_tomb.hip): the LIVE mask, one bit per row slot, 1 = live — [(cap + 63) / 64] words,
    // allocated by the first ott_store_delete_rows and freed again by ott_store_compact; nullptr = no row was ever deleted (and
    // the query path is then exactly what it was).  Every bit at and past `n` is 1 in every word, so appended rows are live
    // without a launch; a reallocation copies the words and fills the new ones with ones.  Owned by the store (workers alias
    // it), changed only under `rw` exclusive.  n_dead: cleared bits below n.  d_livefx: THIS context's scratch for
    // caller mask & live mask (one small kernel per query that carries a row mask of its own).
    uint64_t* d_live = nullptr;
    uint64_t n_dead = 0;
    ott::DevBuf d_livefx;
    // Candidate id lists (ott_gather.hip), THIS context's scratch.  d_idmask: the list as a row mask when a query
    // takes the mask route — [its bits over the store's rows | those & the caller's mask | the ids]; cur_idmask points at it for
    // the duration of that query (compose_row_mask reads it, like cur_tie_sh).  d_gather: [rows the gather kernel scored (u64,
    // 64 B) | raw scores of ott_store_score_rows]
    ott::DevBuf d_idmask, d_gather;
    uint64_t* cur_idmask = nullptr;
    // MMR re-ranking (ott_mmr.hip), THIS context's scratch, allocated by the first ott_query_mmr that runs on it:
    // [candidate rows | relevances | counts | picks | values | the pair scores] (ott_mmr_plan.h: MmrLayout)
    ott::DevBuf d_mmr;
    // Recommend by example (ott_recommend.hip), THIS context's scratch: the rows' best ordinals {bp, bn}, [n] x 8 B,
    // 0 = none; zeroed when it is (re)allocated or after a failed query and left zeroed by the kernel that reads it last
    // (rectable_clean) — or, where a second round could have run and did not, by a memset behind the first round: the flag is then
    // set without draining the stream, because the context's one stream orders the memset before the next query's sweep.  The rows'
    // 8-byte keys go through d_gtable, under its own protocol
    ott::DevBuf d_rectable;
    bool rectable_clean = false;
    // Discovery and context search (ott_discover.hip), THIS context's scratch, allocated by the first
    // ott_query_discover that runs on it.  The rows' 8-byte states {wins | flags, loss bits or target ordinal} live in d_rectable
    // under its protocol (the kernel that reads them last leaves them zeroed), the keys in d_gtable under its own.  d_disc: [the
    // candidates per wins level and the list's cursor | the candidates above the cut level | one byte of wins per row]
    // (ott_discover_plan.h), h_disc: its pinned copy the host reads behind the one wait
    ott::DevBuf d_disc;
    ott::PinBuf h_disc;
    // Grouped search (ott_group.hip).  d_gid: one dense group id per row slot, [cap] words, allocated by
    // ott_store_set_groups and freed by ott_store_clear_groups; nullptr = no groups (and nothing else below exists).  gid_n: the
    // rows the ids cover (a query needs gid_n == n).  Owned by the store (workers alias it), changed only under `rw` exclusive; a
    // reallocation copies the ids (group_grow).  d_gtable: THIS context's table of best keys, [queries per pass][n_groups] x 8 B,
    // left zeroed by every query's select / compact kernel (gtable_clean); d_gctl: the compact kernel's cursor.  ott_group_top.hip keeps
    // [queries][group_size][n_groups] slots in the same buffer under the same protocol (its deeper planes are cleared by a memset)
    uint32_t* d_gid = nullptr;
    uint64_t gid_n = 0;
    uint32_t n_groups = 0;
    ott::DevBuf d_gtable, d_gctl;
    bool gtable_clean = false;
    // Late-interaction search (ott_maxsim.hip), THIS context's scratch: the best score ordinal of every (token,
    // group), [nq][n_groups] x 4 B, 0 = empty; zeroed when it is (re)allocated or after a failed query and left zeroed by every
    // query's reduce kernel (mstable_clean).  The groups' 8-byte keys the reduce makes go through d_gtable, under its own protocol
    ott::DevBuf d_mstable;
    bool mstable_clean = false;
    // Listed MaxSim (ott_maxsim_gather.hip): the group-to-rows index.  d_gix: the rows ordered by group, [gid_n] words
    // (the order inside a group is not defined); gix_start: the groups' extents, [n_groups + 1] prefix sums, kept on the host (it
    // sizes every launch from them).  Built from d_gid by the first listed query that may take the gather, under `rw` exclusive
    // (lock_shared_clean's clean step); gix_ready says that step has been taken for the ids that are set (d_gix stays nullptr where
    // it declined: more than MG_INDEX_MAX_GROUPS groups).  Depends on the group ids alone: group_drop drops it, nothing else does.
    // Owned by the store (workers alias d_gix and read the extents through `owner`).  gix_builds: how often it was built.
    uint32_t* d_gix = nullptr;
    std::vector<uint32_t> gix_start;
    std::atomic<bool> gix_ready{false};
    std::atomic<uint64_t> gix_builds{0};
    // Small appends are STAGED: rows of appends below 256 KB (VecStore::add_vector is one row per call, src/vec.rs:357-371)
    // collect in pinned host memory and go to the GPU together — when 4 MB are full, and before anything looks at the rows
    // (queries, reads, columns, other kinds of append).  A single-row append costs a memcpy instead of a copy + a kernel + a
    // wait (60 us -> well under 1 us); results never depend on it.  Guarded like the rows themselves (exclusive `rw`).
    ott::PinBuf h_pend;            // the pinned memory behind `pend`
    ott::host::StagedRows pend;    // rows staged, not yet in HBM (VecStore::len counts them)
    ott::PinBuf h_stage, h_hits, h_hdr;  // h_hdr: this shard's block header of a sharded query (ott_comm.hip)
    size_t in_off_qinv = 0, in_off_runs = 0, in_off_prefix = 0;  // layout of the per-query input block in d_queries
    // candidate order of the query this context is running right now (query_core sets them, the launch wrappers read them)
    uint32_t cur_tie_sh = 0, cur_tie_off = 0;
    bool cur_flat = false;

    ott::host::QuietWorker* builder = nullptr;  // ott_planes.hip: the background thread behind option hi_prebuild (owner stores only)
    std::vector<ott::Column> columns;
    // Concurrency (ott_query is re-entrant on a store from several host threads, append needs exclusive
    // access).  `rw`: queries hold it shared, everything that changes the store holds it exclusive.  `mu` guards ONE query
    // context = this struct's stream, events and scratch.  When a query arrives while `mu` is taken, it runs on a worker
    // context instead: a second ott_store that aliases the corpus pointers and owns its own stream + scratch (created on
    // first need, at most OTT_MAX_WORKERS), so concurrent callers overlap on the GPU instead of queueing on a lock.
    ott::host::RwGate rw;
    std::mutex mu;
    ott::host::ContextPool<ott_store> pool;  // the worker contexts (ott_host.h)
    bool is_worker = false;
    ott_store* owner = nullptr;            // workers: the store they belong to
    // Rank fusion (ott_fuse.hip), THIS context's scratch, allocated by the first ott_query_fuse that runs on it:
    // [the legs' hit blocks | first leg, legs and weights | counts | fused hits] (ott_fuse_plan.h: FuseLayout); h_fuse: the pinned
    // memory behind the one upload (the first stage may still own h_stage when it is filled)
    ott::DevBuf d_fuse;
    ott::PinBuf h_fuse;
    // Sparse rows (ott_sparse.hip).  d_sparse: the sliced-ELL layout in one allocation (ott_sparse_plan.h:
    // SparseLayout), made by ott_store_set_sparse and freed by ott_store_clear_sparse; nullptr = no sparse rows (and nothing else
    // below exists).  sparse_n: the rows they cover (a query needs sparse_n == n).  sparse_base: the slices' bases on the host
    // ([slices + 1]; read_sparse and the stats' bytes read them through `owner`).  Owned by the store (workers alias d_sparse),
    // changed only under `rw` exclusive; independent of `cap`, so a reallocation of the rows leaves it alone.  d_spq / h_spq: THIS
    // context's copy of a call's queries (CSR).  d_sptable: THIS context's weight table of the table form ([vocab] float4 | presence
    // nibbles), zero whenever a query finds it: the clear kernel behind every pass leaves it so (sptable_clean, ensure_zeroed)
    char* d_sparse = nullptr;
    uint64_t sparse_n = 0, sparse_nnz = 0;
    uint32_t sparse_vocab = 0;
    ott::SparseLayout sparse_lay{};
    std::vector<uint64_t> sparse_base;
    ott::DevBuf d_spq, d_sptable;
    ott::PinBuf h_spq;
    bool sptable_clean = false;
    // Document frequencies of the sparse rows (ott_sparse.hip: sparse_df_ensure), owner store only.  sparse_gen
    // counts what moves them — the sparse rows set or dropped, rows deleted or restored, the live mask replaced — and changes only
    // under `rw` exclusive.  df_gen: the sparse_gen the cache below was built for (0 = never); d_df [vocab] words on the device,
    // df_host the same words on the host, df_ndocs the live rows.  The first call that needs them and finds df_gen != sparse_gen
    // rebuilds them on ITS context's stream under df_mu (the caller holds `rw` shared), so concurrent queries see one build.
    uint64_t sparse_gen = 1;
    std::mutex df_mu;
    uint64_t df_gen = 0;
    uint32_t* d_df = nullptr;
    std::vector<uint32_t> df_host;
    uint64_t df_ndocs = 0;
    std::atomic<uint64_t> df_builds{0};
    // Bit rows (ott_binary.hip).  d_binary: the transposed slice layout in one allocation (ott_binary_plan.h), made by
    // ott_store_set_binary / ott_store_set_binary_sign and freed by ott_store_clear_binary; nullptr = no bit rows.  binary_n: the rows
    // they cover (a query needs binary_n == n).  Owned by the store (workers alias d_binary), changed only under `rw` exclusive.
    // d_bq / h_bq: THIS context's block of a call: chunk runs, query words, gate words and the pair cursor.  bin_ctr (owner only):
    // gated calls, candidate pairs emitted, overflows, table-route calls (ott_store_binary_counters).
    char* d_binary = nullptr;
    uint64_t binary_n = 0;
    uint32_t binary_bits = 0;
    ott::DevBuf d_bq;
    ott::PinBuf h_bq;
    std::atomic<uint64_t> bin_ctr[4] = {};
};

namespace ott {
inline hipError_t use_device(const ott_store* s) { return use_device_raw(s->device, s->logical); }
int store_create(uint32_t dim, int device, int logical, ott_store** out);  // ott_store.hip: ott_store_create with a logical device id
// ott_multi.hip: the multi-GPU store behind the single-store entry points
enum AppendKind { APPEND_HOST = 0, APPEND_DEVICE = 1, APPEND_RANDOM = 2, APPEND_CLUSTERED = 3 };
struct AppendArgs {
    int kind = APPEND_HOST;
    const void* rows = nullptr;
    uint64_t seed = 0;
    uint32_t n_clusters = 0;
    float spread = 0.f, aniso = 0.f;
};
int multi_destroy(ott_store* ms);
int multi_reserve(ott_store* ms, uint64_t n_rows);
int multi_append(ott_store* ms, const AppendArgs& a, uint64_t n_rows);
int multi_write_rows(ott_store* ms, uint64_t first_row, const float* rows_host, uint64_t n_rows);
int multi_set_live(ott_store* ms, bool live, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed);  // delete (live = false) / restore
uint64_t multi_live_len(const ott_store* ms);
int multi_read_live_mask(const ott_store* ms, uint64_t* out_host);
int multi_read(const ott_store* ms, bool inv_norms, uint64_t first_row, uint64_t n_rows, float* out_host);
int multi_set_chunk_size(ott_store* ms, uint64_t chunk_size);
int multi_set_base_offset(ott_store* ms, uint64_t base);
int multi_set_reduce_order(ott_store* ms, uint32_t reduce);
int multi_set_batch_image(ott_store* ms, int enabled);
int multi_set_option(ott_store* ms, const char* name, int64_t value);
int multi_prepare_batch(ott_store* ms);
int multi_sync(ott_store* ms);
int multi_batch_ready(ott_store* ms);
uint64_t multi_exact_finished(ott_store* ms);
int multi_add_column(ott_store* ms, uint32_t dtype, const void* values_host, const uint64_t* nulls, uint64_t n, uint32_t* out_column_id);
int multi_eval_row_mask(ott_store* ms, const ott_leaf* leaves, uint32_t n_leaves, uint32_t n_clauses, uint64_t* out_host);
int multi_zone_stats(ott_store* ms, uint32_t column, uint64_t chunk_size, void* out_min, void* out_max, uint64_t* out_non_null);
int multi_query(ott_store* ms, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);
// ott_store.hip: staged appends.  store_rows = rows appended (resident + staged); store_flush brings the staged ones to the GPU
// (takes the store exclusively when there are any; call it WITHOUT holding the store's locks)
void mfma_warm(hipStream_t stream, int device);  // ott_mfma.hip: loads the batch path's code object and warms the runtime's H2D copy path (background plane builder)
void kick_plane_build(ott_store* s);  // ott_planes.hip: rows were appended — (re)build the first plane in the background if the policy says so
inline uint64_t store_rows(const ott_store* s) { return s->n + s->pend.count(); }
int store_flush(ott_store* s);
int store_flush_locked(ott_store* s);  // the caller holds `rw` exclusively and `mu`
// ott_store.hip: a shard takes over freshly filled buffers (rows moved between the GPUs of a multi-GPU store)
int store_adopt(ott_store* s, float* rows, float* inv, uint8_t* flag, uint32_t* sketch, uint32_t sketch_bits, char* head, uint64_t n, uint64_t cap);

constexpr size_t OTT_MAX_WORKERS = 15;
ott_store* ctx_acquire(ott_store* s);  // returns s or a worker, with its `mu` held
void ctx_release(ott_store* w);
// a query context for the rest of the scope
struct CtxLease {
    ott_store* c;
    explicit CtxLease(ott_store* owner) : c(ctx_acquire(owner)) {}
    ~CtxLease() { ctx_release(c); }
    CtxLease(const CtxLease&) = delete;
    CtxLease& operator=(const CtxLease&) = delete;
};
// the store shared for a query: rows of small appends still staged on the host go to the GPU first (that takes the store exclusively);
// an append may slip in before the shared lock is held, so the staged count is looked at again under it
inline int lock_store_shared(ott_store* s, ott::host::SharedLock& rd) {
    return ott::host::lock_shared_clean(s->rw, rd, [s] { return s->pend.count() != 0; }, [s] { return store_flush(s); });
}
// the context's id mask (cur_idmask) is the caller's for the rest of the scope, and nobody's after it
struct IdMaskGuard {
    ott_store* c;
    ~IdMaskGuard() { c->cur_idmask = nullptr; }
};
// ---- ott_planes.hip: the cascade's planes (struct PlaneSet).  Everything below takes the planes' mutex itself. -----------------
// The steps of the life cycle that belong to whoever changes the store (the caller holds it exclusively, on its device):
void planes_drop(ott_store* own);     // the rows moved or changed wholesale: every plane goes (rebuilt on demand)
bool planes_any(ott_store* own);      // a plane is there (its buffer would be given back by planes_drop)
void planes_release(ott_store* own);  // ott_store_destroy: planes_drop + the loss words
int planes_rewrite(ott_store* s, uint64_t first, uint64_t n);  // rows [first, first + n) were rewritten: converted again where a plane covers them; waits
int planes_clear_marks(ott_store* s, uint64_t n);              // the planes' marks (bits 1, 2) in the flag bytes of rows [0, n), on s->stream
void planes_enable(ott_store* own, bool enabled);              // ott_store_set_batch_image: off = drop and decline all three, on = allow them again
void planes_set_options(ott_store* own, const Options& o);     // own->opt = o; a plane that an option declined is allowed again once the option allows it
// The query side: built / extended on demand
int ensure_batch_image(ott_store* ctx, const uint16_t** img_out);
int ensure_hi_plane(ott_store* ctx, const uint16_t** img_out, float* rel_max_out, bool* f16_out = nullptr, float* scale_out = nullptr);  // *img_out = nullptr when unavailable
bool hi_plane_ready(ott_store* ctx);  // the plane exists and covers every row (nothing is built by asking)
inline bool i8_wanted(const Options& o) { return i8_wanted(o.hi_fmt, o.mfma_f32, o.no_hi_pass, o.no_batch_image); }
// the plane the cascade STARTS with on this store — the int8 plane where the options ask for it and it fits, else the hi plane —
// built / extended now (background builder, ott_store_prepare_batch); an existing hi plane is kept up to date beside it
int ensure_first_plane(ott_store* ctx);
bool first_plane_ready(ott_store* ctx);
// What the planes look like right now, read under the planes' mutex (ensure_i8_plane / ensure_hi_plane change these fields from other query
// contexts while the store is only held shared): the AUTO cost model, the background builder and kick_plane_build decide from this
// snapshot.  A snapshot may be stale by the time it is used — every consumer only chooses a path or skips a build from it, and the
// ensure_* calls that follow re-read the fields under the mutex.
struct PlaneSnapshot {
    bool have_i8, i8_off, have_hi, hi_f16, hi_off, img_off;
    uint64_t i8_rows, hi_rows;
};
PlaneSnapshot plane_snapshot(const ott_store* s);
// the store's int8 plane (option hi_fmt = -1 / 2), built / extended on demand; *img_out = nullptr when it is unavailable
int ensure_i8_plane(ott_store* ctx, const int8_t** img_out, const float** scale_out, float* rel_max_out);
bool i8_plane_ready(ott_store* ctx);
bool i8_plane_peek(ott_store* ctx, const int8_t** img_out, const float** scale_out, float* rel_max_out);  // false unless i8_plane_ready; builds nothing
// f32 rows -> int8 rows of pitch ld8 bytes.  common_scale > 0: every row quantised with THAT scale (the query operand block: one
// scale per batch, so that it folds into the kernel's row factors); else per row max|x| / 127, written to scale_out[r].
// pre[r] (optional): the row is multiplied by it first (cosine: 1 / ||q||).  rel_out[r] (optional) = ||x - s x~|| / ||x||.
int launch_i8_rows(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ld8, uint64_t first, uint64_t n, int8_t* out,
                   const float* pre, float common_scale, float* scale_out, float* rel_out, uint32_t* rel_max, const uint8_t* flag, float rel_flag,
                   uint8_t* flag_rw, int n_cu);
// f32 rows -> bf16 (RNE) rows of pitch ldh elements (optionally row-scaled first); rel_out[r] (optional) = ||x - bf16(x)|| / ||x||
int launch_hi_rows(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ldh, uint64_t n, uint16_t* out,
                   const float* scale, float* rel_out, int n_cu, bool f16 = false, float gscale = 1.0f);  // f16: IEEE half of x * scale[r] * gscale (gscale a power of two)
int launch_split_rows(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ldi, uint64_t n, uint16_t* out,
                      const float* scale, int n_cu);  // f32 rows -> [32 hi | 32 lo] bf16 per 32-k stage (optionally row-scaled first)
}  // namespace ott

namespace ott {

// ---- key transform shared by all top-k code ---------------------------------------------------
// total order on f32 bits (== Rust f32::total_cmp): ascending unsigned == ascending total_cmp
__host__ __device__ inline uint32_t total_key(float f) {
    uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = __float_as_uint(f);
#else
    __builtin_memcpy(&b, &f, 4);
#endif
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// "larger is better" ordinal for the requested take type; 0 is never produced by a non-NaN
__host__ __device__ inline uint32_t ord_of(float f, bool take_max) {
    uint32_t k = total_key(f);
    return take_max ? k : ~k;
}
__host__ __device__ inline float score_of(uint32_t ord, bool take_max) {
    uint32_t k = take_max ? ord : ~ord;
    uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(b);
#else
    __builtin_memcpy(&f, &b, 4);
#endif
    return f;
}

// One candidate in a block/partial list: key = ord<<32 | ~local_row  (bigger = better; lower
// row wins ties), q = query id (lower wins remaining ties).  16 bytes.
struct Cand {
    uint64_t key;
    uint32_t q;
    uint32_t pad;
};

// ---- launch wrappers (defined in the .hip files) ----------------------------------------------
struct ExactParams {
    const float* rows;
    const float* inv;
    const float* queries;  // [nq_total * dimq], zero padded
    const float* qinv;     // [nq_total]
    const uint64_t* row_mask;
    const ott_run* runs;
    const uint32_t* tile_prefix;  // [n_runs + 1]
    Cand* lists;                   // [n_lists_per_block? see ott_exact.hip]
    uint64_t row_mask_bits;
    uint32_t ld, dim, dimq;
    uint32_t n_runs, n_tiles;
    uint32_t q0, nq_total;  // first query of this pass, total queries
    uint32_t metric, take_max, cmp, reduce;
    float thr;
    uint32_t k;      // <= 64*E
    uint32_t perq;   // 1 = one list per query
    uint32_t list_stride;  // entries between consecutive lists in `lists`
    // single-query launches carry their inputs IN the kernel arguments (no H2D copy in front of the launch): the query
    // (zero padded to dimq), its inverse norm, and up to two runs with their tile prefix
    uint32_t tie_sh;  // 0 = canonical tie order (score, row, query); 3 = the reference's visit order (score, row >> 3, query, row & 7)
    uint32_t tie_off; // 0..7, added to the row in every candidate key: the 8-row blocks of the visit order are then counted from row
                      // (8 - tie_off) % 8 of the store instead of row 0 — a chunk whose first row is not a multiple of 8 (tie_order 2,
                      // src/meta_compute.rs:153-192: every chunk is a VecStore of its own); whoever turns keys back into rows subtracts it (tie_base)
    uint32_t flat;    // 1 = every passing score ranks the same: the list keeps the first k passing pairs in visit order (tie_sh = 3)
    uint32_t embedded;
    uint32_t small;  // 1 = small-grid kernel variant (single query, one tile per one-wave workgroup), 2 = rows8 (eight lanes per row, one 8-wave workgroup per tile)
    float eqinv;
    uint32_t eprefix[3];
    ott_run eruns[2];
    // large-k path: every passing (key, query) is appended here instead of the fused top-k
    uint64_t* dump_keys;
    uint32_t* dump_q;
    unsigned long long* dump_cursor;
    uint64_t dump_cap;
    const uint32_t* dump_gate;  // [nq_total] score ordinals a pair must reach to be listed (nullptr = none)
    // int8 candidate sweep of a SINGLE query (round 5, exact_kernel<..., I8>): `rows` is the store's int8 plane (ld = dim = dimq =
    // its row pitch in 4-byte units), the query is int8 too (embedded in qemb), scores are APPROXIMATE — (float)(q~ . v~) x
    // (s_v [x 1/||v||]) x s_Q — and the list keeps the T = k best of them for the exact re-score (run_i8_single, ott_mfma.hip)
    uint32_t i8;
    float i8_qscale;        // s_Q: the query's quantisation scale
    const float* i8_scale;  // [n] s_v
    const uint8_t* flag;    // [n] rows outside the pass's error model (bits 0, 2): always listed, ranked first
    // pruned sweep of a SINGLE query (exact_kernel<..., PRUNE>): at stage prune_stage (0 = off) a row whose
    // score bound (ott_prune.h) ranks strictly below the seed's k-th best is not finished.  prune_seed: the seed launch's merged
    // result block, [count (u64, 64 B) | hits]; prune_qt / prune_qn: upper bounds of ||q[prune_stage * 32:]|| and ||q||
    // Sketch form (prune_sketch != nullptr): the store's tail sign sketch, lines of sk_pitch words whose sign words start at stage
    // sk_stage0 <= prune_stage; prune_q1: an upper bound of the 1-norm of q[prune_stage * 32:].  prune_tails: device counter, += the
    // rows whose tails were finished (both forms)
    uint32_t prune_stage;
    uint32_t sk_pitch, sk_stage0, sk_bits;
    const uint64_t* prune_seed;
    const uint32_t* prune_sketch;
    // the head form of the four-bit sketch (prune_head_codes != nullptr): 16 B of stage 0's codes and rho_all per row, indexed by row
    // like `inv`; the launch then has its checkpoint in front of stage 0 whatever prune_stage says, and the query-side values are
    // taken over the whole query
    const uint32_t* prune_head_codes;
    const float* prune_head_rho;
    unsigned long long* prune_tails;
    double prune_qt, prune_qn, prune_q1;
    // four bits per dim: the quantised query of the integer decode (ott_prune.h: PruneQuant) — the scale 2^e and its reciprocal, an
    // upper bound of the tail's quantisation error in the 1-norm, the tail's integer sum.  The kernel quantises the query itself.
    double prune_qe1;
    float prune_qscale, prune_qinv_scale;
    int32_t prune_qsum;
    // the seed as an estimate pass (head form, ott_exact_plan.h: prune_plan_seed_est): seed_est = 1 runs the launch without a gate —
    // rows are ranked by the decode's estimate and each wave finishes its seed_keep best exactly; no prune_seed, no prune_tails
    uint32_t seed_est, seed_keep;
    // the int8 check of the head form's survivors (gated launch, ott_exact_plan.h: prune_plan_i8_check): chk_plane != nullptr = the
    // store's int8 plane (rows of dim rounded up to 128 bytes), with i8_scale, flag and i8_qscale as on the int8 sweep above; chk_eps:
    // the certified |approximate - exact-order score| of this query (ott_i8_check.h: i8_check_eps).  prune_tails then holds two
    // counters: [0] rows that passed the line gate, [1] rows finished in f32
    const int8_t* chk_plane;
    float chk_eps;
    float qemb[OTT_QEMB_MAX];  // last: the embedded query (kernel arguments are limited to 4 KB)
};
// (OTT_QEMB_MAX and the OTT_SKETCH*_MAX_WORDS limits of the sketch forms: ott_exact_plan.h)
static_assert(sizeof(ExactParams) <= 4096, "kernel arguments are limited to 4 KB");

int launch_exact(ott_store* s, const ExactParams& p, int nq_tile, int E, int grid);
int launch_exact_i8(ott_store* s, const ExactParams& p, int E, int grid);  // p.i8 = 1: one query, approximate int8 scores, list of 64 E candidates
int launch_exact_dump(ott_store* s, const ExactParams& p, int nq_tile, int grid);  // nq_tile: 1 or 4
int exact_grid(const ott_store* s, uint32_t n_tiles);
// merges `n_lists` sorted partial lists of k entries (stride list_stride) per output group
// (groups = 1 for MERGED, nq for PER_QUERY; group g's lists start at g*group_stride) into
// out_hits[g*out_stride ...] and out_counts[g]
int launch_merge(ott_store* s, const Cand* lists, uint32_t n_lists, uint32_t list_stride, uint64_t group_stride,
                 uint32_t groups, uint32_t k, int E, bool take_max, uint64_t base_offset, ott_hit* out_hits,
                 uint64_t out_stride, uint64_t* out_counts, uint32_t tie_sh, unsigned long long* tails = nullptr, unsigned long long* totals = nullptr);
// (totals != nullptr: the pruned sweep's final merge on host output — the launch also copies the two counters at `tails` to `totals`)

// hdr_slots: ott_hit-sized header slots behind every rank's [n_groups][list_len] hits (the blocks of ott_query_sharded); they are
// copied to hdr_out ([n_lists][hdr_slots], e.g. pinned host memory) by the same launch
int launch_merge_hits(ott_store* s, const ott_hit* lists, uint32_t n_lists, uint32_t n_groups, uint32_t list_len, uint32_t k, int E,
                      bool take_max, ott_hit* out, uint64_t* count, uint32_t hdr_slots = 0, ott_hit* hdr_out = nullptr);

// ott_tomb.hip: the live mask of deleted rows.  live_grow: the rows were reallocated to ncap slots (realloc_store); live_drop: the
// mask goes (every row counts as live again: store_adopt, compact); live_load: the mask of rows [0, s->n) from host words (a
// multi-GPU store moves its rows between shards: the bits travel through the host); live_compose: the row mask a query's
// kernels get — the caller's (device words or nullptr) ANDed with the live mask over s->n bits, in the context's scratch; a
// store without deletions gets its arguments back untouched.  All but live_compose need the store exclusively.
int live_grow(ott_store* s, uint64_t ncap);
void live_drop(ott_store* s);
int live_load(ott_store* s, const uint64_t* words_host);
int live_read(const ott_store* s, uint64_t* out_host);  // (n + 63) / 64 words, bits past n zero; the caller holds the store (shared)
int live_compose(ott_store* ctx, const uint64_t** d_mask, uint64_t* mask_bits);
// out[w] = keep[w] & caller[w] over the words of n_bits rows, on the context's stream; caller bits at and past caller_bits count as keep
int mask_and(ott_store* ctx, const uint64_t* keep, const uint64_t* caller, uint64_t caller_bits, uint64_t n_bits, uint64_t* out);
// ott_store.hip: rows [0, new_n) are what ott_store_compact left — sketch lines again, planes and evaluated mask dropped
int store_after_compact(ott_store* s, uint64_t new_n);
int launch_inv_norms(ott_store* s, uint64_t first_row, uint64_t n_rows);  // + the tail sign sketch of the same rows where the store keeps one
bool store_wants_sketch(const ott_store* s);
int update_min_pos_inv(ott_store* s, uint64_t first_row, uint64_t n_rows);  // call after launch_inv_norms; syncs

// surviving chunk runs of one query (candidate_chunks, src/meta.rs:648-659)
struct RunPlan {
    std::vector<ott_run> runs;
    uint64_t rows_scored = 0, total_chunks = 0, evaluated = 0;
};
std::vector<uint32_t> tile_prefix(const RunPlan& pl, uint32_t tile_rows);
void split_plan(const RunPlan& pl, uint64_t m_rows, RunPlan& a, RunPlan& b);  // the first m_rows rows of a plan and the rest

// large-k path (k > 512): score dump + device radix sort.  Entries [0, *n_entries) of (l_keysA|B, l_qA|B) are left sorted in
// canonical order (merged) or grouped by query (per-query); results are copied to `lists`.
int run_large_k(ott_store* s, const float* queries, uint32_t nq, const ott_query_desc* d, bool perq, const RunPlan& pl, uint64_t k_eff,
                const uint64_t* d_mask, uint64_t mask_bits, std::vector<std::vector<ott_hit>>& lists, ott_stats& st);
void fill_exact_params(ott_store* s, const ott_query_desc* d, const RunPlan& pl, uint32_t nq, const uint64_t* d_mask, uint64_t mask_bits,
                       uint32_t n_tiles, ExactParams& p);
float host_inv_norm_exact(const float* v, uint32_t dim);  // ott_api.hip: the query-side inverse norm in the reference's order
// ONE query's inputs into the kernel arguments of `p` (a lean call, ott_exact_plan.h: exact_lean): the query's `query_bytes` bytes, its
// inverse norm, and the plan's at most two runs with their tile prefix.  The query's tail up to dimq is whatever `p` held (zero
// after fill_exact_params); n_runs and n_tiles stay the caller's.
void embed_exact_inputs(ExactParams& p, const void* query, size_t query_bytes, float inv_norm, const RunPlan& pl, const std::vector<uint32_t>& prefix);
int upload_exact_inputs(ott_store* s, const float* queries, uint32_t nq, const RunPlan& pl, const std::vector<uint32_t>& prefix);

// MFMA batch path: per-query exact top-k lists on the host; uncertified[q] != 0 means the
// list for q could not be certified and must be recomputed on the exact path.
// level 0 = hi pass (16-bit hi plane, one MFMA per 16 k; needs mfma_hi_k_ok), level 1 = split-bf16 / f32-pipe pass, level 2 = int8 pass.
// How many candidates a level re-scores and the bound it certifies against: ott_mfma_plan.h (level_budget, error_model)
int run_mfma(ott_store* s, const ott_query_desc* d, const RunPlan& pl, uint64_t k_q, const uint64_t* d_mask, uint64_t mask_bits,
             std::vector<std::vector<ott_hit>>& out, std::vector<uint32_t>& uncertified, ott_stats& st, int level, uint32_t t_min,  // t_min: re-score at least this many (0, 512, 4096; ott_mfma_plan.h: level_budget)
             bool spec_gate);  // speculative emission thresholds between the row rounds (select_kernel); first level of a cascade only
int launch_rand_fill(ott_store* s, uint64_t first_row, uint64_t n_rows, uint64_t seed);
// ott_mfma.hip: the int8 level for ONE query as a streaming sweep (no matrix cores: the query is a vector) — exact_kernel<..., I8>
// over the int8 plane with a wave-list top-T in its epilogue, merge, exact re-score + certification (finalize_kernel): three
// launches and one wait instead of the cascade's five rounds.  Same outputs as run_mfma.
int run_i8_single(ott_store* s, const ott_query_desc* d, const RunPlan& pl, uint64_t k_q, const uint64_t* d_mask, uint64_t mask_bits,
                  std::vector<std::vector<ott_hit>>& out, std::vector<uint32_t>& uncertified, ott_stats& st, uint32_t t_min);

// canonical result order shared with the oracle: better score (total order on the bits), lower row, lower query.
// sh = 3 (tie_order = reference): better score, then the reference's visit order — 8-row block, query, row within the block
// (`base`: the store's base offset; blocks are counted from the store's first row, src/vec.rs:222-303)
struct CanonLess {
    bool tmax;
    uint32_t sh = 0;
    uint64_t base = 0;
    bool operator()(const ott_hit& a, const ott_hit& b) const {
        const uint32_t ka = ord_of(a.score, tmax), kb = ord_of(b.score, tmax);
        if (ka != kb) return ka > kb;
        if (sh) {
            const uint64_t ba = (a.index - base) >> sh, bb = (b.index - base) >> sh;
            if (ba != bb) return ba < bb;
            if (a.query != b.query) return a.query < b.query;
            return a.index < b.index;
        }
        if (a.index != b.index) return a.index < b.index;
        return a.query < b.query;
    }
};
// G-way merge of lists that are each in `less` order: the next n hits go to dst, the heads move on.  The heads' score ordinals
// are kept beside them (smaller = better): the scan compares integers and falls back to the full order only between equal
// scores (recomputing both ordinals in every comparison cost 22 ns per hit on 8 lists).  The caller guarantees n <= the hits left.
inline void merge_heads(std::vector<const ott_hit*>& head, const std::vector<const ott_hit*>& end, const CanonLess& less, ott_hit* dst, uint64_t n) {
    const size_t G = head.size();
    std::vector<size_t> act(G);
    std::vector<uint32_t> key(G);
    size_t n_act = 0;
    for (size_t g = 0; g < G; g++)
        if (head[g] != end[g]) {
            key[n_act] = ~ord_of(head[g]->score, less.tmax);
            act[n_act++] = g;
        }
    for (uint64_t i = 0; i < n; i++) {
        size_t bi = 0;
        for (size_t a = 1; a < n_act; a++)
            if (key[a] < key[bi] || (key[a] == key[bi] && less(*head[act[a]], *head[act[bi]]))) bi = a;
        const size_t b = act[bi];
        dst[i] = *head[b]++;
        if (head[b] == end[b]) {
            --n_act;
            act[bi] = act[n_act];
            key[bi] = key[n_act];
        } else {
            key[bi] = ~ord_of(head[b]->score, less.tmax);
        }
    }
}

// ott_api.hip.  check_desc_enums, check_device_row_mask: the descriptor's enum fields are known ones, and use_device_row_mask has an
// evaluated mask to use — for entry point `who`, which the messages name.  validate_query: argument checks of ott_query.  query_on: one query on a context whose `mu` the caller
// holds (and the owner's `rw`, shared).  Device output (out_dev != nullptr): [groups][cap / groups] slots, sentinel
// padded.  nosync: do not wait for the stream before returning — on the EXACT path nothing then waits on the host at all
// (*events_pending tells the caller to read the kernel timing events ev[3..5] after its own synchronisation).
int check_desc_enums(const char* who, const ott_query_desc* d);
int check_device_row_mask(const char* who, const ott_store* s, const ott_query_desc* d);
int validate_query(const ott_store* s, const ott_query_desc* d);
int query_on(ott_store* s, const ott_query_desc* d, ott_hit* out_host, void* out_dev, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
             void* n_out_dev, ott_stats* stats_out, bool nosync = false, bool* events_pending = nullptr);
// One plain query on a context (what query_on was before the tie orders): `tie_sh` selects the candidate order of every
// kernel and host merge of this call, `flat` makes every passing score rank the same (EXACT path only: the first k passing
// pairs in visit order).  Host output only when either is set.
struct CoreOpts {
    uint32_t tie_sh = 0;
    bool flat = false;
    uint32_t tie_off = 0;  // with tie_sh = 3: 8-row blocks are counted from local row (8 - tie_off) % 8 (see ExactParams::tie_off)
};
// the base that turns a candidate key's row field back into a global index, and from which CanonLess counts 8-row blocks
inline uint64_t tie_base(const ott_store* s) { return s->base_offset - s->cur_tie_off; }
int query_core(ott_store* s, const ott_query_desc* d, ott_hit* out_host, void* out_dev, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
               void* n_out_dev, ott_stats* stats_out, bool nosync, bool* events_pending, const CoreOpts& co);
// ott_api.hip: the row mask the kernels of a query get (caller's or evaluated mask & id list on the mask route & live mask), nullptr = none
int compose_row_mask(ott_store* s, const ott_query_desc* d, const uint64_t** d_mask, uint64_t* mask_bits);
// ott_masks.hip: a row mask per query.  masks_join: the mask a by-mask-group run's kernels get — *d_mask (device words or nullptr)
// ANDed with the context's cur_qmask over s->n rows, in the context's scratch; bits at and beyond either mask's count are kept.
// mask_slots_drop: every device mask slot is emptied and its memory given back (the caller holds the store exclusively, on its device).
// ott_mask.hip: eval_row_mask_into — ott_store_eval_row_mask's checks, kernel and wait for entry point `fn`, the words into `dst`
// (*dst_bits = the rows they cover, 0 while they are being made); the caller holds the store exclusively and `mu`.
int masks_join(ott_store* s, const uint64_t** d_mask, uint64_t* mask_bits);
void mask_slots_drop(ott_store* s);
int eval_row_mask_into(ott_store* s, const char* fn, const ott_leaf* leaves, uint32_t n_leaves, DevBuf& dst, uint64_t* dst_bits, uint64_t* out_host);
// ott_multi.hip: candidate id lists on a multi-GPU store (ott_gather.hip).  ids: ascending, duplicate-free, every id < the store's length
int multi_query_ids(ott_store* ms, const ott_query_desc* d, const std::vector<uint64_t>& ids, ott_hit* out, uint64_t cap, uint64_t* n_out,
                    uint64_t* n_per_query, ott_stats* stats);
int multi_score_rows(ott_store* ms, const float* queries, uint32_t nq, uint32_t metric, const uint64_t* ids, uint64_t n_ids, float* out_scores);
// ott_gather.hip: ott_query_ids on a context whose `mu` the caller holds (and the owner's `rw`, shared), for ott_query_mmr's first stage.
// u: the list ascending and duplicate-free (ids of cleared chunks are dropped from it), d->k = min(k, pool) >= 1, n_listed: the ids as listed
int query_ids_on(ott_store* ctx, const ott_query_desc* d, std::vector<uint64_t>& u, uint64_t n_listed, ott_hit* out, uint64_t cap, uint64_t* n_out,
                 uint64_t* n_per_query, ott_stats* stats);
int check_ids(const char* who, const uint64_t* ids, uint64_t n_ids, uint64_t len);  // an id list's argument errors, for entry point `who`
// Grouped search (ott_group.hip).  group_grow: the rows were reallocated to ncap slots (realloc_store keeps the ids that are there);
// group_drop: the ids go.  make_run_plan (ott_api.hip): chunk mask -> runs of surviving chunks, as every query builds them.
// sort_group_pairs (ott_sort.hip): the n (key, query) pairs a grouped query compacted into (l_keysA, l_qA) through the radix sort,
// grouped by query and best first; lists[q] = the first k of query q's pairs as hits.
int group_grow(ott_store* s, uint64_t ncap);
int group_ids_of_hits(ott_store* s, const ott_hit* hits, uint64_t n, uint32_t* out);  // the groups of hits of this store: a gather from the resident ids
void group_drop(ott_store* s);
void binary_drop(ott_store* s);  // ott_binary.hip: the bit rows go (the caller holds the store exclusively, on its device)
void sparse_drop(ott_store* s);  // ott_sparse.hip: the sparse rows go (the caller holds the store exclusively, on its device)
// ott_sparse.hip, for ott_query_hybrid (ott_fuse.hip).  run_sparse_sweep: the sparse sweep on a context whose `mu` the caller holds
// (and the owner's `rw`, shared); k_eff = min(k, rows the chunk mask leaves) >= 1, the queries checked against the store's vocab.
// sparse_df_ensure: the owner's document frequencies are those of the sparse rows and the live mask as they are now (built on
// ctx's stream when they are not).  sparse_idf_scale: out[e] = fl32(q_val[e] * idf(q_idx[e])) from the cache sparse_df_ensure left.
int run_sparse_sweep(ott_store* s, const ott_query_desc* d, const uint64_t* q_indptr, const uint32_t* q_idx, const float* q_val, uint64_t k_eff, ott_hit* out,
                     uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats_out);
int sparse_df_ensure(ott_store* ctx);
void sparse_idf_scale(const ott_store* own, const uint32_t* q_idx, const float* q_val, uint64_t q_nnz, float* out);
inline void sparse_df_stale(ott_store* s) { s->sparse_gen++; }  // the caller holds the store exclusively
void make_run_plan(const ott_store* s, const uint64_t* chunk_mask, RunPlan& pl);
// id_span: the low key words are ~id with id < id_span (0 = the store's rows, what a grouped query's keys hold; a late-interaction
// query's hold group ids)
int sort_group_pairs(ott_store* s, uint64_t n, uint32_t nq, bool take_max, uint64_t k, std::vector<std::vector<ott_hit>>& lists, uint64_t id_span = 0);
int ensure_group_pairs(ott_store* s, uint64_t cap);  // the pair arrays for up to `cap` pairs
// The host half of a sweep over grouped rows (ott_group.hip; ott_maxsim.hip uses it too).  sweep_prologue: stats, run plan, mask,
// upload, the kernel parameters of ott_sweep_dev.h and the grid (0 = no rows).  ensure_zeroed: a table that is zero when a query
// finds it.  check_group_ids: the ids are set and cover the store, for entry point `fn`, before and under the lock.
struct SweepParams;
// sweep_plan: the part of it that needs no query block — the stats of `nq` queries, the run plan and, where a row survives the chunk
// mask, the composed row mask (ott_sparse.hip's sweep reads no dense rows and takes only this)
int sweep_plan(ott_store* s, const ott_query_desc* d, uint32_t nq, ott_stats* st, RunPlan* pl, const uint64_t** row_mask, uint64_t* row_mask_bits);
int sweep_prologue(ott_store* s, const ott_query_desc* d, ott_stats* st, SweepParams* p, uint32_t* grid);
int sweep_prologue(ott_store* s, const ott_query_desc* d, const float* queries, uint32_t nq, ott_stats* st, SweepParams* p, uint32_t* grid);  // queries: nullptr = nq zeroed slots
int ensure_zeroed(ott_store* s, DevBuf& b, bool& clean, size_t bytes);
int check_group_ids(const ott_store* s, const char* fn, bool locked);
// The top-k over a table of [queries of a pass][n_groups] 8-byte keys in d_gtable (0 = empty): prepare, pass() after every sweep
// (k <= 512: the select kernel's block lists; above: the compact kernel's (key, query) pairs; both leave the slots zeroed), finish
// (launch_merge into the pinned block or sort_group_pairs, hits and counts out, gtable_clean — and *also_clean — after the sync).
struct GroupTopK {
    uint32_t n_groups = 0, nq = 0;  // nq: the queries whose lists come out
    uint64_t k = 0;
    bool take_max = false;
    bool index_is_group = false;    // the keys' low words are ~group, not ~row: a hit's index is the group, the count is cut at k
    bool* also_clean = nullptr;
    uint64_t id_span = 0;           // index_is_group: the ids in the keys stay below this (0 = n_groups; a listed query's table has fewer slots than the store has groups)
    uint64_t q_stride = 0;          // slots between the tables of two queries of a pass; 0 = n_groups (ott_group_top.hip: group_size x n_groups)
    bool lists_path = false;        // from here on: prepare's
    int E = 1;
    uint32_t KS = 0, n_lists = 0;
    uint64_t pair_cap = 0;
    // k <= 512 only: called behind the merge kernel, before the host waits, with the device's view of the pinned hits and counts
    // (ott_discover.hip looks up a per-hit value there); nullptr = nothing
    int (*after_merge)(ott_store* s, void* arg, const ott_hit* d_hits, const uint64_t* d_counts) = nullptr;
    void* after_arg = nullptr;
    int prepare(ott_store* s, const char* too_many_pairs);  // the refusal's text for more than 2^32 - 16 pairs (nullptr: cannot happen)
    int pass(ott_store* s, unsigned long long* table, uint32_t q0, uint32_t nq_here);
    int finish(ott_store* s, bool timing, ott_hit* out, uint64_t* n_out, uint64_t* n_per_query);
};
// ott_recommend.hip: the host frame of a sweep whose queries are EXAMPLE ROWS of the store (recommend, sum_scores, discover), on a
// context whose `mu` the caller holds.  A run calls the steps in this order and puts what is its own between them:
//   begin    sweep_prologue (host_block: a query block that goes up from the host, nullptr = n_slots zeroed slots), bytes_scanned,
//            the 8-byte state per row (d_rectable) and the key table (d_gtable) zero, p->gid = nullptr.  grid == 0 after it: no row
//            survives, nothing else is called but end
//   prepare  the rows to gather and the top-k over the key table with one "group" per row
//   sweep    example_gather_kernel, ev[3], a launch_pass(q0) per pass of `tile` slots, example_clear_kernel (an example is no candidate)
//   rank     behind the run's keys kernel(s): tk.pass, ev[4]
//   finish   tk.finish, the events, the "more hits than k" failure
//   end      total_ns, the stats out
struct ExampleFrame {
    ott_store* s;
    const ott_query_desc* d;
    const char* who;  // the entry point the messages name
    uint64_t k_eff;
    ott_stats* stats_out;
    uint64_t t0 = now_ns();  // total_ns counts from the frame's construction
    ott_stats st;
    uint32_t grid = 0;
    uint32_t n = 0;                      // the store's rows
    uint2* state = nullptr;              // [n]
    unsigned long long* keys = nullptr;  // [n]
    const uint32_t* rows = nullptr;      // the gathered rows, every one below n
    uint32_t n_rows = 0;
    GroupTopK tk;
    bool timing() const { return stats_out != nullptr; }
    int begin(SweepParams* p, const float* host_block, uint32_t n_slots);
    int prepare(const uint32_t* gather_rows, uint32_t n_gather, bool tk_take_max, bool* also_clean);
    int sweep(uint32_t tile, const std::function<int(uint32_t q0)>& launch_pass);
    int rank();
    int finish(ott_hit* out, uint64_t* n_hits);
    void end();
};
// ott_group.hip: the grouped query on a context whose `mu` the caller holds; k_eff = min(k, n_groups) >= 1
int run_groups(ott_store* s, const ott_query_desc* d, uint64_t k_eff, ott_hit* out, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats_out);
// ott_maxsim.hip: the late-interaction query on a context whose `mu` the caller holds; k_eff = min(k, n_groups) >= 1.  The reduce
// kernel's launch: slot g of `table` ([nq][n_slots] ordinals) is group gid_of[g] (nullptr: group g) in the key it writes to keys[g].
int run_maxsim(ott_store* s, const ott_query_desc* d, uint64_t k_eff, ott_hit* out, uint64_t* n_out, ott_stats* stats_out);
int launch_maxsim_reduce(ott_store* s, uint32_t* table, uint32_t n_slots, uint32_t nq, uint32_t take_max, uint32_t cmp, float thr, unsigned long long* keys,
                         const uint32_t* gid_of);
// ott_maxsim_gather.hip: the group-to-rows index of listed MaxSim.  group_index_drop: with the group ids (group_drop calls it; the
// caller holds the store exclusively)
void group_index_drop(ott_store* s);
// ... and what ott_query_maxsim_groups does around and under its lock, for ott_maxsim_batch.hip (`fn`: the entry point the messages
// name).  check_listed_groups: every listed id is below n_groups.  maxsim_groups_lock: the store shared through lock_shared_clean
// (staged appends and the index settled in the clean step).  maxsim_groups_locked: one listed query under that lock — ids and list
// checked again, k_eff, the route, a context, the run.
int check_listed_groups(const char* fn, const uint32_t* groups, uint64_t n_listed, uint32_t n_groups);
int maxsim_groups_lock(ott_store* s, const char* fn, ott::host::SharedLock& rd);
int maxsim_groups_locked(ott_store* s, const ott_query_desc* d, const uint32_t* groups, uint64_t n_groups_listed, ott_hit* out, uint64_t cap, uint64_t* n_out,
                         ott_stats* stats, const char* fn);
// ott_multi.hip: grouped search on a multi-GPU store
int multi_set_groups(ott_store* ms, const uint32_t* gid_host, uint64_t n, uint32_t n_groups);
int multi_clear_groups(ott_store* ms);
int multi_query_groups(ott_store* ms, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);
// ott_ties.hip is written against this: where the candidate lists of a store come from.  `run`: one plain query over what `d`
// selects with take count k, candidates ranked (score, visit order: tie_sh = 3), `flat` = every passing score ranks the same
// (EXACT path); host vectors, PER_QUERY lists concatenated in query order with their counts in `per`.  `run_chunk`: the same
// restricted to ONE chunk (counted from `base`; whatever chunk mask `d` carries is replaced).
struct TieEnv {
    // (run_chunk ranks equal scores by the CHUNK's own 8-row blocks — counted from the chunk's first row, whatever the chunk size:
    //  the chunk is a VecStore of its own in the reference, src/meta_compute.rs:153-192)
    typedef std::function<int(const ott_query_desc& d, uint64_t k, bool flat, std::vector<ott_hit>& out, std::vector<uint64_t>& per, ott_stats* st)> Runner;
    bool tmax = true;
    uint64_t base = 0;        // global index of the (whole) store's first row: 8-row blocks and chunks are counted from here
    uint64_t chunk_size = 1024;
    uint64_t rows = 0;        // the whole store's rows (tie order 2 walks its chunks when the cut runs through the zeros)
    uint32_t dim = 0;
    Runner run;
    std::function<int(uint64_t chunk, const ott_query_desc& d, uint64_t k, bool flat, std::vector<ott_hit>& out, std::vector<uint64_t>& per, ott_stats* st)> run_chunk;
};
int ref_ties_collect(const TieEnv& env, int tie_order, const ott_query_desc* d, ott_hit* out_host, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                     ott_stats* stats_out);
bool ties_ambiguous(bool tmax, const std::vector<ott_hit>& L, uint64_t k);
int ties_resolve(ott_store* s, bool tmax, uint64_t base, const std::vector<ott_hit>& L, uint64_t k, const std::vector<ott_hit>* fill,
                 std::vector<ott_hit>& out);
// ott_ties.hip: the reference's outcome at exact score ties (store option tie_order = 1 / 2), host output
int query_ref_ties(ott_store* s, const ott_query_desc* d, ott_hit* out_host, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                   ott_stats* stats_out);
void read_exact_events(ott_store* s, ott_stats* st);  // after a synchronisation: score_ns / merge_ns from ev[3..5]
int launch_pack_rows(ott_store* s, const float* dense_dev, uint64_t first_row, uint64_t n_rows);

}  // namespace ott
