// ott_store.hip — device-resident VecStore: one contiguous row-major f32 matrix in HBM
// plus per-row inverse norms (src/vec.rs:338-384).  The reference keeps one heap allocation
// per chunk (src/meta.rs:203-281); here a chunk is just a row range of the one matrix.
#include <stdlib.h>
#include <string.h>

#include <thread>

#include <algorithm>

#include "ott_internal.h"
#include "ott_prune.h"

namespace ott {

static thread_local std::string g_err;

void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
const char* last_error() { return g_err.c_str(); }

// ---- per-store options ----------------------------------------------------------------------
namespace {
struct OptName {
    const char* name;
    int kind;  // 0 = bool, 1 = tri-state (-1 automatic / 0 / 1), 2 = non-negative int
};
// the twenty-nine options of the product library (see struct Options) ...
const OptName kOptNames[] = {{"tie_order", 2},       {"hi_fmt", 1},          {"hi_prebuild", 1},          {"stage_appends", 1},       {"multi_transport", 2},
                             {"multi_rebalance", 0}, {"multi_min_shard_rows", 2}, {"exact_small", 1},     {"large_k_from", 2},        {"small_sort", 1},
                             {"mfma_f32", 0},        {"no_hi_pass", 0},      {"no_batch_image", 0},       {"force_fallback", 2},      {"eps_scale_ppm", 2},
                             {"multi_fake_distinct", 0}, {"exact_prune", 1},            {"exact_sketch", 1},
                             {"id_gather", 1},       {"exact_sketch_bits", 2},   {"group_gather", 1},         {"exact_sketch_head", 1},
                             {"masks_sweep", 2},     {"fuse_device", 1},         {"sparse_table", 1},         {"exact_i8_check", 1},
                             {"sparse_df_lds", 1},    {"binary_gate", 1},         {"binary_gate_cap", 2},
#ifdef OTT_MFMA_DEBUG_BUILD
                             // ... and, in the diagnostic build only, kernel tuning, timing ablations and every fallback bit by its own name
                             {"mfma_wg", 2},         {"mfma_growth", 2},     {"mfma_debug", 0},           {"mfma_abl", 2},            {"hi_tmin", 2},
                             {"mfma_no_dense", 0},   {"mfma_coop", 1},       {"mfma_spec", 1},            {"large_k_pre", 1},         {"merge_walk", 0},
                             {"merge_rank1", 1},     {"maxsim_fold", 1},
#endif
};
static_assert(sizeof(kOptNames) / sizeof(kOptNames[0]) <= 29
#ifdef OTT_MFMA_DEBUG_BUILD
                                                            + 12
#endif
              , "the product library's option table stays at twenty-nine entries");
}  // namespace

int option_set(Options& o, const char* name, long long v) {
    if (!name) return -1;
    const std::string n(name);
    auto tri = [&](int& dst) { if (v < -1 || v > 1) return -1; dst = (int)v; return 0; };
    auto flag = [&](bool& dst) { if (v < 0 || v > 1) return -1; dst = v != 0; return 0; };
    if (n == "exact_small") {  // (1, round 2's one-wave variant: diagnostic build only)
#ifdef OTT_MFMA_DEBUG_BUILD
        if (v < -1 || v > 2) return -1;
#else
        if (v < -1 || v > 2 || v == 1) return -1;
#endif
        o.exact_small = (int)v;
        return 0;
    }
    if (n == "force_fallback") {
        if (v < 0 || v > 127) return -1;
        o.force_fallback = (int)v;
        o.merge_walk = (v & 1) != 0;
        o.merge_rank1 = (v & 2) ? 0 : -1;
        o.mfma_coop = (v & 4) ? 0 : -1;
        o.large_k_pre = (v & 8) ? 0 : -1;
        o.mfma_no_dense = (v & 16) != 0;
        o.mfma_spec = (v & 32) ? 0 : -1;
        return 0;
    }
    if (n == "mfma_f32") return flag(o.mfma_f32);
    if (n == "no_hi_pass") return flag(o.no_hi_pass);
    if (n == "no_batch_image") return flag(o.no_batch_image);
    if (n == "hi_fmt") { if (v < -1 || v > 2) return -1; o.hi_fmt = (int)v; return 0; }
    if (n == "small_sort") return tri(o.small_sort);
    if (n == "exact_prune") return tri(o.exact_prune);
    if (n == "exact_sketch") return tri(o.exact_sketch);
    if (n == "exact_sketch_bits") { if (v != 1 && v != 3 && v != 4) return -1; o.exact_sketch_bits = (int)v; return 0; }
    if (n == "exact_sketch_head") return tri(o.exact_sketch_head);
    if (n == "exact_i8_check") return tri(o.exact_i8_check);
    if (n == "id_gather") return tri(o.id_gather);
    if (n == "group_gather") return tri(o.group_gather);
    if (n == "fuse_device") return tri(o.fuse_device);
    if (n == "sparse_table") return tri(o.sparse_table);
    if (n == "sparse_df_lds") return tri(o.sparse_df_lds);
    if (n == "binary_gate") return tri(o.binary_gate);
    if (n == "binary_gate_cap") { if (v < 0 || v > 0x7FFFFFFF) return -1; o.binary_gate_cap = (int)v; return 0; }
    if (n == "masks_sweep") { if (v < 0 || v > 2) return -1; o.masks_sweep = (int)v; return 0; }
#ifdef OTT_MFMA_DEBUG_BUILD
    if (n == "maxsim_fold") return tri(o.maxsim_fold);
    if (n == "mfma_coop") return tri(o.mfma_coop);
    if (n == "mfma_spec") return tri(o.mfma_spec);
    if (n == "mfma_no_dense") return flag(o.mfma_no_dense);
    if (n == "mfma_debug") return flag(o.mfma_debug);
    if (n == "merge_walk") return flag(o.merge_walk);
    if (n == "merge_rank1") return tri(o.merge_rank1);
    if (n == "large_k_pre") return tri(o.large_k_pre);
    if (n == "hi_tmin") { if (v < 0 || v > 512) return -1; o.hi_tmin = (int)v; return 0; }
    if (n == "mfma_abl") { if (v < 0 || v > 63) return -1; o.mfma_abl = (int)v; return 0; }
    if (n == "mfma_wg") { if (v < 0 || v > 8) return -1; o.mfma_wg = (int)v; return 0; }
    if (n == "mfma_growth") { if (v != 0 && (v < 2 || v > 64)) return -1; o.mfma_growth = v ? (int)v : 8; return 0; }
#endif
    if (n == "stage_appends") return tri(o.stage_appends);
    if (n == "hi_prebuild") return tri(o.hi_prebuild);
    if (n == "large_k_from") { if (v < 0 || v > 512) return -1; o.large_k_from = (int)v; return 0; }
    if (n == "eps_scale_ppm") { if (v < 1 || v > 1000000) return -1; o.eps_scale_ppm = (int)v; return 0; }
    if (n == "multi_transport") { if (v < 0 || v > 2) return -1; o.multi_transport = (int)v; return 0; }
    if (n == "multi_fake_distinct") return flag(o.multi_fake_distinct);
    if (n == "multi_rebalance") { if (v < 0 || v > 1) return -1; o.multi_rebalance = (int)v; return 0; }
    if (n == "multi_min_shard_rows") { if (v < 0 || v > 0x7FFFFFFF) return -1; o.multi_min_shard_rows = (int)v; return 0; }
    if (n == "tie_order") { if (v < 0 || v > 2) return -1; o.tie_order = (int)v; return 0; }
    return -1;
}

// OTT_<NAME>=<integer> for every option; a variable that is set but empty counts as 1 (the round-1 knobs were presence tests)
void options_from_env(Options& o) {
    for (const OptName& on : kOptNames) {
        std::string var = "OTT_";
        for (const char* c = on.name; *c; c++) var.push_back((char)(*c >= 'a' && *c <= 'z' ? *c - 32 : *c));
        const char* ev = getenv(var.c_str());
        if (!ev) continue;
        char* end = nullptr;
        long long v = strtoll(ev, &end, 10);
        if (end == ev) v = 1;
        (void)option_set(o, on.name, v);  // an out-of-range value leaves the default
    }
}

int DevBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return OTT_OK;
    size_t want = bytes < 256 ? 256 : bytes;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    OTT_HIP(hipMalloc(&p, want));
    cap = want;
    return OTT_OK;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}
int PinBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return OTT_OK;
    size_t want = bytes < 4096 ? 4096 : bytes;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    OTT_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return OTT_OK;
}
void PinBuf::release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------

// inverse norms in the reference's order (src/vec.rs:365-367): sequential sum of x*x, sqrt,
// 1/norm (0 for a zero norm).  Same lane = row / LDS-transpose scheme as the scorer so the
// loads stay coalesced: a wave stages 64 rows x 128 B per step.
constexpr int NKC = 32;
__global__ __launch_bounds__(256) void inv_norm_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim,
                                                        uint64_t first, uint64_t n, float* __restrict__ inv, uint8_t* __restrict__ flag) {
    __shared__ __attribute__((aligned(16))) float smem[4 * 64 * NKC];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* st = smem + wave * 64 * NKC;
    const uint64_t n_tiles = (n + 63) / 64;
    const int lrow = lane >> 3, lslot = lane & 7, sw = (lane >> 1) & 7;
    const uint32_t nstages = (ld + NKC - 1) / NKC;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wave; t < n_tiles; t += (uint64_t)gridDim.x * 4) {
        const uint64_t row0 = first + t * 64;
        const uint32_t cnt = (n - t * 64) < 64 ? (uint32_t)(n - t * 64) : 64u;
        float s = 0.0f;
        bool nonzero = false;  // any element != 0 (a row of tiny values can have a norm that underflows to 0)
        // branch-free staging like exact_kernel's: every load is issued (rows past a short tile's end clamped to its last
        // row, a column group past `ld` re-reads column 0), out-of-range values are zeroed on their way into LDS; the next
        // stage's loads are in flight while this one is summed; non-temporal (the rows were just written and are read once here)
        typedef float v4f __attribute__((ext_vector_type(4)));
        const float* rp[8];
        bool rok[8];
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint32_t row = 8 * m + lrow;
            rok[m] = row < cnt;
            rp[m] = rows + (row0 + (rok[m] ? row : cnt - 1)) * (uint64_t)ld;
        }
        v4f R[8];
        auto load_stage = [&](uint32_t sg) {
            const uint32_t col = sg * NKC + lslot * 4;
            const uint32_t c = col < ld ? col : 0u;
#pragma unroll
            for (int m = 0; m < 8; m++) R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rp[m] + c));
        };
        load_stage(0);
        for (uint32_t sg = 0; sg < nstages; sg++) {
            const bool cok = sg * NKC + lslot * 4 < ld;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const uint32_t row = 8 * m + lrow;
                const bool ok = rok[m] & cok;
                const v4f v = R[m];
                *reinterpret_cast<float4*>(st + row * NKC + ((lslot ^ ((row >> 1) & 7)) << 2)) =
                    make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (sg + 1 < nstages) load_stage(sg + 1);
#pragma unroll
            for (int j = 0; j < NKC / 4; j++) {
                const float4 a = *reinterpret_cast<const float4*>(st + lane * NKC + ((j ^ sw) << 2));
                const float x[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int l = 0; l < 4; l++)
                    if (sg * NKC + 4 * j + l < dim) {
                        s = __fadd_rn(s, __fmul_rn(x[l], x[l]));
                        nonzero |= x[l] != 0.0f;
                    }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if ((uint32_t)lane < cnt) {
            const float norm = sqrtf(s);  // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt, the default); __fsqrt_rn lowers to the raw 1-ulp v_sqrt_f32
            inv[row0 + lane] = norm != 0.0f ? 1.0f / norm : 0.0f;
            // rows whose norm is inf / NaN / astronomically large break the error bound the MFMA path certifies with:
            // they are flagged and always re-scored exactly there (the exact path needs no flag)
            // ... and rows whose norm is tiny but not zero (below 1e-18: their squares underflow, and the bf16 split may flush
            // their elements): the bound is relative to the norms, so such rows are always re-scored exactly too
            flag[row0 + lane] = (norm <= 1e18f && ((norm == 0.0f && !nonzero) || norm >= 1e-18f)) ? 0 : 1;
        }
    }
}

// synthetic rows: uniform [-1,1), bit-identical to oracle otto_rand_elem
__device__ __forceinline__ float rand_elem(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const uint32_t u = (uint32_t)(z >> 40);
    return __fsub_rn(__fmul_rn((float)u, 1.0f / 8388608.0f), 1.0f);
}

__global__ __launch_bounds__(256) void rand_fill_kernel(float* __restrict__ rows, uint32_t ld, uint32_t dim, uint64_t first,
                                                         uint64_t n, uint64_t global_first, uint64_t seed) {
    // one thread per 4 columns of the padded row
    const uint32_t ld4 = ld / 4;
    const uint64_t total = n * ld4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / ld4;
        const uint32_t c = (uint32_t)(i - r * ld4) * 4;
        float v[4];
#pragma unroll
        for (int l = 0; l < 4; l++) v[l] = (c + l < dim) ? rand_elem(seed, (global_first + r) * dim + c + l) : 0.0f;
        *reinterpret_cast<float4*>(rows + (first + r) * (uint64_t)ld + c) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// Clustered / anisotropic synthetic rows (what embedding corpora look like, and what the batch path's first candidate pass
// may fail to certify): row r belongs to cluster hash(r) % n_clusters and is  centre[cluster][c] + (spread * u(r, c)) * w(c)
// with u uniform [-1,1), w(c) = 1 / (1 + aniso * c / dim) (aniso = 0: the same spread in every dimension).  Counter-based
// and bit-identical to the oracle's otto_clustered_elem, so any row can be rebuilt on the host.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float clustered_elem(uint64_t seed, uint64_t row, uint32_t c, uint32_t dim, uint32_t n_clusters, float spread, float aniso) {
    const uint64_t cl = mix64(seed + 0xC1057E25ull + 0x9E3779B97F4A7C15ull * (row + 1)) % n_clusters;
    const float centre = rand_elem(seed + 0x5EEDull, cl * dim + c);
    const float u = rand_elem(seed, row * dim + c);
    const float w = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(aniso, __fdiv_rn((float)c, (float)dim))));
    return __fadd_rn(centre, __fmul_rn(__fmul_rn(spread, u), w));
}

__global__ __launch_bounds__(256) void clustered_fill_kernel(float* __restrict__ rows, uint32_t ld, uint32_t dim, uint64_t first, uint64_t n,
                                                              uint64_t global_first, uint64_t seed, uint32_t n_clusters, float spread, float aniso) {
    const uint32_t ld4 = ld / 4;
    const uint64_t total = n * ld4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / ld4;
        const uint32_t c = (uint32_t)(i - r * ld4) * 4;
        float v[4];
#pragma unroll
        for (int l = 0; l < 4; l++) v[l] = (c + l < dim) ? clustered_elem(seed, global_first + r, c + l, dim, n_clusters, spread, aniso) : 0.0f;
        *reinterpret_cast<float4*>(rows + (first + r) * (uint64_t)ld + c) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// smallest non-zero inverse norm (positive floats order like their bit patterns)
__global__ __launch_bounds__(256) void min_pos_inv_kernel(const float* __restrict__ inv, uint64_t first, uint64_t n, uint32_t* out) {
    uint32_t best = 0x7F800000u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t b = __float_as_uint(inv[first + i]);
        if (b != 0 && b < best) best = b;  // zero rows (inv = 0) score exactly 0 on every path
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(out, best);
}

int update_min_pos_inv(ott_store* s, uint64_t first_row, uint64_t n_rows) {
    if (!n_rows) return OTT_OK;
    int rc = s->d_minpos.ensure(4);
    if (rc) return rc;
    const uint32_t init = 0x7F800000u;
    OTT_HIP(hipMemcpyAsync(s->d_minpos.p, &init, 4, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(min_pos_inv_kernel, dim3(grid_blocks(n_rows, 256, s->n_cu)), dim3(256), 0, s->stream, s->d_inv, first_row, n_rows,
                       (uint32_t*)s->d_minpos.p);
    OTT_HIP(hipGetLastError());
    uint32_t got = init;
    OTT_HIP(hipMemcpyAsync(&got, s->d_minpos.p, 4, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    float f;
    memcpy(&f, &got, 4);
    if (f < s->min_pos_inv) s->min_pos_inv = f;
    return OTT_OK;
}

// The pruned sweep's tail sketch (ott_prune.h: prune_sketchb_row, the same sums in the same order).  Runs right behind
// inv_norm_kernel for the same rows and reads their sketched stages only (the last quarter of the row at one bit per dim, the last
// 5/8 at three, every stage but the first at four), staged as there: a wave stages 64 rows x 128 B per step, coalesced, then lane = row walks its 32 dims out of LDS.
// BITS > 1: the cell width comes from the tail's largest magnitude, so the stages are walked twice — the maximum first, the codes
// and the sums after it (a rule that needs one walk, the width from the row norm, clips an eighth of the dims of Gaussian rows).
// A lane writes its line in 16-B pieces: the groups of four code words as they fill, [a | rho | word 0 | word 1] at the end.
// BITS = 4: a stage's four code words are one piece, written as the stage ends; [a | rho | 0 | 0] at the end.
// BITS = 4 with a head (head_codes != nullptr; ott_prune.h: prune_sketch4_head_row): stage 0 is walked behind the last sketched
// stage — its codes with the line's cell width into head_codes[4 row ..], its dims added to the line's sums, which then give
// head_rho[row]; the line's own a and rho are taken before that and are what they are without a head.
template <int BITS>
__global__ __launch_bounds__(256) void tail_sketch_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim, uint64_t first, uint64_t n,
                                                           uint32_t stage0, uint32_t n_stages, uint32_t pitch, uint32_t* __restrict__ sketch,
                                                           uint32_t* __restrict__ head_codes, float* __restrict__ head_rho) {
    __shared__ __attribute__((aligned(16))) float smem[4 * 64 * NKC];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* st = smem + wave * 64 * NKC;
    const uint64_t n_tiles = (n + 63) / 64;
    const int lrow = lane >> 3, lslot = lane & 7, sw = (lane >> 1) & 7;
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    auto wave_fence = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wave; t < n_tiles; t += (uint64_t)gridDim.x * 4) {
        const uint64_t row0 = first + t * 64;
        const uint32_t cnt = (n - t * 64) < 64 ? (uint32_t)(n - t * 64) : 64u;
        // branch-free staging as in inv_norm_kernel: rows past a short tile's end clamped to its last row, a column group past
        // `ld` re-reads column 0; lanes past `cnt` sum a copy of the last row and write nothing
        const float* rp[8];
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const uint32_t row = 8 * m + lrow;
            rp[m] = rows + (row0 + (row < cnt ? row : cnt - 1)) * (uint64_t)ld;
        }
        v4f R[8];
        auto load_stage = [&](uint32_t sg) {
            const uint32_t col = sg * NKC + lslot * 4;
            const uint32_t c = col < ld ? col : 0u;
#pragma unroll
            for (int m = 0; m < 8; m++) R[m] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rp[m] + c));
        };
        auto to_lds = [&]() {
#pragma unroll
            for (int m = 0; m < 8; m++)
                *reinterpret_cast<v4f*>(st + (8 * m + lrow) * NKC + ((lslot ^ (((8 * m + lrow) >> 1) & 7)) << 2)) = R[m];
            wave_fence();
        };
        const bool mine = (uint32_t)lane < cnt;
        v4u* line = reinterpret_cast<v4u*>(sketch + (row0 + (mine ? lane : 0)) * (uint64_t)pitch);
        float inv_delta = 0.0f, a_in = 0.0f;
        if constexpr (BITS > 1) {  // first walk: the largest finite magnitude
            uint32_t vmax = 0u;    // (magnitudes of floats order like their bit patterns)
            load_stage(stage0);
            for (uint32_t j = 0; j < n_stages; j++) {
                const uint32_t sg = stage0 + j;
                to_lds();
                if (j + 1 < n_stages) load_stage(sg + 1);
#pragma unroll
                for (int c = 0; c < NKC / 4; c++) {
                    const v4u x = *reinterpret_cast<const v4u*>(st + lane * NKC + ((c ^ sw) << 2));
                    const uint32_t bits[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int l = 0; l < 4; l++) {
                        const uint32_t m = bits[l] & 0x7FFFFFFFu;
                        if (sg * NKC + 4 * c + l < dim && m < 0x7F800000u && m > vmax) vmax = m;
                    }
                }
                wave_fence();
            }
            prune_sketchb_scale(__uint_as_float(vmax), BITS, &inv_delta, &a_in);
        }
        PruneSketchSumsB sums;
        uint32_t w01[2] = {0u, 0u};          // code words 0 and 1: they share the first 16 B with a and rho
        v4u grp = {0u, 0u, 0u, 0u};          // the 16-B piece that is filling (line words 4 g .. 4 g + 3)
        float a = 0.0f, rho = 0.0f;          // the line's, taken behind its last stage
        const uint32_t n_walk = n_stages + ((BITS == 4 && head_codes != nullptr) ? 1u : 0u);
        load_stage(stage0);
        for (uint32_t j = 0; j < n_walk; j++) {
            const uint32_t sg = j < n_stages ? stage0 + j : 0u;  // (the head: stage 0 last)
            to_lds();
            if (j + 1 < n_walk) load_stage(j + 1 < n_stages ? sg + 1 : 0u);
            uint32_t w[BITS];
#pragma unroll
            for (int b = 0; b < BITS; b++) w[b] = 0u;
#pragma unroll
            for (int c = 0; c < NKC / 4; c++) {
                const v4u x = *reinterpret_cast<const v4u*>(st + lane * NKC + ((c ^ sw) << 2));
                const uint32_t bits[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int l = 0; l < 4; l++)
                    if (sg * NKC + 4 * c + l < dim) {  // (dims past `dim` count as zero and are excluded: code 0)
                        int32_t code;
                        if constexpr (BITS > 1) code = prune_sketchb_quant(__uint_as_float(bits[l]), inv_delta, BITS);
                        else code = -(int32_t)(bits[l] >> 31);
                        constexpr uint32_t fmask = (1u << BITS) - 1u;
                        const uint32_t pos = BITS * (4 * c + l), lo = pos & 31u;  // (constants once unrolled)
                        const uint32_t f = (uint32_t)code & fmask;
                        w[pos >> 5] |= f << lo;
                        if (lo + BITS > 32u) w[(pos >> 5) + 1] |= f >> (32u - lo);
                        prune_sketchb_add(sums, bits[l], 2 * code + 1);
                    }
            }
            wave_fence();
            if constexpr (BITS == 4) {  // piece 1 + j is this stage's four words
                if (mine) {
                    if (j < n_stages) line[1 + j] = v4u{w[0], w[1], w[2], w[3]};
                    else reinterpret_cast<v4u*>(head_codes)[row0 + lane] = v4u{w[0], w[1], w[2], w[3]};
                }
            } else {
#pragma unroll
            for (int b = 0; b < BITS; b++) {
                const uint32_t k = 2 + BITS * j + b, slot = k & 3;  // the word's place in the line
                if (k < 4) {
                    w01[0] = k == 2 ? w[b] : w01[0];
                    w01[1] = k == 3 ? w[b] : w01[1];
                } else {
                    grp.x = slot == 0 ? w[b] : grp.x;
                    grp.y = slot == 1 ? w[b] : grp.y;
                    grp.z = slot == 2 ? w[b] : grp.z;
                    grp.w = slot == 3 ? w[b] : grp.w;
                    if (slot == 3 || (j + 1 == n_stages && b == BITS - 1)) {  // (4 (k / 4) + 3 < pitch: the pitch is a multiple of four words)
                        if (mine) line[k >> 2] = grp;
                        grp = v4u{0u, 0u, 0u, 0u};
                    }
                }
            }
            }
            if (j + 1 == n_stages) {
                if constexpr (BITS == 1) a_in = prune_sketchb_mean(sums, dim > stage0 * NKC ? dim - stage0 * NKC : 0u);
                prune_sketchb_finish(sums, a_in, &a, &rho);
            }
        }
        if (mine) line[0] = v4u{__float_as_uint(a), __float_as_uint(rho), w01[0], w01[1]};
        if (n_walk > n_stages) {  // rho_all: the sums over every stage, for the a that is stored
            float a2, rho_all = __builtin_inff();
            if (rho <= 3.4028234e38f) prune_sketchb_finish(sums, a, &a2, &rho_all);
            if (mine) head_rho[row0 + lane] = rho_all;
        }
    }
}

// the head of the four-bit form (ott_prune.h: prune_sketch4_head_row): kept wherever the store keeps four-bit lines, unless the option says never
static bool store_wants_head(const ott_store* s) { return s->d_sketch != nullptr && s->sk_bits == 4 && s->opt.exact_sketch_head != 0; }
static void head_drop(ott_store* s) {
    if (s->d_head) (void)hipFree(s->d_head);
    s->d_head = nullptr;
    s->head_n = 0;
}
// codes at [0, 16 cap), rho_all behind them
static uint32_t* head_codes(const ott_store* s) { return reinterpret_cast<uint32_t*>(s->d_head); }
static float* head_rho(const ott_store* s) { return s->d_head ? reinterpret_cast<float*>(s->d_head + s->cap * (size_t)16) : nullptr; }

bool store_wants_sketch(const ott_store* s) {
    const uint32_t nst = (s->ld + 31) / 32;
    const uint32_t bits = s->d_sketch ? s->sk_bits : (uint32_t)s->opt.exact_sketch_bits;  // (read when the store makes its first line)
    if (s->opt.exact_sketch == 0 || nst < 2 || prune_sketchb_stage0(nst, bits) < 1) return false;
    return s->opt.exact_sketch == 1 || nst >= 8;
}

// rows [first_row, first_row + n_rows) have new values: their sketch lines, and those of every earlier row that has none yet (the
// option was switched on, or a move between shards dropped the buffer).  A store that does not want one drops what it has.
static int update_sketch(ott_store* s, uint64_t first_row, uint64_t n_rows) {
    if (!store_wants_sketch(s)) {
        if (s->d_sketch) {
            OTT_HIP(hipStreamSynchronize(s->stream));
            (void)hipFree(s->d_sketch);
            s->d_sketch = nullptr;
            head_drop(s);
        }
        s->sk_n = 0;
        return OTT_OK;
    }
    const uint32_t nst = (s->ld + 31) / 32;
    if (!s->d_sketch) {
        s->sk_bits = (uint32_t)s->opt.exact_sketch_bits;
        s->sk_stage0 = prune_sketchb_stage0(nst, s->sk_bits);
        s->sk_words = (nst - s->sk_stage0) * s->sk_bits;
        s->sk_pitch = prune_sketch_pitch(s->sk_words);
        s->sk_n = 0;
        const hipError_t e = hipMalloc((void**)&s->d_sketch, s->cap * (size_t)s->sk_pitch * 4);
        if (e != hipSuccess) {  // no room: the store stays without one (the sweep then stops rows at 7/8 of the stages)
            (void)hipGetLastError();
            s->d_sketch = nullptr;
            return OTT_OK;
        }
    }
    // the head, made in the same launch: a store that wants one and has none yet (first line, the option switched back on, rows that
    // arrived with lines alone) gets it for every row; no room for it: the store stays without one (the sweep reads stage 0 then)
    if (!store_wants_head(s)) {
        if (s->d_head) {
            OTT_HIP(hipStreamSynchronize(s->stream));
            head_drop(s);
        }
    } else if (!s->d_head) {
        s->head_n = 0;
        if (hipMalloc((void**)&s->d_head, s->cap * (size_t)20) != hipSuccess) {
            (void)hipGetLastError();
            s->d_head = nullptr;
        }
    }
    const uint64_t have = s->d_head && s->head_n < s->sk_n ? s->head_n : s->sk_n;
    const uint64_t lo = first_row < have ? first_row : have, hi = first_row + n_rows;
    const uint32_t blocks = grid_blocks((hi - lo + 63) / 64, 4, s->n_cu);  // a wave per 64 rows, as launch_inv_norms
    if (s->sk_bits == 4)
        hipLaunchKernelGGL(tail_sketch_kernel<4>, dim3(blocks), dim3(256), 0, s->stream, s->d_rows, s->ld, s->dim, lo, hi - lo, s->sk_stage0,
                           nst - s->sk_stage0, s->sk_pitch, s->d_sketch, head_codes(s), head_rho(s));
    else if (s->sk_bits == 3)
        hipLaunchKernelGGL(tail_sketch_kernel<3>, dim3(blocks), dim3(256), 0, s->stream, s->d_rows, s->ld, s->dim, lo, hi - lo, s->sk_stage0,
                           nst - s->sk_stage0, s->sk_pitch, s->d_sketch, nullptr, nullptr);
    else
        hipLaunchKernelGGL(tail_sketch_kernel<1>, dim3(blocks), dim3(256), 0, s->stream, s->d_rows, s->ld, s->dim, lo, hi - lo, s->sk_stage0,
                           nst - s->sk_stage0, s->sk_pitch, s->d_sketch, nullptr, nullptr);
    OTT_HIP(hipGetLastError());
    if (hi > s->sk_n) s->sk_n = hi;
    if (s->d_head) s->head_n = s->sk_n;  // (lo <= head_n: every line this store has was made, or made again, with its head)
    return OTT_OK;
}

int launch_inv_norms(ott_store* s, uint64_t first_row, uint64_t n_rows) {
    if (!n_rows) return OTT_OK;
    hipLaunchKernelGGL(inv_norm_kernel, dim3(grid_blocks((n_rows + 63) / 64, 4, s->n_cu)), dim3(256), 0, s->stream, s->d_rows, s->ld, s->dim, first_row,
                       n_rows, s->d_inv, s->d_flag);
    OTT_HIP(hipGetLastError());
    return update_sketch(s, first_row, n_rows);
}

int launch_rand_fill(ott_store* s, uint64_t first_row, uint64_t n_rows, uint64_t seed) {
    if (!n_rows) return OTT_OK;
    hipLaunchKernelGGL(rand_fill_kernel, dim3((uint32_t)s->n_cu * 8), dim3(256), 0, s->stream, s->d_rows, s->ld, s->dim,
                       first_row, n_rows, s->base_offset + first_row, seed);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// (re)allocate rows / inv_norms / row flags for `ncap` rows, keeping the first s->n rows
static int realloc_store(ott_store* s, uint64_t ncap) {
    if (ncap > 0xFFFFFFF0ull) return fail(OTT_ERR_UNSUPPORTED, "a store holds at most 2^32-16 rows per GPU");
    {
        const int rcl = live_grow(s, ncap);  // the live mask of deleted rows (ott_tomb.hip) is sized with the row capacity
        if (rcl) return rcl;
        const int rcg = group_grow(s, ncap);  // the group ids of a grouped store (ott_group.hip) likewise: the ids that are there are kept
        if (rcg) return rcg;
    }
    float* nrows = nullptr;
    float* ninv = nullptr;
    uint8_t* nflag = nullptr;
    uint32_t* nsk = nullptr;  // the tail sign sketch is allocated, grown and copied exactly as the inverse norms are
    const bool keep_sk = s->d_sketch != nullptr && store_wants_sketch(s);
    char* nhd = nullptr;  // ... and so is the head of the four-bit form, which goes wherever the lines go
    const bool keep_hd = keep_sk && s->d_head != nullptr && store_wants_head(s);
    hipError_t e = hipSuccess;
    for (int attempt = 0; attempt < 2; attempt++) {
        e = hipMalloc((void**)&nrows, ncap * s->ld * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&ninv, ncap * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&nflag, ncap);
        if (e == hipSuccess && keep_sk) e = hipMalloc((void**)&nsk, ncap * (size_t)s->sk_pitch * 4);
        if (e == hipSuccess && keep_hd) e = hipMalloc((void**)&nhd, ncap * (size_t)20);
        if (e == hipSuccess) break;
        if (nrows) (void)hipFree(nrows);
        if (ninv) (void)hipFree(ninv);
        if (nflag) (void)hipFree(nflag);
        if (nsk) (void)hipFree(nsk);
        if (nhd) (void)hipFree(nhd);
        nrows = ninv = nullptr;
        nflag = nullptr;
        nsk = nullptr;
        nhd = nullptr;
        (void)hipGetLastError();  // reported here: the store stays as it was, and the next launch check must not see this again
        // The store's own copies of the corpus for the batch path (int8 plane, 16-bit plane, split image) are dropped by a
        // reallocation anyway: when the new buffers do not fit NEXT TO them, they go first and the allocation is tried once more
        // (a store that grows without a plan must not fail because the background builder took a quarter of the free memory)
        if (attempt == 1 || e != hipErrorOutOfMemory || !planes_any(s)) break;
        OTT_HIP(hipStreamSynchronize(s->stream));
        planes_drop(s);
    }
    if (e == hipErrorOutOfMemory && keep_sk) {
        // The sketch lines are derived from the rows as well (an eighth of their bytes in the four-bit form): when old and new lines
        // do not fit next to old and new rows, the planes go (if they have not), the rows move alone, and the lines are made again
        // behind them.  One more attempt, and only for a store that keeps lines
        if (planes_any(s)) {
            OTT_HIP(hipStreamSynchronize(s->stream));
            planes_drop(s);
        }
        e = hipMalloc((void**)&nrows, ncap * s->ld * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&ninv, ncap * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&nflag, ncap);
        if (e != hipSuccess) {
            if (nrows) (void)hipFree(nrows);
            if (ninv) (void)hipFree(ninv);
            if (nflag) (void)hipFree(nflag);
            nrows = ninv = nullptr;
            nflag = nullptr;
            (void)hipGetLastError();
        }
    }
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? OTT_ERR_OOM : OTT_ERR_HIP, std::string("hipMalloc(store): ") + hipGetErrorString(e));
    if (s->n) {
        OTT_HIP(hipMemcpyAsync(nrows, s->d_rows, s->n * s->ld * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        OTT_HIP(hipMemcpyAsync(ninv, s->d_inv, s->n * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        OTT_HIP(hipMemcpyAsync(nflag, s->d_flag, s->n, hipMemcpyDeviceToDevice, s->stream));
        if (nsk && s->sk_n) {
            const uint64_t have = s->sk_n < s->n ? s->sk_n : s->n;
            OTT_HIP(hipMemcpyAsync(nsk, s->d_sketch, have * (size_t)s->sk_pitch * 4, hipMemcpyDeviceToDevice, s->stream));
        }
        if (nhd && s->head_n) {  // (the rho_all array sits behind the codes of `cap` rows: two pieces)
            const uint64_t have = s->head_n < s->n ? s->head_n : s->n;
            OTT_HIP(hipMemcpyAsync(nhd, s->d_head, have * (size_t)16, hipMemcpyDeviceToDevice, s->stream));
            OTT_HIP(hipMemcpyAsync(nhd + ncap * (size_t)16, s->d_head + s->cap * (size_t)16, have * (size_t)4, hipMemcpyDeviceToDevice, s->stream));
        }
    }
    if (s->ld != s->dim)  // padding columns must be zero
        OTT_HIP(hipMemsetAsync(nrows + s->n * s->ld, 0, (ncap - s->n) * s->ld * sizeof(float), s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    if (s->d_rows) (void)hipFree(s->d_rows);
    if (s->d_inv) (void)hipFree(s->d_inv);
    if (s->d_flag) (void)hipFree(s->d_flag);
    if (s->d_sketch) (void)hipFree(s->d_sketch);
    if (s->d_head) (void)hipFree(s->d_head);
    s->d_rows = nrows;
    s->d_inv = ninv;
    s->d_flag = nflag;
    s->d_sketch = nsk;
    s->d_head = nhd;
    if (!nsk) s->sk_n = 0;
    if (!nhd) s->head_n = 0;
    s->cap = ncap;
    planes_drop(s);  // rebuilt lazily at the new capacity
    mask_slots_drop(s);  // the device mask slots of ott_query_masks belong to the rows as they lay: filled again by whoever uses them
    if (((keep_sk && !nsk) || (keep_hd && !nhd)) && s->n) {  // the lines, or their heads, did not move with the rows: made again, in the form they had
        const int want = s->opt.exact_sketch_bits;
        s->opt.exact_sketch_bits = (int)s->sk_bits;
        const int rc = update_sketch(s, 0, s->n);
        s->opt.exact_sketch_bits = want;
        if (rc) return rc;
    }
    return OTT_OK;
}

// A shard of a multi-GPU store takes over buffers the relayout filled (rows [0, n) valid, capacity `cap`): the old ones are
// freed, the 16-bit copies of the corpus are dropped (rebuilt lazily), the hi plane's per-row marks are cleared, the smallest
// inverse norm is measured again, the evaluated row mask is forgotten.  The caller holds the multi store exclusively.
int store_adopt(ott_store* s, float* rows, float* inv, uint8_t* flag, uint32_t* sketch, uint32_t sketch_bits, char* head, uint64_t n, uint64_t cap) {
    // the shard's own lock too: its background plane builder reads the rows under it (shared) and must be out before they go
    ott::host::ExclusiveLock wr(s->rw);
    std::lock_guard<std::mutex> g(s->mu);
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    if (s->d_rows) (void)hipFree(s->d_rows);
    if (s->d_inv) (void)hipFree(s->d_inv);
    if (s->d_flag) (void)hipFree(s->d_flag);
    if (s->d_sketch) (void)hipFree(s->d_sketch);
    head_drop(s);
    live_drop(s);  // (the rows are other rows now: whoever moved them loads their live bits afterwards, live_load)
    group_drop(s); // (a store with group ids moves no rows: nothing to drop unless a caller forced the move)
    sparse_drop(s);  // (sparse rows are set on single-GPU stores only)
    binary_drop(s);  // (... and so are bit rows)
    s->d_rows = rows;
    s->d_inv = inv;
    s->d_flag = flag;
    s->d_sketch = sketch;  // (nullptr: the rows came without sketch lines — the next append makes them for the whole shard)
    if (sketch) {
        const uint32_t nst = (s->ld + 31) / 32;
        s->sk_bits = sketch_bits;  // (the form the lines were made in, on whichever shard)
        s->sk_stage0 = prune_sketchb_stage0(nst, s->sk_bits);
        s->sk_words = (nst - s->sk_stage0) * s->sk_bits;
        s->sk_pitch = prune_sketch_pitch(s->sk_words);
    }
    s->sk_n = sketch ? n : 0;
    s->d_head = head;  // (nullptr: lines without heads — the next append makes the head, and the lines again, for the whole shard)
    s->head_n = head ? n : 0;
    s->n = n;
    s->cap = cap;
    planes_drop(s);
    s->evalmask_bits = 0;
    mask_slots_drop(s);
    s->min_pos_inv = __builtin_inff();
    if (!n) return OTT_OK;
    int rc = planes_clear_marks(s, n);
    if (rc) return rc;
    rc = update_min_pos_inv(s, 0, n);
    kick_plane_build(s);
    return rc;
}

// ott_store_compact (ott_tomb.hip) moved the surviving rows, their inverse norms and flag bytes to the front: the store is
// `new_n` rows long now.  What is derived from the rows follows: sketch lines are made again by the ingest kernel (deterministic
// per row: the bits a fresh store of these rows has), the cascade's planes are dropped as by a reallocation and rebuilt on
// demand, their marks in the flag bytes cleared, the smallest inverse norm measured again, the evaluated row mask forgotten.
// The caller holds the store exclusively and `mu`.
int store_after_compact(ott_store* s, uint64_t new_n) {
    s->n = new_n;
    planes_drop(s);
    s->evalmask_bits = 0;
    mask_slots_drop(s);
    s->sk_n = 0;
    s->head_n = 0;
    s->min_pos_inv = __builtin_inff();
    if (!new_n) return OTT_OK;
    int rc = planes_clear_marks(s, new_n);
    if (rc) return rc;
    rc = update_sketch(s, 0, new_n);
    if (rc) return rc;
    rc = update_min_pos_inv(s, 0, new_n);
    kick_plane_build(s);
    return rc;
}

// A store that grows without a plan doubles (round 4: hipMalloc + hipFree of multi-GB buffers cost ~80 ms a pair on this part —
// at 1.5x a 30-GB store built from 100k-row appends spent 1.9 of its 2.4 s in twelve of them), and falls back to smaller steps
// when the doubled size does not fit next to the old buffer: 1.25x, then exactly what is needed.
static int grow(ott_store* s, uint64_t need) {
    if (need <= s->cap) return OTT_OK;
    const uint64_t base = s->cap ? s->cap : 1024;
    uint64_t twice = base;
    while (twice < need) twice = twice * 2 + 1024;
    uint64_t quarter = base;
    while (quarter < need) quarter = quarter + quarter / 4 + 1024;
    int rc = OTT_OK;
    for (uint64_t ncap : {twice, quarter, need}) {
        if (ncap > 0xFFFFFFF0ull && need <= 0xFFFFFFF0ull) ncap = 0xFFFFFFF0ull;  // (the per-GPU row limit is not a reason to refuse a size that fits)
        rc = realloc_store(s, ncap);
        if (rc != OTT_ERR_OOM) return rc;
    }
    return rc;
}

// rows [s->n, s->n + n_rows) from a host buffer: copy, inverse norms, smallest inverse norm (one wait)
static int append_host_locked(ott_store* s, const float* rows_host, uint64_t n_rows) {
    int rc = grow(s, s->n + n_rows);
    if (rc) return rc;
    OTT_HIP(hipMemcpy2DAsync(s->d_rows + s->n * s->ld, (size_t)s->ld * 4, rows_host, (size_t)s->dim * 4, (size_t)s->dim * 4,
                             n_rows, hipMemcpyHostToDevice, s->stream));
    rc = launch_inv_norms(s, s->n, n_rows);
    if (rc) return rc;
    rc = update_min_pos_inv(s, s->n, n_rows);
    if (rc) return rc;
    s->n += n_rows;
    kick_plane_build(s);
    return OTT_OK;
}

constexpr size_t PEND_BYTES = (size_t)4 << 20, PEND_SMALL = (size_t)256 << 10;

int store_flush_locked(ott_store* s) {
    if (!s->pend.count()) return OTT_OK;
    OTT_HIP(use_device(s));
    return s->pend.flush([s](const float* rows, uint64_t n) { return append_host_locked(s, rows, n); });
}

int store_flush(ott_store* s) {
    if (!s || s->multi || !s->pend.count()) return OTT_OK;
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    return store_flush_locked(s);
}

static ott_store* make_worker(ott_store* s) {
    ott_store* w = new ott_store();
    w->is_worker = true;
    w->device = s->device;
    w->logical = s->logical;
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
        delete w;
        return nullptr;
    }
    for (auto& ev : w->ev)
        if (hipEventCreate(&ev) != hipSuccess) {
            ott_store_destroy(w);
            return nullptr;
        }
    return w;
}

// the corpus as the owner sees it now (the caller holds the owner's `rw` shared, so it cannot change underneath)
static void alias_corpus(ott_store* w, const ott_store* s) {
    w->dim = s->dim;
    w->ld = s->ld;
    w->dimq = s->dimq;
    w->n = s->n;
    w->cap = s->cap;
    w->chunk_size = s->chunk_size;
    w->base_offset = s->base_offset;
    w->reduce = s->reduce;
    w->n_cu = s->n_cu;
    w->min_pos_inv = s->min_pos_inv;
    w->opt = s->opt;
    w->d_rows = s->d_rows;
    w->d_inv = s->d_inv;
    w->d_flag = s->d_flag;
    w->d_sketch = s->d_sketch;
    w->d_head = s->d_head;
    w->head_n = s->head_n;
    w->sk_n = s->sk_n;
    w->sk_words = s->sk_words;
    w->sk_bits = s->sk_bits;
    w->sk_pitch = s->sk_pitch;
    w->sk_stage0 = s->sk_stage0;
    w->d_evalmask.p = s->d_evalmask.p;
    w->d_evalmask.cap = 0;
    w->evalmask_bits = s->evalmask_bits;
    w->d_live = s->d_live;
    w->n_dead = s->n_dead;
    w->d_gid = s->d_gid;
    w->gid_n = s->gid_n;
    w->n_groups = s->n_groups;
    w->d_gix = s->d_gix;
    w->d_sparse = s->d_sparse;
    w->sparse_n = s->sparse_n;
    w->sparse_nnz = s->sparse_nnz;
    w->sparse_vocab = s->sparse_vocab;
    w->sparse_lay = s->sparse_lay;
    w->d_binary = s->d_binary;
    w->binary_n = s->binary_n;
    w->binary_bits = s->binary_bits;
}

// the store's own context when it is free, else a worker context that aliases the corpus (ott::host::ContextPool)
ott_store* ctx_acquire(ott_store* s) {
    return s->pool.acquire(
        s, OTT_MAX_WORKERS,
        [s]() -> ott_store* {
            (void)use_device(s);
            ott_store* w = make_worker(s);
            if (w) w->owner = s;
            return w;
        },
        [s](ott_store* w) { alias_corpus(w, s); });
}

void ctx_release(ott_store* w) { (w->owner ? w->owner : w)->pool.release(w); }

}  // namespace ott

using namespace ott;

extern "C" {

int ott_abi_version(void) { return OTT_ABI_VERSION; }
const char* ott_last_error(void) { return ott::last_error(); }

int ott_device_count(int* out) {
    if (!out) return fail(OTT_ERR_INVALID, "ott_device_count: out is NULL");
    int n = 0;
    OTT_HIP(hipGetDeviceCount(&n));
    *out = n;
    return OTT_OK;
}

int ott_store_create(uint32_t dim, int device, ott_store** out) { return ott::store_create(dim, device, device, out); }

}  // extern "C"

int ott::store_create(uint32_t dim, int device, int logical, ott_store** out) {
    if (!out) return fail(OTT_ERR_INVALID, "ott_store_create: out is NULL");
    *out = nullptr;
    if (dim == 0) return fail(OTT_ERR_INVALID, "ott_store_create: dim must be > 0");
    OTT_HIP(use_device_raw(device, logical));
    hipDeviceProp_t prop;
    OTT_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(OTT_ERR_UNSUPPORTED, std::string("libotters_hip is built for gfx950 (MI355X) only; device is ") + prop.gcnArchName);
    ott_store* s = new ott_store();
    s->device = device;
    s->logical = logical;
    s->dim = dim;
    s->ld = (dim + 3u) & ~3u;
    s->dimq = (dim + 7u) & ~7u;
    s->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    options_from_env(s->opt);  // the ONLY place the library reads the environment
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete s;
        return fail(OTT_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    for (auto& ev : s->ev) {
        e = hipEventCreate(&ev);
        if (e != hipSuccess) {
            delete s;
            return fail(OTT_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
        }
    }
    *out = s;
    return OTT_OK;
}

extern "C" {

int ott_store_destroy(ott_store* s) {
    if (!s) return OTT_OK;
    if (s->multi) return multi_destroy(s);
    if (s->builder) {  // the background plane builder finishes what it is at, then goes (~QuietWorker stops and joins)
        delete s->builder;
        s->builder = nullptr;
    }
    (void)use_device(s);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (ott_store* w : s->pool.workers) ott_store_destroy(w);
    s->pool.workers.clear();
    if (s->is_worker) {  // a worker only aliases the corpus and the evaluated row mask
        s->d_rows = nullptr;
        s->d_inv = nullptr;
        s->d_flag = nullptr;
        s->d_sketch = nullptr;
        s->d_head = nullptr;
        s->d_evalmask.p = nullptr;
        s->d_evalmask.cap = 0;
        s->d_live = nullptr;
        s->d_gid = nullptr;
        s->d_gix = nullptr;
        s->d_sparse = nullptr;
        s->d_binary = nullptr;
    }
    if (s->d_df) (void)hipFree(s->d_df);  // (the owner's alone: a worker builds into the owner's and never holds one)
    if (s->d_sparse) (void)hipFree(s->d_sparse);
    if (s->d_binary) (void)hipFree(s->d_binary);
    if (s->d_gix) (void)hipFree(s->d_gix);
    if (s->d_live) (void)hipFree(s->d_live);
    if (s->d_gid) (void)hipFree(s->d_gid);
    if (s->d_rows) (void)hipFree(s->d_rows);
    if (s->d_inv) (void)hipFree(s->d_inv);
    if (s->d_flag) (void)hipFree(s->d_flag);
    if (s->d_sketch) (void)hipFree(s->d_sketch);
    if (s->d_head) (void)hipFree(s->d_head);
    planes_release(s);  // (a worker has none of its own)
    mask_slots_drop(s); // (nor any mask slot)
    for (ott::DevBuf* b : {&s->d_queries, &s->d_qinv, &s->d_rowmask, &s->d_runs, &s->d_prefix, &s->d_lists, &s->d_lists2, &s->d_hits,
                           &s->d_count, &s->d_cand, &s->d_misc, &s->d_prune, &s->d_tails, &s->d_evalmask, &s->d_livefx, &s->d_idmask, &s->d_qmasks, &s->d_gather, &s->d_mmr, &s->d_fuse, &s->d_spq, &s->d_sptable, &s->d_bq, &s->d_rectable, &s->d_disc, &s->d_gtable, &s->d_gctl, &s->d_mstable, &s->d_minpos, &s->m_Q, &s->m_qinv, &s->m_qnorm,
                           &s->m_tau, &s->m_cntA, &s->m_cntB, &s->m_candA, &s->m_candB, &s->m_over, &s->m_out, &s->m_outcnt,
                           &s->m_uncert, &s->m_prefix, &s->x_send, &s->x_recv, &s->l_keysA, &s->l_keysB, &s->l_qA, &s->l_qB, &s->l_tmp, &s->l_cursor, &s->l_hist, &s->l_gate, &s->l_ctl})
        b->release();
    s->h_stage.release();
    s->h_hits.release();
    s->h_fuse.release();
    s->h_spq.release();
    s->h_bq.release();
    s->h_disc.release();
    s->h_hdr.release();
    s->h_pend.release();
    for (auto& c : s->columns) {
        if (c.d_vals) (void)hipFree(c.d_vals);
        if (c.d_nulls) (void)hipFree(c.d_nulls);
    }
    for (auto& ev : s->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return OTT_OK;
}

int ott_store_reserve(ott_store* s, uint64_t n_rows) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_reserve: store is NULL");
    if (s->multi) return multi_reserve(s, n_rows);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    OTT_HIP(use_device(s));
    if (n_rows <= s->cap) return OTT_OK;
    return realloc_store(s, n_rows);  // exact-size allocation
}

int ott_store_append(ott_store* s, const float* rows_host, uint64_t n_rows) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_append: store is NULL");
    if (n_rows == 0) return OTT_OK;
    if (!rows_host) return fail(OTT_ERR_INVALID, "ott_store_append: rows is NULL");
    if (s->multi) {
        AppendArgs a;
        a.kind = APPEND_HOST;
        a.rows = rows_host;
        return multi_append(s, a, n_rows);
    }
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    const size_t bytes = (size_t)n_rows * s->dim * 4;
    int rc;
    if (bytes <= PEND_SMALL && s->opt.stage_appends != 0) {
        // a small append (VecStore::add_vector: one row) is staged in pinned host memory; 4 MB of them travel together
        if (!s->pend.fits(n_rows, s->dim) && (rc = store_flush_locked(s))) return rc;
        if (!s->h_pend.p) {
            OTT_HIP(use_device(s));
            if ((rc = s->h_pend.ensure(PEND_BYTES))) return rc;
            s->pend.buf = (float*)s->h_pend.p;
            s->pend.cap_bytes = PEND_BYTES;
        }
        s->pend.stage(rows_host, n_rows, s->dim);
        return OTT_OK;
    }
    OTT_HIP(use_device(s));
    if ((rc = store_flush_locked(s))) return rc;  // staged rows come first
    return append_host_locked(s, rows_host, n_rows);
}

int ott_store_append_device(ott_store* s, const void* rows_dev, uint64_t n_rows) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_append_device: store is NULL");
    if (n_rows == 0) return OTT_OK;
    if (!rows_dev) return fail(OTT_ERR_INVALID, "ott_store_append_device: rows is NULL");
    if (s->multi) {
        AppendArgs a;
        a.kind = APPEND_DEVICE;
        a.rows = rows_dev;
        return multi_append(s, a, n_rows);
    }
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    OTT_HIP(use_device(s));
    int rc = store_flush_locked(s);  // staged rows come first
    if (rc) return rc;
    if ((rc = grow(s, s->n + n_rows))) return rc;
    OTT_HIP(hipMemcpy2DAsync(s->d_rows + s->n * s->ld, (size_t)s->ld * 4, rows_dev, (size_t)s->dim * 4, (size_t)s->dim * 4,
                             n_rows, hipMemcpyDeviceToDevice, s->stream));
    rc = launch_inv_norms(s, s->n, n_rows);
    if (rc) return rc;
    rc = update_min_pos_inv(s, s->n, n_rows);
    if (rc) return rc;
    s->n += n_rows;
    kick_plane_build(s);
    return OTT_OK;
}

int ott_store_append_random(ott_store* s, uint64_t n_rows, uint64_t seed) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_append_random: store is NULL");
    if (n_rows == 0) return OTT_OK;
    if (s->multi) {
        AppendArgs a;
        a.kind = APPEND_RANDOM;
        a.seed = seed;
        return multi_append(s, a, n_rows);
    }
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    OTT_HIP(use_device(s));
    int rc = store_flush_locked(s);  // staged rows come first
    if (rc) return rc;
    if ((rc = grow(s, s->n + n_rows))) return rc;
    rc = launch_rand_fill(s, s->n, n_rows, seed);
    if (rc) return rc;
    rc = launch_inv_norms(s, s->n, n_rows);
    if (rc) return rc;
    rc = update_min_pos_inv(s, s->n, n_rows);
    if (rc) return rc;
    s->n += n_rows;
    kick_plane_build(s);
    return OTT_OK;
}

int ott_store_append_clustered(ott_store* s, uint64_t n_rows, uint64_t seed, uint32_t n_clusters, float spread, float aniso) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_append_clustered: store is NULL");
    if (n_clusters == 0 || !(spread >= 0.0f) || !(aniso >= 0.0f)) return fail(OTT_ERR_INVALID, "ott_store_append_clustered: n_clusters > 0, spread >= 0, aniso >= 0");
    if (n_rows == 0) return OTT_OK;
    if (s->multi) {
        AppendArgs a;
        a.kind = APPEND_CLUSTERED;
        a.seed = seed;
        a.n_clusters = n_clusters;
        a.spread = spread;
        a.aniso = aniso;
        return multi_append(s, a, n_rows);
    }
    ott::host::ExclusiveLock wr(s->rw);
    std::lock_guard<std::mutex> g(s->mu);
    OTT_HIP(use_device(s));
    int rc = store_flush_locked(s);  // staged rows come first
    if (rc) return rc;
    if ((rc = grow(s, s->n + n_rows))) return rc;
    hipLaunchKernelGGL(clustered_fill_kernel, dim3((uint32_t)s->n_cu * 8), dim3(256), 0, s->stream, s->d_rows, s->ld, s->dim, s->n, n_rows,
                       s->base_offset + s->n, seed, n_clusters, spread, aniso);
    OTT_HIP(hipGetLastError());
    if ((rc = launch_inv_norms(s, s->n, n_rows))) return rc;
    if ((rc = update_min_pos_inv(s, s->n, n_rows))) return rc;
    s->n += n_rows;
    kick_plane_build(s);
    return OTT_OK;
}

int ott_store_set_batch_image(ott_store* s, int enabled) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_batch_image: store is NULL");
    if (s->multi) return multi_set_batch_image(s, enabled);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    if (!enabled && planes_any(s)) OTT_HIP(use_device(s));
    planes_enable(s, enabled != 0);
    return OTT_OK;
}

int ott_store_set_option(ott_store* s, const char* name, int64_t value) {
    if (!s || !name) return fail(OTT_ERR_INVALID, "ott_store_set_option: NULL argument");
    if (s->multi) return multi_set_option(s, name, value);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    Options o = s->opt;
    if (option_set(o, name, (long long)value)) return fail(OTT_ERR_INVALID, std::string("ott_store_set_option: unknown option or bad value: ") + name);
    planes_set_options(s, o);
    return OTT_OK;
}

int ott_store_prepare_batch(ott_store* s) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_prepare_batch: store is NULL");
    if (s->multi) return multi_prepare_batch(s);
    {
        const int rcf = store_flush(s);
        if (rcf) return rcf;
    }
    ott::host::SharedLock rd(s->rw);
    OTT_HIP(use_device(s));
    ott_store* ctx = ott::ctx_acquire(s);
    const int rc = ensure_first_plane(ctx);  // a no-op when it is up to date, switched off, or does not fit
    ott::ctx_release(ctx);
    return rc;
}

int ott_store_batch_ready(const ott_store* cs) {
    ott_store* s = const_cast<ott_store*>(cs);
    if (!s) return 0;
    if (s->multi) return multi_batch_ready(s);
    if (s->pend.count()) return 0;
    return first_plane_ready(s) ? 1 : 0;
}

int ott_store_write_rows(ott_store* s, uint64_t first_row, const float* rows_host, uint64_t n_rows) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_write_rows: store is NULL");
    if (n_rows == 0) return OTT_OK;
    if (!rows_host) return fail(OTT_ERR_INVALID, "ott_store_write_rows: rows is NULL");
    if (s->multi) return multi_write_rows(s, first_row, rows_host, n_rows);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    {
        const int rcf = store_flush_locked(s);
        if (rcf) return rcf;
    }
    if (first_row + n_rows > s->n) return fail(OTT_ERR_INVALID, "ott_store_write_rows: range exceeds store length");
    OTT_HIP(use_device(s));
    OTT_HIP(hipMemcpy2DAsync(s->d_rows + first_row * s->ld, (size_t)s->ld * 4, rows_host, (size_t)s->dim * 4,
                             (size_t)s->dim * 4, n_rows, hipMemcpyHostToDevice, s->stream));
    int rc = launch_inv_norms(s, first_row, n_rows);
    if (rc) return rc;
    if ((rc = planes_rewrite(s, first_row, n_rows))) return rc;
    return update_min_pos_inv(s, first_row, n_rows);
}

uint64_t ott_store_len(const ott_store* s) { return s ? store_rows(s) : 0; }  // staged rows count: they were appended
uint64_t ott_store_exact_finished(const ott_store* s) {
    if (!s) return 0;
    if (s->multi) return multi_exact_finished(const_cast<ott_store*>(s));
    return s->exact_finished.load(std::memory_order_relaxed);
}
uint32_t ott_store_dim(const ott_store* s) { return s ? s->dim : 0; }
int ott_store_device(const ott_store* s) { return s ? s->device : -1; }

int ott_store_set_chunk_size(ott_store* s, uint64_t chunk_size) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_chunk_size: store is NULL");
    if (s->multi) return multi_set_chunk_size(s, chunk_size);
    s->chunk_size = chunk_size < 1 ? 1 : chunk_size;  // src/meta.rs:86-89
    return OTT_OK;
}
int ott_store_set_base_offset(ott_store* s, uint64_t base) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_base_offset: store is NULL");
    if (s->multi) return multi_set_base_offset(s, base);
    s->base_offset = base;
    return OTT_OK;
}
int ott_store_set_reduce_order(ott_store* s, uint32_t reduce) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_reduce_order: store is NULL");
    if (reduce > OTT_REDUCE_SEQ4) return fail(OTT_ERR_INVALID, "ott_store_set_reduce_order: unknown order");
    if (s->multi) return multi_set_reduce_order(s, reduce);
    s->reduce = reduce;
    return OTT_OK;
}

int ott_store_read_rows(const ott_store* s, uint64_t first_row, uint64_t n_rows, float* out_host) {
    if (!s || !out_host) return fail(OTT_ERR_INVALID, "ott_store_read_rows: NULL argument");
    if (!s->multi && store_flush(const_cast<ott_store*>(s))) return OTT_ERR_HIP;
    if (first_row + n_rows > s->n) return fail(OTT_ERR_INVALID, "ott_store_read_rows: range exceeds store length");
    if (!n_rows) return OTT_OK;
    if (s->multi) return multi_read(s, false, first_row, n_rows, out_host);
    ott::host::SharedLock rd(const_cast<ott_store*>(s)->rw);  // the rows cannot be reallocated under the copy
    if (first_row + n_rows > s->n) return fail(OTT_ERR_INVALID, "ott_store_read_rows: range exceeds store length");
    OTT_HIP(use_device(s));
    OTT_HIP(hipMemcpy2D(out_host, (size_t)s->dim * 4, s->d_rows + first_row * s->ld, (size_t)s->ld * 4, (size_t)s->dim * 4,
                        n_rows, hipMemcpyDeviceToHost));
    return OTT_OK;
}

int ott_store_read_inv_norms(const ott_store* s, uint64_t first_row, uint64_t n_rows, float* out_host) {
    if (!s || !out_host) return fail(OTT_ERR_INVALID, "ott_store_read_inv_norms: NULL argument");
    if (!s->multi && store_flush(const_cast<ott_store*>(s))) return OTT_ERR_HIP;
    if (first_row + n_rows > s->n) return fail(OTT_ERR_INVALID, "ott_store_read_inv_norms: range exceeds store length");
    if (!n_rows) return OTT_OK;
    if (s->multi) return multi_read(s, true, first_row, n_rows, out_host);
    ott::host::SharedLock rd(const_cast<ott_store*>(s)->rw);
    if (first_row + n_rows > s->n) return fail(OTT_ERR_INVALID, "ott_store_read_inv_norms: range exceeds store length");
    OTT_HIP(use_device(s));
    OTT_HIP(hipMemcpy(out_host, s->d_inv + first_row, n_rows * sizeof(float), hipMemcpyDeviceToHost));
    return OTT_OK;
}

int ott_store_sync(ott_store* s) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_sync: store is NULL");
    if (s->multi) return multi_sync(s);
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    return OTT_OK;
}

void* ott_store_stream(ott_store* s) { return s ? (void*)s->stream : nullptr; }  // (multi-GPU store: the stream of its merging shard)

}  // extern "C"
