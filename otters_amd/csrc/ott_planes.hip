// ott_planes.hip — the cascade's planes: up to three compact copies of the corpus per store (split-bf16 image, 16-bit hi plane,
// int8 plane; struct PlaneSet in ott_internal.h).  The conversion kernels and their launchers, the steps of the planes' life cycle
// — each written once, each taking the planes' mutex itself — and the background builder.  The two format decisions are in
// ott_plane_policy.h.
#include <string.h>

#include <chrono>

#include "ott_internal.h"

namespace ott {

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------

// The end of a row's conversion (lane 0 of the row's wave, hi and int8 planes): rel = what the conversion lost, from the two f64
// sums — se = ||x - plane(x)||^2, sx = ||x||^2 — rounded up (1 + 1e-4 covers the f64 sums and the f32 conversion; a non-finite row
// measures as 1 = "cannot certify").  It goes to rel_out[i] (optional) and, for a regular row, into the running maximum rel_max[0]
// (optional; float bits).  A row above rel_flag is marked irregular instead (`bit` of flag_rw[r], optional: 2 = outside the HALF hi
// pass's error model only, see mfma_score_kernel; 4 = int8 loses too much of it) and counted in rel_max[1]: how many rows the format
// does not suit.  Rows with flag[r] & 1 are outside every pass's model already and take no part.  unmark: a rewritten row that
// suits the format again has its bit taken back.  (flag and flag_rw may be the same array.)
__device__ __forceinline__ void plane_row_loss(double se, double sx, uint64_t i, uint64_t r, float* __restrict__ rel_out, uint32_t* __restrict__ rel_max,
                                               const uint8_t* flag, float rel_flag, uint8_t* flag_rw, uint8_t bit, bool unmark) {
    float rel = sx > 0.0 ? (float)(sqrt(se / sx) * 1.0001) : 0.0f;
    if (!(rel <= 1.0f)) rel = 1.0f;
    if (rel_out) rel_out[i] = rel;
    bool irregular = flag && (flag[r] & 1u);
    if (flag_rw && !irregular) {
        if (rel > rel_flag) {
            flag_rw[r] = (uint8_t)(flag_rw[r] | bit);
            irregular = true;
            if (rel_max) atomicAdd(rel_max + 1, 1u);
        } else if (unmark && (flag_rw[r] & bit)) {
            flag_rw[r] = (uint8_t)(flag_rw[r] & ~bit);
        }
    }
    // (look first: one atomic per row on ONE address serialises — 10M rows took 113 ms; the running max settles at once)
    if (rel_max && !irregular && __float_as_uint(rel) > __hip_atomic_load(rel_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(rel_max, __float_as_uint(rel));
}

// rows [first, first + n) -> batch image: one thread per (row, 4 floats)
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim, uint32_t ldi,
                                                          uint64_t first, uint64_t n, uint16_t* __restrict__ img,
                                                          const float* __restrict__ scale) {  // scale: optional per-row factor
    const uint32_t quads = ldi / 4;
    const uint64_t total = n * quads;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = first + i / quads;
        const uint32_t c = (uint32_t)(i % quads) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < ld) x = *reinterpret_cast<const float4*>(rows + r * (uint64_t)ld + c);  // ld is a multiple of 4, padded with zeros
        const float v[4] = {x.x, x.y, x.z, x.w};
        uint16_t h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float xe = (c + e < dim) ? (scale ? v[e] * scale[r] : v[e]) : 0.0f;
            const __bf16 hb = (__bf16)xe;
            const __bf16 lb = (__bf16)(xe - (float)hb);
            h[e] = __builtin_bit_cast(uint16_t, hb);
            l[e] = __builtin_bit_cast(uint16_t, lb);
        }
        uint16_t* dst = img + r * (uint64_t)ldi * 2 + (c / 32) * 64 + (c % 32);
        *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
        *reinterpret_cast<uint2*>(dst + 32) = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
    }
}

// rows [first, first + n) -> hi plane (bf16 round-to-nearest of every element), one wave per row.  Also measures what the
// rounding lost: rel = ||x - bf16(x)|| / ||x|| per row (f64 sums: the squares of a 1e-18-norm row underflow in f32), written
// to rel_out[r] (optional) and folded into *rel_max (optional; float bits, rows with flag[r] != 0 excluded — those are always
// re-scored exactly).  This measured figure, not the worst case 2^-8, is what the hi pass's certification uses.
// F16 = false: bf16 (round to nearest even) of every element.  F16 = true (round 3): IEEE half — the same two bytes carry
// 11 significant bits instead of 8, so the measured rounding loss ||v - h(v)|| / ||v|| is ~8x smaller (2.1e-4 against 1.65e-3
// on uniform rows) and the hi pass's error bound with it; the price is half's narrow exponent range, met by ONE
// power-of-two factor for all rows (`gscale`, exact; chosen in ensure_hi_plane).  A row whose elements
// then fall into half's subnormals (a norm far below the store's largest) or overflow (appended after the plane was
// scaled) simply MEASURES a large loss: rows above `rel_flag` are marked irregular (`flag_rw`, bit 1) — excluded from the
// store's maximum, always listed, always re-scored exactly — exactly like rows outside the bf16 pass's error model.
template <bool F16>
__global__ __launch_bounds__(256) void hi_rows_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim, uint32_t ldh,
                                                       uint64_t first, uint64_t n, uint16_t* __restrict__ img,
                                                       const float* __restrict__ scale, float* __restrict__ rel_out,
                                                       uint32_t* __restrict__ rel_max, const uint8_t* flag, float gscale,
                                                       float rel_flag, uint8_t* flag_rw) {  // (flag and flag_rw may be the same array)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (uint64_t)gridDim.x * 4;
    for (uint64_t i = wid; i < n; i += nw) {
        const uint64_t r = first + i;
        const float sc = scale ? __fmul_rn(scale[r], gscale) : gscale;  // gscale is a power of two (1 for bf16): exact
        double se = 0.0, sx = 0.0;
        for (uint32_t c = lane * 4; c < ldh; c += 256) {
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < ld) x = *reinterpret_cast<const float4*>(rows + r * (uint64_t)ld + c);  // ld is a multiple of 4, padded with zeros
            const float v[4] = {x.x, x.y, x.z, x.w};
            uint16_t h[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float xe = (c + e < dim) ? ((scale || F16) ? __fmul_rn(v[e], sc) : v[e]) : 0.0f;
                float back;
                if constexpr (F16) {
                    const _Float16 hb = (_Float16)xe;  // v_cvt_f16_f32: round to nearest even, overflow -> inf, gradual underflow
                    back = (float)hb;
                    h[e] = __builtin_bit_cast(uint16_t, hb);
                } else {
                    const __bf16 hb = (__bf16)xe;
                    back = (float)hb;
                    h[e] = __builtin_bit_cast(uint16_t, hb);
                }
                const double df = (double)xe - (double)back;
                se += df * df;
                sx += (double)xe * (double)xe;
            }
            *reinterpret_cast<uint2*>(img + r * (uint64_t)ldh + c) =
                make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            se += __shfl_xor(se, off);
            sx += __shfl_xor(sx, off);
        }
        if (lane == 0) plane_row_loss(se, sx, i, r, rel_out, rel_max, flag, rel_flag, flag_rw, 2u, false);
    }
}

// smallest non-zero inverse norm over the REGULAR rows (the largest norm the half plane's factor has to accommodate)
__global__ __launch_bounds__(256) void min_regular_inv_kernel(const float* __restrict__ inv, const uint8_t* __restrict__ flag, uint64_t n, uint32_t* out) {
    uint32_t best = 0x7F800000u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t b = __float_as_uint(inv[i]);
        if (b != 0 && b < best && !(flag[i] & 1u)) best = b;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(out, best);
}

__global__ __launch_bounds__(256) void clear_flag_bit_kernel(uint8_t* flag, uint64_t n, uint8_t mask) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) flag[i] = (uint8_t)(flag[i] & mask);
}

// ---- int8 plane (round 5) --------------------------------------------------------------------------------------------------
// rows [first, first + n) -> int8, one wave per row.  Per-row scale s = max|x| / 127 (or the caller's common scale), element =
// rint(x / s) clamped to +-127.  What the rounding lost is MEASURED in f64 against the values actually stored:
// rel = ||x - s x~|| / ||x|| (rounded up), into rel_out[r] and — regular rows only — the running maximum *rel_max; a row above
// rel_flag is marked irregular (bit 2 of flag_rw) and counted in rel_max[1] instead.
__global__ __launch_bounds__(256) void i8_rows_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim, uint32_t ld8, uint64_t first, uint64_t n,
                                                       int8_t* __restrict__ img, const float* __restrict__ pre, float common_scale,
                                                       float* __restrict__ scale_out, float* __restrict__ rel_out, uint32_t* __restrict__ rel_max,
                                                       const uint8_t* flag, float rel_flag, uint8_t* flag_rw) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (uint64_t)gridDim.x * 4;
    for (uint64_t i = wid; i < n; i += nw) {
        const uint64_t r = first + i;
        const float pf = pre ? pre[r] : 1.0f;
        const float* x = rows + r * (uint64_t)ld;
        float s = common_scale;
        if (!(common_scale > 0.0f)) {
            float mx = 0.0f;
            for (uint32_t c = lane * 4; c < ld; c += 256) {
                const float4 v = *reinterpret_cast<const float4*>(x + c);  // ld is a multiple of 4, padded with zeros
                mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x * pf), fabsf(v.y * pf)), fmaxf(fabsf(v.z * pf), fabsf(v.w * pf))));  // (fmaxf drops a NaN operand)
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            s = mx / 127.0f;
            if (!(s < __builtin_inff())) s = 0.0f;  // a non-finite row: flagged at append, always re-scored exactly; its plane row is zeros
        }
        const float inv_s = s > 0.0f ? 1.0f / s : 0.0f;
        double se = 0.0, sx = 0.0;
        for (uint32_t c = lane * 4; c < ld8; c += 256) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < ld) v = *reinterpret_cast<const float4*>(x + c);
            const float xe[4] = {v.x * pf, v.y * pf, v.z * pf, v.w * pf};
            int q[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float t = (c + e < dim) ? rintf(xe[e] * inv_s) : 0.0f;
                t = t == t ? fminf(fmaxf(t, -127.0f), 127.0f) : 0.0f;
                q[e] = (int)t;
                if (c + e < dim) {
                    const double df = (double)xe[e] - (double)s * (double)q[e];
                    se += df * df;
                    sx += (double)xe[e] * (double)xe[e];
                }
            }
            *reinterpret_cast<uint32_t*>(img + r * (uint64_t)ld8 + c) =
                (uint32_t)(uint8_t)q[0] | ((uint32_t)(uint8_t)q[1] << 8) | ((uint32_t)(uint8_t)q[2] << 16) | ((uint32_t)(uint8_t)q[3] << 24);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            se += __shfl_xor(se, off);
            sx += __shfl_xor(sx, off);
        }
        if (lane == 0) {
            if (scale_out) scale_out[r] = s;
            plane_row_loss(se, sx, i, r, rel_out, rel_max, flag, rel_flag, flag_rw, 4u, true);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------

static int launch_split(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ldi, uint64_t first, uint64_t n, uint16_t* out,
                        const float* scale, int n_cu) {
    hipLaunchKernelGGL(split_rows_kernel, dim3(grid_blocks(n * (ldi / 4), 256, n_cu, 16)), dim3(256), 0, stream, rows, ld, dim, ldi, first, n, out, scale);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// the ONE launcher of hi_rows_kernel (a wave per row)
static int launch_hi(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ldh, uint64_t first, uint64_t n, uint16_t* out,
                     const float* scale, float* rel_out, uint32_t* rel_max, const uint8_t* flag, bool f16, float gscale, float rel_flag, uint8_t* flag_rw,
                     int n_cu) {
    const dim3 grid(grid_blocks(n, 4, n_cu));
    if (f16)
        hipLaunchKernelGGL(hi_rows_kernel<true>, grid, dim3(256), 0, stream, rows, ld, dim, ldh, first, n, out, scale, rel_out, rel_max, flag, gscale, rel_flag,
                           flag_rw);
    else
        hipLaunchKernelGGL(hi_rows_kernel<false>, grid, dim3(256), 0, stream, rows, ld, dim, ldh, first, n, out, scale, rel_out, rel_max, flag, 1.0f, rel_flag,
                           flag_rw);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// the query side's operand blocks (ott_mfma.hip): rows [0, n), nothing marked, nothing folded into a maximum
int launch_split_rows(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ldi, uint64_t n, uint16_t* out,
                      const float* scale, int n_cu) {
    return launch_split(stream, rows, ld, dim, ldi, 0, n, out, scale, n_cu);
}
int launch_hi_rows(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ldh, uint64_t n, uint16_t* out,
                   const float* scale, float* rel_out, int n_cu, bool f16, float gscale) {
    return launch_hi(stream, rows, ld, dim, ldh, 0, n, out, scale, rel_out, nullptr, nullptr, f16, gscale, 2.0f, nullptr, n_cu);
}
int launch_i8_rows(hipStream_t stream, const float* rows, uint32_t ld, uint32_t dim, uint32_t ld8, uint64_t first, uint64_t n, int8_t* out,
                   const float* pre, float common_scale, float* scale_out, float* rel_out, uint32_t* rel_max, const uint8_t* flag, float rel_flag,
                   uint8_t* flag_rw, int n_cu) {
    if (!n) return OTT_OK;
    hipLaunchKernelGGL(i8_rows_kernel, dim3(grid_blocks(n, 4, n_cu)), dim3(256), 0, stream, rows, ld, dim, ld8, first, n, out, pre, common_scale, scale_out,
                       rel_out, rel_max, flag, rel_flag, flag_rw);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// rows [first, first + cnt) of the store -> one of its planes, in the plane's format.  Half: scaled by the plane's factor, rows
// above HALF_REL_FLAG marked; bf16 marks nothing; int8: one scale per row, rows above I8_REL_FLAG marked, marks of rows that suit
// the format again taken back.
static uint32_t split_pitch(const ott_store* s) { return (s->dim + 31u) & ~31u; }  // floats
static uint32_t hi_pitch(const ott_store* s) { return (s->dim + 63u) & ~63u; }     // elements
static uint32_t i8_pitch(const ott_store* s) { return (s->dim + 127u) & ~127u; }   // bytes
static int convert_split(ott_store* own, hipStream_t stream, uint64_t first, uint64_t cnt) {
    return launch_split(stream, own->d_rows, own->ld, own->dim, split_pitch(own), first, cnt, (uint16_t*)own->planes.split.d, nullptr, own->n_cu);
}
static int convert_hi(ott_store* own, hipStream_t stream, uint64_t first, uint64_t cnt) {
    const PlaneSet& p = own->planes;
    const HiFormat f = p.hi_format;
    return launch_hi(stream, own->d_rows, own->ld, own->dim, hi_pitch(own), first, cnt, (uint16_t*)p.hi.d, nullptr, nullptr, p.hi.d_rel, own->d_flag, f.f16,
                     f.scale, f.f16 ? HALF_REL_FLAG : 2.0f, f.f16 ? own->d_flag : nullptr, own->n_cu);
}
static int convert_i8(ott_store* own, hipStream_t stream, uint64_t first, uint64_t cnt) {
    const PlaneSet& p = own->planes;
    return launch_i8_rows(stream, own->d_rows, own->ld, own->dim, i8_pitch(own), first, cnt, (int8_t*)p.i8.d, nullptr, 0.0f, p.d_i8_scale, nullptr, p.i8.d_rel,
                          own->d_flag, I8_REL_FLAG, own->d_flag, own->n_cu);
}
typedef int (*ConvertFn)(ott_store* own, hipStream_t stream, uint64_t first, uint64_t cnt);

static int clear_flag_bits(ott_store* s, hipStream_t stream, uint64_t n, uint8_t mask) {
    hipLaunchKernelGGL(clear_flag_bit_kernel, dim3(grid_blocks(n, 256, s->n_cu)), dim3(256), 0, stream, s->d_flag, n, mask);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}
int planes_clear_marks(ott_store* s, uint64_t n) { return clear_flag_bits(s, s->stream, n, 0xF9); }

// ---------------------------------------------------------------------------------------------
// the life cycle (struct Plane in ott_internal.h), one function per step
// ---------------------------------------------------------------------------------------------

static ott_store* owner_of(const ott_store* ctx) { return const_cast<ott_store*>(ctx->owner ? ctx->owner : ctx); }

// The buffer of a plane that is wanted: there already, allocated now, or DECLINED — the options say so (`declined`), it does not
// fit beside `extra` more bytes and 2 GiB of head-room, or the allocation fails.  The plane is then off and the error swallowed:
// the cascade starts one level further down.
static bool plane_alloc(Plane& pl, size_t bytes, size_t extra, bool declined) {
    if (pl.d) return true;
    size_t free_b = 0, total_b = 0;
    if (declined || hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + extra + (size_t)(2ull << 30) || hipMalloc(&pl.d, bytes) != hipSuccess) {
        pl.d = nullptr;
        pl.off = true;
        (void)hipGetLastError();
        return false;
    }
    pl.rows = 0;
    return true;
}

// the loss words of a plane that measures (allocated once), zeroed in front of a build from scratch
static int plane_loss_words(Plane& pl, hipStream_t stream) {
    if (!pl.d_rel) OTT_HIP(hipMalloc((void**)&pl.d_rel, 16));
    if (pl.rows == 0) OTT_HIP(hipMemsetAsync(pl.d_rel, 0, 16, stream));
    return OTT_OK;
}

// {max loss, rows marked} after a conversion, and the wait: what was converted may be published — other contexts' streams may read it at once
static int plane_read_loss(Plane& pl, hipStream_t stream, uint32_t* marked) {
    uint32_t bits[2] = {0, 0};
    OTT_HIP(hipMemcpyAsync(bits, pl.d_rel, 8, hipMemcpyDeviceToHost, stream));
    OTT_HIP(hipStreamSynchronize(stream));
    memcpy(&pl.rel, &bits[0], 4);
    *marked = bits[1];
    return OTT_OK;
}

// rows [pl.rows, own->n) -> the plane; the caller publishes them (pl.rows = own->n) once it has accepted the format
static int plane_extend(ott_store* own, hipStream_t stream, Plane& pl, ConvertFn convert, uint32_t* marked) {
    const int rc = convert(own, stream, pl.rows, own->n - pl.rows);
    return rc ? rc : plane_read_loss(pl, stream, marked);
}

static void planes_drop_locked(PlaneSet& p) {
    for (Plane* pl : {&p.split, &p.hi, &p.i8}) {
        if (pl->d) (void)hipFree(pl->d);
        pl->d = nullptr;
        pl->rows = 0;
    }
    if (p.d_i8_scale) (void)hipFree(p.d_i8_scale);
    p.d_i8_scale = nullptr;
}

// Frees the three planes and the scale array; the `off` flags and the loss words stay.  Every caller holds the store exclusively
// (`rw`), which already keeps queries and the background builder out: the mutex here only orders the writes against
// ott_store_batch_ready, which reads the planes under it without holding the store.
void planes_drop(ott_store* own) {
    std::lock_guard<std::mutex> g(own->planes.mu);
    planes_drop_locked(own->planes);
}

bool planes_any(ott_store* own) {
    const PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(own->planes.mu);
    return p.split.d || p.hi.d || p.i8.d;
}

void planes_release(ott_store* own) {
    planes_drop(own);
    for (Plane* pl : {&own->planes.hi, &own->planes.i8}) {
        if (pl->d_rel) (void)hipFree(pl->d_rel);
        pl->d_rel = nullptr;
    }
}

void planes_enable(ott_store* own, bool enabled) {
    PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(p.mu);
    if (!enabled) planes_drop_locked(p);
    p.split.off = !enabled;
    if (enabled) p.hi.off = p.i8.off = false;
}

void planes_set_options(ott_store* own, const Options& o) {
    PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(p.mu);
    if (own->opt.no_hi_pass && !o.no_hi_pass) p.hi.off = false;
    if (own->opt.no_batch_image && !o.no_batch_image) p.hi.off = p.split.off = p.i8.off = false;
    own->opt = o;
}

// Keeps the planes in step with rewritten rows: the part of [first, first + n) each plane covers is converted again, the hi and
// int8 planes' measured loss read back (it can only grow; the int8 marks of the rewritten rows are re-taken) — one wait per plane.
int planes_rewrite(ott_store* s, uint64_t first, uint64_t n) {
    PlaneSet& p = s->planes;
    std::lock_guard<std::mutex> g(p.mu);
    auto covered = [&](const Plane& pl) { return pl.d && first < pl.rows ? std::min(first + n, pl.rows) - first : (uint64_t)0; };
    int rc = OTT_OK;
    uint32_t marked = 0;
    if (const uint64_t cnt = covered(p.split))
        if ((rc = convert_split(s, s->stream, first, cnt))) return rc;
    if (const uint64_t cnt = covered(p.hi))
        if ((rc = convert_hi(s, s->stream, first, cnt)) || (rc = plane_read_loss(p.hi, s->stream, &marked))) return rc;
    if (const uint64_t cnt = covered(p.i8))
        if ((rc = convert_i8(s, s->stream, first, cnt)) || (rc = plane_read_loss(p.i8, s->stream, &marked))) return rc;
    return OTT_OK;
}

// ---------------------------------------------------------------------------------------------
// built / extended on demand (see ott_internal.h); *img_out = nullptr when the plane is unavailable
// ---------------------------------------------------------------------------------------------

int ensure_batch_image(ott_store* ctx, const uint16_t** img_out) {
    *img_out = nullptr;
    ott_store* own = owner_of(ctx);
    PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(p.mu);
    if (p.split.off || own->n == 0) return OTT_OK;
    // declined: the kernel splits the f32 rows in registers instead
    if (!plane_alloc(p.split, (size_t)own->cap * split_pitch(own) * 4, 0, own->opt.no_batch_image)) return OTT_OK;
    if (p.split.rows < own->n) {
        const int rc = convert_split(own, ctx->stream, p.split.rows, own->n - p.split.rows);
        if (rc) return rc;
        OTT_HIP(hipStreamSynchronize(ctx->stream));  // published below: other contexts' streams may read it at once
        p.split.rows = own->n;
    }
    *img_out = (const uint16_t*)p.split.d;
    return OTT_OK;
}

int ensure_hi_plane(ott_store* ctx, const uint16_t** img_out, float* rel_max_out, bool* f16_out, float* scale_out) {
    *img_out = nullptr;
    if (f16_out) *f16_out = false;
    if (scale_out) *scale_out = 1.0f;
    ott_store* own = owner_of(ctx);
    PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(p.mu);
    if (p.hi.off || p.split.off || own->n == 0) return OTT_OK;
    // declined: the batch path starts at the split pass
    if (!plane_alloc(p.hi, (size_t)own->cap * hi_pitch(own) * 2, 0, own->opt.no_batch_image || own->opt.no_hi_pass)) return OTT_OK;
    int rc = plane_loss_words(p.hi, ctx->stream);
    if (rc) return rc;
    if (p.hi.rows == 0) {
        // the format (hi_plane_format).  Half needs ONE power-of-two factor for all rows, derived from the largest REGULAR row norm
        uint32_t got = 0x7F800000u;
        if (own->opt.hi_fmt != 0) {
            const uint32_t init = got;
            OTT_HIP(hipMemcpyAsync(p.hi.d_rel + 2, &init, 4, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(min_regular_inv_kernel, dim3(grid_blocks(own->n, 256, own->n_cu)), dim3(256), 0, ctx->stream, own->d_inv, own->d_flag, own->n,
                               p.hi.d_rel + 2);
            OTT_HIP(hipGetLastError());
            OTT_HIP(hipMemcpyAsync(&got, p.hi.d_rel + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
            OTT_HIP(hipStreamSynchronize(ctx->stream));
        }
        p.hi_format = hi_plane_format(own->opt.hi_fmt, got);
    }
    if (p.hi.rows < own->n) {
        const bool from_scratch = p.hi.rows == 0;
        const uint64_t cnt = own->n - p.hi.rows;
        uint32_t marked = 0;
        if ((rc = plane_extend(own, ctx->stream, p.hi, convert_hi, &marked))) return rc;
        if (p.hi_format.f16 && from_scratch && format_rejected(marked, cnt)) {
            // half is the wrong format for this store: the marks are taken back and the plane is built again as bf16
            p.hi_format = HiFormat{false, 1.0f};
            if ((rc = clear_flag_bits(own, ctx->stream, own->n, 0xFD))) return rc;
            OTT_HIP(hipMemsetAsync(p.hi.d_rel, 0, 16, ctx->stream));
            if ((rc = plane_extend(own, ctx->stream, p.hi, convert_hi, &marked))) return rc;
        }
        p.hi.rows = own->n;
    }
    *img_out = (const uint16_t*)p.hi.d;
    *rel_max_out = p.hi.rel;
    if (f16_out) *f16_out = p.hi_format.f16;
    if (scale_out) *scale_out = p.hi_format.scale;
    return OTT_OK;
}

// the int8 plane and its scales go and stay away
static void i8_decline(PlaneSet& p) {
    (void)hipFree(p.i8.d);
    if (p.d_i8_scale) (void)hipFree(p.d_i8_scale);
    p.i8.d = nullptr;
    p.d_i8_scale = nullptr;
    p.i8.off = true;
}

int ensure_i8_plane(ott_store* ctx, const int8_t** img_out, const float** scale_out, float* rel_max_out) {
    *img_out = nullptr;
    *scale_out = nullptr;
    ott_store* own = owner_of(ctx);
    PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(p.mu);
    if (p.i8.off || p.split.off || own->n == 0 || !i8_wanted(own->opt) || own->dim < 8) return OTT_OK;
    if (!p.i8.d) {
        // declined: the cascade starts at the hi pass
        if (!plane_alloc(p.i8, (size_t)own->cap * i8_pitch(own), (size_t)own->cap * 4, own->opt.no_batch_image || own->opt.no_hi_pass)) return OTT_OK;
        if (hipMalloc((void**)&p.d_i8_scale, (size_t)own->cap * 4) != hipSuccess) {
            p.d_i8_scale = nullptr;
            i8_decline(p);
            (void)hipGetLastError();
            return OTT_OK;
        }
    }
    int rc = plane_loss_words(p.i8, ctx->stream);
    if (rc) return rc;
    if (p.i8.rows < own->n) {
        const bool from_scratch = p.i8.rows == 0;
        const uint64_t cnt = own->n - p.i8.rows;
        uint32_t marked = 0;
        if ((rc = plane_extend(own, ctx->stream, p.i8, convert_i8, &marked))) return rc;
        if (from_scratch && format_rejected(marked, cnt)) {
            // int8 is the wrong format for this store: the marks are taken back, the plane is freed and declined
            if ((rc = clear_flag_bits(own, ctx->stream, own->n, 0xFB))) return rc;
            OTT_HIP(hipStreamSynchronize(ctx->stream));
            i8_decline(p);
            return OTT_OK;
        }
        p.i8.rows = own->n;
    }
    *img_out = (const int8_t*)p.i8.d;
    *scale_out = p.d_i8_scale;
    *rel_max_out = p.i8.rel;
    return OTT_OK;
}

int ensure_first_plane(ott_store* ctx) {
    ott_store* own = owner_of(ctx);
    float rel = 0.f;
    if (i8_wanted(own->opt)) {
        const int8_t* i8 = nullptr;
        const float* i8s = nullptr;
        const int rc = ensure_i8_plane(ctx, &i8, &i8s, &rel);
        if (rc) return rc;
        if (i8 && !plane_snapshot(own).have_hi) return OTT_OK;  // the hi plane is built when a query first needs it
    }
    const uint16_t* img = nullptr;
    return ensure_hi_plane(ctx, &img, &rel);
}

PlaneSnapshot plane_snapshot(const ott_store* s) {
    ott_store* own = owner_of(s);
    const PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(own->planes.mu);
    return PlaneSnapshot{p.i8.d != nullptr, p.i8.off, p.hi.d != nullptr, p.hi_format.f16, p.hi.off, p.split.off, p.i8.rows, p.hi.rows};
}

// the plane exists and covers every row (nothing is built by asking)
static bool plane_ready(ott_store* own, const Plane& pl) {
    std::lock_guard<std::mutex> g(own->planes.mu);
    return pl.d != nullptr && !pl.off && !own->planes.split.off && own->n != 0 && pl.rows == own->n;
}
bool hi_plane_ready(ott_store* ctx) { return plane_ready(owner_of(ctx), owner_of(ctx)->planes.hi); }
bool i8_plane_ready(ott_store* ctx) { return plane_ready(owner_of(ctx), owner_of(ctx)->planes.i8); }
// ... and, where it is ready, what a reader of it needs, taken under the same lock: the plane, the rows' scales, the measured loss.
// The caller holds the store (shared), so nothing moves the rows; a builder on another context only ever extends a plane that does
// not cover the store yet, and this one does
bool i8_plane_peek(ott_store* ctx, const int8_t** img_out, const float** scale_out, float* rel_max_out) {
    ott_store* own = owner_of(ctx);
    const PlaneSet& p = own->planes;
    std::lock_guard<std::mutex> g(own->planes.mu);
    if (!(p.i8.d != nullptr && !p.i8.off && !p.split.off && own->n != 0 && p.i8.rows == own->n && p.d_i8_scale != nullptr)) return false;
    *img_out = (const int8_t*)p.i8.d;
    *scale_out = p.d_i8_scale;
    *rel_max_out = p.i8.rel;
    return true;
}

bool first_plane_ready(ott_store* ctx) {
    ott_store* own = owner_of(ctx);
    bool i8_on;
    {
        std::lock_guard<std::mutex> g(own->planes.mu);
        i8_on = i8_wanted(own->opt) && !own->planes.i8.off && own->dim >= 8;
    }
    return i8_on ? i8_plane_ready(ctx) : hi_plane_ready(ctx);
}

// ---------------------------------------------------------------------------------------------
// the background builder
// ---------------------------------------------------------------------------------------------

// The first plane off the first batch's critical path (round 4).  A first 256-query batch on a fresh 10M x 768 store took 19 ms:
// 15 of them the allocation and conversion of the 16-bit plane.  With option hi_prebuild (automatic for stores of 262144 rows
// and more) every append ends by waking this thread, which takes the store like a query does (shared), converts the rows that
// are new (~10 ms per 30 GB, on a context of its own) and goes back to sleep; a batch that arrives while it is at work waits for
// it on the planes' mutex exactly as it would have built the plane itself.  Results never depend on it.
//
// One run of the background builder (ott::host::QuietWorker calls it once the appends have been quiet for 20 ms: a store loaded
// in pieces is not converted piece by piece — each conversion holds the store shared, i.e. the next append waits for it, and a
// growing store's reallocation drops the plane again: a 30-GB load in 100k-row pieces went from 2.4 to 4.0 s without the wait)
static void plane_builder_run(ott_store* s) {
    ott::host::SharedLock rd(s->rw);
    if (use_device(s) != hipSuccess) return;
    if (s->opt.hi_prebuild < 0) {  // automatic: only while the plane is a modest share of what is free
        size_t free_b = 0, total_b = 0;
        const PlaneSnapshot ps = plane_snapshot(s);
        const bool i8 = i8_wanted(s->opt) && !ps.i8_off;
        const size_t bytes = i8 ? (size_t)s->cap * i8_pitch(s) : (size_t)s->cap * hi_pitch(s) * 2;
        if (!(i8 ? ps.have_i8 : ps.have_hi) && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 4)) return;
    }
    ott_store* ctx = ctx_acquire(s);
    mfma_warm(ctx->stream, s->device);  // the batch path's kernels onto the device first: the first batch of a process paid 10-15 ms for that
    (void)ensure_first_plane(ctx);  // (a failure leaves the plane to the first batch, as before)
    ctx_release(ctx);
    (void)hipGetLastError();
}

void kick_plane_build(ott_store* s) {
    if (s->is_worker || s->multi) return;
    const int pol = s->opt.hi_prebuild;
    const PlaneSnapshot ps = plane_snapshot(s);
    if (pol == 0 || s->opt.no_hi_pass || s->opt.no_batch_image || s->opt.mfma_f32 || ps.hi_off || ps.img_off) return;
    if (pol < 0 && s->n < 262144) return;
    if (s->dim < 8) return;
    {
        const bool i8 = i8_wanted(s->opt) && !ps.i8_off;
        const bool i8_stale = i8 && ps.i8_rows < s->n, hi_stale = (!i8 || ps.have_hi) && ps.hi_rows < s->n;
        if (!i8_stale && !hi_stale) return;
    }
    if (!s->builder) s->builder = new ott::host::QuietWorker([s] { plane_builder_run(s); }, std::chrono::milliseconds(20));
    s->builder->kick();
}

}  // namespace ott
