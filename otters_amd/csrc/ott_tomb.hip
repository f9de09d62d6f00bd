// ott_tomb.hip — deleted rows: the store's device-resident LIVE mask, the delete / restore kernel, the
// composition of the live mask with a query's own row mask, and physical compaction.
//
// A deleted row keeps its slot, its data, its inverse norm and its sketch line; only its bit in the live mask is cleared.  The
// mask reaches the kernels through the ONE place every query path takes its row mask from (query_core, "row mask -> device"):
// a query without a row mask of its own gets the live mask itself (no launch), one with a host mask or the evaluated device mask
// gets `caller & live` from and_live_kernel, written into the query context's scratch (the evaluated mask is never changed: a
// later restore shows through).  A store that never had a deletion has no mask and runs exactly what it ran before.
//
// Invariant of the words: every bit at and past the store's length is 1 (in every allocated word), so appends need nothing.
#include <string.h>

#include <vector>

#include "ott_internal.h"

using namespace ott;

namespace {

// rows[i] < the store's length (checked on the host): bit rows[i] of the live mask is set (make_live) or cleared.  The OLD bit
// tells whether this thread changed the row's state — a row listed twice, or already in that state, counts once or not at all —
// and one atomic per wave adds the wave's changes to *changed.
__global__ __launch_bounds__(256) void set_live_kernel(uint64_t* __restrict__ live, const uint64_t* __restrict__ rows, uint64_t n, uint32_t make_live,
                                                       unsigned long long* __restrict__ changed) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    uint32_t mine = 0;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += step) {  // (i0 is uniform over the workgroup)
        const uint64_t i = i0 + threadIdx.x;
        if (i < n) {
            const uint64_t r = rows[i];
            const unsigned long long bit = 1ull << (r & 63);
            unsigned long long* w = reinterpret_cast<unsigned long long*>(live) + (r >> 6);
            const unsigned long long old = make_live ? atomicOr(w, bit) : atomicAnd(w, ~bit);
            mine += make_live ? ((old & bit) == 0) : ((old & bit) != 0);
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(changed, (unsigned long long)mine);
}

// out[w] = live[w] & caller[w] over the words of n_bits rows; caller bits at and past caller_bits count as keep (src/vec.rs:234:
// the partial boundary word too), caller == nullptr is caller_bits = 0
__global__ __launch_bounds__(256) void and_live_kernel(const uint64_t* __restrict__ live, const uint64_t* __restrict__ caller, uint64_t caller_bits,
                                                       uint64_t n_bits, uint64_t* __restrict__ out) {
    const uint64_t words = (n_bits + 63) / 64;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t c = ~0ull;
        if (w * 64 < caller_bits) {
            c = caller[w];
            if (caller_bits - w * 64 < 64) c |= ~0ull << (caller_bits - w * 64);
        }
        out[w] = live[w] & c;
    }
}

// prefix[w] = live rows below word w (rows at and past n_bits do not count), prefix[words] = all of them.  One workgroup walks
// the words 1024 at a time with a running carry: 10M rows are 153 steps.
__global__ __launch_bounds__(1024) void live_scan_kernel(const uint64_t* __restrict__ live, uint64_t n_bits, uint32_t* __restrict__ prefix) {
    __shared__ uint32_t wsum[16];
    const uint64_t words = (n_bits + 63) / 64;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < words; base += 1024) {
        const uint64_t w = base + threadIdx.x;
        uint32_t c = 0;
        if (w < words) {
            uint64_t v = live[w];
            if (w == words - 1 && (n_bits & 63)) v &= (1ull << (n_bits & 63)) - 1;
            c = (uint32_t)__popcll(v);
        }
        uint32_t x = c;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if ((int)lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t j = 0; j < 16; j++) {
            before += j < wave ? wsum[j] : 0u;
            total += wsum[j];
        }
        if (w < words) prefix[w] = carry + before + x - c;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) prefix[words] = carry;
}

// live rows of the source window [r0, r1) -> bounce slots, in order: slot = (live rows below the row) - d0.  One thread per
// (row, 16 B); the thread of a row's first piece takes its inverse norm and its flag byte along.
__global__ __launch_bounds__(256) void compact_gather_kernel(const float* __restrict__ rows, const float* __restrict__ inv, const uint8_t* __restrict__ flag,
                                                             const uint64_t* __restrict__ live, const uint32_t* __restrict__ prefix, uint32_t ld, uint64_t r0,
                                                             uint64_t r1, uint64_t d0, float* __restrict__ b_rows, float* __restrict__ b_inv,
                                                             uint8_t* __restrict__ b_flag) {
    const uint32_t quads = ld / 4;
    const uint64_t total = (r1 - r0) * quads;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = r0 + i / quads;
        const uint32_t c = (uint32_t)(i % quads);
        const uint64_t word = live[r >> 6];
        if (!((word >> (r & 63)) & 1)) continue;
        const uint64_t slot = (uint64_t)prefix[r >> 6] + (uint64_t)__popcll(word & ((1ull << (r & 63)) - 1)) - d0;
        reinterpret_cast<float4*>(b_rows)[slot * quads + c] = reinterpret_cast<const float4*>(rows)[r * quads + c];
        if (c == 0) {
            b_inv[slot] = inv[r];
            b_flag[slot] = flag[r];
        }
    }
}

uint64_t live_words(uint64_t bits) { return (bits + 63) / 64; }

// the mask of a store that has none yet: every slot live
int live_alloc(ott_store* s) {
    if (s->d_live) return OTT_OK;
    const size_t bytes = (size_t)live_words(s->cap) * 8;
    OTT_HIP(hipMalloc((void**)&s->d_live, bytes));
    OTT_HIP(hipMemsetAsync(s->d_live, 0xFF, bytes, s->stream));
    s->n_dead = 0;
    return OTT_OK;
}

// argument checks shared by delete and restore, before any device work
int check_rows(const char* who, const ott_store* s, const uint64_t* rows_host, uint64_t n, uint64_t len) {
    if (!s) return fail(OTT_ERR_INVALID, std::string(who) + ": store is NULL");
    if (n && !rows_host) return fail(OTT_ERR_INVALID, std::string(who) + ": rows is NULL");
    for (uint64_t i = 0; i < n; i++)
        if (rows_host[i] >= len)
            return fail(OTT_ERR_INVALID, std::string(who) + ": row " + std::to_string(rows_host[i]) + " is out of range (the store holds " +
                                             std::to_string(len) + " rows)");
    return OTT_OK;
}

int set_live(ott_store* s, bool make_live, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed) {
    const char* who = make_live ? "ott_store_restore_rows" : "ott_store_delete_rows";
    if (n_changed) *n_changed = 0;
    if (!s) return fail(OTT_ERR_INVALID, std::string(who) + ": store is NULL");
    if (n && !rows_host) return fail(OTT_ERR_INVALID, std::string(who) + ": rows is NULL");
    if (s->multi) return multi_set_live(s, make_live, rows_host, n, n_changed);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = check_rows(who, s, rows_host, n, store_rows(s));  // (staged rows count: they were appended)
    if (rc) return rc;
    if ((rc = store_flush_locked(s))) return rc;
    if (!n || (make_live && !s->d_live)) return OTT_OK;  // nothing was ever deleted: nothing to restore
    OTT_HIP(use_device(s));
    if ((rc = live_alloc(s))) return rc;
    // [changed (u64, 64 B) | the indices], one copy up
    if ((rc = s->d_livefx.ensure(64 + (size_t)n * 8))) return rc;
    unsigned long long* d_changed = (unsigned long long*)s->d_livefx.p;
    uint64_t* d_rows_idx = (uint64_t*)((char*)s->d_livefx.p + 64);
    OTT_HIP(hipMemsetAsync(d_changed, 0, 8, s->stream));
    OTT_HIP(hipMemcpyAsync(d_rows_idx, rows_host, (size_t)n * 8, hipMemcpyHostToDevice, s->stream));
    uint64_t blocks = (n + 255) / 256;
    if (blocks > (uint64_t)s->n_cu * 8) blocks = (uint64_t)s->n_cu * 8;
    hipLaunchKernelGGL(set_live_kernel, dim3((uint32_t)blocks), dim3(256), 0, s->stream, s->d_live, d_rows_idx, n, make_live ? 1u : 0u, d_changed);
    OTT_HIP(hipGetLastError());
    unsigned long long changed = 0;
    OTT_HIP(hipMemcpyAsync(&changed, d_changed, 8, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    if (make_live) s->n_dead -= changed;
    else s->n_dead += changed;
    if (changed) sparse_df_stale(s);  // the document frequencies count live rows
    if (n_changed) *n_changed = changed;
    return OTT_OK;
}

}  // namespace

namespace ott {

int live_grow(ott_store* s, uint64_t ncap) {
    if (!s->d_live) return OTT_OK;
    const size_t old_w = (size_t)live_words(s->cap), new_w = (size_t)live_words(ncap);
    if (new_w <= old_w) return OTT_OK;
    uint64_t* nl = nullptr;
    OTT_HIP(hipMalloc((void**)&nl, new_w * 8));
    OTT_HIP(hipMemcpyAsync(nl, s->d_live, old_w * 8, hipMemcpyDeviceToDevice, s->stream));
    OTT_HIP(hipMemsetAsync(nl + old_w, 0xFF, (new_w - old_w) * 8, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    (void)hipFree(s->d_live);
    s->d_live = nl;
    return OTT_OK;
}

void live_drop(ott_store* s) {
    if (s->d_live) (void)hipFree(s->d_live);
    s->d_live = nullptr;
    s->n_dead = 0;
    sparse_df_stale(s);
}

int live_load(ott_store* s, const uint64_t* words_host) {
    const uint64_t n = s->n, words = live_words(n);
    std::vector<uint64_t> w(words_host, words_host + words);
    if (n & 63) w[(size_t)words - 1] |= ~0ull << (n & 63);
    uint64_t dead = 0;
    for (uint64_t v : w) dead += 64 - (uint64_t)__builtin_popcountll(v);
    OTT_HIP(hipStreamSynchronize(s->stream));
    live_drop(s);
    if (!dead) return OTT_OK;
    int rc = live_alloc(s);
    if (rc) return rc;
    OTT_HIP(hipMemcpyAsync(s->d_live, w.data(), (size_t)words * 8, hipMemcpyHostToDevice, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    s->n_dead = dead;
    return OTT_OK;
}

int live_read(const ott_store* s, uint64_t* out_host) {
    const uint64_t n = s->n, words = live_words(n);
    if (!words) return OTT_OK;
    if (s->d_live) {
        OTT_HIP(use_device(s));
        OTT_HIP(hipMemcpy(out_host, s->d_live, (size_t)words * 8, hipMemcpyDeviceToHost));
    } else {
        memset(out_host, 0xFF, (size_t)words * 8);
    }
    if (n & 63) out_host[words - 1] &= (1ull << (n & 63)) - 1;
    return OTT_OK;
}

int mask_and(ott_store* ctx, const uint64_t* keep, const uint64_t* caller, uint64_t caller_bits, uint64_t n_bits, uint64_t* out) {
    const uint64_t words = live_words(n_bits);
    uint64_t blocks = (words + 255) / 256;
    if (blocks > (uint64_t)ctx->n_cu * 4) blocks = (uint64_t)ctx->n_cu * 4;
    if (!blocks) return OTT_OK;
    hipLaunchKernelGGL(and_live_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, keep, caller, caller_bits, n_bits, out);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

int live_compose(ott_store* ctx, const uint64_t** d_mask, uint64_t* mask_bits) {
    if (!ctx->d_live || !ctx->n_dead) return OTT_OK;
    if (!*d_mask) {  // the kernels read the live mask itself
        *d_mask = ctx->d_live;
        *mask_bits = ctx->n;
        return OTT_OK;
    }
    const uint64_t words = live_words(ctx->n);
    int rc = ctx->d_livefx.ensure((size_t)words * 8);
    if (rc) return rc;
    if ((rc = mask_and(ctx, ctx->d_live, *d_mask, *mask_bits, ctx->n, (uint64_t*)ctx->d_livefx.p))) return rc;
    *d_mask = (const uint64_t*)ctx->d_livefx.p;
    *mask_bits = ctx->n;
    return OTT_OK;
}

}  // namespace ott

extern "C" {

int ott_store_delete_rows(ott_store* s, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed) { return set_live(s, false, rows_host, n, n_changed); }
int ott_store_restore_rows(ott_store* s, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed) { return set_live(s, true, rows_host, n, n_changed); }

uint64_t ott_store_live_len(const ott_store* s) {
    if (!s) return 0;
    if (s->multi) return multi_live_len(s);
    return store_rows(s) - s->n_dead;
}

int ott_store_read_live_mask(const ott_store* cs, uint64_t* out_host) {
    ott_store* s = const_cast<ott_store*>(cs);
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_read_live_mask: store is NULL");
    if (!out_host) return fail(OTT_ERR_INVALID, "ott_store_read_live_mask: out is NULL");
    if (s->multi) return multi_read_live_mask(s, out_host);
    const int rcf = store_flush(s);
    if (rcf) return rcf;
    ott::host::SharedLock rd(s->rw);
    return live_read(s, out_host);
}

int ott_store_compact(ott_store* s, uint64_t* out_new_index) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_compact: store is NULL");
    if (s->multi) return fail(OTT_ERR_UNSUPPORTED, "ott_store_compact: not on a multi-GPU store (the shards' row ranges are pinned to chunk multiples)");
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    if (!s->columns.empty())
        return fail(OTT_ERR_UNSUPPORTED, "ott_store_compact: rows cannot move once metadata columns are resident");
    if (s->d_gid)  // group ids count as a resident column (ott_group.hip)
        return fail(OTT_ERR_UNSUPPORTED, "ott_store_compact: rows cannot move while group ids are set (ott_store_clear_groups first, set them again afterwards)");
    if (s->d_sparse)  // ... and so do sparse rows (ott_sparse.hip)
        return fail(OTT_ERR_UNSUPPORTED, "ott_store_compact: rows cannot move while sparse rows are set (ott_store_clear_sparse first, set them again afterwards)");
    if (s->d_binary)  // ... and bit rows (ott_binary.hip)
        return fail(OTT_ERR_UNSUPPORTED, "ott_store_compact: rows cannot move while bit rows are set (ott_store_clear_binary first, set them again afterwards)");
    int rc = store_flush_locked(s);
    if (rc) return rc;
    const uint64_t n = s->n;
    if (!s->n_dead) {  // nothing to remove: every row keeps its index (a mask that has no cleared bit left goes all the same)
        if (out_new_index)
            for (uint64_t r = 0; r < n; r++) out_new_index[r] = r;
        if (s->d_live) {
            OTT_HIP(use_device(s));
            OTT_HIP(hipStreamSynchronize(s->stream));
            live_drop(s);
        }
        return OTT_OK;
    }
    OTT_HIP(use_device(s));
    const uint64_t words = live_words(n);
    // the scan: live rows below every word.  Its host copy plans the windows and gives out_new_index
    if ((rc = s->d_livefx.ensure((size_t)(words + 1) * 4))) return rc;
    uint32_t* d_prefix = (uint32_t*)s->d_livefx.p;
    hipLaunchKernelGGL(live_scan_kernel, dim3(1), dim3(1024), 0, s->stream, s->d_live, n, d_prefix);
    OTT_HIP(hipGetLastError());
    std::vector<uint32_t> prefix((size_t)words + 1);
    std::vector<uint64_t> mask((size_t)words);
    OTT_HIP(hipMemcpyAsync(prefix.data(), d_prefix, (size_t)(words + 1) * 4, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipMemcpyAsync(mask.data(), s->d_live, (size_t)words * 8, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));
    const uint64_t n_live = prefix[(size_t)words];
    if (n_live != n - s->n_dead) return fail(OTT_ERR_HIP, "ott_store_compact: the live mask's count does not match the store's");
    // The move.  A window of W source rows (a multiple of 64: whole mask words) has at most W live rows: they go to the bounce
    // buffer in order (one launch), then from there to their destination (copies on the same stream).  The destination
    // [d0, d0 + cnt) ends at or below the window's end, so it never reaches rows a later window still has to read; it may overlap
    // the window's own rows, which are already in the bounce buffer.  A window without a deleted row in or before it stays put.
    const size_t row_bytes = (size_t)s->ld * 4;
    uint64_t W = (((size_t)128 << 20) / (row_bytes + 5)) & ~(uint64_t)63;
    if (W < 64) W = 64;
    if (W > words * 64) W = words * 64;
    char* bounce = nullptr;
    const size_t off_inv = (size_t)W * row_bytes, off_flag = off_inv + (size_t)W * 4;
    OTT_HIP(hipMalloc((void**)&bounce, off_flag + (size_t)W));
    for (uint64_t r0 = 0; r0 < n; r0 += W) {
        const uint64_t r1 = r0 + W < n ? r0 + W : n;
        const uint64_t d0 = prefix[(size_t)(r0 >> 6)], d1 = (r1 & 63) ? n_live : prefix[(size_t)(r1 >> 6)], cnt = d1 - d0;
        if (!cnt || (d0 == r0 && cnt == r1 - r0)) continue;
        const uint64_t work = (r1 - r0) * (s->ld / 4);
        uint64_t blocks = (work + 255) / 256;
        if (blocks > (uint64_t)s->n_cu * 16) blocks = (uint64_t)s->n_cu * 16;
        hipLaunchKernelGGL(compact_gather_kernel, dim3((uint32_t)blocks), dim3(256), 0, s->stream, s->d_rows, s->d_inv, s->d_flag, s->d_live, d_prefix, s->ld,
                           r0, r1, d0, (float*)bounce, (float*)(bounce + off_inv), (uint8_t*)(bounce + off_flag));
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(s->d_rows + d0 * s->ld, bounce, (size_t)cnt * row_bytes, hipMemcpyDeviceToDevice, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s->d_inv + d0, bounce + off_inv, (size_t)cnt * 4, hipMemcpyDeviceToDevice, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s->d_flag + d0, bounce + off_flag, (size_t)cnt, hipMemcpyDeviceToDevice, s->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s->stream);
            (void)hipFree(bounce);
            return fail(OTT_ERR_HIP, std::string("ott_store_compact: ") + hipGetErrorString(e));
        }
    }
    hipError_t e = hipStreamSynchronize(s->stream);
    (void)hipFree(bounce);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(OTT_ERR_HIP, std::string("ott_store_compact: ") + hipGetErrorString(e));
    }
    if (out_new_index) {
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t word = mask[(size_t)(r >> 6)];
            out_new_index[r] = ((word >> (r & 63)) & 1) ? (uint64_t)prefix[(size_t)(r >> 6)] + (uint64_t)__builtin_popcountll(word & ((1ull << (r & 63)) - 1)) : UINT64_MAX;
        }
    }
    live_drop(s);
    return store_after_compact(s, n_live);
}

}  // extern "C"
