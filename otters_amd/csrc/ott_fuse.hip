// ott_fuse.hip — rank fusion: ott_query_fuse turns the hit lists of several queries ("legs") into one ranking per
// request, by reciprocal rank fusion, distribution-based score fusion or min-max score fusion.
//
// The first stage is the library's own query (query_on) on the call's context with k = min(fetch, rows), PER_QUERY: a leg's list IS
// what ott_query returns for that vector, on every path and tie order.  On the device route the lists stay in the context's scratch
// as sentinel-padded blocks (query_on's device output, no host wait); on the host route they come back, are staged in pinned memory
// and go up in one copy.  fuse_kernel is the second stage on both: one workgroup per request, one launch per call — the legs'
// statistics (one wave per leg), one 64-bit key and one f32 contribution per entry, a bitonic sort by (row, leg), the serial sum of
// every run of equal rows in leg order, a second bitonic sort by the fused score, the best min(k, rows) written out.
// Host decisions (refusals, capacity, layout, key packing, padded counts, route) and the host statement of the formulas:
// ott_fuse_plan.h.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "ott_internal.h"
#include "ott_fuse_plan.h"

namespace ott {

struct FuseParams {
    const ott_hit* blocks;   // [nq][stride] the legs' lists, best first, sentinels (index = all ones) behind the real hits
    const uint32_t* first;   // [n_requests] a request's first leg
    const uint32_t* legs;    // [n_requests] its legs: 1 .. FUSE_MAX_LEGS, first + legs <= nq (checked on the host)
    const float* weights;    // [nq], or nullptr = all 1
    uint32_t* counts;        // [n_requests] fused hits of each request
    ott_hit* hits;           // [n_requests][kout]
    uint64_t base_offset, n_rows;
    uint32_t stride, kout, fusion, take_max;
    float rrf_k;
};

// Bitonic network over key[0 .. P) (P a power of two >= 64), ascending or descending; PAYLOAD: con[] moves with its key.  Thread t of
// a step owns the pair (i, i | j) with i = t's bits spread around bit j: every compare-exchange touches two slots nobody else does.
template <bool DESC, bool PAYLOAD>
__device__ __forceinline__ void fuse_bitonic(unsigned long long* key, float* con, uint32_t P, uint32_t tid, uint32_t T) {
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (P >> 1); t += T) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
                const unsigned long long a = key[i], c = key[x];
                const bool up = ((i & k) == 0) != DESC;
                if (up ? a > c : a < c) {
                    key[i] = c;
                    key[x] = a;
                    if (PAYLOAD) {
                        const float f = con[i];
                        con[i] = con[x];
                        con[x] = f;
                    }
                }
            }
            __syncthreads();
        }
}

// Dynamic LDS: [P] 64-bit keys, [P] f32 contributions, P the request's padded entry count (ott_fuse_plan.h: fuse_padded).  The launch
// sizes both by the call's largest request; a smaller request runs its own, smaller network.
__global__ __launch_bounds__(FUSE_THREADS) void fuse_kernel(FuseParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fuse_smem[];
    __shared__ double sWorst[FUSE_MAX_LEGS], sSpan[FUSE_MAX_LEGS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6, n_waves = T >> 6;
    const uint32_t first = p.first[b], legs = p.legs[b];
    const uint32_t entries = legs * p.stride;  // <= FUSE_MAX_ENTRIES
    uint32_t P = 64;
    while (P < entries) P <<= 1;
    unsigned long long* key = (unsigned long long*)fuse_smem;
    float* con = (float*)(fuse_smem + (size_t)P * 8);
    const bool tmax = p.take_max != 0;

    // per-leg statistics, one wave per leg: the 64 strided partials are the lanes, the tree is the lane reduction
    if (p.fusion != FUSE_RRF) {
        for (uint32_t l = wave; l < legs; l += n_waves) {
            const ott_hit* list = p.blocks + (size_t)(first + l) * p.stride;
            uint32_t n = 0;
            for (uint32_t i = lane; i < p.stride; i += 64) n += list[i].index != ~0ull ? 1u : 0u;
#pragma unroll
            for (int h = 32; h > 0; h >>= 1) n += __shfl_xor(n, h);
            double worst = 0.0, span = 0.0;
            if (n != 0 && p.fusion == FUSE_MINMAX) {
                const double best = (double)list[0].score;
                worst = (double)list[n - 1].score;
                span = tmax ? __dsub_rn(best, worst) : __dsub_rn(worst, best);
            } else if (n != 0) {
                const double dn = (double)n;
                double a = 0.0;
                for (uint32_t i = lane; i < n; i += 64) a = __dadd_rn(a, (double)list[i].score);
#pragma unroll
                for (int h = 32; h > 0; h >>= 1) a = __dadd_rn(a, __shfl_down(a, h));
                const double mean = __ddiv_rn(__shfl(a, 0), dn);
                a = 0.0;
                for (uint32_t i = lane; i < n; i += 64) {
                    const double df = __dsub_rn((double)list[i].score, mean);
                    a = __dadd_rn(a, __dmul_rn(df, df));
                }
#pragma unroll
                for (int h = 32; h > 0; h >>= 1) a = __dadd_rn(a, __shfl_down(a, h));
                const double var = __ddiv_rn(__shfl(a, 0), dn);
                const double sd3 = __dmul_rn(3.0, __dsqrt_rn(var));
                const double lo = __dsub_rn(mean, sd3), hi = __dadd_rn(mean, sd3);
                worst = tmax ? lo : hi;
                span = __dsub_rn(hi, lo);
            }
            if (lane == 0) {
                sWorst[l] = worst;
                sSpan[l] = span;
            }
        }
        __syncthreads();
    }

    // entries: key and contribution; a sentinel, a slot past the request's entries and a row outside the store pad
    for (uint32_t e = tid; e < P; e += T) {
        unsigned long long k = FUSE_PAD_KEY;
        float c = 0.0f;
        if (e < entries) {
            const uint32_t l = e / p.stride, r = e - l * p.stride;
            const ott_hit h = p.blocks[(size_t)(first + l) * p.stride + r];
            const uint64_t row = h.index - p.base_offset;
            if (h.index != ~0ull && row < p.n_rows) {
                const float w = p.weights ? p.weights[first + l] : 1.0f;
                if (p.fusion == FUSE_RRF) {
                    c = __fdiv_rn(w, __fadd_rn(p.rrf_k, (float)(r + 1u)));
                } else {
                    float nrm = 0.5f;
                    const double span = sSpan[l];
                    if (span > 0.0) {
                        const double s = (double)h.score, worst = sWorst[l];
                        nrm = __double2float_rn(__ddiv_rn(tmax ? __dsub_rn(s, worst) : __dsub_rn(worst, s), span));
                    }
                    c = __fmul_rn(w, nrm);
                }
                k = (row << 13) | ((unsigned long long)l << 9) | r;
            }
        }
        key[e] = k;
        con[e] = c;
    }
    __syncthreads();
    fuse_bitonic<false, true>(key, con, P, tid, T);

    // a run of equal rows lies in leg order: its head adds the run's contributions serially and keeps F in its own slot (a head
    // reads and writes its own run only)
    for (uint32_t i = tid; i < P; i += T) {
        const unsigned long long k = key[i];
        if (k == FUSE_PAD_KEY || (i != 0 && (key[i - 1] >> 13) == (k >> 13))) continue;
        float F = 0.0f;
        for (uint32_t j = i; j < P && (key[j] >> 13) == (k >> 13) && key[j] != FUSE_PAD_KEY; j++) F = __fadd_rn(F, con[j]);
        con[i] = F;
    }
    __syncthreads();
    // everything but a head gets a NaN, which the next step drops like a head whose F is NaN ...
    for (uint32_t i = tid; i < P; i += T) {
        const unsigned long long k = key[i];
        if (k == FUSE_PAD_KEY || (i != 0 && (key[i - 1] >> 13) == (k >> 13))) con[i] = __uint_as_float(0x7FC00000u);
    }
    __syncthreads();
    // ... and every slot's key becomes ord(F) << 32 | ~head position << 13 | (leg, position): head positions ascend with the row, so
    // among equal F the lower row sorts first; the low 13 bits say where the row's index is read back from
    for (uint32_t i = tid; i < P; i += T) {
        const float F = con[i];
        const unsigned long long at = key[i] & 0x1FFFull;
        key[i] = F != F ? 0ull : ((unsigned long long)ord_of(F, true) << 32) | ((unsigned long long)(~i & 0x1FFFu) << 13) | at;
    }
    __syncthreads();
    fuse_bitonic<true, false>(key, con, P, tid, T);

    ott_hit* out = p.hits + (size_t)b * p.kout;
    for (uint32_t i = tid; i < P; i += T) {
        const unsigned long long k = key[i];
        if (k == 0ull) {
            if (i == 0) p.counts[b] = 0;
            continue;
        }
        if (i + 1 == P || key[i + 1] == 0ull) p.counts[b] = i + 1 < p.kout ? i + 1 : p.kout;  // the last ranked head: the count
        if (i < p.kout) {
            const uint32_t l = (uint32_t)(k >> 9) & 15u, r = (uint32_t)k & 511u;
            ott_hit h;
            h.index = p.blocks[(size_t)(first + l) * p.stride + r].index;
            h.score = score_of((uint32_t)(k >> 32), true);
            h.query = b;
            out[i] = h;
        }
    }
}

namespace {

int fuse_fail(FuseRefusal r, uint64_t bad, uint64_t v) { return fail(fuse_refusal_status(r), fuse_refusal_text(r, bad, v)); }

struct FuseCall {
    const ott_query_desc* d;
    const uint32_t* legs;
    uint32_t n_requests, fusion;
    float rrf_k;
    const float* weights;
    uint64_t stride;
    uint32_t max_legs;
};

// the meta block of the upload: [first | legs | weights] (weights all 1 when the caller gave none: the same bits)
void fill_meta(const FuseCall& c, const FuseLayout& L, char* base) {
    uint32_t* first = (uint32_t*)(base + L.off_first);
    uint32_t* legs = (uint32_t*)(base + L.off_legs);
    float* w = (float*)(base + L.off_weights);
    uint32_t at = 0;
    for (uint32_t b = 0; b < c.n_requests; b++) {
        first[b] = at;
        legs[b] = c.legs[b];
        at += c.legs[b];
    }
    for (uint32_t l = 0; l < c.d->nq; l++) w[l] = c.weights ? c.weights[l] : 1.0f;
}

int launch_fuse(ott_store* s, const FuseCall& c, const FuseLayout& L) {
    char* dm = (char*)s->d_fuse.p;
    FuseParams p;
    memset(&p, 0, sizeof(p));
    p.blocks = (const ott_hit*)(dm + L.off_blocks);
    p.first = (const uint32_t*)(dm + L.off_first);
    p.legs = (const uint32_t*)(dm + L.off_legs);
    p.weights = (const float*)(dm + L.off_weights);
    p.counts = (uint32_t*)(dm + L.off_counts);
    p.hits = (ott_hit*)(dm + L.off_hits);
    p.base_offset = s->base_offset;
    p.n_rows = s->n;
    p.stride = (uint32_t)c.stride;
    p.kout = L.kout;
    p.fusion = c.fusion;
    p.take_max = c.d->take == OTT_TAKE_MAX;
    p.rrf_k = c.rrf_k;
    const uint32_t padded = fuse_padded(c.max_legs * (uint32_t)c.stride);  // the network of the call's largest request
    const size_t smem = fuse_lds_bytes(padded);
    if (smem > 48 * 1024) {  // more dynamic LDS than the default limit: the opt-in, once per device
        static std::atomic<uint64_t> attr_set{0};
        if (attr_needed(attr_set, s->device)) {
            OTT_HIP(hipFuncSetAttribute((const void*)fuse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fuse_lds_bytes(FUSE_MAX_ENTRIES)));
            attr_done(attr_set, s->device);
        }
    }
    hipLaunchKernelGGL(fuse_kernel, dim3(c.n_requests), dim3(fuse_threads(padded)), smem, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

// Both stages on a context the caller holds.
int run_fuse(ott_store* s, const FuseCall& c, ott_hit* out, uint64_t* n_out, uint64_t* n_per_request, ott_stats* st, bool timing) {
    int rc;
    OTT_HIP(use_device(s));
    const ott_query_desc* d = c.d;
    const uint32_t nq = d->nq;
    const FuseLayout L = fuse_layout(nq, c.n_requests, c.stride, d->k, c.max_legs);
    if ((rc = s->d_fuse.ensure(L.total))) return rc;
    if ((rc = s->h_fuse.ensure(L.upload_bytes))) return rc;
    char* dm = (char*)s->d_fuse.p;
    char* hs = (char*)s->h_fuse.p;
    ott_query_desc d1 = *d;
    d1.k = c.stride;  // the first stage: the same descriptor with k = min(fetch, rows)
    ott_stats* st1 = timing ? st : nullptr;  // (kernel timing costs event records: only when the caller asked for stats)
    bool events_pending = false;
    if (fuse_take_device(s->opt.fuse_device, s->opt.tie_order, c.stride)) {
        // device route: the meta block goes up, the first stage writes the blocks behind it on the stream, nothing waits
        fill_meta(c, L, hs);
        OTT_HIP(hipMemcpyAsync(dm + L.off_first, hs + L.off_first, L.meta_bytes, hipMemcpyHostToDevice, s->stream));
        if ((rc = query_on(s, &d1, nullptr, dm + L.off_blocks, (uint64_t)nq * c.stride, nullptr, nullptr, nullptr, st1, true, &events_pending))) return rc;
    } else {
        // host route: the lists come back as ott_query's, are laid out as the same blocks and go up with the meta block in one copy
        std::vector<ott_hit> cand((size_t)nq * c.stride);
        std::vector<uint64_t> per(nq, 0);
        uint64_t n_cand = 0;
        if ((rc = query_on(s, &d1, cand.data(), nullptr, cand.size(), &n_cand, per.data(), nullptr, st1))) return rc;
        memset(hs, 0xFF, L.block_bytes);
        size_t at = 0;
        for (uint32_t l = 0; l < nq; l++) {
            if (per[l] > c.stride) return fail(OTT_ERR_HIP, "ott_query_fuse: the first stage returned more hits than fetch");
            for (uint64_t i = 0; i < per[l]; i++)
                if (cand[at + i].index - s->base_offset >= s->n) return fail(OTT_ERR_HIP, "ott_query_fuse: the first stage returned a row outside the store");
            if (per[l]) memcpy(hs + ((size_t)l * c.stride) * sizeof(ott_hit), &cand[at], (size_t)per[l] * sizeof(ott_hit));
            at += per[l];
        }
        fill_meta(c, L, hs);
        OTT_HIP(hipMemcpyAsync(dm, hs, L.upload_bytes, hipMemcpyHostToDevice, s->stream));
    }
    if (timing) OTT_HIP(hipEventRecord(s->ev[0], s->stream));
    if ((rc = launch_fuse(s, c, L))) return rc;
    if (timing) OTT_HIP(hipEventRecord(s->ev[1], s->stream));
    if ((rc = s->h_hits.ensure(L.result_bytes))) return rc;
    OTT_HIP(hipMemcpyAsync(s->h_hits.p, dm + L.off_counts, L.result_bytes, hipMemcpyDeviceToHost, s->stream));
    OTT_HIP(hipStreamSynchronize(s->stream));  // the device route's one host wait on the EXACT path
    if (timing) {
        if (events_pending) read_exact_events(s, st);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) st->merge_ns += (uint64_t)(ms * 1e6);
    }
    const uint32_t* counts = (const uint32_t*)s->h_hits.p;
    const ott_hit* hits = (const ott_hit*)((const char*)s->h_hits.p + (L.off_hits - L.off_counts));
    uint64_t total = 0;
    for (uint32_t b = 0; b < c.n_requests; b++) {
        const uint32_t nb = counts[b];
        if (nb > fuse_request_cap(d->k, c.legs[b], c.stride)) return fail(OTT_ERR_HIP, "ott_query_fuse: the kernel returned more hits than a request can have");
        if (nb) memcpy(out + total, hits + (size_t)b * L.kout, (size_t)nb * sizeof(ott_hit));
        if (n_per_request) n_per_request[b] = nb;
        total += nb;
    }
    if (n_out) *n_out = total;
    return OTT_OK;
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_fuse(ott_store* s, const ott_query_desc* d, const void* legs_per_request, uint32_t n_requests, uint32_t fusion, float rrf_k,
                   const float* leg_weights, uint64_t fetch, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_request, ott_stats* stats) {
    if (!d) return fail(OTT_ERR_INVALID, "ott_query_fuse: desc is NULL");
    const uint32_t* legs = (const uint32_t*)legs_per_request;
    uint64_t bad = 0, v = 0;
    FuseRefusal why = fuse_check_args(d->mode == OTT_MODE_PER_QUERY, legs, n_requests, d->nq, fetch, fusion, rrf_k, leg_weights, d->k, &bad, &v);  // before the store is looked at
    if (why != FUSE_OK) return fuse_fail(why, bad, v);
    int rc = validate_query(s, d);
    if (rc) return rc;
    const uint64_t len = ott_store_len(s);
    if ((why = fuse_check_store(s->multi != nullptr, len)) != FUSE_OK) return fuse_fail(why, 0, 0);
    if ((why = fuse_check_cap(out, cap, fuse_cap_needed(legs, n_requests, d->k, fetch, len))) != FUSE_OK) return fuse_fail(why, 0, 0);
    if (n_out) *n_out = 0;
    if (n_per_request)
        for (uint32_t b = 0; b < n_requests; b++) n_per_request[b] = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    const uint64_t t0 = now_ns();
    if (len == 0) return OTT_OK;  // an empty store: a valid call with no hits

    ott::host::SharedLock rd;  // the corpus cannot change between the two stages
    if ((rc = lock_store_shared(s, rd))) return rc;
    CtxLease ctx(s);  // one query context for both stages
    FuseCall c{d, legs, n_requests, fusion, rrf_k, leg_weights, fuse_stride(fetch, len), 0};
    for (uint32_t b = 0; b < n_requests; b++) c.max_legs = std::max(c.max_legs, legs[b]);
    ott_stats st;
    memset(&st, 0, sizeof(st));
    if ((rc = run_fuse(ctx.c, c, out, n_out, n_per_request, &st, stats != nullptr))) return rc;
    st.total_ns = now_ns() - t0;
    if (stats) *stats = st;
    return OTT_OK;
}

}  // extern "C"
