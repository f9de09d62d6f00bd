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
//
// ott_query_hybrid is the same second stage over two kinds of first stage on one context: the dense legs through
// query_on, the sparse legs through ott_sparse.hip's sweep, both kinds of list laid out as the one block the kernel reads (a
// request's dense legs, then its sparse legs) and uploaded in one copy.  The kernel normalises every leg under that leg's own take
// (FuseParams::leg_take_max: a byte per leg behind the weights; nullptr = the call's take, which is what ott_query_fuse passes).
// Host decisions: ott_hybrid_plan.h.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "ott_internal.h"
#include "ott_fuse_plan.h"
#include "ott_hybrid_plan.h"

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
    const uint8_t* leg_take_max;  // [nq] 1 = the leg's list is best first under take Max; nullptr = take_max for every leg (ott_query_fuse)
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
            const bool lmax = p.leg_take_max ? p.leg_take_max[first + l] != 0 : tmax;  // the leg's own take (ott_query_hybrid)
            uint32_t n = 0;
            for (uint32_t i = lane; i < p.stride; i += 64) n += list[i].index != ~0ull ? 1u : 0u;
#pragma unroll
            for (int h = 32; h > 0; h >>= 1) n += __shfl_xor(n, h);
            double worst = 0.0, span = 0.0;
            if (n != 0 && p.fusion == FUSE_MINMAX) {
                const double best = (double)list[0].score;
                worst = (double)list[n - 1].score;
                span = lmax ? __dsub_rn(best, worst) : __dsub_rn(worst, best);
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
                worst = lmax ? lo : hi;
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
                        const bool lmax = p.leg_take_max ? p.leg_take_max[first + l] != 0 : tmax;
                        nrm = __double2float_rn(__ddiv_rn(lmax ? __dsub_rn(s, worst) : __dsub_rn(worst, s), span));
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

// off_take: where the legs' take bytes lie in the scratch (ott_query_hybrid), 0 = every leg ranks under the call's take
int launch_fuse(ott_store* s, const FuseCall& c, const FuseLayout& L, size_t off_take = 0) {
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
    p.leg_take_max = off_take ? (const uint8_t*)(dm + off_take) : nullptr;
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

int fuse_second_stage(ott_store* s, const FuseCall& c, const FuseLayout& L, size_t off_take, bool events_pending, ott_hit* out, uint64_t* n_out,
                      uint64_t* n_per_request, ott_stats* st, bool timing, const char* who);

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
    return fuse_second_stage(s, c, L, 0, events_pending, out, n_out, n_per_request, st, timing, "ott_query_fuse");
}

// The second stage behind the upload: the kernel, the fused hits back, the one host wait.  c.legs: every request's legs.
int fuse_second_stage(ott_store* s, const FuseCall& c, const FuseLayout& L, size_t off_take, bool events_pending, ott_hit* out, uint64_t* n_out,
                      uint64_t* n_per_request, ott_stats* st, bool timing, const char* who) {
    int rc;
    const ott_query_desc* d = c.d;
    char* dm = (char*)s->d_fuse.p;
    if (timing) OTT_HIP(hipEventRecord(s->ev[0], s->stream));
    if ((rc = launch_fuse(s, c, L, off_take))) return rc;
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
        if (nb > fuse_request_cap(d->k, c.legs[b], c.stride)) return fail(OTT_ERR_HIP, std::string(who) + ": the kernel returned more hits than a request can have");
        if (nb) memcpy(out + total, hits + (size_t)b * L.kout, (size_t)nb * sizeof(ott_hit));
        if (n_per_request) n_per_request[b] = nb;
        total += nb;
    }
    if (n_out) *n_out = total;
    return OTT_OK;
}

int hybrid_fail(HybridRefusal r, uint64_t bad, uint64_t v) { return fail(hybrid_refusal_status(r), hybrid_refusal_text(r, bad, v)); }

// ott_query_hybrid's arguments past the checks
struct HybridCall {
    const ott_query_desc* d;  // the dense side; d->k = fused hits per request
    const uint32_t *dense_per, *sparse_per;
    const uint64_t* sq_indptr;
    const uint32_t* sq_idx;
    const float* sq_val;  // (already scaled where OTT_HYBRID_IDF is set)
    uint32_t n_sparse, sparse_cmp;
    float sparse_thr;
    uint32_t n_requests, fusion;
    float rrf_k;
    const float* weights;
    uint64_t stride;
};

// a stage's lists (`per[i]` hits of query i back to back in `cand`) into the blocks of the legs `leg_at` names
int hybrid_place(const ott_store* s, const HybridCall& h, char* blocks, const std::vector<ott_hit>& cand, const std::vector<uint64_t>& per, const uint32_t* leg_at) {
    size_t at = 0;
    for (size_t i = 0; i < per.size(); i++) {
        if (per[i] > h.stride) return fail(OTT_ERR_HIP, "ott_query_hybrid: a leg returned more hits than fetch");
        for (uint64_t j = 0; j < per[i]; j++)
            if (cand[at + j].index - s->base_offset >= s->n) return fail(OTT_ERR_HIP, "ott_query_hybrid: a leg returned a row outside the store");
        if (per[i]) memcpy(blocks + ((size_t)leg_at[i] * h.stride) * sizeof(ott_hit), &cand[at], (size_t)per[i] * sizeof(ott_hit));
        at += per[i];
    }
    return OTT_OK;
}

// The dense stage (query_on), the sparse stage (run_sparse_sweep) and the fuse kernel on one context the caller holds: the host route.
int run_hybrid(ott_store* s, const HybridCall& h, ott_hit* out, uint64_t* n_out, uint64_t* n_per_request, ott_stats* st, bool timing) {
    int rc;
    OTT_HIP(use_device(s));
    const ott_query_desc* d = h.d;
    const uint32_t nd = d->nq, ns = h.n_sparse, legs = nd + ns;
    std::vector<uint32_t> first(h.n_requests), total(h.n_requests), dense_at(nd), sparse_at(ns);
    const uint32_t max_legs = hybrid_leg_order(h.dense_per, h.sparse_per, h.n_requests, first.data(), total.data(), dense_at.data(), sparse_at.data());
    const HybridLayout L = hybrid_layout(legs, h.n_requests, h.stride, d->k, max_legs);
    if ((rc = s->d_fuse.ensure(L.f.total))) return rc;
    if ((rc = s->h_fuse.ensure(L.f.upload_bytes))) return rc;
    char* hs = (char*)s->h_fuse.p;  // (no stage touches h_fuse: the lists are placed as they arrive)
    memset(hs, 0xFF, L.f.block_bytes);
    ott_stats* st1 = timing ? st : nullptr;
    st->path_used = OTT_PATH_EXACT;  // (what a call without a dense stage reports)
    if (nd) {
        ott_query_desc d1 = *d;
        d1.k = h.stride;  // a dense leg's list: ott_query's hits with k = min(fetch, rows)
        std::vector<ott_hit> cand((size_t)nd * h.stride);
        std::vector<uint64_t> per(nd, 0);
        uint64_t n_cand = 0;
        if ((rc = query_on(s, &d1, cand.data(), nullptr, cand.size(), &n_cand, per.data(), nullptr, st1))) return rc;
        if ((rc = hybrid_place(s, h, hs, cand, per, dense_at.data()))) return rc;
    }
    if (ns) {
        ott_query_desc d2 = *d;  // the same chunk mask, row mask or evaluated mask; the live mask is the store's
        d2.queries = nullptr;
        d2.nq = ns;
        d2.metric = OTT_METRIC_DOT;
        d2.take = OTT_TAKE_MAX;
        d2.filter_cmp = h.sparse_cmp;
        d2.filter_thr = h.sparse_thr;
        d2.mode = OTT_MODE_PER_QUERY;
        d2.path = OTT_PATH_EXACT;
        RunPlan rp;
        make_run_plan(s, d->chunk_mask, rp);
        const uint64_t k_eff = h.stride < rp.rows_scored ? h.stride : rp.rows_scored;  // a list never outgrows the pool
        d2.k = k_eff;
        if (k_eff) {
            std::vector<ott_hit> cand((size_t)ns * k_eff);
            std::vector<uint64_t> per(ns, 0);
            uint64_t n_cand = 0;
            ott_stats st2;
            memset(&st2, 0, sizeof(st2));
            rc = run_sparse_sweep(s, &d2, h.sq_indptr, h.sq_idx, h.sq_val, k_eff, cand.data(), &n_cand, per.data(), timing ? &st2 : nullptr);
            if (rc) {
                (void)hipStreamSynchronize(s->stream);  // nothing of this call is in flight when the context is given back
                return rc;
            }
            if ((rc = hybrid_place(s, h, hs, cand, per, sparse_at.data()))) return rc;
            if (timing) {  // the sums of both stages
                st->passes += st2.passes;
                st->bytes_scanned += st2.bytes_scanned;
                st->vectors_compared += st2.vectors_compared;
                st->score_ns += st2.score_ns;
                st->merge_ns += st2.merge_ns;
                if (!nd) {
                    st->total_chunks = st2.total_chunks;
                    st->evaluated_chunks = st2.evaluated_chunks;
                    st->pruned_chunks = st2.pruned_chunks;
                }
            }
        }
    }
    // the one upload: [blocks | first | legs | weights | take]
    memcpy(hs + L.f.off_first, first.data(), (size_t)h.n_requests * 4);
    memcpy(hs + L.f.off_legs, total.data(), (size_t)h.n_requests * 4);
    float* w = (float*)(hs + L.f.off_weights);
    for (uint32_t l = 0; l < legs; l++) w[l] = h.weights ? h.weights[l] : 1.0f;
    uint8_t* tk = (uint8_t*)(hs + L.off_take);
    memset(tk, 0, L.f.upload_bytes - L.off_take);
    for (uint32_t i = 0; i < nd; i++) tk[dense_at[i]] = d->take == OTT_TAKE_MAX;  // a dense leg is best first under d->take
    for (uint32_t j = 0; j < ns; j++) tk[sparse_at[j]] = 1;                       // a sparse leg under take Max
    OTT_HIP(hipMemcpyAsync((char*)s->d_fuse.p, hs, L.f.upload_bytes, hipMemcpyHostToDevice, s->stream));
    const FuseCall c{d, total.data(), h.n_requests, h.fusion, h.rrf_k, h.weights, h.stride, max_legs};
    return fuse_second_stage(s, c, L.f, L.off_take, false, out, n_out, n_per_request, st, timing, "ott_query_hybrid");
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

int ott_query_hybrid(ott_store* s, const ott_query_desc* d, const void* dense_per_request, const uint64_t* sq_indptr, const void* sq_indices, const float* sq_values,
                     uint32_t n_sparse, const void* sparse_per_request, uint32_t sparse_cmp, float sparse_thr, uint32_t sparse_flags, uint32_t n_requests,
                     uint32_t fusion, float rrf_k, const float* leg_weights, uint64_t fetch, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_request,
                     ott_stats* stats) {
    if (!d) return fail(OTT_ERR_INVALID, "ott_query_hybrid: desc is NULL");
    const uint32_t* dense_per = (const uint32_t*)dense_per_request;
    const uint32_t* sparse_per = (const uint32_t*)sparse_per_request;
    const uint32_t* sq_idx = (const uint32_t*)sq_indices;
    uint64_t bad = 0, v = 0;
    HybridRefusal why = hybrid_check_args(d->mode == OTT_MODE_PER_QUERY, dense_per, sparse_per, n_requests, d->nq, n_sparse, fetch, fusion, rrf_k, leg_weights, d->k,
                                          sparse_cmp, OTT_CMP_EQ, sparse_flags, sq_indptr, sq_idx, sq_values, &bad, &v);  // before the store is looked at
    if (why != HYBRID_OK) return hybrid_fail(why, bad, v);
    int rc;
    if (d->nq) {
        if ((rc = validate_query(s, d))) return rc;  // what ott_query refuses
    } else {  // no dense leg: d->queries is not read
        if (!s) return fail(OTT_ERR_INVALID, "ott_query_hybrid: store is NULL");
        if ((rc = check_desc_enums("ott_query_hybrid", d))) return rc;
        if ((rc = check_device_row_mask("ott_query_hybrid", s, d))) return rc;
    }
    if (s->multi) return hybrid_fail(HYBRID_MULTI_GPU, 0, 0);  // (the front of a multi-GPU store holds no rows)
    const uint64_t len = ott_store_len(s);
    const auto zero_outputs = [&] {
        if (n_out) *n_out = 0;
        if (n_per_request)
            for (uint32_t b = 0; b < n_requests; b++) n_per_request[b] = 0;
        if (stats) memset(stats, 0, sizeof(*stats));
    };
    const uint64_t t0 = now_ns();
    if (len == 0) {  // an empty store: a valid call with no hits
        if (!out && cap) return hybrid_fail(HYBRID_NULL_OUT, 0, 0);
        zero_outputs();
        return OTT_OK;
    }

    ott::host::SharedLock rd;  // the corpus, the sparse rows and the live mask cannot change between the stages
    if ((rc = lock_store_shared(s, rd))) return rc;
    if ((why = hybrid_check_store(false, len, s->opt.tie_order)) != HYBRID_OK) return hybrid_fail(why, 0, 0);
    if (n_sparse) {  // ott_query_sparse's own checks, under this entry point's name
        uint64_t a = 0, b = 0;
        SparseRefusal r = sparse_check_store(false, s->d_sparse != nullptr, s->sparse_n, s->n, s->opt.tie_order, &a, &b);
        if (r == SPARSE_OK) r = sparse_check_query(n_sparse, sq_indptr, sq_idx, sq_values, s->sparse_vocab, &a, &b);
        if (r != SPARSE_OK) return hybrid_fail(hybrid_from_sparse(r), a, b);
    }
    const uint64_t stride = fuse_stride(fetch, len);
    uint64_t need = 0;
    for (uint32_t b = 0; b < n_requests; b++) need += fuse_request_cap(d->k, (dense_per ? dense_per[b] : 0) + (sparse_per ? sparse_per[b] : 0), stride);
    if (cap < need) return hybrid_fail(HYBRID_CAP, 0, 0);
    if (!out && cap) return hybrid_fail(HYBRID_NULL_OUT, 0, 0);

    CtxLease ctx(s);  // one query context for every stage
    std::vector<float> scaled;
    if ((sparse_flags & HYBRID_IDF) && n_sparse && sq_indptr[n_sparse] != 0) {
        // the query weights times idf on the host (the document frequencies are built where they are stale)
        if ((rc = sparse_df_ensure(ctx.c))) return rc;
        scaled.resize(sq_indptr[n_sparse]);
        sparse_idf_scale(s, sq_idx, sq_values, sq_indptr[n_sparse], scaled.data());
        uint64_t a = 0, b = 0;
        const SparseRefusal r = sparse_check_query(n_sparse, sq_indptr, sq_idx, scaled.data(), s->sparse_vocab, &a, &b);
        if (r != SPARSE_OK) return hybrid_fail(hybrid_from_sparse(r), a, b);
        sq_values = scaled.data();
    }
    zero_outputs();
    const HybridCall h{d, dense_per, sparse_per, sq_indptr, sq_idx, sq_values, n_sparse, sparse_cmp, sparse_thr, n_requests, fusion, rrf_k, leg_weights, stride};
    ott_stats st;
    memset(&st, 0, sizeof(st));
    if ((rc = run_hybrid(ctx.c, h, out, n_out, n_per_request, &st, stats != nullptr))) return rc;
    st.total_ns = now_ns() - t0;
    if (stats) *stats = st;
    return OTT_OK;
}

}  // extern "C"
