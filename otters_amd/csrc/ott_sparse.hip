// ott_sparse.hip — sparse rows and the exact sparse dot search.  Row r of a store may carry a sparse row beside its
// dense one (ott_store_set_sparse, attached like group ids); ott_query_sparse ranks the rows that share an index with a sparse query
// by S = the sum, in the ROW's index order, of fl(value x weight) over the shared indices, one rounded f32 operation at a time
// (ott_sparse_plan.h states the score and the overlap rule for the host; tests/sparse_ref.py is the numpy model).  Row ids, chunk
// masks, row masks, the evaluated mask and deleted rows mean what they mean for a dense query.
//
// Device layout: sliced ELL, 64 rows per slice (ott_sparse_plan.h: SparseLayout), built on the host slice batch by slice batch and
// uploaded as it is — the CSR never reaches HBM.  Lane = row: entry p of the 64 rows of a slice lies in 64 consecutive words, so a
// wave's loads coalesce while every lane adds its own row's products serially.
//
//   sparse_lds_kernel     LDS form (vocab <= 32768): one query per pass.  A workgroup of 16 waves, one per CU, first builds the query's
//                         dense f32 table and presence bitmap in LDS (up to 132 KiB), then its waves walk slices: a persistent grid.
//   sparse_table_kernel   table form (any vocab): four queries per pass.  The weights come from a device table [vocab] float4 — one
//                         16-byte gather serves four queries — with a presence nibble per index beside it; sparse_scatter_kernel
//                         fills the entries of the pass's queries in front of the sweep, sparse_clear_kernel zeroes exactly those
//                         behind it, so the table is zero whenever a query finds it (ensure_zeroed's protocol, context scratch).
//   both                  sparse_walk: per slice the composed row mask and the chunk runs decide each lane's row; a slice with no
//                         surviving row is not read.  A lane keeps U entries in registers while the next U are in flight, looks
//                         every weight up (no branch on membership: a weight outside the query is +0.0 and leaves S's bits alone),
//                         tracks the overlap apart, and writes ord(S) << 32 | ~row to table[q][row] for a candidate that passes the
//                         NaN drop and the filter: a (query, row) pair has one writer, a plain store.  The table is d_gtable.
//   GroupTopK             grouped search's top-k with one "group" per row: pass() after every sweep, finish() once — one host wait.
//
//   sparse_df_kernel      document frequencies: one pass over the index array alone, the same geometry, integer adds into
//                         a histogram in LDS (vocab <= 32768) or straight into HBM; cached per store, rebuilt by whoever needs the
//                         counts first after the sparse rows or the live mask changed (sparse_df_ensure).  IDF query weights are
//                         made from them on the host (ott_query_sparse_idf), and the scaled query runs through the unchanged sweep.
//
// Dense and sparse legs fused per request: ott_query_hybrid (ott_fuse.hip), which calls run_sparse_sweep.
// Out of scope: BM25's term-frequency saturation and length normalisation (the caller stores those values), vocabularies above 2^20
// or hashed 32-bit token ids (the caller remaps), multi-GPU stores, reordering rows to cut padding, compaction with sparse rows
// resident.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_exact_dev.h"

namespace ott {

static_assert(SPARSE_MAX_VOCAB == OTT_SPARSE_MAX_VOCAB && SPARSE_MAX_QUERIES == OTT_SPARSE_MAX_QUERIES, "ott_sparse_plan.h restates the header's constants");

constexpr int SP_U = 8;            // entries a lane holds while the next SP_U are in flight
constexpr int SP_LDS_WAVES = 16;   // LDS form: one workgroup of 1024 threads per CU (its LDS leaves room for one), 16 x 2 x SP_U loads in flight
constexpr int SP_TAB_WAVES = 4;    // table form: workgroups of 256 threads
constexpr int SP_TAB_BLOCKS_PER_CU = 8;

struct SparseParams {
    const uint32_t* idx;   // [padded]
    const float* val;      // [padded]
    const uint64_t* base;  // [n_slices + 1]
    const uint32_t* len;   // [n_slices * 64]
    const uint64_t* row_mask;
    uint64_t row_mask_bits;
    const ott_run* runs;  // the surviving chunk runs, ascending
    uint32_t n_runs;
    uint32_t n_slices;
    uint64_t n_rows;
    unsigned long long* table;  // [queries of the pass][n_rows] candidate key per (query, row); 0 = empty
    const uint64_t* q_indptr;   // the call's queries as CSR, on the device
    const uint32_t* q_idx;
    const float* q_val;
    const float4* wtab;     // table form: [vocab] the four weights of the pass's queries
    const uint32_t* wpres;  // ... and a presence nibble per index, eight to a word
    uint32_t q0, nq_here;
    uint32_t vocab_pad;
    uint32_t take_max, cmp;
    float thr;
};

// whether `row` lies in a surviving chunk run (binary search; one run is the common case)
__device__ __forceinline__ bool sparse_row_in_runs(const ott_run* runs, uint32_t n_runs, uint64_t row) {
    uint32_t lo = 0, hi = n_runs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (runs[mid].start <= row) lo = mid;
        else hi = mid;
    }
    const uint64_t start = runs[lo].start;
    return row >= start && row - start < runs[lo].count;
}

// The slices of wave gw of nw.  look(index, value, S, hit): S[q] = fl(S[q] + fl(value x weight_q(index))), hit |= the presence bits.
template <int NQ, class Lookup>
__device__ __forceinline__ void sparse_walk(const SparseParams& p, uint32_t gw, uint32_t nw, Lookup&& look) {
    const uint32_t lane = threadIdx.x & 63;
    const bool take_max = p.take_max != 0;
    for (uint32_t t = gw; t < p.n_slices; t += nw) {
        const uint64_t row = (uint64_t)t * 64 + lane;
        bool valid = row < p.n_rows && sparse_row_in_runs(p.runs, p.n_runs, row);
        if (p.row_mask != nullptr && valid && row < p.row_mask_bits) valid = (p.row_mask[row >> 6] >> (row & 63)) & 1;  // src/vec.rs:231-237
        if (__ballot(valid) == 0) continue;  // no surviving row: the slice is not read
        const uint32_t len = valid ? p.len[row] : 0u;  // (a lane without a row loads nothing: every load below is guarded by len)
        const uint64_t at = p.base[t] + lane;          // entry e of this lane's row: at + 64 e, below base[t + 1] while e < len <= L_t
        const uint32_t* ip = p.idx + at;
        const float* vp = p.val + at;
        float S[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) S[q] = 0.0f;
        uint32_t hit = 0;
        uint32_t ci[SP_U];
        float cv[SP_U];
#pragma unroll
        for (int u = 0; u < SP_U; u++) {
            const bool ok = (uint32_t)u < len;
            ci[u] = ok ? __builtin_nontemporal_load(ip + (uint64_t)u * 64) : 0u;  // streamed once per pass
            cv[u] = ok ? __builtin_nontemporal_load(vp + (uint64_t)u * 64) : 0.0f;
        }
        for (uint32_t e0 = 0; e0 < len; e0 += SP_U) {
            uint32_t ni[SP_U];
            float nv[SP_U];
#pragma unroll
            for (int u = 0; u < SP_U; u++) {  // the next entries are in flight while these are consumed
                const uint32_t e = e0 + SP_U + u;
                const bool ok = e < len;
                ni[u] = ok ? __builtin_nontemporal_load(ip + (uint64_t)e * 64) : 0u;
                nv[u] = ok ? __builtin_nontemporal_load(vp + (uint64_t)e * 64) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < SP_U; u++)  // in the row's index order
                if (e0 + u < len) look(ci[u], cv[u], S, hit);
#pragma unroll
            for (int u = 0; u < SP_U; u++) {
                ci[u] = ni[u];
                cv[u] = nv[u];
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float s = S[q];
            // a candidate shares an index with the query, whatever the values are; NaN dropped (vec_compute.rs:237); the filter acts on S
            if ((uint32_t)q < p.nq_here && ((hit >> q) & 1) && !(s != s) && cmp_holds(s, p.cmp, p.thr))
                p.table[(size_t)q * p.n_rows + row] = ((unsigned long long)ord_of(s, take_max) << 32) | (uint32_t)(~(uint32_t)row);
        }
    }
}

__global__ __launch_bounds__(64 * SP_LDS_WAVES) void sparse_lds_kernel(SparseParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sp_lds[];
    float* w = (float*)sp_lds;                 // [vocab_pad] the query's weights, +0.0 outside it
    uint32_t* pres = sp_lds + p.vocab_pad;     // [vocab_pad / 32] bit i: index i is one of the query's
    const uint32_t words = p.vocab_pad + p.vocab_pad / 32;
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) sp_lds[i] = 0u;
    __syncthreads();
    const uint64_t e0 = p.q_indptr[p.q0], e1 = p.q_indptr[p.q0 + 1];
    for (uint64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {  // indices are distinct and below vocab (checked on the host)
        const uint32_t i = p.q_idx[e];
        w[i] = p.q_val[e];
        atomicOr(&pres[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    sparse_walk<1>(p, blockIdx.x * SP_LDS_WAVES + wave, gridDim.x * SP_LDS_WAVES, [&](uint32_t i, float v, float (&S)[1], uint32_t& hit) {
        S[0] = __fadd_rn(S[0], __fmul_rn(v, w[i]));
        hit |= (pres[i >> 5] >> (i & 31)) & 1u;
    });
}

__global__ __launch_bounds__(64 * SP_TAB_WAVES) void sparse_table_kernel(SparseParams p) {
    const uint32_t wave = threadIdx.x >> 6;
    const float4* __restrict__ wtab = p.wtab;
    const uint32_t* __restrict__ wpres = p.wpres;
    sparse_walk<(int)SPARSE_TABLE_NQ>(p, blockIdx.x * SP_TAB_WAVES + wave, gridDim.x * SP_TAB_WAVES,
                                      [&](uint32_t i, float v, float (&S)[SPARSE_TABLE_NQ], uint32_t& hit) {
                                          const float4 t = wtab[i];
                                          S[0] = __fadd_rn(S[0], __fmul_rn(v, t.x));
                                          S[1] = __fadd_rn(S[1], __fmul_rn(v, t.y));
                                          S[2] = __fadd_rn(S[2], __fmul_rn(v, t.z));
                                          S[3] = __fadd_rn(S[3], __fmul_rn(v, t.w));
                                          hit |= (wpres[i >> 3] >> ((i & 7) * 4)) & 15u;
                                      });
}

// The entries [e_first, e_end) of the pass's queries q0 .. q0 + nq_here - 1 into the table (FILL) or out of it again (!FILL):
// afterwards exactly the words a query of the pass touched are zero again.
template <bool FILL>
__global__ __launch_bounds__(256) void sparse_scatter_kernel(const uint64_t* __restrict__ q_indptr, const uint32_t* __restrict__ q_idx, const float* __restrict__ q_val,
                                                             uint32_t q0, uint32_t nq_here, uint64_t e_first, uint64_t e_end, float* wtab, uint32_t* wpres) {
    const uint64_t e = e_first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= e_end) return;
    uint32_t q = 0;
    while (q + 1 < nq_here && q_indptr[q0 + q + 1] <= e) q++;
    const uint32_t i = q_idx[e];
    if (FILL) {
        wtab[(size_t)i * 4 + q] = q_val[e];
        atomicOr(&wpres[i >> 3], 1u << ((i & 7) * 4 + q));
    } else {
        wtab[(size_t)i * 4 + q] = 0.0f;
        wpres[i >> 3] = 0u;  // (every writer of the word writes 0)
    }
}

// Document frequencies: one pass over the index array with sparse_walk's geometry — wave per slice, lane = row, the
// entry loads guarded by the row's length, a slice without a live row not read.  df[i] += 1 for every stored index i of a live row:
// integer adds, so the words do not depend on the order of arrival.  LDS: the workgroup counts in a histogram of its own
// ([vocab_pad] words of dynamic LDS) and adds every non-zero bin to df once at the end; otherwise every entry is a global atomic.
struct SparseDfParams {
    const uint32_t* idx;   // [padded]
    const uint64_t* base;  // [n_slices + 1]
    const uint32_t* len;   // [n_slices * 64]
    const uint64_t* live;  // the live mask, word t = the rows of slice t; nullptr = every row is live
    uint32_t n_slices;
    uint64_t n_rows;
    uint32_t* df;          // [vocab], zero when the kernel starts
    uint32_t vocab, vocab_pad;
};

constexpr int SP_DF_WAVES = 16;
constexpr int SP_DF_U = 8;  // index loads a lane has in flight

template <bool LDS>
__global__ __launch_bounds__(64 * SP_DF_WAVES) void sparse_df_kernel(SparseDfParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t df_lds[];
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < p.vocab_pad; i += blockDim.x) df_lds[i] = 0u;
        __syncthreads();
    }
    uint32_t* bins = LDS ? df_lds : p.df;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nw = gridDim.x * SP_DF_WAVES;
    for (uint32_t t = blockIdx.x * SP_DF_WAVES + wave; t < p.n_slices; t += nw) {
        const uint64_t row = (uint64_t)t * 64 + lane;
        bool valid = row < p.n_rows;
        if (p.live != nullptr && valid) valid = (p.live[t] >> lane) & 1;  // (word t exists: t < ceil(n_rows / 64) <= the mask's words)
        if (__ballot(valid) == 0) continue;  // no live row: the slice is not read
        const uint32_t len = valid ? p.len[row] : 0u;
        const uint32_t* ip = p.idx + p.base[t] + lane;  // entry e of this lane's row: + 64 e, below base[t + 1] while e < len <= L_t
        for (uint32_t e0 = 0; e0 < len; e0 += SP_DF_U) {
            uint32_t ci[SP_DF_U];
#pragma unroll
            for (int u = 0; u < SP_DF_U; u++) ci[u] = e0 + u < len ? __builtin_nontemporal_load(ip + (uint64_t)(e0 + u) * 64) : 0u;
#pragma unroll
            for (int u = 0; u < SP_DF_U; u++)
                if (e0 + u < len && ci[u] < p.vocab) atomicAdd(&bins[ci[u]], 1u);  // (every stored index is below vocab: set_sparse checked it)
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < p.vocab; i += blockDim.x) {
            const uint32_t c = df_lds[i];
            if (c) atomicAdd(&p.df[i], c);
        }
    }
}

void sparse_drop(ott_store* s) {
    if (s->d_df) (void)hipFree(s->d_df);
    s->d_df = nullptr;
    s->df_host.clear();
    s->df_host.shrink_to_fit();
    s->df_gen = 0;
    s->df_ndocs = 0;
    sparse_df_stale(s);
    if (s->d_sparse) (void)hipFree(s->d_sparse);
    s->d_sparse = nullptr;
    s->sparse_n = 0;
    s->sparse_nnz = 0;
    s->sparse_vocab = 0;
    s->sparse_lay = SparseLayout{};
    s->sparse_base.clear();
    s->sparse_base.shrink_to_fit();
}

namespace {

int refuse(SparseRefusal r, uint64_t a, uint64_t b) { return fail(sparse_refusal_status(r), sparse_refusal_text(r, a, b)); }

constexpr uint64_t SP_BATCH_ENTRIES = 8ull << 20;  // host staging of the layout's entries: 32 MiB of indices and of values at a time

// The layout of `n` rows from the caller's CSR into a fresh allocation; the caller holds the store exclusively, on its device.
int sparse_build(ott_store* s, const uint64_t* indptr, const uint32_t* indices, const float* values, uint64_t n, uint32_t vocab) {
    std::vector<uint64_t> base(sparse_slices(n) + 1);
    const uint64_t padded = sparse_slice_bases(indptr, n, base.data());
    const SparseLayout lay = sparse_layout(n, padded);
    char* d = nullptr;
    OTT_HIP(hipMalloc((void**)&d, (size_t)lay.bytes));
    const auto bail = [&](hipError_t e) {
        (void)hipFree(d);
        return fail(e == hipErrorOutOfMemory ? OTT_ERR_OOM : OTT_ERR_HIP, std::string("ott_store_set_sparse: ") + hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMemcpy(d + lay.off_bases, base.data(), base.size() * 8, hipMemcpyHostToDevice)) != hipSuccess) return bail(e);
    if (lay.n_slices) {
        std::vector<uint32_t> len(lay.n_slices * SPARSE_SLICE, 0u);  // rows past n in the last slice have no entries
        for (uint64_t r = 0; r < n; r++) len[r] = (uint32_t)(indptr[r + 1] - indptr[r]);  // (an entry count is below vocab <= 2^20)
        if ((e = hipMemcpy(d + lay.off_lengths, len.data(), len.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return bail(e);
    }
    std::vector<uint32_t> bi;
    std::vector<float> bv;
    for (uint64_t t0 = 0; t0 < lay.n_slices;) {  // slices [t0, t1): as many as fit the staging (at least one)
        uint64_t t1 = t0 + 1;
        while (t1 < lay.n_slices && base[t1 + 1] - base[t0] <= SP_BATCH_ENTRIES) t1++;
        const uint64_t cnt = base[t1] - base[t0];
        if (cnt) {
            bi.assign(cnt, 0u);  // the padding: index 0, value +0.0 (never consumed: a lane stops at its row's length)
            bv.assign(cnt, 0.0f);
            const uint64_t r1 = t1 * SPARSE_SLICE < n ? t1 * SPARSE_SLICE : n;
            for (uint64_t r = t0 * SPARSE_SLICE; r < r1; r++) {
                const uint64_t b = base[r / SPARSE_SLICE] - base[t0];
                for (uint64_t j = indptr[r], p = 0; j < indptr[r + 1]; j++, p++) {
                    const uint64_t at = sparse_entry_offset(b, p, r);
                    bi[at] = indices[j];
                    bv[at] = values[j];
                }
            }
            if ((e = hipMemcpy(d + base[t0] * 4, bi.data(), cnt * 4, hipMemcpyHostToDevice)) != hipSuccess) return bail(e);
            if ((e = hipMemcpy(d + lay.off_values + base[t0] * 4, bv.data(), cnt * 4, hipMemcpyHostToDevice)) != hipSuccess) return bail(e);
        }
        t0 = t1;
    }
    s->d_sparse = d;
    s->sparse_n = n;
    s->sparse_nnz = indptr[n];
    s->sparse_vocab = vocab;
    s->sparse_lay = lay;
    s->sparse_base.swap(base);
    return OTT_OK;
}

// the layout bytes of the slices the chunk runs touch (a slice two runs share counts once)
uint64_t sparse_run_bytes(const ott_store* own, const RunPlan& pl) {
    uint64_t bytes = 0, done = 0;  // slices below `done` are counted
    for (const ott_run& r : pl.runs) {
        uint64_t t0 = r.start / SPARSE_SLICE;
        const uint64_t t1 = (r.start + r.count + SPARSE_SLICE - 1) / SPARSE_SLICE;
        if (t0 < done) t0 = done;
        if (t1 > t0) bytes += sparse_slice_bytes(own->sparse_base.data(), t0, t1);
        if (t1 > done) done = t1;
    }
    return bytes;
}

int launch_sparse_lds(ott_store* s, const SparseParams& p, uint32_t vocab) {
    const size_t smem = sparse_lds_bytes(vocab);
    if (smem > 48 * 1024) {  // more dynamic LDS than the default limit: the opt-in, once per device
        static std::atomic<uint64_t> attr_set{0};
        if (attr_needed(attr_set, s->device)) {
            OTT_HIP(hipFuncSetAttribute((const void*)sparse_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sparse_lds_bytes(SPARSE_LDS_MAX_VOCAB)));
            attr_done(attr_set, s->device);
        }
    }
    const uint32_t grid = grid_blocks(p.n_slices, SP_LDS_WAVES, s->n_cu, 1);
    hipLaunchKernelGGL(sparse_lds_kernel, dim3(grid), dim3(64 * SP_LDS_WAVES), smem, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

}  // namespace

// The sparse sweep on a context whose `mu` the caller holds (and the owner's `rw`, shared).  k_eff = min(k, rows the chunk mask
// leaves) >= 1.  The layout is the owner's; the queries were checked against its vocab.
int run_sparse_sweep(ott_store* s, const ott_query_desc* d, const uint64_t* q_indptr, const uint32_t* q_idx, const float* q_val, uint64_t k_eff, ott_hit* out,
                     uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const ott_store* own = s->owner ? s->owner : s;
    const uint32_t nq = d->nq, vocab = s->sparse_vocab;
    const uint64_t n = s->n;
    const uint64_t t0 = now_ns();
    ott_stats st;
    RunPlan pl;
    SparseParams p{};
    uint64_t total = 0;
    // (the descriptor's own mask — caller's or evaluated, live mask — is composed here)
    if ((rc = sweep_plan(s, d, nq, &st, &pl, &p.row_mask, &p.row_mask_bits))) return rc;
    if (pl.rows_scored != 0) {
        const SparseLayout& lay = s->sparse_lay;
        const bool table_form = sparse_take_table(s->opt.sparse_table, vocab, nq);
        const uint32_t passes = sparse_passes(table_form, nq);
        const uint32_t tile = table_form ? std::min(nq, SPARSE_TABLE_NQ) : 1u;
        // one block, one copy: [runs | q_indptr | q_idx | q_val]
        const uint64_t q_nnz = q_indptr[nq];
        const size_t off_ptr = pl.runs.size() * sizeof(ott_run), off_idx = off_ptr + ((size_t)nq + 1) * 8, off_val = off_idx + (size_t)q_nnz * 4;
        const size_t block = off_val + (size_t)q_nnz * 4;
        if ((rc = s->h_spq.ensure(block))) return rc;
        char* hs = (char*)s->h_spq.p;
        memcpy(hs, pl.runs.data(), off_ptr);
        memcpy(hs + off_ptr, q_indptr, ((size_t)nq + 1) * 8);
        if (q_nnz) {
            memcpy(hs + off_idx, q_idx, (size_t)q_nnz * 4);
            memcpy(hs + off_val, q_val, (size_t)q_nnz * 4);
        }
        if ((rc = s->d_spq.ensure(block))) return rc;
        OTT_HIP(hipMemcpyAsync(s->d_spq.p, hs, block, hipMemcpyHostToDevice, s->stream));
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)tile * n * 8))) return rc;
        if (table_form && (rc = ensure_zeroed(s, s->d_sptable, s->sptable_clean, sparse_table_bytes(vocab)))) return rc;

        p.idx = (const uint32_t*)s->d_sparse;
        p.val = (const float*)(s->d_sparse + lay.off_values);
        p.base = (const uint64_t*)(s->d_sparse + lay.off_bases);
        p.len = (const uint32_t*)(s->d_sparse + lay.off_lengths);
        p.runs = (const ott_run*)s->d_spq.p;
        p.n_runs = (uint32_t)pl.runs.size();
        p.n_slices = (uint32_t)lay.n_slices;  // (n < 2^32 - 16: sparse_check_store)
        p.n_rows = n;
        p.table = (unsigned long long*)s->d_gtable.p;
        p.q_indptr = (const uint64_t*)((const char*)s->d_spq.p + off_ptr);
        p.q_idx = (const uint32_t*)((const char*)s->d_spq.p + off_idx);
        p.q_val = (const float*)((const char*)s->d_spq.p + off_val);
        float* wtab = (float*)s->d_sptable.p;
        uint32_t* wpres = table_form ? (uint32_t*)((char*)s->d_sptable.p + (size_t)vocab * 16) : nullptr;
        p.wtab = (const float4*)wtab;
        p.wpres = wpres;
        p.vocab_pad = sparse_vocab_pad(vocab);
        p.take_max = d->take == OTT_TAKE_MAX;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;

        GroupTopK tk;
        tk.n_groups = (uint32_t)n;
        tk.nq = nq;
        tk.k = k_eff;
        tk.take_max = p.take_max != 0;
        if (table_form) tk.also_clean = &s->sptable_clean;  // behind the one wait every pass's clear kernel has run
        if ((rc = tk.prepare(s, nullptr))) return rc;
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        for (uint32_t ps = 0; ps < passes; ps++) {
            p.q0 = ps * tile;
            p.nq_here = (nq - p.q0) < tile ? (nq - p.q0) : tile;
            const uint64_t e_first = q_indptr[p.q0], e_end = q_indptr[p.q0 + p.nq_here];
            if (e_end > e_first) {  // (a pass of empty queries has no candidate: nothing to sweep)
                if (table_form) {
                    const uint32_t sblocks = (uint32_t)((e_end - e_first + 255) / 256);
                    hipLaunchKernelGGL(sparse_scatter_kernel<true>, dim3(sblocks), dim3(256), 0, s->stream, p.q_indptr, p.q_idx, p.q_val, p.q0, p.nq_here, e_first, e_end,
                                       wtab, wpres);
                    OTT_HIP(hipGetLastError());
                    const uint32_t grid = grid_blocks(p.n_slices, SP_TAB_WAVES, s->n_cu, SP_TAB_BLOCKS_PER_CU);
                    hipLaunchKernelGGL(sparse_table_kernel, dim3(grid), dim3(64 * SP_TAB_WAVES), 0, s->stream, p);
                    OTT_HIP(hipGetLastError());
                    hipLaunchKernelGGL(sparse_scatter_kernel<false>, dim3(sblocks), dim3(256), 0, s->stream, p.q_indptr, p.q_idx, p.q_val, p.q0, p.nq_here, e_first, e_end,
                                       wtab, wpres);
                    OTT_HIP(hipGetLastError());
                } else if ((rc = launch_sparse_lds(s, p, vocab))) {
                    return rc;
                }
            }
            if ((rc = tk.pass(s, p.table, p.q0, p.nq_here))) return rc;
        }
        if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
        std::vector<uint64_t> per(nq, 0);
        if ((rc = tk.finish(s, timing, out, &total, per.data()))) return rc;
        if (timing) read_exact_events(s, &st);
        uint64_t at = 0;
        for (uint32_t b = 0; b < nq; b++) {  // hit.query = b
            for (uint64_t i = 0; i < per[b]; i++) out[at + i].query = b;
            at += per[b];
            if (n_per_query) n_per_query[b] = per[b];
        }
        st.passes = passes;
        st.bytes_scanned = sparse_bytes_scanned(passes, sparse_run_bytes(own, pl));
    }
    if (n_out) *n_out = total;
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

// The owner's document frequencies are those of the sparse rows and the live mask as they are now.  The caller holds the owner's
// `rw` shared (sparse_gen cannot move) and ctx's `mu`; the build runs on ctx's stream under the owner's df_mu and is waited for,
// so whoever finds df_gen == sparse_gen afterwards reads finished words.
int sparse_df_ensure(ott_store* ctx) {
    ott_store* own = ctx->owner ? ctx->owner : ctx;
    std::lock_guard<std::mutex> g(own->df_mu);
    if (own->df_gen == own->sparse_gen) return OTT_OK;
    OTT_HIP(use_device(ctx));
    const uint32_t vocab = own->sparse_vocab;
    const SparseLayout& lay = own->sparse_lay;
    if (!own->d_df) OTT_HIP(hipMalloc((void**)&own->d_df, (size_t)vocab * 4));
    OTT_HIP(hipMemsetAsync(own->d_df, 0, (size_t)vocab * 4, ctx->stream));
    if (lay.n_slices && lay.padded_entries) {
        SparseDfParams p{};
        p.idx = (const uint32_t*)own->d_sparse;
        p.base = (const uint64_t*)(own->d_sparse + lay.off_bases);
        p.len = (const uint32_t*)(own->d_sparse + lay.off_lengths);
        p.live = own->d_live;
        p.n_slices = (uint32_t)lay.n_slices;
        p.n_rows = own->sparse_n;
        p.df = own->d_df;
        p.vocab = vocab;
        p.vocab_pad = sparse_vocab_pad(vocab);
        if (sparse_df_take_lds(own->opt.sparse_df_lds, vocab)) {
            const size_t smem = sparse_df_lds_bytes(vocab);
            if (smem > 48 * 1024) {  // more dynamic LDS than the default limit: the opt-in, once per device
                static std::atomic<uint64_t> attr_set{0};
                if (attr_needed(attr_set, ctx->device)) {
                    OTT_HIP(hipFuncSetAttribute((const void*)sparse_df_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)sparse_df_lds_bytes(SPARSE_LDS_MAX_VOCAB)));
                    attr_done(attr_set, ctx->device);
                }
            }
            const uint32_t grid = grid_blocks(p.n_slices, SP_DF_WAVES, ctx->n_cu, 1);
            hipLaunchKernelGGL(sparse_df_kernel<true>, dim3(grid), dim3(64 * SP_DF_WAVES), smem, ctx->stream, p);
        } else {
            const uint32_t grid = grid_blocks(p.n_slices, SP_DF_WAVES, ctx->n_cu, 2);
            hipLaunchKernelGGL(sparse_df_kernel<false>, dim3(grid), dim3(64 * SP_DF_WAVES), 0, ctx->stream, p);
        }
        OTT_HIP(hipGetLastError());
    }
    own->df_host.assign(vocab, 0u);
    OTT_HIP(hipMemcpyAsync(own->df_host.data(), own->d_df, (size_t)vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
    OTT_HIP(hipStreamSynchronize(ctx->stream));
    own->df_ndocs = own->sparse_n - own->n_dead;
    own->df_gen = own->sparse_gen;
    own->df_builds.fetch_add(1, std::memory_order_relaxed);
    return OTT_OK;
}

void sparse_idf_scale(const ott_store* own, const uint32_t* q_idx, const float* q_val, uint64_t q_nnz, float* out) {
    for (uint64_t e = 0; e < q_nnz; e++) out[e] = sparse_idf_weight(q_val[e], sparse_idf(own->df_ndocs, own->df_host[q_idx[e]]));
}

}  // namespace ott

using namespace ott;

extern "C" {

int ott_store_set_sparse(ott_store* s, const uint64_t* indptr, const void* indices_void, const float* values, uint64_t n, uint32_t vocab) {
    const uint32_t* indices = (const uint32_t*)indices_void;
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_sparse: store is NULL");
    uint64_t a = 0, b = 0;
    SparseRefusal r = sparse_check_set(s->multi != nullptr, indptr, indices, values, n, vocab, ott_store_len(s), &a, &b);  // before any device work
    if (r != SPARSE_OK) return refuse(r, a, b);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    if (n != s->n) return fail(OTT_ERR_INVALID, "ott_store_set_sparse: the store's length changed during the call");
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    sparse_drop(s);
    return sparse_build(s, indptr, indices, values, n, vocab);
}

int ott_store_clear_sparse(ott_store* s) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_clear_sparse: store is NULL");
    if (s->multi) return OTT_OK;  // (a multi-GPU store never holds any)
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    if (!s->d_sparse) return OTT_OK;
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    sparse_drop(s);
    return OTT_OK;
}

int ott_store_sparse_info(const ott_store* s, uint32_t* vocab, uint64_t* nnz, uint64_t* padded_entries, uint64_t* bytes) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_sparse_info: store is NULL");
    ott::host::SharedLock rd(const_cast<ott_store*>(s)->rw);
    if (vocab) *vocab = s->sparse_vocab;  // 0: no sparse rows are set
    if (nnz) *nnz = s->sparse_nnz;
    if (padded_entries) *padded_entries = s->sparse_lay.padded_entries;
    if (bytes) *bytes = s->d_sparse ? s->sparse_lay.bytes : 0;
    return OTT_OK;
}

int ott_store_read_sparse(const ott_store* cs, uint64_t first_row, uint64_t n_rows, uint64_t* indptr_out, void* indices_out, float* values_out, uint64_t entry_cap) {
    ott_store* s = const_cast<ott_store*>(cs);
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_read_sparse: store is NULL");
    if (!indptr_out) return fail(OTT_ERR_INVALID, "ott_store_read_sparse: indptr_out is NULL");
    ott::host::SharedLock rd(s->rw);
    if (!s->d_sparse) return fail(OTT_ERR_INVALID, "ott_store_read_sparse: no sparse rows are set (ott_store_set_sparse)");
    if (first_row > s->sparse_n || n_rows > s->sparse_n - first_row) return refuse(SPARSE_READ_RANGE, first_row, first_row + n_rows);
    indptr_out[0] = 0;
    if (n_rows == 0) return OTT_OK;
    OTT_HIP(use_device(s));
    const SparseLayout& lay = s->sparse_lay;
    std::vector<uint32_t> len(n_rows);
    OTT_HIP(hipMemcpy(len.data(), s->d_sparse + lay.off_lengths + first_row * 4, n_rows * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n_rows; i++) indptr_out[i + 1] = indptr_out[i] + len[i];
    const uint64_t need = indptr_out[n_rows];
    if (need > entry_cap) return refuse(SPARSE_READ_CAP, need, 0);
    if (need == 0) return OTT_OK;
    if (!indices_out || !values_out) return fail(OTT_ERR_INVALID, "ott_store_read_sparse: indices_out or values_out is NULL");
    uint32_t* io = (uint32_t*)indices_out;
    const std::vector<uint64_t>& base = s->sparse_base;
    const uint64_t ts = first_row / SPARSE_SLICE, te = (first_row + n_rows + SPARSE_SLICE - 1) / SPARSE_SLICE;
    std::vector<uint32_t> bi;
    std::vector<float> bv;
    for (uint64_t t0 = ts; t0 < te;) {
        uint64_t t1 = t0 + 1;
        while (t1 < te && base[t1 + 1] - base[t0] <= SP_BATCH_ENTRIES) t1++;
        const uint64_t cnt = base[t1] - base[t0];
        if (cnt) {
            bi.resize(cnt);
            bv.resize(cnt);
            OTT_HIP(hipMemcpy(bi.data(), s->d_sparse + base[t0] * 4, cnt * 4, hipMemcpyDeviceToHost));
            OTT_HIP(hipMemcpy(bv.data(), s->d_sparse + lay.off_values + base[t0] * 4, cnt * 4, hipMemcpyDeviceToHost));
            const uint64_t r0 = std::max(first_row, t0 * SPARSE_SLICE), r1 = std::min(first_row + n_rows, t1 * SPARSE_SLICE);
            for (uint64_t r = r0; r < r1; r++) {
                const uint64_t b = base[r / SPARSE_SLICE] - base[t0], o = indptr_out[r - first_row];
                for (uint64_t p = 0; p < len[r - first_row]; p++) {
                    const uint64_t at = sparse_entry_offset(b, p, r);
                    io[o + p] = bi[at];
                    values_out[o + p] = bv[at];
                }
            }
        }
        t0 = t1;
    }
    return OTT_OK;
}

// ott_query_sparse (idf = false) and ott_query_sparse_idf: the same checks, the same sweep; with idf the weights are scaled on the
// host first (the document frequencies are built where they are stale: the one piece of device work in front of the last refusal)
static int query_sparse(ott_store* s, const ott_query_desc* d, const uint64_t* q_indptr, const uint32_t* q_indices, const float* q_values, bool idf, ott_hit* out,
                        uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats) {
    const char* who = idf ? "ott_query_sparse_idf" : "ott_query_sparse";  // the entry point the messages name
    const auto refuse = [who](SparseRefusal r, uint64_t a, uint64_t b) { return fail(sparse_refusal_status(r), sparse_refusal_text(r, a, b, who)); };
    if (!d) return fail(OTT_ERR_INVALID, std::string(who) + ": desc is NULL");
    int rc;
    if (d->nq != 0 && (rc = check_desc_enums(who, d))) return rc;
    // what the arguments alone decide comes first: these refusals need no store
    uint64_t a = 0, b = 0;
    SparseRefusal r = sparse_check_query_args(d->nq, d->mode, d->metric, d->path, q_indptr, q_indices, q_values, &a);
    if (r != SPARSE_OK) return refuse(r, a, 0);
    if (!s) return fail(OTT_ERR_INVALID, std::string(who) + ": store is NULL");
    if ((rc = check_device_row_mask(who, s, d))) return rc;
    const uint32_t nq = d->nq;
    if (s->multi) return refuse(SPARSE_Q_MULTI_GPU, 0, 0);  // (the front of a multi-GPU store holds no rows)

    ott::host::SharedLock rd;  // the corpus and the sparse rows cannot change while the call runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    if ((r = sparse_check_store(false, s->d_sparse != nullptr, s->sparse_n, s->n, s->opt.tie_order, &a, &b)) != SPARSE_OK) return refuse(r, a, b);
    if ((r = sparse_check_query(nq, q_indptr, q_indices, q_values, s->sparse_vocab, &a, &b)) != SPARSE_OK) return refuse(r, a, b);
    RunPlan rp;
    make_run_plan(s, d->chunk_mask, rp);
    const uint64_t k_eff = d->k < rp.rows_scored ? d->k : rp.rows_scored;  // a list never outgrows the pool
    if ((r = sparse_check_cap(cap, nq, k_eff, s->n)) != SPARSE_OK) return refuse(r, 0, 0);
    if (!out && cap) return fail(OTT_ERR_INVALID, std::string(who) + ": out is NULL");
    std::vector<float> scaled;
    if (idf && q_indptr[nq] != 0) {
        scaled.resize(q_indptr[nq]);
        {
            CtxLease lease(s);
            if ((rc = sparse_df_ensure(lease.c))) return rc;
        }
        sparse_idf_scale(s, q_indices, q_values, q_indptr[nq], scaled.data());
        if ((r = sparse_check_query(nq, q_indptr, q_indices, scaled.data(), s->sparse_vocab, &a, &b)) != SPARSE_OK) return refuse(r, a, b);
        q_values = scaled.data();
    }
    if (n_out) *n_out = 0;
    if (n_per_query) memset(n_per_query, 0, (size_t)nq * sizeof(uint64_t));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (k_eff == 0) return OTT_OK;  // k == 0 or nothing to score (an empty store): a valid call with no hits

    {
        CtxLease lease(s);
        ott_store* ctx = lease.c;
        rc = run_sparse_sweep(ctx, d, q_indptr, q_indices, q_values, k_eff, out, n_out, n_per_query, stats);
        if (rc) (void)hipStreamSynchronize(ctx->stream);  // nothing of this call is in flight when the context is given back
    }
    return rc;
}

int ott_query_sparse(ott_store* s, const ott_query_desc* d, const uint64_t* q_indptr, const void* q_indices, const float* q_values, ott_hit* out, uint64_t cap,
                     uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats) {
    return query_sparse(s, d, q_indptr, (const uint32_t*)q_indices, q_values, false, out, cap, n_out, n_per_query, stats);
}

int ott_query_sparse_idf(ott_store* s, const ott_query_desc* d, const uint64_t* q_indptr, const void* q_indices, const float* q_values, ott_hit* out, uint64_t cap,
                         uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats) {
    return query_sparse(s, d, q_indptr, (const uint32_t*)q_indices, q_values, true, out, cap, n_out, n_per_query, stats);
}

int ott_store_sparse_df(ott_store* s, void* df_out, uint64_t* n_docs_out) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_sparse_df: store is NULL");
    if (s->multi) return fail(OTT_ERR_UNSUPPORTED, "ott_store_sparse_df: a multi-GPU store is not served (sparse rows live on one GPU)");
    int rc;
    ott::host::SharedLock rd;  // the sparse rows and the live mask cannot change while the call runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    if (!s->d_sparse) return fail(OTT_ERR_INVALID, "ott_store_sparse_df: no sparse rows are set (ott_store_set_sparse)");
    if (s->sparse_n != s->n)
        return fail(OTT_ERR_INVALID, "ott_store_sparse_df: the sparse rows cover " + std::to_string(s->sparse_n) + " rows, the store holds " + std::to_string(s->n) +
                                         " (rows were appended since ott_store_set_sparse: set them again)");
    {
        CtxLease lease(s);
        if ((rc = sparse_df_ensure(lease.c))) return rc;
    }
    if (df_out) memcpy(df_out, s->df_host.data(), (size_t)s->sparse_vocab * 4);
    if (n_docs_out) *n_docs_out = s->df_ndocs;
    return OTT_OK;
}

uint64_t ott_store_sparse_df_builds(const ott_store* s) { return s ? s->df_builds.load(std::memory_order_relaxed) : 0ull; }

}  // extern "C"
