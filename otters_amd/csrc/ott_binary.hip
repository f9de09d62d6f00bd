// ott_binary.hip — bit rows and the exact Hamming search.  Row r of a store may carry a bit row of n_bits bits beside
// its dense one (ott_store_set_binary, or ott_store_set_binary_sign: bit j = row[j] > 0, made on the device from the dense rows);
// ott_query_binary ranks the rows by S = (float) popcount(q XOR v), the L1 distance of the bit vectors (ott_binary_plan.h states the
// score, the layout and the route for the host; tests/binary_ref.py is the numpy model).  Row ids, chunk masks, row masks, the
// evaluated mask and deleted rows mean what they mean for a dense query.
//
// Device layout: slices of 64 rows, transposed (ott_binary_plan.h): unit p (16 bytes) of a slice's 64 rows lies in 64 consecutive
// units.  Lane = row: one dwordx4 load per lane is a coalesced 1-KiB wave load, and every lane counts its own row's bits.
//
//   binary_walk           both routes: a persistent grid, wave per slice.  The composed row mask and the chunk runs decide each lane's
//                         row; a slice with no surviving row is not read.  A lane keeps BIN_U units in registers while the next BIN_U
//                         are in flight (unconditional non-temporal loads, the unit index clamped: the compiled loop waits with
//                         vmcnt(BIN_U); the layout is streamed once per pass); the queries of the pass are
//                         wave-uniform and come through the constant address space (scalar loads); per unit and query four XOR and
//                         four accumulating population counts.
//   binary_table_kernel   the table route: ord(S) << 32 | ~row into d_gtable[q][row] for a candidate that passes the filter, a plain
//                         store, one writer per pair; GroupTopK (prepare, pass, finish) does the rest.  Serves every call.
//   binary_gate_kernel    the gated route: no key table.  Per workgroup and query of the pass LDS holds a histogram of the levels
//                         let through and a gate word; a candidate at or inside the gate is counted, the wave recomputes the gate
//                         from the histogram (the smallest level that k counted rows reach), publishes it to the workgroup and to
//                         one global word per query, and appends what is still inside to the pair arrays: one ballot and ONE
//                         global atomic add on the cursor per wave and query.  sort_group_pairs ranks the pairs behind the sweep.
//                         A level is the distance (take Min) or n_bits minus the distance (take Max): the gate only falls.
//   binary_sign_kernel    ott_store_set_binary_sign: a wave per (row, 64 dims), a ballot of x > 0, one 8-byte store.
//
// Out of scope: Jaccard / Tanimoto, binary legs in ott_query_fuse / ott_query_hybrid, multi-GPU stores, extending bit rows on append,
// compaction with bit rows resident, asymmetric scoring of an f32 query.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ott_internal.h"
#include "ott_exact_dev.h"

namespace ott {

static_assert(BINARY_MAX_BITS == OTT_BINARY_MAX_BITS && BINARY_MAX_QUERIES == OTT_BINARY_MAX_QUERIES, "ott_binary_plan.h restates the header's constants");
static_assert(BINARY_METRIC_MANHATTAN == OTT_METRIC_MANHATTAN, "ott_binary_plan.h restates the metric");

constexpr int BIN_U = 4;              // units a lane holds while the next BIN_U are in flight (2 x 4 x 16 B per lane)
constexpr int BIN_WAVES = 4;          // workgroups of 256 threads
constexpr int BIN_BLOCKS_PER_CU = 8;  // table route; the gated route's LDS decides its own residency

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) v4u* const_v4u_ptr;  // the constant address space: uniform loads become scalar loads

struct BinaryParams {
    const v4u* rows;  // the layout
    const uint64_t* row_mask;
    uint64_t row_mask_bits;
    const ott_run* runs;  // the surviving chunk runs, ascending
    uint32_t n_runs;
    uint32_t n_slices;
    uint64_t n_rows;
    uint32_t units, n_bits;
    const v4u* q;  // [nq_total][units] the call's queries, zero padded to whole units
    uint32_t q0, nq_here, nq_total;
    uint32_t take_max, cmp;
    float thr;
    unsigned long long* table;  // table route: [queries of the pass][n_rows] candidate key per (query, row); 0 = empty
    uint32_t* gate;             // gated route: [nq_total] the global gate words, n_bits when the call starts
    unsigned long long* cursor; // ... the pair cursor (keeps counting past cap)
    uint64_t* keys;             // ... [cap] pair keys
    uint32_t* qs;               // ... [cap] pair queries
    uint64_t cap;
    uint32_t k;
};

// whether `row` lies in a surviving chunk run (binary search; one run is the common case)
__device__ __forceinline__ bool binary_row_in_runs(const ott_run* runs, uint32_t n_runs, uint64_t row) {
    uint32_t lo = 0, hi = n_runs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (runs[mid].start <= row) lo = mid;
        else hi = mid;
    }
    const uint64_t start = runs[lo].start;
    return row >= start && row - start < runs[lo].count;
}

// popcount(x) + acc in ONE instruction.  Written as `__popc(x) + acc` the compiler counts into zero and folds the sums of two words into
// a three-operand add: five instructions per two words and query where four do (read in the assembly).
__device__ __forceinline__ uint32_t popc_acc(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// The slices of wave gw of nw.  epi(row, valid, d): d[q] = popcount(query q0 + q XOR the lane's row).
template <int NQ, class Epilogue>
__device__ __forceinline__ void binary_walk(const BinaryParams& p, uint32_t gw, uint32_t nw, Epilogue&& epi) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t units = p.units;
    const_v4u_ptr qp[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {  // (a slot behind the pass's queries reads the call's last query: its result is never used)
        const uint32_t qi = p.q0 + q < p.nq_total ? p.q0 + q : p.nq_total - 1;
        qp[q] = (const_v4u_ptr)(uintptr_t)(p.q + (size_t)qi * units);
    }
    for (uint32_t t = gw; t < p.n_slices; t += nw) {
        const uint64_t row = (uint64_t)t * 64 + lane;
        bool valid = row < p.n_rows && binary_row_in_runs(p.runs, p.n_runs, row);
        if (p.row_mask != nullptr && valid && row < p.row_mask_bits) valid = (p.row_mask[row >> 6] >> (row & 63)) & 1;  // src/vec.rs:231-237
        if (__ballot(valid) == 0) continue;  // no surviving row: the slice is not read
        // unit u of this lane's row: rp[64 u], inside the slice for u < units (the last slice is padded to 64 rows: every lane loads).
        // Every load is UNCONDITIONAL — a unit index at or past `units` is clamped to the row's last unit, whose copy is never consumed —
        // so the compiler counts the loads and waits with vmcnt(BIN_U): the next units stay in flight while these are consumed (behind a
        // branch per load it waited for all of them, vmcnt(0), in front of the first XOR: read in the assembly).  The price is up to
        // BIN_U loads of the last unit again per row, served by the L1: about 5 % of the sweep's time at 1024 bits (measured).  A loop of
        // unguarded full groups with a guarded last group avoids them but compiled to 97 VGPRs and a vmcnt(0) in the loop: not taken
        const v4u* rp = p.rows + (uint64_t)t * units * 64 + lane;
        const uint32_t last = units - 1;
        uint32_t d[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) d[q] = 0u;
        v4u cur[BIN_U];
#pragma unroll
        for (int u = 0; u < BIN_U; u++) cur[u] = __builtin_nontemporal_load(rp + (uint64_t)((uint32_t)u < last ? (uint32_t)u : last) * 64);
        for (uint32_t u0 = 0; u0 < units; u0 += BIN_U) {
            v4u nxt[BIN_U];
#pragma unroll
            for (int u = 0; u < BIN_U; u++) {  // the next units are in flight while these are consumed
                const uint32_t e = u0 + BIN_U + u;
                nxt[u] = __builtin_nontemporal_load(rp + (uint64_t)(e < last ? e : last) * 64);
            }
#pragma unroll
            for (int u = 0; u < BIN_U; u++) {
                if (u0 + u < units) {
#pragma unroll
                    for (int q = 0; q < NQ; q++) {
                        const v4u w = qp[q][u0 + u];
                        d[q] = popc_acc(cur[u].x ^ w.x, d[q]);
                        d[q] = popc_acc(cur[u].y ^ w.y, d[q]);
                        d[q] = popc_acc(cur[u].z ^ w.z, d[q]);
                        d[q] = popc_acc(cur[u].w ^ w.w, d[q]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < BIN_U; u++) cur[u] = nxt[u];
        }
        epi(row, valid, d);
    }
}

template <int NQ>
__global__ __launch_bounds__(64 * BIN_WAVES) void binary_table_kernel(BinaryParams p) {
    const uint32_t wave = threadIdx.x >> 6;
    const bool take_max = p.take_max != 0;
    binary_walk<NQ>(p, blockIdx.x * BIN_WAVES + wave, gridDim.x * BIN_WAVES, [&](uint64_t row, bool valid, const uint32_t (&d)[NQ]) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float s = (float)d[q];  // exact: at most 16384
            if ((uint32_t)q < p.nq_here && valid && cmp_holds(s, p.cmp, p.thr))
                p.table[(size_t)q * p.n_rows + row] = ((unsigned long long)ord_of(s, take_max) << 32) | (uint32_t)(~(uint32_t)row);
        }
    });
}

// The smallest level T' <= T with h[0] + .. + h[T'] >= k, or T when the counts do not reach k: the wave scans 64 levels at a time.
// Other waves may be adding meanwhile: a count read too low only leaves the result too high.
__device__ __forceinline__ uint32_t binary_gate_scan(const volatile uint32_t* h, uint32_t T, uint32_t k) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t run = 0;
    for (uint32_t base = 0; base <= T; base += 64) {
        const uint32_t idx = base + lane;
        uint32_t sc = idx <= T ? h[idx] : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {  // inclusive prefix sum over the lanes
            const uint32_t up = __shfl_up(sc, o);
            if (lane >= (uint32_t)o) sc += up;
        }
        const uint32_t total = __shfl(sc, 63);
        if (run + total >= k) return base + (uint32_t)__builtin_ctzll(__ballot(run + sc >= k));
        run += total;
    }
    return T;
}

template <int NQ>
__global__ __launch_bounds__(64 * BIN_WAVES) void binary_gate_kernel(BinaryParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bg_lds[];  // per query of the pass: h[0 .. n_bits] | the gate word
    const uint32_t stride = p.n_bits + 2, gate_at = p.n_bits + 1;
    for (uint32_t i = threadIdx.x; i < (uint32_t)NQ * stride; i += blockDim.x) bg_lds[i] = (i % stride) == gate_at ? p.n_bits : 0u;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool take_max = p.take_max != 0;
    binary_walk<NQ>(p, blockIdx.x * BIN_WAVES + wave, gridDim.x * BIN_WAVES, [&](uint64_t row, bool valid, const uint32_t (&d)[NQ]) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            if ((uint32_t)q >= p.nq_here) continue;  // (wave-uniform)
            uint32_t* h = bg_lds + (uint32_t)q * stride;
            uint32_t* g = p.gate + p.q0 + q;
            // the gate this tile starts under: the workgroup's and the grid's, plain loads (a stale value is only higher)
            const uint32_t tl = *(volatile uint32_t*)(h + gate_at), tg = *(volatile uint32_t*)g;
            const uint32_t T = tl < tg ? tl : tg;
            const float s = (float)d[q];  // exact: at most 16384
            const uint32_t level = take_max ? p.n_bits - d[q] : d[q];
            bool pass = valid && cmp_holds(s, p.cmp, p.thr) && level <= T;
            if (__ballot(pass) == 0) continue;
            if (pass) atomicAdd(h + level, 1u);
            __threadfence_block();  // this wave's adds are in the histogram before it reads it
            // k counted rows lie at or below T2: the k-th best level of the call is at most T2, and a row above it is no hit
            const uint32_t T2 = binary_gate_scan(h, T, p.k);
            if (T2 < T && lane == 0) {
                atomicMin(h + gate_at, T2);
                atomicMin(g, T2);
            }
            pass = pass && level <= T2;
            const uint64_t m = __ballot(pass);
            if (m == 0) continue;
            unsigned long long base = 0;
            if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(p.cursor, (unsigned long long)__popcll(m));
            base = rl64(base, (int)__builtin_ctzll(m));
            if (pass) {
                const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                if (at < p.cap) {  // (the cursor keeps counting: the host sees the overflow)
                    p.keys[at] = ((unsigned long long)ord_of(s, take_max) << 32) | (uint32_t)(~(uint32_t)row);
                    p.qs[at] = p.q0 + q;
                }
            }
        }
    });
}

// ott_store_set_binary_sign: wave gw takes (row, word) pairs; lane j holds dim 64 word + j of the row, the ballot of x > 0 (on the
// bits: ott_binary_plan.h: binary_sign_bit_of) is the word.  The layout was zeroed first: padding words and rows stay zero.
__global__ __launch_bounds__(256) void binary_sign_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim, uint64_t n_rows, uint32_t words, uint32_t units,
                                                          char* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6), total = n_rows * words;
    for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < total; i += nw) {
        const uint64_t row = i / words;
        const uint32_t w = (uint32_t)(i - row * words), j = w * 64 + lane;
        const uint32_t bits = j < dim ? __float_as_uint(rows[row * ld + j]) : 0u;
        const uint64_t m = __ballot(bits - 1u < 0x7F800000u);
        // (ott_binary_plan.h: binary_word_offset, which is host code)
        const uint64_t at = (((row >> 6) * units + (w >> 1)) * 64 + (row & 63)) * 16 + (uint64_t)(w & 1u) * 8;
        if (lane == 0) *(uint64_t*)(out + at) = m;
    }
}

void binary_drop(ott_store* s) {
    if (s->d_binary) (void)hipFree(s->d_binary);
    s->d_binary = nullptr;
    s->binary_n = 0;
    s->binary_bits = 0;
}

namespace {

int refuse(BinaryRefusal r, uint64_t a, uint64_t b) { return fail(binary_refusal_status(r), binary_refusal_text(r, a, b)); }

constexpr uint64_t BIN_BATCH_BYTES = 32ull << 20;  // host staging of the layout: 32 MiB of slices at a time

// The layout of `n` rows from the caller's row-major words into a fresh allocation; the caller holds the store exclusively, on its device.
int binary_build(ott_store* s, const uint64_t* words, uint64_t n, uint32_t n_bits) {
    const uint32_t W = binary_words(n_bits), units = binary_units(n_bits);
    const uint64_t n_slices = binary_slices(n), slice_bytes = binary_slice_bytes(units), bytes = binary_layout_bytes(n, n_bits);
    char* d = nullptr;
    OTT_HIP(hipMalloc((void**)&d, (size_t)(bytes ? bytes : 256)));
    const uint64_t per_batch = std::max<uint64_t>(1, BIN_BATCH_BYTES / slice_bytes);
    std::vector<uint64_t> buf;
    for (uint64_t t0 = 0; t0 < n_slices; t0 += per_batch) {
        const uint64_t t1 = std::min(n_slices, t0 + per_batch), r1 = std::min(n, t1 * BINARY_SLICE);
        buf.assign((size_t)((t1 - t0) * slice_bytes / 8), 0ull);  // the padding: zero bits, zero rows
        const uint64_t off0 = t0 * slice_bytes;
        for (uint64_t r = t0 * BINARY_SLICE; r < r1; r++)
            for (uint32_t w = 0; w < W; w++) buf[(size_t)((binary_word_offset(r, w, units) - off0) / 8)] = words[r * W + w];
        const hipError_t e = hipMemcpy(d + off0, buf.data(), buf.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(e == hipErrorOutOfMemory ? OTT_ERR_OOM : OTT_ERR_HIP, std::string("ott_store_set_binary: ") + hipGetErrorString(e));
        }
    }
    s->d_binary = d;
    s->binary_n = n;
    s->binary_bits = n_bits;
    return OTT_OK;
}

static_assert(sizeof(ott_run) == 16 && offsetof(ott_run, start) == 0 && offsetof(ott_run, count) == 8, "binary_run_bytes reads a run as a (start, count) pair");

template <int NQ>
int launch_table(ott_store* s, const BinaryParams& p) {
    const uint32_t grid = grid_blocks(p.n_slices, BIN_WAVES, s->n_cu, BIN_BLOCKS_PER_CU);
    hipLaunchKernelGGL(binary_table_kernel<NQ>, dim3(grid), dim3(64 * BIN_WAVES), 0, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

template <int NQ>
int launch_gate(ott_store* s, const BinaryParams& p) {
    const size_t smem = binary_gate_lds_bytes(p.n_bits, NQ);
    if (smem > 48 * 1024) {  // more dynamic LDS than the default limit: the opt-in, once per device
        static std::atomic<uint64_t> attr_set{0};
        if (attr_needed(attr_set, s->device)) {
            OTT_HIP(hipFuncSetAttribute((const void*)binary_gate_kernel<NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BINARY_GATE_LDS_BYTES));
            attr_done(attr_set, s->device);
        }
    }
    // workgroups per CU: what the histograms leave of 160 KiB of LDS, at most the table route's
    const uint32_t fit = (uint32_t)std::max<size_t>(1, std::min<size_t>(BIN_BLOCKS_PER_CU, (size_t)(160 * 1024) / std::max<size_t>(smem, 1)));
    const uint32_t grid = grid_blocks(p.n_slices, BIN_WAVES, s->n_cu, fit);
    hipLaunchKernelGGL(binary_gate_kernel<NQ>, dim3(grid), dim3(64 * BIN_WAVES), smem, s->stream, p);
    OTT_HIP(hipGetLastError());
    return OTT_OK;
}

}  // namespace

// The binary sweep on a context whose `mu` the caller holds (and the owner's `rw`, shared).  k_eff = min(k, rows the chunk mask
// leaves) >= 1.  q_words: the call's queries, checked.
int run_binary_sweep(ott_store* s, const ott_query_desc* d, const uint64_t* q_words, uint64_t k_eff, ott_hit* out, uint64_t* n_out, uint64_t* n_per_query,
                     ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    ott_store* own = s->owner ? s->owner : s;
    const uint32_t nq = d->nq, n_bits = s->binary_bits, W = binary_words(n_bits), units = binary_units(n_bits);
    const uint64_t n = s->n;
    const uint64_t t0 = now_ns();
    ott_stats st;
    RunPlan pl;
    BinaryParams p{};
    uint64_t total = 0;
    std::vector<uint64_t> per(nq, 0);
    // (the descriptor's own mask — caller's or evaluated, live mask — is composed here)
    if ((rc = sweep_plan(s, d, nq, &st, &pl, &p.row_mask, &p.row_mask_bits))) return rc;
    if (pl.rows_scored != 0) {
        const uint64_t cap_opt = (uint64_t)s->opt.binary_gate_cap;
        bool gated = binary_take_gate(s->opt.binary_gate, n_bits, nq, k_eff, n, cap_opt);
        const uint64_t cap = gated ? binary_gate_capacity(cap_opt, nq, n) : 0;
        // one block, one copy: [runs | queries padded to whole units | gate words | cursor]
        const size_t off_q = pl.runs.size() * sizeof(ott_run), q_bytes = (size_t)nq * units * BINARY_UNIT_BYTES;
        const size_t off_gate = off_q + q_bytes, off_cur = (off_gate + (size_t)nq * 4 + 15) & ~(size_t)15, block = off_cur + 16;
        if ((rc = s->h_bq.ensure(block + 16))) return rc;  // (+ 16: where the cursor comes back to)
        char* hs = (char*)s->h_bq.p;
        memcpy(hs, pl.runs.data(), off_q);
        memset(hs + off_q, 0, block - off_q);
        for (uint32_t b = 0; b < nq; b++) memcpy(hs + off_q + (size_t)b * units * BINARY_UNIT_BYTES, q_words + (size_t)b * W, (size_t)W * 8);
        for (uint32_t b = 0; b < nq; b++) ((uint32_t*)(hs + off_gate))[b] = n_bits;
        if ((rc = s->d_bq.ensure(block))) return rc;
        OTT_HIP(hipMemcpyAsync(s->d_bq.p, hs, block, hipMemcpyHostToDevice, s->stream));

        p.rows = (const v4u*)s->d_binary;
        p.runs = (const ott_run*)s->d_bq.p;
        p.n_runs = (uint32_t)pl.runs.size();
        p.n_slices = (uint32_t)binary_slices(n);  // (n < 2^32 - 16: binary_check_store)
        p.n_rows = n;
        p.units = units;
        p.n_bits = n_bits;
        p.q = (const v4u*)((const char*)s->d_bq.p + off_q);
        p.nq_total = nq;
        p.take_max = d->take == OTT_TAKE_MAX;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;
        p.gate = (uint32_t*)((char*)s->d_bq.p + off_gate);
        p.cursor = (unsigned long long*)((char*)s->d_bq.p + off_cur);
        p.k = (uint32_t)std::min<uint64_t>(k_eff, BINARY_GATE_MAX_K);
        const bool timing = stats_out != nullptr;
        const uint64_t run_bytes = binary_run_bytes((const uint64_t*)pl.runs.data(), pl.runs.size(), units);
        bool done = false;

        // (a context that cannot allocate the pair arrays answers on the table route, which needs none)
        if (gated && ensure_group_pairs(s, cap) != OTT_OK) gated = false;
        if (gated) {
            own->bin_ctr[0].fetch_add(1, std::memory_order_relaxed);
            const uint32_t tile = binary_gate_tile(n_bits, nq), passes = binary_passes(tile, nq);
            p.keys = (uint64_t*)s->l_keysA.p;
            p.qs = (uint32_t*)s->l_qA.p;
            p.cap = cap;
            if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
            for (uint32_t ps = 0; ps < passes; ps++) {
                p.q0 = ps * tile;
                p.nq_here = (nq - p.q0) < tile ? (nq - p.q0) : tile;
                if ((rc = tile == 4 ? launch_gate<4>(s, p) : tile == 2 ? launch_gate<2>(s, p) : launch_gate<1>(s, p))) return rc;
            }
            if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
            unsigned long long* h_cur = (unsigned long long*)(hs + block);
            OTT_HIP(hipMemcpyAsync(h_cur, p.cursor, 8, hipMemcpyDeviceToHost, s->stream));
            OTT_HIP(hipStreamSynchronize(s->stream));  // the one host wait of a gated call that does not overflow
            const uint64_t emitted = *h_cur;
            own->bin_ctr[1].fetch_add(emitted < cap ? emitted : cap, std::memory_order_relaxed);
            st.passes += passes;
            st.bytes_scanned += binary_bytes_scanned(passes, run_bytes);
            if (emitted > cap) {  // pairs were dropped: the table route answers the call (a second sweep and a second wait)
                own->bin_ctr[2].fetch_add(1, std::memory_order_relaxed);
            } else {
                std::vector<std::vector<ott_hit>> lists;
                if ((rc = sort_group_pairs(s, emitted, nq, p.take_max != 0, k_eff, lists))) return rc;
                if (timing) {
                    OTT_HIP(hipEventRecord(s->ev[5], s->stream));
                    OTT_HIP(hipStreamSynchronize(s->stream));
                    read_exact_events(s, &st);
                }
                for (uint32_t b = 0; b < nq; b++) {
                    const std::vector<ott_hit>& l = lists[b];
                    if (!l.empty()) memcpy(out + total, l.data(), l.size() * sizeof(ott_hit));
                    per[b] = l.size();
                    total += l.size();
                }
                done = true;
            }
        }
        if (!done) {
            own->bin_ctr[3].fetch_add(1, std::memory_order_relaxed);
            const uint32_t tile = std::min(nq, BINARY_TABLE_NQ) >= 4 ? 4u : nq >= 2 ? 2u : 1u, passes = binary_passes(tile, nq);
            if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)tile * n * 8))) return rc;
            p.table = (unsigned long long*)s->d_gtable.p;
            GroupTopK tk;
            tk.n_groups = (uint32_t)n;
            tk.nq = nq;
            tk.k = k_eff;
            tk.take_max = p.take_max != 0;
            if ((rc = tk.prepare(s, nullptr))) return rc;
            if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
            for (uint32_t ps = 0; ps < passes; ps++) {
                p.q0 = ps * tile;
                p.nq_here = (nq - p.q0) < tile ? (nq - p.q0) : tile;
                if ((rc = tile == 4 ? launch_table<4>(s, p) : tile == 2 ? launch_table<2>(s, p) : launch_table<1>(s, p))) return rc;
                if ((rc = tk.pass(s, p.table, p.q0, p.nq_here))) return rc;
            }
            if (timing) OTT_HIP(hipEventRecord(s->ev[4], s->stream));
            if ((rc = tk.finish(s, timing, out, &total, per.data()))) return rc;
            if (timing) read_exact_events(s, &st);
            st.passes += passes;
            st.bytes_scanned += binary_bytes_scanned(passes, run_bytes);
        }
        uint64_t at = 0;
        for (uint32_t b = 0; b < nq; b++) {  // hit.query = b
            for (uint64_t i = 0; i < per[b]; i++) out[at + i].query = b;
            at += per[b];
        }
    }
    if (n_per_query) memcpy(n_per_query, per.data(), (size_t)nq * sizeof(uint64_t));
    if (n_out) *n_out = total;
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

}  // namespace ott

using namespace ott;

extern "C" {

int ott_store_set_binary(ott_store* s, const void* words_void, uint64_t n, uint32_t n_bits) {
    const uint64_t* words = (const uint64_t*)words_void;
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_binary: store is NULL");
    uint64_t a = 0, b = 0;
    BinaryRefusal r = binary_check_set(s->multi != nullptr, words, n, n_bits, ott_store_len(s), &a, &b);  // before any device work
    if (r != BINARY_OK) return refuse(r, a, b);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    if (n != s->n) return fail(OTT_ERR_INVALID, "ott_store_set_binary: the store's length changed during the call");
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    binary_drop(s);
    return binary_build(s, words, n, n_bits);
}

int ott_store_set_binary_sign(ott_store* s) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_set_binary_sign: store is NULL");
    uint64_t a = 0;
    BinaryRefusal r = binary_check_sign(s->multi != nullptr, s->dim, &a);
    if (r != BINARY_OK) return refuse(r, a, 0);
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    binary_drop(s);
    const uint64_t n = s->n;
    const uint32_t n_bits = s->dim, W = binary_words(n_bits), units = binary_units(n_bits);
    const uint64_t bytes = binary_layout_bytes(n, n_bits);
    char* d = nullptr;
    OTT_HIP(hipMalloc((void**)&d, (size_t)(bytes ? bytes : 256)));
    hipError_t e = bytes ? hipMemsetAsync(d, 0, (size_t)bytes, s->stream) : hipSuccess;
    if (e == hipSuccess && n != 0) {
        const uint32_t grid = grid_blocks(n * W, 4, s->n_cu, 8);
        hipLaunchKernelGGL(binary_sign_kernel, dim3(grid), dim3(256), 0, s->stream, (const float*)s->d_rows, s->ld, s->dim, n, W, units, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(OTT_ERR_HIP, std::string("ott_store_set_binary_sign: ") + hipGetErrorString(e));
    }
    s->d_binary = d;
    s->binary_n = n;
    s->binary_bits = n_bits;
    return OTT_OK;
}

int ott_store_clear_binary(ott_store* s) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_clear_binary: store is NULL");
    if (s->multi) return OTT_OK;  // (a multi-GPU store never holds any)
    ott::host::ExclusiveLock wr(s->rw);  // no query is running on any context
    std::lock_guard<std::mutex> g(s->mu);
    int rc = store_flush_locked(s);
    if (rc) return rc;
    if (!s->d_binary) return OTT_OK;
    OTT_HIP(use_device(s));
    OTT_HIP(hipStreamSynchronize(s->stream));
    binary_drop(s);
    return OTT_OK;
}

int ott_store_binary_info(const ott_store* s, uint32_t* n_bits, uint64_t* bytes) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_binary_info: store is NULL");
    ott::host::SharedLock rd(const_cast<ott_store*>(s)->rw);
    if (n_bits) *n_bits = s->d_binary ? s->binary_bits : 0;  // 0: no bit rows are set
    if (bytes) *bytes = s->d_binary ? binary_layout_bytes(s->binary_n, s->binary_bits) : 0;
    return OTT_OK;
}

int ott_store_read_binary(const ott_store* cs, uint64_t first_row, uint64_t n_rows, void* words_out) {
    ott_store* s = const_cast<ott_store*>(cs);
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_read_binary: store is NULL");
    ott::host::SharedLock rd(s->rw);
    if (!s->d_binary) return fail(OTT_ERR_INVALID, "ott_store_read_binary: no bit rows are set (ott_store_set_binary)");
    if (first_row > s->binary_n || n_rows > s->binary_n - first_row) return refuse(BINARY_READ_RANGE, first_row, first_row + n_rows);
    if (n_rows == 0) return OTT_OK;
    if (!words_out) return fail(OTT_ERR_INVALID, "ott_store_read_binary: words_out is NULL");
    OTT_HIP(use_device(s));
    uint64_t* wo = (uint64_t*)words_out;
    const uint32_t W = binary_words(s->binary_bits), units = binary_units(s->binary_bits);
    const uint64_t slice_bytes = binary_slice_bytes(units), per_batch = std::max<uint64_t>(1, BIN_BATCH_BYTES / slice_bytes);
    const uint64_t ts = first_row / BINARY_SLICE, te = (first_row + n_rows + BINARY_SLICE - 1) / BINARY_SLICE;
    std::vector<uint64_t> buf;
    for (uint64_t t0 = ts; t0 < te; t0 += per_batch) {
        const uint64_t t1 = std::min(te, t0 + per_batch), off0 = t0 * slice_bytes;
        buf.resize((size_t)((t1 - t0) * slice_bytes / 8));
        OTT_HIP(hipMemcpy(buf.data(), s->d_binary + off0, buf.size() * 8, hipMemcpyDeviceToHost));
        const uint64_t r0 = std::max(first_row, t0 * BINARY_SLICE), r1 = std::min(first_row + n_rows, t1 * BINARY_SLICE);
        for (uint64_t r = r0; r < r1; r++)
            for (uint32_t w = 0; w < W; w++) wo[(r - first_row) * W + w] = buf[(size_t)((binary_word_offset(r, w, units) - off0) / 8)];
    }
    return OTT_OK;
}

int ott_query_binary(ott_store* s, const ott_query_desc* d, const void* q_words_void, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                     ott_stats* stats) {
    const char* who = "ott_query_binary";
    const uint64_t* q_words = (const uint64_t*)q_words_void;
    if (!d) return fail(OTT_ERR_INVALID, "ott_query_binary: desc is NULL");
    int rc;
    if (d->nq != 0 && (rc = check_desc_enums(who, d))) return rc;
    // what the arguments alone decide comes first: these refusals need no store
    uint64_t a = 0, b = 0;
    BinaryRefusal r = binary_check_query_args(d->nq, d->mode, d->metric, d->path, q_words, &a);
    if (r != BINARY_OK) return refuse(r, a, 0);
    if (!s) return fail(OTT_ERR_INVALID, "ott_query_binary: store is NULL");
    if ((rc = check_device_row_mask(who, s, d))) return rc;
    const uint32_t nq = d->nq;
    if (s->multi) return refuse(BINARY_Q_MULTI_GPU, 0, 0);  // (the front of a multi-GPU store holds no rows)

    ott::host::SharedLock rd;  // the corpus and the bit rows cannot change while the call runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    if ((r = binary_check_store(false, s->d_binary != nullptr, s->binary_n, s->n, s->opt.tie_order, &a, &b)) != BINARY_OK) return refuse(r, a, b);
    if ((r = binary_check_query(q_words, nq, s->binary_bits, &a, &b)) != BINARY_OK) return refuse(r, a, b);
    RunPlan rp;
    make_run_plan(s, d->chunk_mask, rp);
    const uint64_t k_eff = d->k < rp.rows_scored ? d->k : rp.rows_scored;  // a list never outgrows the pool
    if ((r = binary_check_cap(cap, nq, k_eff, s->n)) != BINARY_OK) return refuse(r, 0, 0);
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_binary: out is NULL");
    if (n_out) *n_out = 0;
    if (n_per_query) memset(n_per_query, 0, (size_t)nq * sizeof(uint64_t));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (k_eff == 0) return OTT_OK;  // k == 0 or nothing to score (an empty store): a valid call with no hits

    {
        CtxLease lease(s);
        ott_store* ctx = lease.c;
        rc = run_binary_sweep(ctx, d, q_words, k_eff, out, n_out, n_per_query, stats);
        if (rc) (void)hipStreamSynchronize(ctx->stream);  // nothing of this call is in flight when the context is given back
    }
    return rc;
}

int ott_store_binary_counters(const ott_store* s, uint64_t* out) {
    if (!s) return fail(OTT_ERR_INVALID, "ott_store_binary_counters: store is NULL");
    if (!out) return fail(OTT_ERR_INVALID, "ott_store_binary_counters: out is NULL");
    for (int i = 0; i < 4; i++) out[i] = s->bin_ctr[i].load(std::memory_order_relaxed);
    return OTT_OK;
}

}  // extern "C"
