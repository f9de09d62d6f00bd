// ott_boost.hip — score boosting: ott_query_boost ranks by a formula of the score and metadata columns.  Every
// candidate row r and query b get a final score F = Sw + B (OTT_BOOST_SUM) or Sw * (1 + B) (OTT_BOOST_MULT), Sw = score_weight * S
// with S the exact path's score, B the sum in the caller's order of weight_j * g_j over at most OTT_BOOST_MAX_TERMS terms: a
// column's value minus an origin (VALUE), a linear decay of that distance (LIN_DECAY), or the bit of a device mask slot (MASK).
// All of it IEEE f32, one rounded operation at a time (ott_boost_plan.h states the formula for the host; tests/boost_ref.py is the
// numpy model); a NaN F drops the row, the filter acts on F, the hits are ordered by F in ott_query's canonical order.  A boost
// lifts rows that were never among the best k by raw score, so the formula is applied to EVERY surviving row: one streaming sweep.
//
//   boost_sweep_kernel    sweep_tiles (ott_sweep_dev.h) and this epilogue per valid row: B once per row — the term descriptors
//                         ride in the kernel arguments and are read through the constant address space (scalar loads, wave-uniform
//                         branches on kind and dtype), the column elements, NULL words and mask words are per-lane loads with
//                         lane = row, so they coalesce — then per query of the pass F, the NaN drop, cmp_holds, key =
//                         ord(F) << 32 | ~row and a PLAIN store to table[q][row]: a (query, row) pair has one writer.  The table
//                         is d_gtable under its zero-when-found protocol.
//   GroupTopK             grouped search's top-k over the table with n_groups = rows: pass() after every sweep, finish() once —
//                         one host wait for the whole call.  The host runner follows run_masks_sweep (ott_masks.hip) step for step.
#include <string.h>

#include <vector>

#include "ott_boost_plan.h"
#include "ott_internal.h"
#include "ott_sweep_dev.h"

namespace ott {

static_assert(BOOST_NQ == SW_NQ, "the plan's passes are the sweep's");
static_assert(BOOST_MAX_TERMS == OTT_BOOST_MAX_TERMS && BOOST_MAX_QUERIES == OTT_BOOST_MAX_QUERIES && BOOST_SLOTS == OTT_MASK_SLOTS,
              "ott_boost_plan.h restates the header's constants");
static_assert(BOOST_SUM == OTT_BOOST_SUM && BOOST_MULT == OTT_BOOST_MULT && BOOST_VALUE == OTT_BOOST_VALUE && BOOST_LIN_DECAY == OTT_BOOST_LIN_DECAY &&
                  BOOST_MASK == OTT_BOOST_MASK,
              "ott_boost_plan.h restates the header's enums");
static_assert(BOOST_DT_INT32 == OTT_DT_INT32 && BOOST_DT_INT64 == OTT_DT_INT64 && BOOST_DT_FLOAT32 == OTT_DT_FLOAT32 && BOOST_DT_FLOAT64 == OTT_DT_FLOAT64 &&
                  BOOST_DT_DATETIME == OTT_DT_DATETIME,
              "ott_boost_plan.h restates the header's dtypes");
static_assert(sizeof(BoostTerm) == sizeof(ott_boost_term) && offsetof(ott_boost_term, origin) == 16 && offsetof(ott_boost_term, missing) == 24 &&
                  offsetof(ott_boost_term, reserved) == 28,
              "ott_boost_plan.h restates ott_boost_term");

struct BoostTermDev {
    const void* vals;       // VALUE, LIN_DECAY: the column's elements
    const uint64_t* nulls;  // ... and its NULL words, 1 = NULL; may be null
    const uint64_t* mask;   // MASK: the slot's words
    uint64_t mask_bits;     // ... and the rows they cover; rows at and beyond count as set
    double origin;
    float weight, scale, missing;
    uint32_t kind, dtype;
};
static_assert(sizeof(BoostTermDev) == 64, "eight of them ride in the kernel arguments");

struct BoostParams : SweepParams {
    unsigned long long* table;  // [NQ][n_rows] candidate key per (query of the pass, row); 0 = empty
    uint64_t n_rows;
    uint32_t cmp;
    float thr;
    float score_weight;
    uint32_t combine, n_terms;
    uint32_t terms_off;  // byte offset of `terms` in this struct: where the kernel finds them in its argument segment
    BoostTermDev terms[OTT_BOOST_MAX_TERMS];
};

template <typename T>
__device__ __forceinline__ double column_f64(const void* vals, uint64_t row);
template <>
__device__ __forceinline__ double column_f64<int32_t>(const void* vals, uint64_t row) { return (double)((const int32_t*)vals)[row]; }  // exact
template <>
__device__ __forceinline__ double column_f64<float>(const void* vals, uint64_t row) { return (double)((const float*)vals)[row]; }  // exact
template <>
__device__ __forceinline__ double column_f64<double>(const void* vals, uint64_t row) { return ((const double*)vals)[row]; }
template <>
__device__ __forceinline__ double column_f64<int64_t>(const void* vals, uint64_t row) { return __ll2double_rn(((const int64_t*)vals)[row]); }

template <int MK, int NQ>
__global__ __launch_bounds__(64 * SW_WAVES) void boost_sweep_kernel(BoostParams p) {
    typedef __attribute__((address_space(4))) const BoostTermDev* CTERM;
    typedef __attribute__((address_space(4))) const char* CCH;
    const CTERM terms = (CTERM)((CCH)__builtin_amdgcn_kernarg_segment_ptr() + p.terms_off);
    const bool take_max = p.take_max != 0;
    // `valid`: the row survived the composed row mask (and the tile's end); my_row < n_rows then
    sweep_tiles<MK, NQ>(p, [&](uint64_t my_row, bool valid, uint32_t, const float (&sc)[NQ], uint32_t nq_here) {
        float B = 0.0f;
        if (valid) {
            for (uint32_t j = 0; j < p.n_terms; j++) {  // in the caller's order; kind and dtype are wave-uniform
                const uint32_t kind = terms[j].kind;
                float g;
                if (kind == OTT_BOOST_MASK) {
                    const uint64_t* m = terms[j].mask;
                    g = 1.0f;  // rows at and beyond the slot's bit count: src/vec.rs:234
                    if (my_row < terms[j].mask_bits) g = ((m[my_row >> 6] >> (my_row & 63)) & 1) ? 1.0f : 0.0f;
                } else {
                    const void* vals = terms[j].vals;
                    const uint64_t* nulls = terms[j].nulls;
                    double x;
                    switch (terms[j].dtype) {
                        case OTT_DT_INT32: x = column_f64<int32_t>(vals, my_row); break;
                        case OTT_DT_FLOAT32: x = column_f64<float>(vals, my_row); break;
                        case OTT_DT_FLOAT64: x = column_f64<double>(vals, my_row); break;
                        default: x = column_f64<int64_t>(vals, my_row); break;  // Int64 / DateTime
                    }
                    const bool is_null = nulls != nullptr && ((nulls[my_row >> 6] >> (my_row & 63)) & 1);
                    g = __double2float_rn(__dsub_rn(x, terms[j].origin));  // the subtraction in f64, one rounding to f32
                    if (kind == OTT_BOOST_LIN_DECAY) {
                        const float u = __fdiv_rn(fabsf(g), terms[j].scale);
                        g = u >= 1.0f ? 0.0f : __fsub_rn(1.0f, u);  // a NaN u fails the comparison and gives NaN
                    }
                    if (is_null) g = terms[j].missing;
                }
                const float c = __fmul_rn(terms[j].weight, g);
                B = j == 0 ? c : __fadd_rn(B, c);
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            if ((uint32_t)q < nq_here) {
                const float sw = __fmul_rn(p.score_weight, sc[q]);
                float f = sw;
                if (p.n_terms != 0) f = p.combine == OTT_BOOST_SUM ? __fadd_rn(sw, B) : __fmul_rn(sw, __fadd_rn(1.0f, B));
                if (valid && !(f != f) && cmp_holds(f, p.cmp, p.thr))  // NaN dropped: vec_compute.rs:237
                    p.table[(size_t)q * p.n_rows + my_row] = ((unsigned long long)ord_of(f, take_max) << 32) | (uint32_t)(~(uint32_t)my_row);
            }
        }
    });
}

namespace {

int refuse(BoostRefusal r, uint32_t nq, uint32_t n_terms, uint32_t bad, const BoostTerm* terms) {
    return fail(boost_refusal_status(r), boost_refusal_text(r, nq, n_terms, bad, terms && bad < n_terms ? terms + bad : nullptr));
}

// The boosted sweep on a context whose `mu` the caller holds (and the owner's `rw`, shared).  k_eff = min(k, rows the chunk mask
// leaves) >= 1.  The columns and the slots are the owner's.
int run_boost_sweep(ott_store* s, const ott_query_desc* d, uint32_t combine, float score_weight, const BoostTerm* terms, uint32_t n_terms, uint64_t k_eff,
                    ott_hit* out, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats_out) {
    int rc;
    OTT_HIP(use_device(s));
    const ott_store* own = s->owner ? s->owner : s;
    const uint32_t nq = d->nq;
    const uint64_t n = s->n;
    const uint64_t t0 = now_ns();
    ott_stats st;
    BoostParams p{};
    uint32_t grid = 0;
    uint64_t total = 0;
    // (the descriptor's own mask — caller's or evaluated, live mask — is composed here)
    if ((rc = sweep_prologue(s, d, &st, &p, &grid))) return rc;
    if (grid != 0) {
        p.gid = nullptr;  // no group ids are read
        const uint32_t tile = nq == 1 ? 1u : SW_NQ;
        if ((rc = ensure_zeroed(s, s->d_gtable, s->gtable_clean, (size_t)tile * n * 8))) return rc;
        p.table = (unsigned long long*)s->d_gtable.p;
        p.n_rows = n;
        p.cmp = d->filter_cmp;
        p.thr = d->filter_thr;
        p.score_weight = score_weight;
        p.combine = combine;
        p.n_terms = n_terms;
        p.terms_off = (uint32_t)((const char*)p.terms - (const char*)&p);
        uint32_t column_dtype[OTT_BOOST_MAX_TERMS] = {};
        BoostTerm by_slot[OTT_BOOST_MAX_TERMS];  // the terms with `source` = their own position: boost_bytes_scanned reads column_dtype[source]
        for (uint32_t j = 0; j < n_terms; j++) {
            BoostTermDev& t = p.terms[j];
            t.kind = terms[j].kind;
            t.weight = terms[j].weight;
            t.scale = terms[j].scale;
            t.origin = terms[j].origin;
            t.missing = terms[j].missing;
            by_slot[j] = terms[j];
            by_slot[j].source = j;
            if (terms[j].kind == OTT_BOOST_MASK) {
                t.mask = (const uint64_t*)own->d_mslot[terms[j].source].p;
                t.mask_bits = own->mslot_bits[terms[j].source];
            } else {
                const Column& c = own->columns[terms[j].source];
                t.vals = c.d_vals;
                t.nulls = c.d_nulls;
                t.dtype = c.dtype;
                column_dtype[j] = c.dtype;
            }
        }

        GroupTopK tk;
        tk.n_groups = (uint32_t)n;  // (n < 2^32 - 16: boost_check_store)
        tk.nq = nq;
        tk.k = k_eff;
        tk.take_max = p.take_max != 0;
        if ((rc = tk.prepare(s, nullptr))) return rc;
        const bool timing = stats_out != nullptr;
        if (timing) OTT_HIP(hipEventRecord(s->ev[3], s->stream));
        const uint32_t passes = boost_passes(nq);
        for (uint32_t ps = 0; ps < passes; ps++) {
            p.q0 = ps * tile;
            const uint32_t nq_here = (nq - p.q0) < tile ? (nq - p.q0) : tile;
            if ((rc = launch_sweep(s->stream, p, tile, grid, OTT_SWEEP_KERNEL(boost_sweep_kernel)))) return rc;
            if ((rc = tk.pass(s, p.table, p.q0, nq_here))) return rc;
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
        st.bytes_scanned = boost_bytes_scanned(passes, st.vectors_compared / nq, s->dim, d->metric == OTT_METRIC_COSINE, by_slot, n_terms, column_dtype);
    }
    if (n_out) *n_out = total;
    st.total_ns = now_ns() - t0;
    if (stats_out) *stats_out = st;
    return OTT_OK;
}

}  // namespace

}  // namespace ott

using namespace ott;

extern "C" {

int ott_query_boost(ott_store* s, const ott_query_desc* d, uint32_t combine, float score_weight, const void* terms_in, uint32_t n_terms, ott_hit* out, uint64_t cap,
                    uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats) {
    const BoostTerm* terms = (const BoostTerm*)terms_in;
    if (!d) return fail(OTT_ERR_INVALID, "ott_query_boost: desc is NULL");
    // what the arguments alone decide comes first: these refusals need no store
    uint32_t bad = 0;
    BoostRefusal r = boost_check_args(d->nq, d->mode, d->path, combine, score_weight, terms, n_terms, &bad);
    if (r != BOOST_OK) return refuse(r, d->nq, n_terms, bad, terms);
    if (!s) return fail(OTT_ERR_INVALID, "ott_query_boost: store is NULL");
    int rc = validate_query(s, d);
    if (rc) return rc;
    const uint32_t nq = d->nq;
    if ((r = boost_check_store(s->multi != nullptr, 0, 0)) != BOOST_OK) return refuse(r, nq, n_terms, 0, terms);  // (the front of a multi-GPU store holds no rows)

    ott::host::SharedLock rd;  // the corpus, the columns and the slots cannot change while the call runs
    if ((rc = lock_store_shared(s, rd))) return rc;
    if ((r = boost_check_store(false, s->opt.tie_order, s->n)) != BOOST_OK) return refuse(r, nq, n_terms, 0, terms);
    {
        std::vector<uint64_t> column_rows(s->columns.size());
        for (size_t c = 0; c < s->columns.size(); c++) column_rows[c] = s->columns[c].n;
        if ((r = boost_check_sources(terms, n_terms, column_rows.data(), column_rows.size(), s->n, s->mslot_bits, &bad)) != BOOST_OK)
            return refuse(r, nq, n_terms, bad, terms);
    }
    RunPlan rp;
    make_run_plan(s, d->chunk_mask, rp);
    const uint64_t k_eff = d->k < rp.rows_scored ? d->k : rp.rows_scored;  // ott_query's rule with one query per list: a list never outgrows the pool
    if ((r = boost_check_cap(cap, nq, k_eff, s->n)) != BOOST_OK) return refuse(r, nq, n_terms, 0, terms);
    if (!out && cap) return fail(OTT_ERR_INVALID, "ott_query_boost: out is NULL");
    if (n_out) *n_out = 0;
    if (n_per_query) memset(n_per_query, 0, (size_t)nq * sizeof(uint64_t));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (k_eff == 0) return OTT_OK;  // k == 0 or nothing to score: a valid call with no hits

    {
        CtxLease lease(s);
        ott_store* ctx = lease.c;
        rc = run_boost_sweep(ctx, d, combine, score_weight, terms, n_terms, k_eff, out, n_out, n_per_query, stats);
        if (rc) (void)hipStreamSynchronize(ctx->stream);  // nothing of this call is in flight when the context is given back
    }
    return rc;
}

}  // extern "C"
