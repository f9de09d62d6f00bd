/*
 * otters_hip.h — C ABI of libotters_hip.so, the MI355X (gfx950) backend for the otters
 * exact-vector-search hot path.
 *
 * The reference (AtharvBhat/otters, Rust) has no FFI seam; this header defines the one a
 * patched otters would bind with an `extern "C"` block.  It replaces,
 * and only replaces:
 *
 *   VecStore::{new, add_vector, add_vectors, len}          src/vec.rs:346-384
 *   the body of VecQueryPlan::collect                      src/vec.rs:206-311
 *     (dot_product / cosine_similarity / euclidean_distance_squared  src/vec_compute.rs:9-54,
 *      filter_mask_bits :56-74, TopKCollector :76-294)
 *   the score + merge block of MetaQueryPlan::collect      src/meta.rs:671-709
 *     (process_chunk  src/meta_compute.rs:153-192, rayon fan-out src/meta.rs:678-691)
 *   GPU-side evaluation of build_row_mask_for_chunk        src/meta_compute.rs:194-289,
 *                                                          src/type_utils.rs:306-444, 587-736
 *
 * Everything above that (plan builders, validation + error strings, Expr::compile, zonemap
 * pruning build_chunk_mask_for_plan, result materialisation) stays in the host language.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function returns 0 on
 * success or a negative ott_status; ott_last_error() gives a thread-local message.  Input
 * pointers are borrowed for the duration of the call only.  The library owns all device
 * memory behind the opaque ott_store.  An ott_store lives on one GPU (ott_store_create) or spans
 * several GPUs of the host's one process (ott_store_create_multi: one shard per device, every call
 * below works on it unchanged); a multi-PROCESS job instead holds one single-GPU store per rank,
 * with different base offsets, and joins them with an ott_comm (ott_query_sharded).
 * Threading: queries (ott_query, ott_query_device, ott_merge_hits_device*) may be called on one
 * store from several host threads at once, like the reference's `&self` query (src/vec.rs:387):
 * overlapping calls run on separate streams with their own scratch.  Calls that change the
 * store (append*, reserve, write_rows, set_*, add_column, eval_row_mask, zone_stats) need and
 * take exclusive access (they wait for running queries).  A query that uses the device row
 * mask reads whatever the last ott_store_eval_row_mask left: pair the two calls under one
 * caller-side lock if several threads filter (the reference's MetaStore is !Sync, src/meta.rs:54).
 * Different stores are independent.
 */
#ifndef OTTERS_HIP_H
#define OTTERS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTT_ABI_VERSION 4

typedef enum {
    OTT_OK = 0,
    OTT_ERR_INVALID = -1, /* bad argument */
    OTT_ERR_HIP = -2,     /* HIP runtime failure (message has the hipError string) */
    OTT_ERR_OOM = -3,
    OTT_ERR_UNSUPPORTED = -4
} ott_status;

/* src/vec.rs:11-16.  MANHATTAN (L1: the sum of |q[i] - v[i]|, default take MIN) is an extension on the EXACT path only; its
 * summation order is the other metrics' (eight chains over chunks_exact(8), reduce_add, then the sequential remainder). */
typedef enum { OTT_METRIC_COSINE = 0, OTT_METRIC_EUCLIDEAN = 1, OTT_METRIC_DOT = 2, OTT_METRIC_MANHATTAN = 3 } ott_metric;
/* src/vec.rs:18-22 */
typedef enum { OTT_TAKE_MIN = 0, OTT_TAKE_MAX = 1 } ott_take;
/* src/vec.rs:24-31; NONE = no filter_criteria */
typedef enum { OTT_CMP_NONE = 0, OTT_CMP_LT = 1, OTT_CMP_GT = 2, OTT_CMP_LTE = 3, OTT_CMP_GTE = 4, OTT_CMP_EQ = 5 } ott_cmp;
/* src/expr.rs:83-91 */
typedef enum { OTT_OP_EQ = 0, OTT_OP_NEQ = 1, OTT_OP_LT = 2, OTT_OP_LTE = 3, OTT_OP_GT = 4, OTT_OP_GTE = 5 } ott_op;
/* src/type_utils.rs:11-19 (String columns stay host-side) */
typedef enum { OTT_DT_INT32 = 0, OTT_DT_INT64 = 1, OTT_DT_FLOAT32 = 2, OTT_DT_FLOAT64 = 3, OTT_DT_DATETIME = 5 } ott_dtype;

/* MERGED is the reference's semantics: one top-k over the flattened nq x n score matrix
 * (src/vec.rs:217-219).  PER_QUERY is an extension: k hits for each query. */
typedef enum { OTT_MODE_MERGED = 0, OTT_MODE_PER_QUERY = 1 } ott_mode;

/* Which scoring kernel family runs.  EXACT returns exactly what scoring every row in the reference's summation order returns
 * (one pass over the f32 rows per 4 queries); a single query may skip the last dims of rows that provably miss the top-k
 * (option "exact_prune": a bound on the rest of the dot product against a seed's k-th best).  That bound may use a per-row
 * sketch of the row's last dims (options "exact_sketch", "exact_sketch_bits": four bits per dim of everything behind the row's first
 * 32 dims, a half cell width and a remainder norm — 384 B beside a 3072-B row at dim 768, 1/8 of the store's HBM; or three bits per
 * dim of the last 5/8 of the row, 192 B; or one sign bit per dim of the last quarter, 32 B — made once when rows are appended and valid for every later query): per-row metadata of the same kind as the inverse norm, not a plane a query could be answered from — every returned row
 * is still finished over all of its f32 dims in the reference's summation order.  MFMA is the certified cascade, cosine / Euclidean / dot, k <= 484: candidate passes over compact copies of the corpus
 * — an int8 plane first (k <= 128: a quarter of the f32 bytes; batches on the matrix cores, a single cosine / dot query as a
 * streaming sweep), a 16-bit hi plane for what that cannot certify, split bf16 behind it — every candidate
 * re-scored in the reference's order, the top-k CERTIFIED against a measured error bound, uncertifiable queries recomputed on
 * EXACT — so both return the same bits.  AUTO: a cost model picks the cheaper one.  A single query takes EXACT (no copy of the
 * corpus is BUILT for the most common call) unless the cascade's first plane is already resident and covers every row (the
 * background build after appends, a batch query or ott_store_prepare_batch made it) and the store is large enough for a quarter
 * of the bytes to pay (~200k x 768 rows): then it takes the cascade, same bits.  Batches: 2+ queries on large stores, 5+
 * elsewhere — except small batches (up to 16 queries) on small stores (up to ~65k rows), which stay on EXACT while its
 * small-store kernel (8 queries per pass) is cheaper than the cascade's fixed cost.  MANHATTAN is EXACT only: AUTO sends it
 * there before the cost model runs (it never builds, extends or waits for a plane) and MFMA refuses it (OTT_ERR_UNSUPPORTED). */
typedef enum { OTT_PATH_AUTO = 0, OTT_PATH_EXACT = 1, OTT_PATH_MFMA = 2 } ott_path;

/* Horizontal-sum order of wide::f32x8::reduce_add (third-party, unpinned by the reference's tests; see
 * oracle/otters_oracle.h).  It follows the Rust build: AVX = ((l0+l4)+(l2+l6))+((l1+l5)+(l3+l7)), what the crate compiles to
 * under target_feature = "avx" (e.g. -C target-cpu=native); SEQ4 = (((l0+l1)+l2)+l3)+(((l4+l5)+l6)+l7), the two-f32x4
 * fallback of a default x86_64 build (the reference ships no .cargo/config.toml).  bindings/rust/patch/vec_hip.rs selects
 * it by cfg!(target_feature = "avx").  Default: AVX. */
typedef enum { OTT_REDUCE_AVX = 0, OTT_REDUCE_SEQ4 = 1 } ott_reduce;

/* SearchResult, src/vec.rs:34-38; `index` is the global row (shard base + local,
 * src/meta_compute.rs:185); `query` is informational (the reference drops it). */
typedef struct {
    uint64_t index;
    float score;
    uint32_t query;
} ott_hit;

typedef struct {
    const float* queries;       /* [nq * dim] row-major, host memory */
    uint32_t nq;
    uint32_t metric;            /* ott_metric */
    uint32_t take;              /* ott_take */
    uint32_t filter_cmp;        /* ott_cmp */
    float filter_thr;
    uint32_t mode;              /* ott_mode */
    uint64_t k;                 /* take_count */
    const uint64_t* chunk_mask; /* n_chunks bits, BitVec<usize,Lsb0> words; NULL = all chunks.
                                   Output of build_chunk_mask_for_plan, src/meta.rs:407-428 */
    const uint64_t* row_mask;   /* row_mask_bits bits over this store's LOCAL rows, 1 = keep;
                                   rows >= row_mask_bits are kept (src/vec.rs:234). NULL = none */
    uint64_t row_mask_bits;
    uint32_t use_device_row_mask; /* 1 = use the mask last built by ott_store_eval_row_mask */
    uint32_t path;              /* ott_path */
} ott_query_desc;

/* MetaQueryStats, src/meta.rs:832-842, plus device-side facts. */
typedef struct {
    uint64_t total_chunks, pruned_chunks, evaluated_chunks, vectors_compared;
    uint64_t prune_ns, score_ns, merge_ns, total_ns; /* score_ns / merge_ns: hipEvent time of the kernels (the pruned EXACT sweep of one
                                                        query on a store from 1 310 720 rows, k <= 64, no score filter, host output: score_ns
                                                        spans its whole chain, the merges included, and merge_ns is 0 — no event is
                                                        recorded inside the chain) */
    uint64_t bytes_scanned;     /* algorithmic: 4*dim*rows_scored (+4*rows_scored for cosine), per pass */
    uint32_t path_used;         /* ott_path */
    uint32_t passes;            /* corpus passes (EXACT path: ceil(nq / queries per pass)) */
    uint64_t rescored;          /* MFMA path: candidates re-scored in reference order.  EXACT path, pruned sweep of one query (host
                                   output): rows that passed the checkpoint and had their last stages read (of the rows behind the
                                   seed; where the seed is an estimate pass — the head form, k <= 64, no filter, stores from 1 310 720
                                   rows — of ALL rows, which the gated launch then covers: the few rows the estimate pass itself
                                   finished are not counted; 0 when the sweep was not pruned) */
    uint32_t retries;           /* MFMA path: queries no candidate pass could certify, recomputed on the exact path */
    uint32_t refined;           /* MFMA path: queries the hi pass (bf16 hi plane) could not certify, re-run through the split pass */
    float err_ratio_max;        /* MFMA path: max over the re-scored candidates of |approximate - exact score| / eps, eps the error bound
                                   the certification assumes for that query and pass.  <= 1 or the bound did not hold: see
                                   bound_violations */
    uint32_t gate_failed;       /* MFMA path: queries whose speculative emission threshold turned out too tight (fewer rows above it than
                                   the sample of rows seen so far suggested); answered by the next cascade level like any uncertified query */
    uint32_t bound_violations;  /* MFMA path: queries for which a re-scored candidate MEASURED |approximate - exact| > eps, i.e. the error
                                   bound the certification rests on did not hold (never observed; the matrix unit's accumulation order is
                                   not documented, so the library checks).  Such a query is treated as uncertified: next cascade level,
                                   finally the exact-order kernel — the result is the reference's either way */
    uint32_t i8_refined;        /* MFMA path: queries the int8 pass (the cascade's first level at k <= 128) could not certify,
                                   re-run through the hi pass (the field was `reserved` until round 5: same offset, same size) */
    uint64_t exchange_ns;       /* sharded queries (ott_query_sharded, a multi-GPU store): hipEvent time from the end of this GPU's own
                                   scoring to the start of the cross-GPU merge — the candidate exchange plus waiting for slower shards;
                                   merge_ns then includes the cross-GPU merge kernel */
} ott_stats;

/* One leaf of a compiled CNF filter (ColumnFilter::Numeric, src/expr.rs:199-205) bound to a
 * device-resident column; literal already coerced as src/meta_compute.rs:249-283 does. */
typedef struct {
    uint32_t column;  /* id returned by ott_store_add_column */
    uint32_t op;      /* ott_op */
    uint32_t clause;  /* leaves with the same clause id are OR-ed; clauses are AND-ed */
    uint32_t reserved;
    int64_t lit_i64;  /* for INT32 / INT64 / DATETIME columns */
    double lit_f64;   /* for FLOAT32 (narrowed to f32) / FLOAT64 columns */
} ott_leaf;

typedef struct ott_store ott_store;

int ott_abi_version(void);
const char* ott_last_error(void);
int ott_device_count(int* out);

/* VecStore::new, src/vec.rs:348-355.  `device` = HIP device ordinal. */
int ott_store_create(uint32_t dim, int device, ott_store** out);
/* The same store over SEVERAL GPUs of this process: one shard per entry of dev_ids, each holding a contiguous
 * range of chunks in row order (shard g holds lower rows than shard g + 1; ranges start on multiples of lcm(chunk size, 8)
 * rows).  Every function of this header that takes an ott_store works on it unchanged: appends / write_rows / read_rows /
 * add_column / eval_row_mask / zone_stats route by row range, and ott_query is the reference's own fan-out and merge
 * (src/meta.rs:678-709) with GPUs in place of rayon tasks — every shard scores its rows (chunk mask, row mask and metadata
 * columns sliced per shard), ONE exchange of fixed-size candidate blocks to the first shard's GPU, merge_hits_kernel there,
 * one host wait.  Results are bit-identical to the same rows in one single-GPU store (all metrics, k, modes, tie orders).
 * Exchange: a grouped ncclAllGather over one RCCL communicator per device (ncclCommInitAll) when the ordinals are distinct and
 * librccl loads; peer copies ordered by events otherwise (option "multi_transport": 0 automatic, 1 peer copies, 2 RCCL).
 * dev_ids may repeat an ordinal (several shards on one GPU: tests on a one-GPU box, or oversubscription) — then peer copies.
 * Layout: ott_store_reserve(n) plans the even split of n rows and appends fill it in order; without a plan rows go to the last
 * shard that has any and are moved between the GPUs before the next query (hipMemcpyPeerAsync; when a shard holds more than
 * 1.25x its even share; option "multi_rebalance" = 0 turns that off) — results never depend on where rows live.  Rows can no
 * longer move once metadata columns are resident: reserve, set the chunk size and append before ott_store_add_column.
 * Small stores stay on ONE GPU: a shard is brought in per "multi_min_shard_rows" rows (option / OTT_MULTI_MIN_SHARD_ROWS, default
 * 32768; 0 = always split evenly), the others stay empty; while one shard holds every row ott_query is that shard's own query —
 * no fan-out, no exchange (the fan-out over N GPUs costs 50-150 us per query, more than a 10k-row store's whole query).
 * Not on a multi-GPU store: ott_query_device, ott_merge_hits_device*, ott_query_sharded (OTT_ERR_UNSUPPORTED).
 * ott_store_device / ott_store_stream: the first shard's. */
int ott_store_create_multi(uint32_t dim, uint32_t n_dev, const int* dev_ids, ott_store** out);
/* The layout ott_store_reserve(n_rows) plans on a store of n_dev shards with this chunk size, without a store or a GPU: shard g
 * starts at out_first_rows[g] (a multiple of lcm(chunk_size, 8), clamped to n_rows) and ends where shard g + 1 starts (the last
 * one at n_rows; shards the store is too small for — "multi_min_shard_rows", read from the environment like a store created
 * now would — start at n_rows).  For hosts that slice their own per-row data the same way (and for the tests of the layout arithmetic). */
int ott_multi_plan(uint64_t n_rows, uint64_t chunk_size, uint32_t n_dev, uint64_t* out_first_rows);
/* Shards of a store (1 for a single-GPU store) and where shard `shard` lives: its device, its first row (counted from the
 * store's first row) and its row count.  Any out pointer may be NULL. */
int ott_store_shard_count(const ott_store* s);
int ott_store_shard_info(const ott_store* s, uint32_t shard, int* device, uint64_t* first_row, uint64_t* n_rows);
/* "none" (single-GPU store), "peer" or "rccl"; "undecided" before the first query of a multi-GPU store. */
const char* ott_store_transport(const ott_store* s);
int ott_store_destroy(ott_store* s);
/* Pre-size device storage for n_rows rows (avoids re-allocation while appending). */
int ott_store_reserve(ott_store* s, uint64_t n_rows);
/* VecStore::add_vectors, src/vec.rs:357-376: copy rows to HBM (row-major, host pointer)
 * and compute their inverse norms on the GPU in the reference's order.  Appends below 256 KB (VecStore::add_vector is one row
 * per call) are staged in pinned host memory and travel 4 MB at a time, and before anything looks at the rows (queries, reads,
 * columns, other kinds of append, ott_store_len counts them): a single-row append costs a memcpy, not a copy, a kernel and a
 * wait (measured 60 us -> under 1 us per row).  Option "stage_appends" = 0 sends every append at once. */
int ott_store_append(ott_store* s, const float* rows_host, uint64_t n_rows);
/* Same, rows already in device memory of this store's GPU ([n_rows*dim], dense). */
int ott_store_append_device(ott_store* s, const void* rows_dev, uint64_t n_rows);
/* Append synthetic rows: uniform [-1,1) (examples/demo.rs:4-7) from a counter-based
 * generator keyed (seed, global element index); bit-identical to oracle otto_rand_fill. */
int ott_store_append_random(ott_store* s, uint64_t n_rows, uint64_t seed);
/* Append synthetic CLUSTERED rows (the shape of real embedding corpora; what the batch path's cheapest candidate pass may
 * fail to certify): row r belongs to cluster hash(seed, r) % n_clusters, element c = centre[cluster][c] + spread * u * w(c),
 * u uniform [-1,1), centres uniform [-1,1), w(c) = 1 / (1 + aniso * c / dim) (aniso = 0: isotropic).  Counter-based, keyed by
 * the GLOBAL row; bit-identical to oracle otto_clustered_fill, so any row can be regenerated on the host. */
int ott_store_append_clustered(ott_store* s, uint64_t n_rows, uint64_t seed, uint32_t n_clusters, float spread, float aniso);
/* Overwrite existing rows [first, first+n) from host memory (tests plant known vectors). */
int ott_store_write_rows(ott_store* s, uint64_t first_row, const float* rows_host, uint64_t n_rows);
uint64_t ott_store_len(const ott_store* s);  /* VecStore::len, src/vec.rs:378 */
uint32_t ott_store_dim(const ott_store* s);
int ott_store_device(const ott_store* s);
/* Deleting rows (an extension: the reference's stores only grow).  A deleted row keeps its slot: row indices are stable, and
 * ott_store_len keeps counting every slot (cap and k arithmetic do not change); ott_store_live_len counts the rest.  A deleted
 * row is never scored into a result, on any path, mode, metric, k or tie order: a query returns exactly the hits it would
 * return with nothing deleted and a row mask that ALSO clears the deleted rows — ANDed with the caller's own row_mask or with
 * what ott_store_eval_row_mask left (which is not modified).  Stats fields may differ, hits may not.  The deleted set is a live
 * mask in HBM that belongs to the store (allocated by the first delete; a store that never had one runs exactly what it ran
 * before) and joins every query at the one place the row mask reaches the kernels; the exact kernel never reads a tile whose
 * rows are all masked.  Appended rows are live; ott_store_write_rows on a deleted row writes the data and leaves it deleted;
 * restore brings a row back exactly as it was (data, inverse norm and sketch line are kept while it is deleted).
 * rows_host: n indices counted from the store's first row (like row_mask: not base_offset-shifted).  Listing a row twice, or
 * one already in that state, is not an error: *n_changed (may be NULL) = rows whose state changed.  An index >= ott_store_len
 * fails with OTT_ERR_INVALID before anything changes.  Both take the store exclusively, like append (staged appends go first).
 * Multi-GPU store: routed by row range, like ott_store_write_rows. */
int ott_store_delete_rows(ott_store* s, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed);
int ott_store_restore_rows(ott_store* s, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed);
uint64_t ott_store_live_len(const ott_store* s);
/* (len+63)/64 words, bit = 1: live; bits past len are 0.  For tests / hosts that mirror the state. */
int ott_store_read_live_mask(const ott_store* s, uint64_t* out_host);
/* Physically removes the deleted rows, order preserved: len becomes live_len, and HBM behind it is free for appends again.
 * out_new_index (may be NULL): old-len entries, the row's new index or UINT64_MAX for a removed row.  Rows, inverse norms and
 * flags move in place through a bounded bounce buffer (no second copy of the store); sketch lines are made again (the same bits
 * a fresh store of the surviving rows has), the cascade's planes are dropped and rebuilt on demand, the evaluated row mask is
 * forgotten, the live mask is freed.  With nothing deleted it does nothing.  Takes the store exclusively.
 * OTT_ERR_UNSUPPORTED on a multi-GPU store (the shards' row ranges are pinned to chunk multiples) and while metadata columns
 * are resident (they would have to move with the rows: the restriction of ott_store_create_multi's rebalancing). */
int ott_store_compact(ott_store* s, uint64_t* out_new_index);
/* MetaStore chunking: chunk c = local rows [c*chunk_size, ...) (src/meta.rs:203-281).  Default 1024. */
int ott_store_set_chunk_size(ott_store* s, uint64_t chunk_size);
/* The certified cascade (query batches; single queries once its first plane is resident) keeps compact copies of the corpus in
 * HBM: the INT8 plane (every row as int8 with one f32 scale: a QUARTER of the f32 rows; every metric at k <= 128), the hi plane
 * (every element as an IEEE half — or bf16, option "hi_fmt" — HALF the size of the f32 rows; built only once a query needs it:
 * k > 128, or what the int8 level could not certify) and, only once a query falls through the hi pass's
 * certification too, the batch image (every row pre-split into bf16 hi + bf16 lo, the SAME size as the f32 rows).  All are
 * extended after appends, refreshed by write_rows, dropped by a reallocation (and FIRST, when the new rows would not fit next to
 * them), and skipped on their own when HBM has no room (the cascade then starts further down and splits the rows in registers).
 * enabled = 0 frees them and keeps them off; 1 (the default) allows them again.  Results never depend on them. */
int ott_store_set_batch_image(ott_store* s, int enabled);
/* Builds (or extends after appends) the cascade's first plane now instead of inside the first batch query (~5 ms per 30 GB of
 * rows for the int8 plane).  Optional: queries do it on demand.  Takes the store like a query does (shared). */
int ott_store_prepare_batch(ott_store* s);
/* 1 when the cascade's first plane exists and covers every row (the next batch query starts scoring at once), else 0.  With option
 * "hi_prebuild" (-1 automatic: stores of 262144 rows and more while the plane takes at most a quarter of the free HBM; 0 never;
 * 1 always) the plane is built or extended in the background right after every append, so a host that loads and then queries
 * normally finds it ready without calling ott_store_prepare_batch. */
int ott_store_batch_ready(const ott_store* s);
/* Rows that the pruned exact sweeps of this store (option "exact_prune") have finished in f32 after their checkpoint so far, a
 * running total over all queries and query contexts with host output (a multi-GPU store: over its shards).  Without the int8
 * check of the survivors (option "exact_i8_check") a query adds what it adds to ott_stats.rescored; with it, the rows that the
 * int8 plane could not rule out, a small part of that.  A measurement aid: results never depend on it. */
uint64_t ott_store_exact_finished(const ott_store* s);

/* Behaviour switches of one store.  The library reads the environment exactly once per store, in ott_store_create
 * (OTT_<NAME>=<int> presets the option of the same name); after that only this call changes them — the query path never calls
 * getenv.  Twenty-six options (round 5 retired the rest: experiment switches whose measurements are in DESIGN.md 3.4 and profiles/dead_ends_rounds_2_4.md).
 * Behaviour a host may want:
 *   "tie_order"  0 (default): canonical total order — better score, lower row, lower query.  1: the reference's own outcome at
 *                exact score ties, ONE TopKCollector over the store (VecStore, src/vec.rs:217-310, src/vec_compute.rs:236-277).
 *                2: one collector per chunk, then concat-sort-truncate (MetaStore, src/meta.rs:678-709), for any chunk size
 *                (src/meta.rs:86-89).  Signed zeros follow the collector too: a pair is admitted by IEEE comparison with the
 *                k-th score (-0.0 == +0.0) and placed by total order (+0.0 above -0.0).  See INTEGRATION.md 6a.
 *   "hi_fmt"     which compact copies of the corpus the cascade keeps: -1 (default) / 2: an INT8 plane as its first level (one f32
 *                scale per row, a quarter of the f32 bytes; k <= 128) with an IEEE-half plane behind it that is built
 *                only once a query needs it (k > 128, or what the int8 level could not certify); 1: the half plane
 *                alone (11 significant bits; falls back to bf16 by itself on stores whose row norms spread over many binades);
 *                0: a bf16 plane alone.  Takes effect when a plane is (re)built.
 *   "hi_prebuild"  -1 (default) automatic / 0 never / 1 always: the hi plane is built in the background after appends
 *                (ott_store_batch_ready).   "stage_appends"  0: every append goes to the GPU at once (default: small ones are staged).
 *   "multi_transport", "multi_rebalance", "multi_min_shard_rows": the multi-GPU store, see ott_store_create_multi.
 * Which of several equivalent paths runs (results never depend on them; the tests hold each to the oracle):
 *   "exact_small" (-1 auto / 0 streaming kernel / 2 rows8, eight lanes per row: which kernel answers on a small store),
 *   "exact_prune" (-1 auto, from 2^20 rows and dim 225 / 0 off / 1 forced: a single cosine / dot query on EXACT scores a tenth of
 *   the rows first, then skips the last eighth of the dims of rows whose score bound misses that seed's k-th best),
 *   "exact_sketch" (-1 auto: stores of dim >= 225 / 0 never / 1 always: the store keeps the pruned sweep's tail sign sketch — per
 *   row the sign bits of the last quarter of its 32-dim stages, the mean of their magnitudes and an upper bound of the norm of
 *   what the two leave out; 32 B per row at dim 768, computed behind the inverse norms on every append — and the sweep then
 *   stops a row after three quarters of its dims instead of seven eighths.  Set it before rows are appended: switched on later,
 *   the sketch is made at the next append; a store without one takes the 7/8 form),
 *   "exact_sketch_bits" (4, the default / 3 / 1: the sketch's form, read when the store makes its first line.  4 = a four-bit code per
 *   dim of every 32-dim stage but the first, a half cell width and the remainder norm: 384 B per row at dim 768, 1/8 of the row
 *   bytes — 3.84 GB of HBM beside a 30.7-GB store of 10M rows, and nearly two reads of the row when it is appended — and the sweep
 *   stops a row after its first 32 dims; 3 = a three-bit code per dim of the last 5/8 of the stages: 192 B per row at dim 768, 1/16
 *   of the row bytes, 1.92 GB at 10M rows, and the sweep stops a row after three eighths of its dims; 1 = the sign sketch above,
 *   32 B per row),
 *   "exact_sketch_head" (-1, the default, and 1: wherever the store keeps four-bit lines it keeps a head beside them — per row the
 *   four-bit codes of the first 32 dims and the norm of what all codes leave out, 20 B per row, 0.2 GB at 10M rows, made with the
 *   lines — and the sweep then reads no f32 dims of a row whose bound misses the gate; 0 = never: the sweep reads the first 32 dims
 *   of every row, as on a store without a head.  The sweep reads the option on every query: set to 0, the very next query reads the
 *   first 32 dims again, whether the store still holds a head or not.  The head itself is dropped, or made for every row, at the
 *   next append after a switch, so switched back on the option shows from that append.  Lists of k > 256 always take the sweep
 *   without a head: the head kernel's registers leave one wave per SIMD there, and it measured slower),
 *   "exact_i8_check" (-1, the default, and 1: in the sweep without f32 dims in front, k <= 64, a row whose four-bit bound reaches the
 *   gate is first scored on the cascade's int8 plane — a quarter of its bytes — and its f32 dims are read only unless that score plus
 *   the int8 level's certified error still ranks below the gate; 0 = never.  Only while that plane exists and covers every row
 *   (ott_store_batch_ready on a store whose first plane is the int8 one): asking builds nothing.  Hits and ott_stats.rescored are
 *   the same either way; ott_store_exact_finished counts the rows whose f32 dims were read),
 *   "id_gather" (-1 auto: lists of up to 10000 ids / 0 never / 1 wherever eligible: whether ott_query_ids scores the listed rows with the gather kernel or
 *   turns the list into a row mask and takes ott_query's paths),
 *   "group_gather" (-1 auto: lists whose groups hold up to 1000000 rows / 0 never / 1 wherever eligible: whether ott_query_maxsim_groups
 *   scores the listed groups' rows with the gather kernel, through the store's group-to-rows index, or turns the list into a row mask
 *   and runs ott_query_maxsim's sweep; environment preset OTT_GROUP_GATHER, as for every option),
 *   "masks_sweep" (2 auto, the default / 0 always by mask group / 1 the masks sweep wherever eligible: which route answers
 *   ott_query_masks; environment preset OTT_MASKS_SWEEP),
 *   "fuse_device" (-1 auto, the default: the host route / 0 never / 1 wherever eligible: whether ott_query_fuse's first stage leaves the legs' lists
 *   in HBM for the fuse kernel or returns them to the host first; environment preset OTT_FUSE_DEVICE),
 *   "sparse_table" (-1 auto, the default / 0 the LDS form wherever eligible / 1 always the device table: where ott_query_sparse's
 *   kernel looks the query's weights up; environment preset OTT_SPARSE_TABLE),
 *   "sparse_df_lds" (-1 auto, the default / 0 global atomic adds / 1 a histogram in LDS wherever the vocab fits: how
 *   ott_store_sparse_df's kernel counts; environment preset OTT_SPARSE_DF_LDS),
 *   "binary_gate" (-1 auto, the default / 0 always the key table / 1 the gated sweep wherever eligible: which route answers
 *   ott_query_binary; environment preset OTT_BINARY_GATE), "binary_gate_cap" (0, the default: the plan's pair capacity; otherwise
 *   the gated sweep's capacity in pairs: tests reach the overflow branch with it),
 *   "large_k_from" (k above which host-output queries take the sort path; 0 = default: 512 for one query or a small store,
 *   128 for several queries on a large one), "small_sort" (0: results of up to 16384 (row, query) pairs with k > 512 through
 *   the radix sort instead of the rank sort), "mfma_f32" (batch path: one candidate pass on the f32 matrix pipe),
 *   "no_hi_pass" (batch path starts at the split-bf16 pass), "no_batch_image" (no 16-bit copies of the corpus).
 * Tests only:
 *   "force_fallback"  bit mask of code paths the library otherwise takes only in rare conditions: 1 block lists merged by
 *                insertion, 2 k <= 64 through sorted heads + tree fold, 4 the 256-query blocks of a row tile one after the other,
 *                8 the sort path without its prefix gate, 16 the open first round through cursor atomics, 32 conservative
 *                emission thresholds between the row rounds, 64 the sort path in slices of 2^14 (row, query) pairs.
 *   "eps_scale_ppm"  the batch path's error bound multiplied by this many millionths, to show that a violated bound is noticed.
 *   "multi_fake_distinct"  (environment only, at creation) every shard of a multi-GPU store counts as a device of its own.
 * Kernel tuning and timing ablations ("mfma_wg", "mfma_growth", "mfma_abl", "mfma_debug", "hi_tmin", and each fallback bit under
 * its own name) exist by name only in a library built with -DOTT_MFMA_DEBUG_BUILD.
 * Takes the store exclusively, like append. */
int ott_store_set_option(ott_store* s, const char* name, int64_t value);

/* Global index of local row 0 (shard base for multi-GPU; src/meta_compute.rs:185). */
int ott_store_set_base_offset(ott_store* s, uint64_t base);
int ott_store_set_reduce_order(ott_store* s, uint32_t reduce /* ott_reduce */);
/* Read back for tests / debugging. */
int ott_store_read_rows(const ott_store* s, uint64_t first_row, uint64_t n_rows, float* out_host);
int ott_store_read_inv_norms(const ott_store* s, uint64_t first_row, uint64_t n_rows, float* out_host);

/* Metadata columns resident in HBM for GPU-side row-mask evaluation
 * (src/col.rs storage: values + BitVec null mask, 1 = NULL).  values: n elements of the
 * dtype; nulls may be NULL.  n must equal the store length. */
int ott_store_add_column(ott_store* s, uint32_t dtype, const void* values_host, const uint64_t* nulls,
                         uint64_t n, uint32_t* out_column_id);
/* Zone statistics of an HBM-resident column for every chunk of `chunk_size` rows at once
 * (build_zone_stat_for_range, src/meta_compute.rs:41-98, 117-130): min / max over the non-null
 * rows and the non-null count.  Integer / datetime columns: out_min / out_max are int64[n_chunks]
 * (i64::MAX / i64::MIN for an all-null chunk); float columns: double[n_chunks] (+inf / -inf;
 * f64::min/max semantics: a NaN value is ignored).  out_non_null: uint64[n_chunks].  Host pointers. */
int ott_store_zone_stats(ott_store* s, uint32_t column, uint64_t chunk_size, void* out_min, void* out_max,
                         uint64_t* out_non_null);

/* build_row_mask_for_chunk over all rows at once (src/meta_compute.rs:194-232): CNF of
 * numeric leaves -> device row mask used by queries with use_device_row_mask = 1.
 * If out_host != NULL the mask words ((len+63)/64) are also copied back. */
int ott_store_eval_row_mask(ott_store* s, const ott_leaf* leaves, uint32_t n_leaves, uint32_t n_clauses,
                            uint64_t* out_host);

/* The hot path: VecQueryPlan::collect body (src/vec.rs:206-311) / MetaQueryPlan::collect
 * score+merge (src/meta.rs:671-709).  Writes up to `cap` hits, best first; *n_out = count.
 * cap must be >= min(k, rows*nq) (MERGED) or nq*min(k, rows) (PER_QUERY; hits grouped by
 * query, each group best first, *n_out = total, per-query counts in n_per_query if non-NULL). */
int ott_query(ott_store* s, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out,
              uint64_t* n_per_query, ott_stats* stats);

/* Candidate id lists (an extension; FAISS has IDSelectorArray, Qdrant has_id): rank only the listed rows.  ids: n_ids row indices
 * counted from the store's first row (like row_mask and ott_store_delete_rows: not base_offset-shifted), in any order, duplicates
 * allowed.  The query returns exactly the hits — index, score bits, order, per-query counts — that ott_query returns with a row
 * mask that keeps only the listed rows, ANDed with the caller's row_mask or the evaluated device mask, with the live mask of
 * deleted rows and with chunk_mask: every metric, mode, take, filter, k and tie order.  Stats fields may differ, hits may not.
 * cap need only be min(k, n_unique * nq) (MERGED) or nq * min(k, n_unique) (PER_QUERY).  An id >= ott_store_len, or ids == NULL
 * with n_ids > 0, fails with OTT_ERR_INVALID before any device work; n_ids == 0 is a valid query with no hits.
 * The work follows the list, not the store: a gather kernel scores the listed rows (eight lanes per row, the reference's summation
 * order) where it is eligible — canonical tie order, k <= 128, at most 65536 distinct ids, at most 16 queries of at most 2048
 * floats, path AUTO or EXACT, a single-GPU store; stats: path_used = EXACT, vectors_compared = listed rows after unique, chunk mask
 * and row mask (x nq), bytes_scanned = their bytes per pass.  Everything else turns the list into a row mask on the device (a
 * multi-GPU store: on the host) and runs ott_query's own paths with it.  Option "id_gather" chooses.  Takes the store shared,
 * like ott_query (staged appends go first). */
int ott_query_ids(ott_store* s, const ott_query_desc* d, const uint64_t* ids, uint64_t n_ids, ott_hit* out, uint64_t cap,
                  uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);
/* Raw scores of given rows: out_scores[q * n_ids + i] = the f32 score of query q against row ids[i] — the exact path's and the
 * oracle's bits, entries in the list's order, duplicates allowed, no filter, no top-k, a NaN score returned as NaN.  It reads stored
 * data, as ott_store_read_rows does: a DELETED row's score is returned like any other.  Any number of ids (launches of 65536);
 * rows of at most 2048 floats.  Errors as ott_query_ids.  Takes the store shared. */
int ott_store_score_rows(ott_store* s, const float* queries, uint32_t nq, uint32_t metric, const uint64_t* ids, uint64_t n_ids,
                         float* out_scores);

/* Batch search with a row mask per query (an extension; a metadata filter per request: Qdrant's search_batch, FAISS's per-query
 * IDSelector).  masks: n_masks host masks back to back, each (mask_bits + 63) / 64 words of BitVec<usize, Lsb0>, 1 = keep.
 * mask_of_query points at d->nq uint32_t (declared const void*, as the group ids are): [b] < n_masks names a host mask,
 * OTT_MASK_SLOT_BASE + slot a device mask slot (below), OTT_NO_MASK no mask of its own.  d->mode must be OTT_MODE_PER_QUERY.
 * Query b's hits are exactly the hits ott_query returns for that query alone — index, score bits, order and count — with the same
 * descriptor and a row mask equal to the descriptor's own mask (row_mask or use_device_row_mask, joined with the live mask of
 * deleted rows and chunk_mask, as in ott_query) ANDed with mask mask_of_query[b]: every metric, take, filter, k, path and tie order.
 * Rows at or beyond a mask's bit count are kept (src/vec.rs:234).  hit.query is b; the lists come out in the caller's query order,
 * their lengths in n_per_query; cap follows ott_query's PER_QUERY rule (nq * min(k, rows)).  Stats may differ from the per-query
 * calls, hits may not.
 * Two routes, the same bits.  BY MASK GROUP serves everything: under one shared lock, one PER_QUERY run of ott_query's own
 * internals per distinct mask id with all of that mask's queries (so queries that share a mask get the batch paths), the mask
 * joined where every row mask reaches the kernels.  THE MASKS SWEEP (canonical tie order, path AUTO or EXACT, a single-GPU store
 * of fewer than 2^32 - 16 rows): the queries are ordered stably by mask id and swept four per pass; all masks are on the device
 * (host masks in one upload, slots in place); per pass a small kernel writes common AND (m0 OR m1 OR m2 OR m3) as the pass's row
 * mask, so a tile in which no query of the pass has a surviving row is never read; the sweep's epilogue tests each query's own
 * mask bit and stores the candidate key into a table of 4 x rows 8-byte slots (scratch of the query context); grouped search's
 * top-k takes each query's list from the table; one host wait for the whole batch.  Option "masks_sweep" chooses: 0 = always by
 * mask group, 1 = the sweep wherever eligible, 2 (default) = auto (ott_masks_plan.h: measured constants).
 * Refused with OTT_ERR_INVALID before any device work, with nothing written: d->nq of 0 or above OTT_MASKS_MAX_QUERIES,
 * OTT_MODE_MERGED, mask_of_query NULL, masks NULL with n_masks > 0, an entry at or above n_masks that is neither a slot
 * reference nor OTT_NO_MASK, a reference to a slot at or above OTT_MASK_SLOTS or to one that was never filled (or was dropped
 * since), and what ott_query refuses.  A multi-GPU store is answered by mask group with host masks (use_device_row_mask together
 * with a per-query mask is OTT_ERR_UNSUPPORTED there).  Takes the store shared, like ott_query (staged appends go first).
 *
 * Device mask slots: OTT_MASK_SLOTS row masks resident in HBM beside the single mask of ott_store_eval_row_mask (which they never
 * touch), so a filter evaluated on the GPU never travels to the host and back.  eval: ott_store_eval_row_mask's kernel and
 * semantics, written into slot `slot` (out_host, if given, receives the words too).  write: n_bits bits of a host mask into the
 * slot (n_bits == 0 empties it).  clear: every slot is emptied.  A slot covers the rows the store had when it was filled (rows
 * appended later are kept, as with any mask); every slot is dropped when the rows are reallocated or compacted or a shard adopts
 * moved rows.  All three take the store exclusively, like ott_store_eval_row_mask; slot >= OTT_MASK_SLOTS is OTT_ERR_INVALID; on
 * a multi-GPU store they return OTT_ERR_UNSUPPORTED. */
#define OTT_NO_MASK 4294967295u        /* 0xFFFFFFFF: mask_of_query[b] = no mask of its own */
#define OTT_MASK_SLOT_BASE 2147483648u /* 0x80000000: mask_of_query[b] = OTT_MASK_SLOT_BASE + slot, a device slot */
#define OTT_MASK_SLOTS 64
#define OTT_MASKS_MAX_QUERIES 1024
int ott_query_masks(ott_store* s, const ott_query_desc* d, const uint64_t* masks, uint32_t n_masks, uint64_t mask_bits,
                    const void* mask_of_query /* uint32_t[d->nq] */, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                    ott_stats* stats);
int ott_store_eval_row_mask_slot(ott_store* s, uint32_t slot, const ott_leaf* leaves, uint32_t n_leaves, uint32_t n_clauses,
                                 uint64_t* out_host);
int ott_store_write_row_mask_slot(ott_store* s, uint32_t slot, const uint64_t* bits, uint64_t n_bits);
int ott_store_clear_row_mask_slots(ott_store* s);

/* Score boosting (an extension; Qdrant's score boosting / formula queries, Elasticsearch's function_score): rank by a formula of
 * the score and metadata columns.  It cannot be built on top of take(k): a boost lifts rows that were never among the best k by raw
 * score, so the formula is applied to EVERY candidate row, in one more streaming sweep.  terms points at n_terms ott_boost_term
 * (declared const void*, as the group ids and mask_of_query are).
 * THE FINAL SCORE.  Every candidate row r and query b get a final score F; all of it IEEE f32, round to nearest even, nothing
 * fused, no flush to zero.  S = the row's score with query b: the exact path's bits.  Sw = fl(score_weight * S).  For each term j,
 * in the caller's order, a value g_j:
 *   VALUE      a NULL row: g_j = missing; otherwise g_j = (float)((double)x - origin), x the column's element (INT32, INT64,
 *              DATETIME, FLOAT32, FLOAT64 each to double by the IEEE conversion), the subtraction in f64, ONE rounding to f32;
 *   LIN_DECAY  a NULL row: g_j = missing; otherwise, with t VALUE's result and u = fl(|t| / scale): g_j = (u >= 1) ? +0.0f :
 *              fl(1 - u); a NaN u gives NaN;
 *   MASK       g_j = 1.0f where the slot's bit for the row is set, and for rows at or beyond the slot's bit count (the rule every
 *              mask follows, src/vec.rs:234); otherwise 0.0f.
 * c_j = fl(weight_j * g_j); B = c_0, then B = fl(B + c_j) for j = 1 ...  With n_terms == 0, F = Sw; with OTT_BOOST_SUM,
 * F = fl(Sw + B); with OTT_BOOST_MULT, F = fl(Sw * fl(1.0f + B)).
 * CANDIDATES AND ORDER.  The candidates are the rows that survive chunk_mask, the descriptor's row mask (the caller's or the
 * evaluated device mask) and the live mask of deleted rows, exactly as in ott_query.  A row whose F is NaN is dropped; the filter
 * (filter_cmp, filter_thr) acts on F; the hits are ordered by F under `take`, equal F by the lower row — ott_query's canonical
 * order, signed zeros included.  hit.score = F, hit.query = b.  d->mode: OTT_MODE_PER_QUERY, or OTT_MODE_MERGED with nq == 1; cap
 * is at least nq * min(k, rows).  With n_terms == 0 and score_weight == 1.0f the hits are exactly ott_query's on OTT_PATH_EXACT
 * with the canonical tie order: index, score bits, order and count.
 * Refused on the host before any device work, each with its own message (ott_boost_plan.h).  OTT_ERR_INVALID: nq == 0 or above
 * OTT_BOOST_MAX_QUERIES; MERGED with nq > 1; n_terms above OTT_BOOST_MAX_TERMS; terms NULL with n_terms > 0; an unknown combine
 * or kind; reserved != 0; a score_weight, weight, origin or missing that is not finite; a LIN_DECAY scale that is not finite or
 * <= 0; an unknown column id, or a column whose length differs from the store's; a slot at or above OTT_MASK_SLOTS, or an empty
 * one; cap too small; and what ott_query refuses.  OTT_ERR_UNSUPPORTED: OTT_PATH_MFMA (AUTO takes the sweep and never builds,
 * extends or waits for a plane); tie_order 1 or 2; a multi-GPU store; a store of 2^32 - 16 rows or more; k_eff > 512 with more
 * than 2^26 (query, row) pairs.  Takes the store shared, like ott_query (staged appends go first); worker contexts serve
 * concurrent callers.  Stats: path_used = OTT_PATH_EXACT, passes = ceil(nq / 4), vectors_compared as in the masks sweep,
 * bytes_scanned its figure plus, per row and pass, the element sizes of the VALUE and LIN_DECAY columns. */
#define OTT_BOOST_MAX_TERMS 8
#define OTT_BOOST_MAX_QUERIES 1024
typedef enum { OTT_BOOST_SUM = 0, OTT_BOOST_MULT = 1 } ott_boost_combine;
typedef enum { OTT_BOOST_VALUE = 0, OTT_BOOST_LIN_DECAY = 1, OTT_BOOST_MASK = 2 } ott_boost_kind;
typedef struct {
    uint32_t kind;      /* ott_boost_kind */
    uint32_t source;    /* VALUE, LIN_DECAY: column id of ott_store_add_column; MASK: device mask slot */
    float    weight;
    float    scale;     /* LIN_DECAY: finite, > 0; otherwise 0 */
    double   origin;    /* VALUE, LIN_DECAY: subtracted from the value, in f64 */
    float    missing;   /* VALUE, LIN_DECAY: g of a NULL row */
    uint32_t reserved;  /* 0 */
} ott_boost_term;       /* 32 bytes, offsets 0 4 8 12 16 24 28 */
int ott_query_boost(ott_store* s, const ott_query_desc* d, uint32_t combine, float score_weight,
                    const void* terms /* ott_boost_term[n_terms] */, uint32_t n_terms,
                    ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);

/* Rank fusion (an extension; Qdrant's fusion queries over prefetches, Elasticsearch's rrf retriever, Weaviate's hybrid fusion):
 * several queries' hit lists become ONE ranking per request, by reciprocal rank fusion (OTT_FUSE_RRF), distribution-based score
 * fusion (OTT_FUSE_DBSF) or min-max "relative score" fusion (OTT_FUSE_MINMAX).  The normative statement is the numpy model
 * tests/fuse_ref.py; ott_fuse_plan.h states the same formulas in C.
 * LAYOUT (ott_query_maxsim_groups_batch's convention).  d->queries holds the legs of request 0, then of request 1, ...; d->nq is
 * their total; legs_per_request[b] (uint32_t, declared const void* as the group ids are) says how many belong to request b.  The
 * whole call shares the metric, the take, the filter, the chunk mask, the row mask (the caller's or the device mask), the live
 * mask and the path.  d->k = fused hits per request; d->mode must be OTT_MODE_PER_QUERY.
 * A LEG'S LIST is exactly what ott_query returns for that one query vector with k = min(fetch, rows), PER_QUERY, everything else of
 * d unchanged: rows, score bits and order, on every path and tie order.  The filter acts on the leg's score: it is part of the leg.
 * Positions are r = 0, 1, ...; a list may be shorter than fetch, or empty.
 * CONTRIBUTION of the entry at position r with score s in leg l, w = leg_weights[l] (1 when leg_weights is NULL):
 *   RRF     c = w / (rrf_k + (float)(r + 1)): one f32 addition, then one f32 division, each rounded to nearest.
 *   MINMAX  best, worst = the list's first and last score (it is best first under d->take), taken to f64; span = best - worst
 *           under OTT_TAKE_MAX, worst - best under OTT_TAKE_MIN.  If !(span > 0) every entry of the list gets nrm = 0.5f; otherwise
 *           nrm = (float)(dist / span) with dist = s - worst (Max) or worst - s (Min), s in f64, every operation a rounded f64 one,
 *           nothing fused.  c = w * nrm, one f32 multiplication.
 *   DBSF    the same with worst = mean - 3 sigma (Max) or mean + 3 sigma (Min) and span = (mean + 3 sigma) - (mean - 3 sigma); dist may
 *           be negative or exceed span: there is no clamp.  mean and the population variance are f64 sums over the list in ONE order:
 *           partial t (0 <= t < 64) adds the terms at positions t, t + 64, t + 128, ... ascending from +0.0; then p[t] += p[t + h] for
 *           h = 32, 16, 8, 4, 2, 1; p[0] is divided by n.  The variance's terms are (s - mean) * (s - mean), a rounded f64 product of
 *           a rounded f64 difference; sigma is the correctly rounded f64 square root; 3 sigma one f64 product.
 * FUSED SCORE of a row in request b: F = +0.0f, then over b's legs in ascending order, for every leg whose list holds the row,
 * F = F + c, one rounded f32 addition each.  A row absent from a leg's list gets nothing from that leg.
 * RANKING: F descending whatever d->take is, equal F to the lower row; a row whose F is NaN is dropped (as ott_query_boost does).
 * Request b returns min(k, rows with a non-NaN F) hits, score = F, index = the global row, query = b; the lists come out back to
 * back in request order, n_per_request[b] holds their lengths, *n_out their sum.  cap is at least the sum over b of
 * min(k, legs_b x min(fetch, ott_store_len)).
 * The first stage runs through ott_query's own internals on one query context.  On the device route its hits stay in HBM as
 * sentinel-padded blocks and never travel (one host wait per call on the EXACT path); on the host route they come back, are
 * staged in pinned memory and go up in one copy (tie orders 1 and 2 always take it).  Store option "fuse_device": -1 automatic
 * (the host route: the device route measured no faster than the first stage's own spread, profiles/fuse/README.md), 0 never, 1
 * wherever eligible; both routes run the same kernel and give the same bits.  The kernel: one workgroup per request,
 * one launch per call; a bitonic sort of 64-bit keys (local row << 13 | leg << 9 | position) in LDS brings a row's entries together in
 * leg order, the head of each run adds them serially (no atomics), a second sort ranks by F.  12 B of LDS per padded entry.
 * Refused on the host before any device work, with nothing written, each with its own message (ott_fuse_plan.h).
 * OTT_ERR_UNSUPPORTED: a mode other than PER_QUERY; a multi-GPU store; a store of 2^51 rows or more.  OTT_ERR_INVALID: n_requests
 * 0 or above OTT_FUSE_MAX_REQUESTS; legs_per_request NULL; fetch 0 or above OTT_FUSE_MAX_FETCH; a request with 0 legs or more than
 * OTT_FUSE_MAX_LEGS; legs_b x fetch above OTT_FUSE_MAX_ENTRIES; a sum of legs_per_request other than d->nq; an unknown fusion;
 * with RRF an rrf_k that is not finite or below 0; a weight that is not finite; k == 0; cap too small; out NULL with cap > 0; and
 * what ott_query refuses.  An empty store is a valid call with no hits.  Takes the store shared, like ott_query, once for both
 * stages.  Stats: the first stage's (path_used, passes, bytes_scanned, ...); merge_ns carries the fuse kernel's event time on top;
 * total_ns is the whole call.
 * OUT OF SCOPE: a mask, filter or metric per leg (legs with their own filters are ott_query_masks' business; combining the two is a
 * later change); multi-GPU stores; nested prefetches; legs that are stored rows.  (Sparse legs beside the dense ones:
 * ott_query_hybrid, below the sparse vectors.) */
typedef enum { OTT_FUSE_RRF = 0, OTT_FUSE_DBSF = 1, OTT_FUSE_MINMAX = 2 } ott_fusion;
#define OTT_FUSE_MAX_LEGS 16
#define OTT_FUSE_MAX_FETCH 512
#define OTT_FUSE_MAX_ENTRIES 8192
#define OTT_FUSE_MAX_REQUESTS 1024
int ott_query_fuse(ott_store* s, const ott_query_desc* d, const void* legs_per_request /* uint32_t[n_requests] */, uint32_t n_requests,
                   uint32_t fusion /* ott_fusion */, float rrf_k, const float* leg_weights /* [d->nq] or NULL = all 1 */, uint64_t fetch,
                   ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_request, ott_stats* stats);

/* MMR diversity re-ranking (an extension; maximal marginal relevance, Carbonell and Goldstein — LangChain's
 * max_marginal_relevance_search, Qdrant's mmr query): of a query's best fetch_k hits, pick d->k greedily, each pick the most relevant
 * and the least similar to what is already picked.  The CANDIDATES are exactly the hits ott_query (ott_query_ids when ids is given)
 * returns for the same descriptor with k = fetch_k — index, score bits and order, under every metric, take, filter, mask, path and
 * tie order; candidate i has row r_i, relevance rel_i and position i; n <= fetch_k of them exist.  g(x) = x for OTT_TAKE_MAX, -x for
 * OTT_TAKE_MIN.  The PAIR SCORE P[s][c] is the metric's score with candidate s's STORED row as the query and candidate c's stored
 * row as the row, the exact path's bits in the store's reduce order; cosine is (dot * inv[r_s]) * inv[r_c] with the store's inverse
 * norms (the roundings are not symmetric: the selected row plays the query).  Pair scores read stored data: masks and the filter
 * act on the first stage only.  SELECTION, in f32, every operation rounded on its own (no FMA), om = 1.0f - lambda: pick 0 is
 * candidate 0 with value lambda * g(rel_0); every unpicked c keeps red_c, set to g(P[s_0][c]) after pick 0 and after each later pick
 * s, with x = g(P[s][c]): unchanged if x is NaN, else x if red_c is NaN, else x if x > red_c; value_c = (lambda * g(rel_c)) -
 * (om * red_c); the next pick has the largest ordinal of its value (the library's total order, +0.0 above -0.0, a NaN value below
 * every other), equal ordinals go to the lower position; k_eff = min(k, n) picks.  OUTPUT: one ott_hit per pick in pick order, as
 * the first stage gave it (index, relevance bits, query); out_values[i], if given, the f32 value of pick i (a NaN value is written
 * as 0x7FC00000).  With lambda = 1 and finite scores the result is the first k_eff candidates; with fetch_k = k it is the plain
 * top-k as a set.  OTT_MODE_MERGED takes one query; OTT_MODE_PER_QUERY runs one independent MMR per query (hits grouped by query,
 * counts in n_per_query, as ott_query).  cap >= min(k, rows) (rows: ott_store_len, or the distinct listed ids), x nq in PER_QUERY;
 * out_values holds cap floats.  stats is the first stage's; total_ns covers both stages and the event time of the two kernels below
 * is added to merge_ns.
 * The first stage runs through ott_query's own internals and hands its hits over the host (one more wait, an upload of at most
 * 12 KB per query).  A pair kernel then fills P across the GPU — the gather kernel's geometry, eight lanes per row, with eight
 * candidates' rows read from the store BY ID into LDS as a workgroup's queries; nothing is gathered to a temporary — and a greedy
 * kernel, one workgroup per query and one thread per candidate, runs every round in one launch.  Scratch (nq x fetch_k^2 x 4 B of
 * pair scores) belongs to the query context.  A store that never makes this call allocates and launches nothing for it.
 * Refused on the host before any device work, with nothing written: d->k == 0, d->k > fetch_k, fetch_k > OTT_MMR_MAX_FETCH, lambda
 * outside [0, 1] or NaN (OTT_ERR_INVALID, checked before the store is looked at); the errors of ott_query and ott_query_ids; cap too
 * small (OTT_ERR_INVALID); OTT_MODE_MERGED with nq > 1, a multi-GPU store (candidate rows lie on different shards), rows longer than
 * 2048 floats, nq x fetch_k^2 x 4 B above 256 MiB (OTT_ERR_UNSUPPORTED).  Takes the store shared, like ott_query, once for both stages. */
#define OTT_MMR_MAX_FETCH 1024
int ott_query_mmr(ott_store* s, const ott_query_desc* d, const uint64_t* ids, uint64_t n_ids, /* NULL, 0: no id list */
                  uint64_t fetch_k, float lambda, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                  float* out_values /* may be NULL; cap floats */, ott_stats* stats);

/* Recommend by example rows (an extension; Qdrant's recommend with the best_score strategy): "more like these rows, less like
 * those".  The examples are rows of the store, named by id counted from the store's first row like ott_query_ids' (not shifted by
 * base_offset); duplicates inside one list count once; a deleted row may be an example (stored data is read, as in
 * ott_store_score_rows).  d carries metric, take, filter, k, chunk_mask, row_mask / use_device_row_mask and path; d->queries must be
 * NULL, d->nq 0 and d->mode MERGED.
 * PAIR SCORE: P[e][r] is ott_query_mmr's — example e's STORED row as the query and row r as the row, the exact path's bits in the
 * store's reduce order; cosine is (dot * inv[e]) * inv[r] with the store's inverse norms.  All four metrics.
 * BEST SCORES: ord(x) = the library's 32-bit ordinal of x under d->take (larger is better; the total order, +0.0 above -0.0 under
 * Max).  bp(r) = the largest ord(P[p][r]) over the positives p whose pair score is not NaN, bn(r) the same over the negatives, 0 =
 * none; BP and BN are the scores those ordinals decode to.
 * CANDIDATES: rows that survive chunk_mask, the caller's row mask or the evaluated device mask and the live mask of deleted rows,
 * are not themselves an example (positive or negative), have bp != 0, and whose BP passes the score filter (the filter always acts
 * on BP, on both sides).
 * SIDES: positive (side_of_hit = 1) when bn == 0 or bp > bn; negative (side_of_hit = 0) when bp <= bn — a comparison of ordinals: a
 * row as close to a negative as to its best positive is on the negative side.
 * ORDER: first every positive-side candidate by bp descending, then the lower row; then, only with OTT_RECOMMEND_FILL, the
 * negative-side candidates by bn ASCENDING (the row least like its nearest negative first), then the lower row; cut at
 * k_eff = min(k, ott_store_len).  Always this canonical order, whatever option "tie_order" says.
 * OUTPUT: one ott_hit per pick — index = base_offset + row, score = BP on the positive side and BN on the negative side, query = 0;
 * side_of_hit[i], if given, the side of hit i.  cap >= k_eff.  With one positive and no negative the hits are the plain top-k of
 * that stored row used as a query with the row itself masked out; with no negatives the flag has no effect.
 * One streaming sweep scores four examples per pass (one pass for a single example, else ceil(examples / 4)) and keeps every row's
 * {bp, bn} in an 8-byte state (scratch of the query context, [rows] x 8 B); a keys kernel and grouped search's top-k give the
 * positive side, and a second keys kernel and top-k the negative side — only when the flag is set, negatives exist and the positive
 * side returned fewer than k_eff (one more host wait in that case alone).  The examples' rows are gathered on the device.
 * stats: path_used = EXACT, passes, vectors_compared = rows scored x examples, bytes_scanned per pass, score_ns / merge_ns as
 * ott_query_maxsim counts them (the first round's).
 * Refused on the host before any device work, with nothing written: n_positive == 0, more than OTT_RECOMMEND_MAX_EXAMPLES distinct
 * examples, a list pointer NULL with a count above 0, an id >= ott_store_len, a row listed as both positive and negative, unknown
 * flag bits, d->nq != 0 or d->queries != NULL, cap < k_eff, out == NULL with cap > 0 (OTT_ERR_INVALID); OTT_MODE_PER_QUERY,
 * OTT_PATH_MFMA (AUTO takes the sweep and never builds, extends or waits for a plane), a multi-GPU store (the examples' rows lie on
 * different shards), a store of more than 2^32 - 16 rows (OTT_ERR_UNSUPPORTED).  Takes the store shared, like ott_query (staged
 * appends go first). */
#define OTT_RECOMMEND_MAX_EXAMPLES 64
#define OTT_RECOMMEND_FILL 1u /* flags bit 0 */
int ott_query_recommend(ott_store* s, const ott_query_desc* d, const uint64_t* positive, uint64_t n_positive, const uint64_t* negative,
                        uint64_t n_negative, uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out,
                        uint32_t* side_of_hit /* may be NULL; cap entries */, ott_stats* stats);

/* Recommend by example rows with a STRATEGY (an extension; Qdrant's three recommend strategies).  OTT_RECOMMEND_BEST_SCORE is
 * ott_query_recommend itself: the same arguments, results, refusals and messages (they name ott_query_recommend).  For the other
 * two the examples are checked and laid out as there — slots e_0 .. e_{m-1}: the distinct positives in first-occurrence order, then
 * the distinct negatives, at most OTT_RECOMMEND_MAX_EXAMPLES; a deleted row may be an example; an example is never a hit —,
 * d->queries must be NULL, d->nq 0, d->mode MERGED and flags 0 (OTT_RECOMMEND_FILL belongs to best_score).  chunk_mask, the caller's
 * row mask or the evaluated device mask and the live mask of deleted rows all apply.  side_of_hit[i], if given, is 1 for every hit.
 * SUM_SCORES: with the pair score P[e][r] of ott_query_recommend, S(r) starts as P[e_0][r] itself (a -0.0 stays -0.0); for i = 1 ..
 * m - 1 in slot order S = S + P[e_i][r] for a positive e_i, S = S - P[e_i][r] for a negative one — each step one f32 operation,
 * round to nearest, no contraction; a NaN pair score or inf - inf makes S NaN.  CANDIDATES: rows that survive the masks, are no
 * example, have an S that is not NaN and passes the score filter.  ORDER: ord(S) under d->take descending, then the lower row; cut
 * at k_eff = min(k, ott_store_len); always this canonical order, whatever option "tie_order" says.  OUTPUT: {base_offset + row, S,
 * 0}.  OTT_PATH_MFMA is refused; AUTO and EXACT take ott_query_recommend's sweep (four examples per pass, the running sum in the
 * same 8-byte state) and never build or wait for a plane.  stats as ott_query_recommend counts them.
 * AVERAGE_VECTOR: q[i] = mp (no negatives) or (mp + mp) - mn, with sp = row(p_0)[i], sp = sp + row(p_j)[i] in slot order, mp = sp /
 * (float)n_pos (one correctly rounded f32 division), mn likewise over the negatives; stored f32 values, nothing normalised.  The
 * vector is built on the device and comes back once (dim floats: ott_query's host side computes the query norm).  The hits are
 * EXACTLY ott_query's for d with queries = q, nq = 1 and one more row mask, every bit set but the examples': the same path choice
 * (AUTO / EXACT / MFMA as ott_query treats them for the metric), options ("tie_order" included), stats and k_eff.
 * Refused on the host before any device work, with nothing written, in messages that name ott_query_recommend_strategy: an unknown
 * strategy, nonzero flags, and what ott_query_recommend refuses for its arguments (OTT_ERR_INVALID); OTT_MODE_PER_QUERY,
 * OTT_PATH_MFMA with SUM_SCORES, a multi-GPU store, a store of more than 2^32 - 16 rows (OTT_ERR_UNSUPPORTED).  Takes the store
 * shared, like ott_query_recommend. */
typedef enum { OTT_RECOMMEND_BEST_SCORE = 0, OTT_RECOMMEND_AVERAGE_VECTOR = 1, OTT_RECOMMEND_SUM_SCORES = 2 } ott_recommend_strategy;
int ott_query_recommend_strategy(ott_store* s, const ott_query_desc* d, uint32_t strategy, const uint64_t* positive,
                                 uint64_t n_positive, const uint64_t* negative, uint64_t n_negative, uint32_t flags, ott_hit* out,
                                 uint64_t cap, uint64_t* n_out, uint32_t* side_of_hit /* may be NULL */, ott_stats* stats);

/* Discovery and context search (an extension; Qdrant's Discovery API): rank the rows by CONTEXT PAIRS of stored rows, each a
 * (positive, negative), and optionally by a TARGET.  Pair i is (positive[i], negative[i]), i < n_pairs, 1 <= n_pairs <=
 * OTT_DISCOVER_MAX_PAIRS; ids are counted from the store's first row like ott_query_recommend's (not shifted by base_offset).  A row
 * may occur in several pairs, on either side; nothing is deduplicated: slot 2i of the sweep is the positive and slot 2i + 1 the
 * negative of pair i.  A deleted row may be an example.  positive[i] == negative[i] is refused.
 * TARGET: a vector — d->queries with d->nq == 1: the target score T[r] is exactly ott_query's exact-path score of that vector, the
 * host-side query norm included; a stored row — target_row != OTT_NO_ROW with d->nq == 0: T[r] is the pair score of that row; none —
 * d->nq == 0 and target_row == OTT_NO_ROW: context search.  A vector together with a row is refused.
 * PAIR SCORE: P[e][r] is ott_query_mmr's / ott_query_recommend's — example e's STORED row as the query, the exact path's bits in the
 * store's reduce order; cosine is (dot * inv[e]) * inv[r] with the store's inverse norms.  All four metrics.
 * WINS: ord(x) = the library's 32-bit ordinal of x under d->take.  Pair i is won by r iff ord(P[pos_i][r]) > ord(P[neg_i][r]);
 * wins(r) = the number of pairs won, 0 .. n_pairs.
 * LOSS: starts at +0.0f; for i = 0 .. n_pairs - 1 in that order: d = P[pos_i][r] - P[neg_i][r] under take Max, P[neg_i][r] -
 * P[pos_i][r] under take Min (one f32 subtraction, round to nearest); t = (d < 0) ? d : 0.0f (a NaN d from inf - inf gives 0);
 * loss = loss + t (one f32 addition).
 * CANDIDATES: rows that survive chunk_mask, the caller's row mask or the evaluated device mask and the live mask of deleted rows,
 * are no example and not the target row, have no NaN pair score, wins(r) >= min_wins, with a target a T[r] that is not NaN, and whose
 * score — T[r] with a target, loss(r) without — passes the score filter.
 * ORDER: with a target: wins descending, then ord(T[r]) descending, then the lower row.  Without: loss descending in the total order
 * (take Max's ordinal of the loss, whatever d->take is), then the lower row.  Cut at k_eff = min(k, ott_store_len).  Always this
 * canonical order, whatever option "tie_order" says.
 * OUTPUT: ott_hit{index = base_offset + row, score = T[r] or loss(r), query = 0}; wins_of_hit[i], if given, the hit's wins.
 * cap >= k_eff.
 * One streaming sweep scores four slots — two whole pairs — per pass, passes = ceil((2 * n_pairs + T) / 4) with T = 1 with a target:
 * the target rides in the last pass's free slots when n_pairs is odd and takes a pass of its own otherwise.  Every row keeps
 * {wins, loss or target ordinal} in an 8-byte state (scratch of the query context, [rows] x 8 B, shared with ott_query_recommend).
 * Without a target a keys kernel and grouped search's top-k finish.  With one, a count kernel makes the candidates per wins level, a
 * select kernel derives the level L* the k_eff-th hit lies on, hands that level's rows to the top-k and lists the fewer than k_eff
 * rows above it; the host sorts that list behind the one wait.  The examples' rows are gathered on the device.
 * stats: path_used = EXACT, passes, vectors_compared = rows scored x (2 * n_pairs + T), bytes_scanned per pass as
 * ott_query_recommend counts it, score_ns / merge_ns.
 * Refused on the host before any device work, with nothing written: n_pairs == 0 or above OTT_DISCOVER_MAX_PAIRS, a NULL list, an
 * id >= ott_store_len (the target row included), a pair with the same row on both sides, a vector target together with a target
 * row, d->nq > 1 (or d->queries and d->nq that disagree), min_wins > n_pairs, nonzero flags, cap < k_eff, out == NULL with cap > 0
 * (OTT_ERR_INVALID); OTT_MODE_PER_QUERY, OTT_PATH_MFMA (AUTO takes the sweep and never builds, extends or waits for a plane), a
 * multi-GPU store, a store of more than 2^32 - 16 rows (OTT_ERR_UNSUPPORTED).  Takes the store shared, like ott_query (staged
 * appends go first). */
#define OTT_DISCOVER_MAX_PAIRS 32
#define OTT_NO_ROW UINT64_MAX /* target_row: no stored row is the target */
int ott_query_discover(ott_store* s, const ott_query_desc* d, uint64_t target_row, const uint64_t* positive, const uint64_t* negative,
                       uint64_t n_pairs, uint32_t min_wins, uint32_t flags, ott_hit* out, uint64_t cap, uint64_t* n_out,
                       uint32_t* wins_of_hit /* may be NULL; cap entries */, ott_stats* stats);

/* Grouped search (an extension; Elasticsearch field collapse, Qdrant search_groups, Milvus group_by_field): one best hit per group,
 * top-k over the groups — top-10 DOCUMENTS of a store of chunks.  A store may carry one dense group id per row (uint32, < n_groups,
 * resident in HBM at 4 B per row).  ott_query_groups returns exactly the hits — index, score bits, order, per-query counts — of the
 * same query with the default take (every passing pair in the canonical order: better score, lower row, lower query) after dropping
 * every hit whose group occurred earlier in that list, cut at k; per query in PER_QUERY mode.  chunk_mask, the caller's row_mask or
 * the evaluated device mask, the live mask of deleted rows and the score filter all apply BEFORE grouping: a masked, deleted or
 * filtered row never represents its group, the group's best surviving row does; NaN scores are dropped as everywhere.  All four
 * metrics, both takes, every comparator.  The order among equal scores is ALWAYS the canonical one, whatever option "tie_order"
 * says: the reference has no grouped query whose tie outcome could be reproduced.
 * k_eff = min(k, n_groups); cap >= k_eff (MERGED) or nq * k_eff (PER_QUERY).
 * One sweep over the rows keeps, per (query, group), the best candidate key in a table of n_groups 8-byte slots (scratch of the
 * query context); the top-k is taken over the slots (k_eff <= 512: register lists + the block-list merge; above: the radix sort).
 * Refused: OTT_MODE_MERGED with nq > 1 (OTT_ERR_UNSUPPORTED: one winner per group ACROSS queries is left out; use PER_QUERY) and
 * OTT_PATH_MFMA (OTT_ERR_UNSUPPORTED; AUTO takes the exact sweep and never builds, extends or waits for a plane).  OTT_ERR_INVALID,
 * checked on the host before any device work: no group ids are set, or they cover a different number of rows than ott_store_len
 * (rows were appended since: set them again).  Takes the store shared, like ott_query (staged appends go first).
 *
 * ott_store_set_groups: gid_host points at n uint32_t (declared const void*, as ott_store_add_column's values), [i] = group of row i, n must equal ott_store_len, every id < n_groups (else OTT_ERR_INVALID, checked
 * on the host before any device work); a second call replaces the first.  ott_store_clear_groups drops them.  Both take the store
 * exclusively, like ott_store_add_column, and flush staged appends first.  Group ids count as a resident metadata column: while they
 * are set ott_store_compact is refused (OTT_ERR_UNSUPPORTED) and a multi-GPU store no longer moves rows between its shards;
 * clear_groups lifts both.  A reallocation on append keeps the ids that are there.  A store without groups runs exactly what it ran
 * before: nothing is allocated, no launch is added.  ott_store_group_count: n_groups, 0 = none set.
 * Multi-GPU store: ids are global and routed by row range; every shard answers for its rows, the host merges the shards' lists by the
 * canonical order and keeps each group's first hit (a group in the global top-k is in its own shard's top-k). */
int ott_store_set_groups(ott_store* s, const void* gid_host /* uint32_t[n] */, uint64_t n, uint32_t n_groups);
int ott_store_clear_groups(ott_store* s);
uint32_t ott_store_group_count(const ott_store* s);
int ott_query_groups(ott_store* s, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query,
                     ott_stats* stats);

/* Grouped search with up to group_size hits per group (Qdrant search_groups' and Milvus group_by_field's group_size, Elasticsearch
 * collapse with inner_hits): the top-10 documents and the best 3 passages of each, from one call.  Let L be the hits of the same
 * query with the default take (every passing pair in the canonical order: better score, then lower row), after chunk_mask, the
 * caller's row_mask or the evaluated device mask, the live mask of deleted rows, the score filter and the NaN drop — exactly as in
 * ott_query_groups.  With group_size = m: (1) a hit of L is kept iff fewer than m earlier hits of L have its group; (2) groups are
 * ranked by the position of their first kept hit, which is ott_query_groups' ranking of the groups; (3) the first k_eff = min(k,
 * n_groups) groups are kept; (4) they come out in that rank order, each group's hits (1 .. m of them) contiguous and in their order
 * in L.  Per query in PER_QUERY mode.  Four metrics, both takes, every comparator; always the canonical tie order, whatever option
 * "tie_order" says.  A group with fewer than m surviving rows returns what it has.  With m = 1 the output is ott_query_groups' on
 * every field (and it IS that query: no kernel and no launch is added; group_of_hit then comes from one small gather).
 * cap >= nq * k_eff * group_size, and group_of_hit — if given — holds as many uint32: [i] = the dense group id of out[i].
 * n_per_query[q] = the number of HITS of query q.  Stats as ott_query_groups counts them.
 * m >= 2: the sweep keeps, per (query, group), the m best candidate keys in a table of nq x m x n_groups 8-byte slots (scratch of the
 * query context, all queries at once) by a cascade of vector atomicMax — a key that takes slot j sends the slot's old key on to slot
 * j + 1 — the groups are ranked over the first slots by ott_query_groups' own top-k, and the winners' other slots are read back.
 * Refused on the host before any device work: group_size == 0 or > OTT_GROUP_SIZE_MAX (OTT_ERR_INVALID); OTT_MODE_MERGED with nq > 1
 * and OTT_PATH_MFMA (OTT_ERR_UNSUPPORTED, as ott_query_groups; AUTO takes the sweep); no group ids set, or ids that cover a different
 * number of rows than ott_store_len (OTT_ERR_INVALID); nq x group_size x n_groups x 8 bytes above 2 GiB (OTT_ERR_UNSUPPORTED); a
 * multi-GPU store (OTT_ERR_UNSUPPORTED).  Why the last: a group's second-best row may sit in a shard where the group is not among
 * that shard's top-k groups (its best row there loses to k other groups' bests), so — unlike for one hit per group — the shards'
 * lists of k_eff groups do not contain the answer; a second round that asks every shard for the winning groups' rows would be needed.
 * Takes the store shared, like ott_query_groups (staged appends go first). */
#define OTT_GROUP_SIZE_MAX 16
int ott_query_groups_top(ott_store* s, const ott_query_desc* d, uint32_t group_size, ott_hit* out, uint64_t cap, uint64_t* n_out,
                         uint64_t* n_per_query, uint32_t* group_of_hit /* may be NULL */, ott_stats* stats);

/* Late-interaction (MaxSim) search over grouped rows (an extension; ColBERT / ColPali scoring as Qdrant's multivector MaxSim, Vespa
 * and Milvus serve it): the d->nq query vectors are the TOKENS of ONE query, the rows are token or passage embeddings, the store's
 * group ids (ott_store_set_groups) say which document a row belongs to, and the answer is the top-k DOCUMENTS by
 *     score(g) = best[0][g] + best[1][g] + ... + best[nq-1][g],   best[t][g] = the best score of token t among the rows of g
 * that survive chunk_mask, the caller's row_mask or the evaluated device mask, and the live mask of deleted rows.  "Best" follows
 * d->take (largest for OTT_TAKE_MAX, smallest for OTT_TAKE_MIN: with Euclidean or Manhattan the sum of minimum distances) in the
 * library's total order (+0.0 beats -0.0 under Max); NaN pair scores are dropped as everywhere; pair scores are the exact path's
 * bits for all four metrics.  A group is a candidate only if EVERY token has a best (it has a surviving row, and no token for which
 * all of them scored NaN).  The sum is f32, round to nearest, in token order, started from best[0] (a -0.0 stays -0.0); a NaN sum
 * (+inf + -inf) drops the group.  filter_cmp / filter_thr apply to the SUM: every returned score satisfies the filter (a filter on
 * the single pair scores is not offered).  Candidates are ranked by the sum (total order, by d->take), then the lower group id, and
 * cut at k_eff = min(k, n_groups): always this canonical order, whatever option "tie_order" says.  Hits: index = the dense group id
 * (NOT shifted by base_offset), score = the sum, query = 0.  With nq = 1 the hits are ott_query_groups' for that query without a
 * score filter, each row replaced by its group (between groups of EQUAL score that call prefers the lower row, this one the lower group).  cap >= k_eff.
 * One sweep per four tokens keeps the best score ordinal of every (token, group) in a table of nq x n_groups 4-byte slots (scratch
 * of the query context), a reduce kernel sums every group's slots into an 8-byte key, and the top-k over the keys is grouped
 * search's.  Stats: path_used = EXACT, passes = corpus passes (ceil(nq / 4); 1 for one token), vectors_compared = rows scored x nq,
 * bytes_scanned and score_ns / merge_ns as ott_query_groups counts them.
 * Refused on the host before any device work: OTT_MODE_PER_QUERY (OTT_ERR_UNSUPPORTED: a batch of token sets is left out),
 * OTT_PATH_MFMA (OTT_ERR_UNSUPPORTED; AUTO takes the sweep and never builds, extends or waits for a plane), a multi-GPU store
 * (OTT_ERR_UNSUPPORTED: a group may span shards, the maxima would have to be joined before the sum), no group ids set or ids that
 * cover a different number of rows than ott_store_len (OTT_ERR_INVALID, as ott_query_groups), nq x n_groups x 4 bytes above 2 GiB
 * (OTT_ERR_UNSUPPORTED: the table holds all tokens at once), cap < k_eff (OTT_ERR_INVALID).  Takes the store shared, like
 * ott_query_groups (staged appends go first). */
int ott_query_maxsim(ott_store* s, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out, ott_stats* stats);

/* MaxSim re-ranking (an extension; the second stage of a ColBERT / ColPali pipeline: a cheap first stage names the candidate
 * documents, late interaction ranks only those): ott_query_maxsim over a LISTED set of groups.  groups points at n_groups_listed dense
 * group ids (uint32_t, declared const void* as ott_store_set_groups' ids; each < ott_store_group_count), in any order, duplicates allowed.  The call returns exactly the hits of
 * ott_query_maxsim for the same descriptor — the dense group id in `index`, the score bits of the sum, the order, query = 0 — with
 * one more row mask: only rows whose group is listed are kept, ANDed with chunk_mask, the caller's row_mask or the evaluated device
 * mask, and the live mask of deleted rows.  Everything ott_query_maxsim's contract says holds unchanged: four metrics, both takes,
 * "best" in the total order, NaN pair scores dropped, a group needs a best for every token, the f32 sum in token order from
 * best[0], a NaN sum drops the group, the filter applies to the sum, ties go to the lower group id whatever "tie_order" says.
 * k_eff = min(k, number of DISTINCT listed groups); cap >= k_eff.  n_groups_listed == 0 is a valid query with no hits.
 * The work follows the list, not the store.  The gather route walks only the listed groups' rows: the store keeps a group-to-rows
 * index in HBM (the rows ordered by group, 4 B per row, and the groups' extents on the host), built on the device from the group
 * ids by the first call that may use it, under the store's exclusive lock like a flush of staged appends, and dropped only when the
 * group ids change (ott_store_set_groups, ott_store_clear_groups); a store that never makes this call allocates and launches nothing
 * for it.  A workgroup per listed group scores its rows against up to 32 tokens at a time (32 while the padded dim is <= 512, 16 while
 * <= 1024, 8 while <= 2048) with the exact path's additions in the exact path's order, keeps one running maximum per token and — when
 * the tokens fit one pass — sums them itself; a 32 x 128 query reads every listed row once.  Served by the gather: a single-GPU
 * store, path AUTO or EXACT, a padded dim of at most 2048 floats, a store of at most 2^26 groups, at most 2^24 distinct listed
 * groups holding at most 2^30 rows.  Everything else, and option "group_gather" = 0, takes the mask route: a small kernel turns the
 * list into row-mask words (no index is needed) and ott_query_maxsim's sweep runs with them.  Same bits either way.
 * Stats on the gather route: path_used = EXACT, passes = token passes, vectors_compared = the listed groups' rows x nq (before the
 * masks), bytes_scanned = their bytes per pass; on the mask route ott_query_maxsim's.  ott_store_group_index_builds: how many times
 * this store has built the index (tests and diagnostics: it rises by one per build, never on a query that found the index there).
 * Refused on the host before any device work: OTT_MODE_PER_QUERY, OTT_PATH_MFMA and a multi-GPU store (OTT_ERR_UNSUPPORTED, as
 * ott_query_maxsim); a listed id >= ott_store_group_count, groups == NULL with n_groups_listed > 0, no group ids set or ids that
 * cover a different number of rows than ott_store_len (OTT_ERR_INVALID); cap < k_eff (OTT_ERR_INVALID); on the mask route nq x
 * n_groups x 4 bytes above 2 GiB (OTT_ERR_UNSUPPORTED).  Takes the store shared, like ott_query_maxsim (staged appends go first). */
int ott_query_maxsim_groups(ott_store* s, const ott_query_desc* d, const void* groups, /* uint32_t[n_groups_listed] */ uint64_t n_groups_listed,
                            ott_hit* out, uint64_t cap, uint64_t* n_out, ott_stats* stats);
uint64_t ott_store_group_index_builds(const ott_store* s);

/* MaxSim re-ranking in batches (an extension; a server that re-ranks for many users at once): B = n_queries queries, each with its
 * own tokens and its own candidate list, through one upload, one gather launch, one top-k and one host wait.  d->queries holds the
 * tokens of query 0, then of query 1, and so on; tokens_per_query[b] (uint32_t, declared const void* as the group ids are) says how
 * many belong to query b, and d->nq is their total.  groups holds the lists in the same order, listed_per_query[b] dense ids each:
 * any order, duplicates allowed, two queries may list the same group, and listed_per_query[b] == 0 is a valid query with no hits.
 * The whole batch shares metric, take, the filter, k, chunk_mask, the row mask (the caller's or the device mask) and the live mask
 * of deleted rows.  For every b the call returns exactly the hits of ott_query_maxsim_groups with d->queries / d->nq replaced by
 * query b's tokens and with query b's list — the same dense group ids, the same score bits, the same order — except that their
 * `query` field is b.  The lists come out back to back in query order; n_per_query[b] (n_queries entries, may be NULL) is their
 * lengths and *n_out their sum.  k_eff_b = min(k, distinct listed groups of b); cap >= the sum of the k_eff_b.  Everything the
 * contracts of ott_query_maxsim and ott_query_maxsim_groups say holds per query.
 * The batched gather serves the batch when ott_query_maxsim_groups' gather would serve every query alone and every query's tokens
 * fit one pass (32 tokens while the padded dim is <= 512, 16 while <= 1024, 8 while <= 2048), n_queries x the largest number of
 * distinct listed groups stays within 2^24 and the listed rows of all queries within 2^30: the slots of all queries lie back to
 * back, a persistent workgroup walks a contiguous range of them balanced by listed rows and reloads the token block in LDS where
 * the query changes; one top-k serves all queries.  Option "group_gather": 1 = wherever eligible, -1 = when every query alone
 * would take the gather, 0 = never.  Everything else takes the loop route: the queries are answered one by one as
 * ott_query_maxsim_groups answers them, under the one shared lock.  Same bits either way.
 * Stats: path_used = EXACT; on the batched gather passes = 1, vectors_compared = the sum over the queries of listed rows x tokens
 * (before the masks), bytes_scanned = the listed rows' bytes; on the loop route each is the sum of the queries' own.
 * Refused on the host before any device work, with nothing written: OTT_MODE_PER_QUERY and OTT_PATH_MFMA (OTT_ERR_UNSUPPORTED,
 * before the store is looked at), a multi-GPU store (OTT_ERR_UNSUPPORTED); n_queries == 0 or above OTT_MAXSIM_BATCH_MAX (it bounds
 * the staged token block to about 75 MB at 32 x 128 tokens), tokens_per_query or listed_per_query NULL, groups NULL with a listed
 * id, tokens_per_query[b] == 0, a sum of tokens_per_query other than d->nq, a listed id >= ott_store_group_count (the message names
 * b and the id), no group ids set or ids that cover a different number of rows than ott_store_len, cap below the sum of the k_eff_b
 * (all OTT_ERR_INVALID).  Takes the store shared, like ott_query_maxsim_groups: staged appends and the group-to-rows index are
 * settled first, once for the whole batch. */
#define OTT_MAXSIM_BATCH_MAX 4096
int ott_query_maxsim_groups_batch(ott_store* s, const ott_query_desc* d, const void* tokens_per_query, /* uint32_t[n_queries] */
                                  const uint64_t* listed_per_query, uint32_t n_queries, const void* groups, /* uint32_t[sum of listed_per_query] */
                                  ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);

/* Same, but the result stays on the GPU: out_dev holds `cap` ott_hit slots in device memory
 * of the store's GPU, padded with sentinel hits (index = UINT64_MAX); *n_out_dev (device
 * uint64) receives the count.  PER_QUERY mode: cap must be a multiple of nq; query q's hits
 * start at slot q * (cap / nq), each group sentinel padded.  Every slot below cap holds a hit or a sentinel whose 16 bytes are all
 * 0xFF; slots at and past cap are never written, on any route.  With groups = 1 (MERGED) or nq (PER_QUERY): a block of exactly
 * cap / groups == 64 * list_E(k) slots per group (list_E: 1 up to k = 64, 2 up to 128, 4 up to 256, 8 up to 512 — what
 * ott_query_sharded asks for) is the merge kernel's own geometry and is written IN PLACE, hits and sentinels by the one kernel;
 * any other cap is filled with sentinels first and receives the hits by a copy of min(cap / groups, 64 * list_E(k)) slots per
 * group; k > 512 and the cascade's results are staged on the host and arrive as one block of cap slots.
 * Launched on the calling context's stream; returns once the kernels have
 * completed (the caller's collective runs on another stream).  Used for the multi-GPU
 * all-gather of candidates. */
int ott_query_device(ott_store* s, const ott_query_desc* d, void* out_dev, uint64_t cap, void* n_out_dev,
                     ott_stats* stats);
int ott_store_sync(ott_store* s);
/* HIP stream the store launches on (hipStream_t as void*), for event timing by the caller. */
void* ott_store_stream(ott_store* s);

/* Final merge of candidate lists (src/meta.rs:699-709: concat, sort, truncate(k)) on the
 * GPU: `lists_dev` = n_lists * list_len ott_hit in device memory (sentinels ignored), output
 * k best hits (canonical order) to out_host. */
int ott_merge_hits_device(ott_store* s, const void* lists_dev, uint64_t n_lists, uint64_t list_len,
                          uint32_t take, uint64_t k, ott_hit* out_host, uint64_t* n_out);
/* The same merge for PER_QUERY results: `lists_dev` = [n_lists][n_groups][list_len] ott_hit (what an
 * all-gather of per-GPU ott_query_device PER_QUERY blocks produces, group = query); every group is
 * merged on its own.  out_host receives the groups' hits back to back (at most k each, needs
 * n_groups * min(k, n_lists*list_len) slots), *n_out the total, n_per_group[g] each group's count. */
int ott_merge_hits_device_grouped(ott_store* s, const void* lists_dev, uint64_t n_lists, uint64_t n_groups,
                                  uint64_t list_len, uint32_t take, uint64_t k, ott_hit* out_host,
                                  uint64_t* n_out, uint64_t* n_per_group);

/* ---- multi-GPU: the corpus sharded by contiguous chunk ranges, one process (and one ott_store) per GPU -------------------
 * The reference fans chunks out over a rayon pool and concat-sort-truncates the per-chunk top-k lists
 * (src/meta.rs:678-709).  Across GPUs the same two steps are: every rank scores ITS shard (no data-path collective), then
 * ONE exchange — an all-gather of fixed-size, sentinel-padded per-GPU candidate blocks — and the same merge kernel on
 * every rank.  An ott_comm is that exchange.  Two transports:
 *   RCCL  (ott_comm_create): ncclAllGather over xGMI on the store's stream; score -> gather -> merge run back to back on
 *         that stream with no host synchronisation in between.  librccl.so.1 is dlopen'ed on first use.
 *   HOST  (ott_comm_create_host): the caller supplies an all-gather of host buffers (MPI, gloo, sockets ...); blocks are
 *         staged through pinned memory.  For hosts without RCCL bootstrap and for tests that put two ranks on one GPU
 *         (RCCL refuses duplicate devices). */
typedef struct ott_comm ott_comm;
#define OTT_COMM_ID_BYTES 128
/* all-gather callback of the HOST transport: every rank contributes `bytes` bytes at `send`; `recv` (world * bytes)
 * receives the blocks in rank order.  Returns 0 on success.  Called from the thread that called into the library. */
typedef int (*ott_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes);

/* ncclGetUniqueId: rank 0 creates the id (OTT_COMM_ID_BYTES bytes) and hands it to the other ranks out of band. */
int ott_comm_unique_id(void* id_out);
/* ncclCommInitRank on `device` (collective: every rank calls it with the same id and world). */
int ott_comm_create(const void* unique_id, int rank, int world, int device, ott_comm** out);
int ott_comm_create_host(int rank, int world, ott_allgather_fn fn, void* user, ott_comm** out);
int ott_comm_destroy(ott_comm* c);
int ott_comm_rank(const ott_comm* c);
int ott_comm_world(const ott_comm* c);
/* "rccl" or "host" */
const char* ott_comm_transport(const ott_comm* c);
/* What the transport itself reports: *nranks = ncclCommCount of the communicator (HOST transport: the world given at creation),
 * *version = ncclGetVersion (e.g. 22606; 0 for the HOST transport).  Either pointer may be NULL. */
int ott_comm_info(const ott_comm* c, int* nranks, int* version);
/* RCCL transport with world > 1: how long ott_comm_create may wait for the other ranks at the rendezvous, and how long a
 * collective (ott_query_sharded, ott_comm_all_gather_host) may stay unfinished, before the call returns OTT_ERR_HIP with a
 * message naming the incomplete exchange instead of waiting for a peer that died.  Default 120 000 ms; the environment
 * variable OTT_COMM_TIMEOUT_MS presets it (read once, in ott_comm_create); 0 = wait for ever.  After such an error the comm
 * is only good for ott_comm_destroy. */
int ott_comm_set_timeout_ms(ott_comm* c, int64_t timeout_ms);
/* All-gather of small HOST buffers over the comm's transport (control data: shard sizes, stats, timing, the
 * materialised cells of the k hits).  recv_host holds world * bytes.  RCCL transport: staged through device memory of
 * the comm's GPU, synchronous.  Also serves as a barrier. */
int ott_comm_all_gather_host(ott_comm* c, const void* send_host, void* recv_host, uint64_t bytes);

/* The hot path across shards: ott_query on this rank's shard, the candidate exchange, the final merge
 * (MetaQueryPlan::collect's score + merge block, src/meta.rs:671-709, with GPUs in place of rayon tasks).  Collective:
 * every rank calls it with the same queries / metric / take / filter / k / mode; chunk_mask, row_mask and
 * use_device_row_mask refer to the rank's own shard.  The store's base offset must be the shard's first global row, and
 * shards must be in rank order (rank r holds lower global rows than rank r + 1: ties then resolve like on one GPU).
 * Every rank receives the same result: up to k hits (MERGED) or k per query (PER_QUERY), best first, in `out`
 * (cap >= k, or nq * k; hits beyond what exists are not written).  `stats` describes this rank's shard.
 * k <= 512: fixed-size blocks, one device merge.  k > 512 (e.g. the reference's default take = every row,
 * src/meta.rs:638-644): every rank's sorted list is exchanged whole (counts first) and merged on the host. */
int ott_query_sharded(ott_store* s, ott_comm* c, const ott_query_desc* d, ott_hit* out, uint64_t cap, uint64_t* n_out,
                      uint64_t* n_per_query, ott_stats* stats);

/* ---- sparse vectors: a sparse row per stored row, exact sparse dot search ------------------------------
 * Row r of a store may carry a sparse row beside its dense one: ascending distinct indices below `vocab` with finite f32 values
 * (learned sparse encoders, BM25 weights).  The rows are attached to the store the way group ids are, so row ids, chunk masks,
 * row masks, the evaluated mask, mask slots and deleted rows mean the same for a dense and a sparse query, and a later change can
 * fuse both kinds of list without translating ids.  A collection that has only sparse vectors is a store of dim 1.
 *
 * ott_store_set_sparse: the rows as CSR (indptr[n + 1], indices uint32_t[nnz], values[nnz]), n == ott_store_len.  Everything is
 * checked on the host before any device work, and a refused call changes nothing: indptr[0] == 0, non-decreasing; every index
 * below vocab; strictly ascending inside a row; every value finite; 1 <= vocab <= OTT_SPARSE_MAX_VOCAB.  Rows without entries
 * and stored values of 0.0 / -0.0 are allowed and kept.  A second call replaces the first; ott_store_clear_sparse drops the rows.
 * Both take the store exclusively and flush staged appends first.  While sparse rows are set they count as a resident metadata
 * column (ott_store_compact is refused).  Rows appended afterwards leave the sparse rows in place, and a sparse query then fails
 * with OTT_ERR_INVALID ("set them again"), as a grouped query does.  OTT_ERR_UNSUPPORTED on a multi-GPU store.
 * In HBM the rows are a sliced ELL layout, 64 rows per slice: slice t is as long as its longest row, entry p of row r lies at
 * base_t + p * 64 + (r & 63).  ott_store_sparse_info reports vocab (0 = no sparse rows), nnz, padded_entries (the sum of 64 L_t)
 * and the bytes of the layout.  ott_store_read_sparse returns the CSR of a row range from that layout, bit for bit (indptr_out
 * counts from 0); an entry_cap below the range's entries is OTT_ERR_INVALID with the needed count in the message.
 *
 * ott_query_sparse: d->nq sparse queries as CSR (q_indptr[nq + 1], q_indices uint32_t[], q_values); d->queries is not read,
 * d->metric must be OTT_METRIC_DOT; take, filter, k, chunk mask, row mask or evaluated mask mean what they mean in ott_query_boost.
 * PER_QUERY, or MERGED with nq == 1; at most OTT_SPARSE_MAX_QUERIES queries; cap >= nq * min(k, rows).  A query's indices are below
 * the store's vocab and distinct, in any order; its weights are finite; a query without entries returns no hits.
 * The score (tests/sparse_ref.py is the normative model, ott_sparse_plan.h states it in C), IEEE f32, round to nearest even,
 * nothing fused, no flush to zero: S = +0.0f; for the row's entries j in ascending index order, wherever index_j is one of the
 * query's, S = fl(S + fl(value_j * weight(index_j))).  A row is a CANDIDATE iff it shares at least one index with the query,
 * whatever the values are (a row whose shared entries cancel to +0.0 is a hit, a row that shares nothing is not).  A NaN S drops
 * the row, the filter acts on S, the order is S under `take` with equal S going to the lower row; hit.score = S, hit.query = b.
 * OTT_ERR_UNSUPPORTED: OTT_PATH_MFMA (AUTO takes the sweep and never touches a plane), tie orders 1 and 2, a multi-GPU store, a
 * store of 2^32 - 16 rows or more, k_eff > 512 with more than 2^26 (query, row) pairs.
 * Store option "sparse_table" chooses where the kernel looks the weights up: -1 automatic, 0 a table in LDS wherever the vocab
 * allows (<= 32768; one query per pass), 1 always a device table (four queries per pass).  Both give the same bits.
 * stats: path_used = OTT_PATH_EXACT, passes, vectors_compared = the rows the chunk mask leaves per query, bytes_scanned = the
 * layout bytes of the slices those rows lie in, per pass.
 * Out of scope: BM25's term-frequency saturation and length normalisation (the caller stores those values; the collection statistic
 * is ott_store_sparse_df, dense and sparse legs in one fusion are ott_query_hybrid, both below), vocabularies above 2^20 or
 * hashed 32-bit token ids (the caller remaps), multi-GPU stores, reordering rows to cut padding, compaction with sparse rows. */
#define OTT_SPARSE_MAX_VOCAB 1048576 /* 2^20 */
#define OTT_SPARSE_MAX_QUERIES 1024
int ott_store_set_sparse(ott_store* s, const uint64_t* indptr /* [n + 1] */, const void* indices /* uint32_t[nnz] */,
                         const float* values /* [nnz] */, uint64_t n, uint32_t vocab);
int ott_store_clear_sparse(ott_store* s);
int ott_store_sparse_info(const ott_store* s, uint32_t* vocab, uint64_t* nnz, uint64_t* padded_entries, uint64_t* bytes);
int ott_store_read_sparse(const ott_store* s, uint64_t first_row, uint64_t n_rows, uint64_t* indptr_out /* [n_rows + 1] */,
                          void* indices_out, float* values_out, uint64_t entry_cap);
int ott_query_sparse(ott_store* s, const ott_query_desc* d, const uint64_t* q_indptr /* [d->nq + 1] */,
                     const void* q_indices /* uint32_t[] */, const float* q_values,
                     ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);

/* ---- document frequencies and IDF query weights (Qdrant's sparse vector `modifier: idf`) -------------------
 * ott_store_sparse_df: df_out[i] (uint32_t[vocab], may be NULL) = the LIVE rows (not deleted) whose sparse row stores index i (a
 * stored value of 0.0 counts); *n_docs_out (may be NULL) = the live rows, rows without entries included.  A collection statistic:
 * chunk masks and row masks play no part.  One kernel pass over the index array of the sliced-ELL layout (wave per slice, lane =
 * row, a slice without a live row is not read), integer adds: in a histogram private to the workgroup in LDS where the vocab fits
 * (<= 32768), flushed with one atomic add per non-zero bin, or with global atomic adds for any vocab; both give the same words.
 * Store option "sparse_df_lds": -1 automatic (the LDS form where it fits), 0 never, 1 wherever it fits.  The counts are CACHED on
 * the device and on the host and rebuilt by the first call that needs them after ott_store_set_sparse, ott_store_clear_sparse,
 * ott_store_delete_rows, ott_store_restore_rows or ott_store_compact; concurrent callers see one build.
 * ott_store_sparse_df_builds: how many times they were built.  OTT_ERR_INVALID: no sparse rows are set, or rows were appended
 * since; OTT_ERR_UNSUPPORTED: a multi-GPU store.
 * IDF: idf(i) = (float) log(1.0 + (n_docs - df[i] + 0.5) / (df[i] + 0.5)), f64 with the C library's log, every operation rounded,
 * rounded once to f32.  ott_query_sparse_idf takes ott_query_sparse's arguments and returns exactly ott_query_sparse's hits for
 * the weights fl32(weight * idf(index)) (one f32 multiplication, on the host); its messages name ott_query_sparse_idf.  A scaled
 * weight that is not finite is refused like a weight that is not — the one refusal behind device work: the counts are built
 * first where they are stale.  tests/hybrid_ref.py is the normative model, ott_sparse_plan.h states the formula in C. */
int ott_store_sparse_df(ott_store* s, void* df_out /* uint32_t[vocab] or NULL */, uint64_t* n_docs_out);
uint64_t ott_store_sparse_df_builds(const ott_store* s);
int ott_query_sparse_idf(ott_store* s, const ott_query_desc* d, const uint64_t* q_indptr /* [d->nq + 1] */,
                         const void* q_indices /* uint32_t[] */, const float* q_values,
                         ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);

/* ---- hybrid search: dense and sparse legs fused per request ------------------------------------------------
 * ott_query_fuse with sparse legs beside the dense ones (Qdrant's prefetch + fusion, Elasticsearch's rrf retriever over kNN and
 * sparse_vector, Weaviate's hybrid).  The normative statement is the numpy model tests/hybrid_ref.py.
 * d is the dense side exactly as in ott_query_fuse: d->queries holds the dense legs of request 0, then of request 1, ...; d->nq
 * their total (0: no dense stage runs and d->queries is not read); metric, take, filter, chunk mask, row mask or evaluated mask,
 * path; d->mode OTT_MODE_PER_QUERY; d->k = fused hits per request.  dense_per_request[b] and sparse_per_request[b] (uint32_t
 * [n_requests], either may hold zeros; NULL where the side has no leg at all) say how many legs of each kind request b has; the
 * sparse queries are CSR as ott_query_sparse takes them, request 0's first.
 * LEGS of request b: its dense legs in the caller's order, then its sparse legs in the caller's order; 1 to OTT_FUSE_MAX_LEGS in
 * all, legs x min(fetch, rows) at most OTT_FUSE_MAX_ENTRIES.  leg_weights ([d->nq + n_sparse] or NULL = all 1) follows that order,
 * request by request.
 * A DENSE LEG'S LIST is ott_query_fuse's: ott_query's hits for that vector with k = min(fetch, rows), on every path.
 * A SPARSE LEG'S LIST is ott_query_sparse's hits for that query with k = min(fetch, rows), take Max, the filter sparse_cmp /
 * sparse_thr (an ott_cmp; OTT_CMP_NONE = no filter: the filter in d acts on the dense legs only), the same chunk mask, row mask
 * and live mask as the dense legs, and — with OTT_HYBRID_IDF in sparse_flags — the weights scaled as ott_query_sparse_idf does.
 * The sparse stage is the sweep whatever d->path says.  A list may be shorter than fetch, or empty.
 * CONTRIBUTION, FUSED SCORE and RANKING are ott_query_fuse's, word for word, with one difference: MINMAX and DBSF normalise a leg
 * under THAT LEG'S take — d->take for a dense leg, Max for a sparse leg (a squared-L2 leg beside a sparse dot leg is the ordinary
 * case).  A call without sparse legs returns exactly ott_query_fuse's hits.
 * Both stages run on one query context under one shared lock; both kinds of list go up in one copy as the blocks the fuse kernel
 * reads, with one take byte per leg.  Stats: path_used is the dense stage's (OTT_PATH_EXACT without one); passes, bytes_scanned and
 * vectors_compared are the sums of both stages; merge_ns carries the fuse kernel's event time on top; total_ns is the whole call.
 * Refused on the host before any device work, with nothing written, each with its own message (ott_hybrid_plan.h): what
 * ott_query_fuse refuses, the leg count being dense plus sparse; per-request counts that do not add up to d->nq or n_sparse; an
 * unknown sparse_cmp or flag; and what ott_query_sparse refuses for the sparse side — no sparse rows set, rows appended since, an
 * index at or above the vocab or twice in a query, a weight that is not finite, more than OTT_SPARSE_MAX_QUERIES sparse legs,
 * a multi-GPU store, and tie orders 1 and 2 (for the whole call, whether or not a sparse leg exists).  An empty store is a valid
 * call with no hits.  One refusal comes behind device work: with OTT_HYBRID_IDF the document frequencies are built where they are
 * stale (ott_store_sparse_df's kernel) before a scaled weight that is not finite is refused; nothing is written then either.
 * OUT OF SCOPE: a metric, mask or fetch per leg; nested prefetches; legs that are stored rows; multi-GPU stores; a device route
 * for the lists; IDF restricted to a filtered subset. */
#define OTT_HYBRID_IDF 1u
int ott_query_hybrid(ott_store* s, const ott_query_desc* d, const void* dense_per_request /* uint32_t[n_requests] */,
                     const uint64_t* sq_indptr /* [n_sparse + 1] */, const void* sq_indices /* uint32_t[] */, const float* sq_values,
                     uint32_t n_sparse, const void* sparse_per_request /* uint32_t[n_requests] */,
                     uint32_t sparse_cmp /* ott_cmp */, float sparse_thr, uint32_t sparse_flags,
                     uint32_t n_requests, uint32_t fusion /* ott_fusion */, float rrf_k,
                     const float* leg_weights /* [d->nq + n_sparse] or NULL = all 1 */, uint64_t fetch,
                     ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_request, ott_stats* stats);

/* ---- binary vectors: a bit row per stored row, exact Hamming search -----------------------------------------
 * Row r of a store may carry a bit row of n_bits bits beside its dense one (Milvus' BINARY_VECTOR with HAMMING, the first stage of
 * Qdrant's and Elasticsearch's binary quantisation, embedders that emit bits).  The rows are attached to the store the way sparse
 * rows are, so row ids, chunk masks, row masks, the evaluated mask, mask slots and deleted rows mean the same for a dense and a
 * binary query.  A collection that has only bit rows is a store of dim 1.
 *
 * BITS: bit j of a row lies in bit j % 64 of 64-bit word j / 64 (the mask convention of this header); a row is ceil(n_bits / 64)
 * words, 1 <= n_bits <= OTT_BINARY_MAX_BITS, and the bits at and above n_bits in its last word are zero, in rows and in queries (a
 * set padding bit is OTT_ERR_INVALID).
 * ott_store_set_binary: `words` row-major, n == ott_store_len.  Checked on the host before any device work; a refused call changes
 * nothing.  ott_store_set_binary_sign: n_bits = dim and bit j of row r = (row[j] > 0.0f) in f32 — NaN, -0.0 and +0.0 give 0,
 * +denormals give 1: Qdrant's binary quantisation — made by a kernel from the dense rows, no host copy; refused where dim >
 * OTT_BINARY_MAX_BITS.  A second set replaces the first; ott_store_clear_binary drops the rows.  All three take the store
 * exclusively and flush staged appends first.  While bit rows are set they count as a resident metadata column (ott_store_compact
 * is refused).  Rows appended afterwards leave the bit rows in place, and a binary query then fails with OTT_ERR_INVALID ("set them
 * again").  OTT_ERR_UNSUPPORTED on a multi-GPU store.
 * In HBM the rows lie in slices of 64 rows, transposed: 16-byte unit p of the slice's 64 rows in 64 consecutive units, rows padded
 * to whole units.  ott_store_binary_info reports n_bits (0 = no bit rows) and the bytes of the layout; ott_store_read_binary
 * returns the words of a row range from that layout, row-major again, bit for bit.
 *
 * ott_query_binary: d->nq queries as q_words (uint64_t[nq * ceil(n_bits / 64)]); d->queries is not read, d->metric must be
 * OTT_METRIC_MANHATTAN (the Hamming distance is the L1 distance of the bit vectors); take (the default of that metric is Min; Max is
 * served), filter, k, chunk mask, row mask or evaluated mask mean what they mean in ott_query_sparse.  PER_QUERY, or MERGED with nq
 * == 1; at most OTT_BINARY_MAX_QUERIES queries; cap >= nq * min(k, rows).
 * The score (tests/binary_ref.py is the normative model, ott_binary_plan.h states it in C): S = (float) popcount(q XOR v), exact.
 * Every row the masks leave is a candidate; the filter acts on S; the order is S under `take` with equal S going to the lower row;
 * hit.score = S, hit.query = b.
 * OTT_ERR_UNSUPPORTED: OTT_PATH_MFMA (AUTO takes the sweep), tie orders 1 and 2, a multi-GPU store, a store of 2^32 - 16 rows or
 * more, k_eff > 512 with more than 2^26 (query, row) pairs.
 * TWO ROUTES, the same bits: the TABLE route writes a key per (query, row) and the shared top-k reads it back; the GATED route
 * fuses the selection into the sweep (a histogram of distances and a gate per workgroup and query, candidates appended to a pair
 * list, one sort) and is eligible for k_eff <= 512.  Store option "binary_gate": -1 automatic (ott_binary_plan.h), 0 always the
 * table, 1 the gated sweep wherever eligible.  The gated sweep's pair list has a capacity ("binary_gate_cap": 0 = the plan's); a
 * call that emits more is answered by the table route (a second sweep, a second host wait) and counted.
 * ott_store_binary_counters: out[0] gated calls, out[1] candidate pairs they emitted, out[2] overflows, out[3] table-route calls.
 * stats: path_used = OTT_PATH_EXACT, passes, vectors_compared = the rows the chunk mask leaves per query, bytes_scanned = the
 * layout bytes of the slices those rows lie in, per pass (an overflowed call counts both sweeps).
 * Out of scope: Jaccard / Tanimoto, binary legs in ott_query_fuse or ott_query_hybrid, multi-GPU stores, extending bit rows on
 * append, compaction with bit rows resident, asymmetric scoring of an f32 query against bit rows. */
#define OTT_BINARY_MAX_BITS 16384
#define OTT_BINARY_MAX_QUERIES 1024
int ott_store_set_binary(ott_store* s, const void* words /* uint64_t[n * ceil(n_bits / 64)] row-major */, uint64_t n, uint32_t n_bits);
int ott_store_set_binary_sign(ott_store* s);
int ott_store_clear_binary(ott_store* s);
int ott_store_binary_info(const ott_store* s, uint32_t* n_bits, uint64_t* bytes);
int ott_store_read_binary(const ott_store* s, uint64_t first_row, uint64_t n_rows, void* words_out);
int ott_query_binary(ott_store* s, const ott_query_desc* d, const void* q_words /* uint64_t[d->nq * ceil(n_bits / 64)] */,
                     ott_hit* out, uint64_t cap, uint64_t* n_out, uint64_t* n_per_query, ott_stats* stats);
int ott_store_binary_counters(const ott_store* s, uint64_t* out /* [4] */);

#ifdef __cplusplus
}
#endif
#endif
