"""Host-side mirror of otters' `meta` module (src/meta.rs) over the MI355X backend.

    meta = MetaStore.from_columns([age, grade]).with_vectors(vectors).with_chunk_size(2).build()
    res = meta.query(q, Metric.Cosine).meta_filter(col("age").gt(15) & col("grade").eq("A")).vec_filter(0.5, Cmp.Gt).take(4).collect()

What stays on the host (as in a patched otters): builders, Expr::compile, the zonemap chunk
prune (build_chunk_mask_for_plan, src/meta.rs:407-544), string predicates, result
materialisation.  What runs on the GPU: the vectors (one contiguous HBM matrix; a chunk is a
row range), numeric/datetime row predicates (ott_store_eval_row_mask), scoring of the
surviving chunks, score filter, top-k and the merge (ott_query).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math
import threading
import time
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from . import _native as N
from ._native import OttersError
from .col import Column, DataType, format_datetime, parse_datetime_millis
from .expr import CmpOp, ColumnFilter, CompiledFilter, Expr, ExprError
from .vec import GROUP_SIZE_MAX, BinaryQueryPlan, BoostCombine, BoostTerm, Cmp, DiscoverPlan, FusePlan, HybridPlan, Metric, Mode, Path, RecommendPlan, RecommendStrategy, ResolvedQuery, SparseQueryPlan, TakeType, VecStore, as_row_ids, boost_args, infer_default_take_type, mmr_args

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1


def _wrap_i32(v: int) -> int:  # Rust `i64 as i32`
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _sat_i(v: float, lo: int, hi: int) -> int:  # Rust `f64 as i32/i64`: saturating, NaN -> 0
    if math.isnan(v):
        return 0
    if v <= lo:
        return lo
    if v >= hi:
        return hi
    return int(v)


class Bloom:
    """Per-chunk string zonemap (src/meta_compute.rs:99-116 uses the fastbloom crate, which is
    randomly seeded per build; false-positive patterns are therefore not part of the contract —
    only "no false negatives", which this deterministic double-hashing filter also guarantees)."""

    def __init__(self, n_bits: int, n_hashes: int):
        self.m = max(int(n_bits), 64)
        self.k = max(int(n_hashes), 1)
        self.bits = np.zeros((self.m + 63) // 64, dtype=np.uint64)

    @staticmethod
    def with_false_pos(p: float, expected: int) -> "Bloom":
        n = max(expected, 1)
        m = int(math.ceil(-n * math.log(p) / (math.log(2) ** 2)))
        return Bloom(m, round(m / n * math.log(2)))

    @staticmethod
    def with_num_bits(bits: int, expected: int) -> "Bloom":
        n = max(expected, 1)
        return Bloom(bits, round(bits / n * math.log(2)))

    @staticmethod
    def hash_pair(s: str):
        d = hashlib.blake2b(s.encode("utf-8"), digest_size=16).digest()
        return int.from_bytes(d[:8], "little"), int.from_bytes(d[8:], "little") | 1

    def _positions(self, s: str, hp=None):
        h1, h2 = hp if hp is not None else Bloom.hash_pair(s)
        return [(h1 + i * h2) % self.m for i in range(self.k)]

    def insert(self, s: str) -> None:
        for p in self._positions(s):
            self.bits[p >> 6] |= np.uint64(1) << np.uint64(p & 63)

    def contains(self, s: str) -> bool:
        return all((int(self.bits[p >> 6]) >> (p & 63)) & 1 for p in self._positions(s))


@dataclass
class MetaQueryStats:  # src/meta.rs:832-842 (durations in seconds) + device facts
    total_chunks: int
    pruned_chunks: int
    evaluated_chunks: int
    vectors_compared: int
    prune_duration: float
    score_duration: float
    merge_duration: float
    total_duration: float
    bytes_scanned: int = 0
    path_used: int = 0
    gpu_score_ms: float = 0.0

    def format(self) -> str:  # format_query_stats, display.rs:221-249
        rows = [("total_chunks", str(self.total_chunks)), ("pruned_chunks", str(self.pruned_chunks)),
                ("evaluated_chunks", str(self.evaluated_chunks)), ("vectors_compared", str(self.vectors_compared)),
                ("prune_ms", f"{self.prune_duration * 1e3:.3f}"), ("score_ms", f"{self.score_duration * 1e3:.3f}"),
                ("merge_ms", f"{self.merge_duration * 1e3:.3f}"), ("total_ms", f"{self.total_duration * 1e3:.3f}")]
        return ascii_table(["metric", "value"], rows, title="Last Meta Query Stats")


@dataclass
class MetaBuildStats:  # src/meta.rs:844-852
    n_rows: int
    dim: int
    n_chunks: int
    vectors_ingest_duration: float
    zonemap_build_duration: float
    build_total_duration: float

    def format(self) -> str:  # format_build_stats, display.rs:196-219
        rows = [("rows", str(self.n_rows)), ("dimensions", str(self.dim)), ("chunks", str(self.n_chunks)),
                ("vector_ingest_ms", f"{self.vectors_ingest_duration * 1e3:.3f}"),
                ("zonemap_build_ms", f"{self.zonemap_build_duration * 1e3:.3f}"),
                ("build_total_ms", f"{self.build_total_duration * 1e3:.3f}")]
        return ascii_table(["metric", "value"], rows, title="MetaStore Build Stats")


def ascii_table(headers, rows, title=None) -> str:  # AsciiTable::render, display.rs:32-96 (the title, when set, is the first line)
    if not headers:
        return ""
    w = [len(h) for h in headers]
    for r in rows:
        for i, c in enumerate(r):
            w[i] = max(w[i], len(c))
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+"
    line = lambda r: "|" + "|".join(" " + c.ljust(w[i]) + " " for i, c in enumerate(r)) + "|"
    return "\n".join(([title] if title is not None else []) + [sep, line(headers), sep] + [line(r) for r in rows] + [sep])


def _fmt_cell(c: Column, i: int) -> str:
    v = c.get(i)
    if v is None:
        return "NULL"
    dt = c.dtype()
    if dt in (DataType.Float32, DataType.Float64):
        return f"{v:.4f}"
    if dt == DataType.DateTime:
        return format_datetime(v)
    return str(v)


class MetaQueryResults:  # src/meta.rs:23-40
    def __init__(self, columns, data, indices, scores):
        self.columns: List[str] = columns
        self.data: Dict[str, Column] = data
        self.indices: List[int] = indices
        self.scores: List[float] = scores

    def len(self) -> int:
        return len(self.indices)

    def __len__(self) -> int:
        return len(self.indices)

    def is_empty(self) -> bool:
        return not self.indices

    def column(self, name: str) -> Optional[Column]:
        return self.data.get(name)

    def __str__(self) -> str:  # display.rs:164-188
        headers = ["index", "score"] + self.columns
        rows = [[str(ix), f"{sc:.6f}"] + [_fmt_cell(self.data[c], i) for c in self.columns]
                for i, (ix, sc) in enumerate(zip(self.indices, self.scores))]
        return ascii_table(headers, rows)  # (no title at this revision, display.rs:164-188; the README's sample, from an earlier one, shows "Query Results" above it)


class _Zone:
    """PackedRanges (src/meta.rs:71-76): SoA min / max / non_null per chunk, in the packed dtype."""

    def __init__(self, kind, mn, mx, non_null):
        self.kind, self.min, self.max, self.non_null = kind, mn, mx, non_null


def _build_numeric_zone(c: Column, chunk_size: int, n_chunks: int) -> _Zone:
    """build_zone_stat_for_range (src/meta_compute.rs:41-98, 117-130) for every chunk at once, then
    the packing of src/meta.rs:237-271 (f64 -> f32 narrowing, i64 -> i32 wrapping)."""
    dt = c.dtype()
    vals, nulls = c.values(), c.null_mask()
    n = vals.size
    pad = n_chunks * chunk_size - n
    live = ~nulls
    if dt in (DataType.Float32, DataType.Float64):
        v = vals.astype(np.float64)
        lo = np.where(live, v, np.inf)
        hi = np.where(live, v, -np.inf)
        lo = np.concatenate([lo, np.full(pad, np.inf)]).reshape(n_chunks, chunk_size)
        hi = np.concatenate([hi, np.full(pad, -np.inf)]).reshape(n_chunks, chunk_size)
        mn = np.fmin.reduce(lo, axis=1, initial=np.inf)  # f64::min ignores NaN
        mx = np.fmax.reduce(hi, axis=1, initial=-np.inf)
        if dt == DataType.Float32:
            with np.errstate(over="ignore"):
                mn, mx = mn.astype(np.float32), mx.astype(np.float32)
            kind = "f32"
        else:
            kind = "f64"
    else:
        v = vals.astype(np.int64)
        lo = np.where(live, v, I64_MAX)
        hi = np.where(live, v, I64_MIN)
        lo = np.concatenate([lo, np.full(pad, I64_MAX, dtype=np.int64)]).reshape(n_chunks, chunk_size)
        hi = np.concatenate([hi, np.full(pad, I64_MIN, dtype=np.int64)]).reshape(n_chunks, chunk_size)
        mn, mx = lo.min(axis=1), hi.max(axis=1)
        if dt == DataType.Int32:
            mn, mx = mn.astype(np.int32), mx.astype(np.int32)  # `as i32` wraps (all-null chunk: -1 / 0)
            kind = "i32"
        else:
            kind = "i64"
    nn = np.concatenate([live, np.zeros(pad, bool)]).reshape(n_chunks, chunk_size).sum(axis=1).astype(np.uint64)
    return _Zone(kind, mn, mx, nn)


def _range_sat(mn, mx, op: CmpOp, thr):
    """zonemap test, src/type_utils.rs:762-769"""
    if op == CmpOp.Eq:
        return (mn <= thr) & (thr <= mx)
    if op == CmpOp.Lt:
        return mn < thr
    if op == CmpOp.Lte:
        return mn <= thr
    if op == CmpOp.Gt:
        return mx > thr
    if op == CmpOp.Gte:
        return mx >= thr
    return np.ones(mn.shape, bool)  # Neq: always (still gated by non_null)


def _range_all(mn, mx, op: CmpOp, thr):
    """every value of a chunk with these bounds satisfies the ROW test (the universal counterpart of _range_sat)"""
    if op == CmpOp.Eq:
        return (mn == thr) & (mx == thr)
    if op == CmpOp.Neq:
        return (mx < thr) | (mn > thr)
    if op == CmpOp.Lt:
        return mx < thr
    if op == CmpOp.Lte:
        return mx <= thr
    if op == CmpOp.Gt:
        return mn > thr
    return mn >= thr


def _row_sat(v, op: CmpOp, thr):
    """row test, src/type_utils.rs:609-616"""
    with np.errstate(invalid="ignore"):
        if op == CmpOp.Eq:
            return v == thr
        if op == CmpOp.Neq:
            return v != thr
        if op == CmpOp.Lt:
            return v < thr
        if op == CmpOp.Lte:
            return v <= thr
        if op == CmpOp.Gt:
            return v > thr
        return v >= thr


class MetaStoreBuilder:  # src/meta.rs:62-306
    def __init__(self, schema: Dict[str, DataType], columns: Dict[str, Column], device: Optional[int] = None, devices=None):
        self.schema = schema
        self.columns = columns
        self.vectors = None
        self.chunk_size = 1024
        self.bloom = ("Fpr", 0.01)
        self.device = device
        self.devices = devices  # several GPUs of this process: one store over all of them (VecStore(devices=...))
        self.sparse = None      # with_sparse: (indptr, indices, values, vocab)
        self.binary = None      # with_binary: (bits, n_bits); with_binary_sign: "sign"

    def with_vectors(self, vectors) -> "MetaStoreBuilder":
        self.vectors = vectors
        return self

    def with_chunk_size(self, chunk_size: int) -> "MetaStoreBuilder":  # src/meta.rs:86-89
        self.chunk_size = max(int(chunk_size), 1)
        return self

    def with_bloom_fpr(self, fpr: float) -> "MetaStoreBuilder":  # src/meta.rs:92-101
        f = min(max(fpr, 1e-2), 0.5) if math.isfinite(fpr) else 0.01
        self.bloom = ("Fpr", f)
        return self

    def with_bloom_bits(self, bits: int) -> "MetaStoreBuilder":  # src/meta.rs:106-110
        self.bloom = ("Bits", max(int(bits), 64))
        return self

    def with_column(self, name: str, column: Column) -> "MetaStoreBuilder":  # src/meta.rs:113-128
        if name not in self.schema:
            raise OttersError(f"unknown column '{name}' not present in schema")
        if self.schema[name] != column.dtype():
            raise OttersError(f"dtype mismatch for column '{name}': schema {self.schema[name].name}, got {column.dtype().name}")
        self.columns[name] = column
        return self

    def with_columns(self, columns) -> "MetaStoreBuilder":  # src/meta.rs:131-148
        for name, c in columns:
            self.with_column(name, c)
        return self

    def with_sparse(self, indptr, indices, values, vocab: int) -> "MetaStoreBuilder":
        """extension: a sparse row per row, as CSR (VecStore.set_sparse), for MetaStore.sparse_query.  A sparse-only collection gives
        with_vectors a matrix of dim 1."""
        self.sparse = (indptr, indices, values, int(vocab))
        return self

    def with_binary(self, bits, n_bits: Optional[int] = None) -> "MetaStoreBuilder":
        """extension: a bit row per row (VecStore.set_binary), for MetaStore.binary_query.  A binary-only collection gives
        with_vectors a matrix of dim 1."""
        self.binary = (bits, n_bits)
        return self

    def with_binary_sign(self) -> "MetaStoreBuilder":
        """extension: bit rows made from the vectors' signs on the device (VecStore.set_binary_sign)."""
        self.binary = "sign"
        return self

    def with_random_vectors(self, n_rows: int, dim: int, seed: int) -> "MetaStoreBuilder":
        """extension: rows generated on the GPU (benchmarks at sizes no host list could hold)"""
        self.vectors = ("random", int(n_rows), int(dim), int(seed))
        return self

    def build(self, _host_only: bool = False) -> "MetaStore":  # src/meta.rs:151-305
        if self.vectors is None:
            raise OttersError("vectors must be provided to build MetaStore")
        t0 = time.perf_counter()
        if isinstance(self.vectors, tuple) and self.vectors and self.vectors[0] == "random":
            _, n_rows, dim, seed = self.vectors
            mat = None
        else:
            seed = None
            if isinstance(self.vectors, np.ndarray) and self.vectors.ndim == 2:
                mat = np.ascontiguousarray(self.vectors, dtype=np.float32)
                n_rows, dim = mat.shape
            else:
                rows = [np.asarray(v, dtype=np.float32).ravel() for v in self.vectors]
                n_rows = len(rows)
                dim = rows[0].size if n_rows else 0
                for i, v in enumerate(rows):
                    if v.size != dim:
                        raise OttersError(f"vector at index {i} has dim {v.size}, expected {dim}")
                mat = np.stack(rows) if n_rows else np.zeros((0, 0), np.float32)
        for name in self.schema:
            if name not in self.columns:
                raise OttersError(f"missing column '{name}' in builder columns")
            c = self.columns[name]
            if c.len() != n_rows:
                raise OttersError(f"column '{name}' length {c.len()} does not match vectors length {n_rows}")
        if dim == 0 and n_rows > 0:
            raise OttersError("vector dimension cannot be zero")

        cs = self.chunk_size
        n_chunks = (n_rows + cs - 1) // cs
        t_ing = time.perf_counter()
        store = None
        if n_rows and not _host_only:
            store = VecStore(dim, self.device, self.devices)
            if store._options.get("tie_order") == 1:  # OTTERS_TIE_ORDER=reference: a MetaStore's outcome is one collector PER CHUNK
                store._options["tie_order"] = 2  # (any chunk size, src/meta.rs:86-89: 8-row blocks are counted from the chunk's first row)
            store.set_chunk_size(cs)
            store.reserve(n_rows)
            if mat is None:
                store.append_random(n_rows, seed)
            else:
                store.add_vectors(mat)
            if self.sparse is not None:
                store.set_sparse(*self.sparse)
            if self.binary == "sign":
                store.set_binary_sign()
            elif self.binary is not None:
                store.set_binary(*self.binary)
        elif self.sparse is not None and len(self.sparse[0]) != n_rows + 1:
            raise OttersError(f"with_sparse: indptr has {len(self.sparse[0])} entries for {n_rows} rows")
        ingest = time.perf_counter() - t_ing

        tz = time.perf_counter()
        zones: Dict[str, _Zone] = {}
        blooms: Dict[str, list] = {}
        str_nonnull: Dict[str, np.ndarray] = {}
        for name, dt in self.schema.items():
            c = self.columns[name]
            if n_chunks == 0:
                continue
            if dt == DataType.String:
                vals, nulls = c.values(), c.null_mask()
                bl, nn = [], np.zeros(n_chunks, dtype=np.uint64)
                for ch in range(n_chunks):
                    lo, hi = ch * cs, min((ch + 1) * cs, n_rows)
                    b = Bloom.with_false_pos(self.bloom[1], hi - lo) if self.bloom[0] == "Fpr" else Bloom.with_num_bits(self.bloom[1], hi - lo)
                    live = ~nulls[lo:hi]
                    for v in {v for v, ok in zip(vals[lo:hi], live) if ok}:  # inserting a value twice changes nothing
                        b.insert(v)
                    bl.append(b)
                    nn[ch] = int(live.sum())
                blooms[name], str_nonnull[name] = bl, nn
            elif store is None:
                zones[name] = _build_numeric_zone(c, cs, n_chunks)  # host numpy (CPU-only builds: tests)
        ms = MetaStore(dict(self.schema), dict(self.columns), cs, n_rows, dim, n_chunks, store, zones, blooms, str_nonnull)
        if store is not None and n_chunks:
            # numeric / datetime columns go to HBM once (row predicates run there) and their zonemaps are built there too
            for name, dt in self.schema.items():
                if dt != DataType.String:
                    zones[name] = ms.zone_stats_device(name)
        zdur = time.perf_counter() - tz
        ms._build_stats = MetaBuildStats(n_rows, dim, n_chunks, ingest, zdur, time.perf_counter() - t0)
        return ms


class MetaStore:  # src/meta.rs:48-60, 308-577
    def __init__(self, schema, columns, chunk_size, n_rows, dim, n_chunks, store, zones, blooms, str_nonnull):
        self._schema, self._columns = schema, columns
        self._chunk_size, self._n_rows, self._dim, self._n_chunks = chunk_size, n_rows, dim, n_chunks
        self._store: Optional[VecStore] = store
        self._zones, self._blooms, self._str_nonnull = zones, blooms, str_nonnull
        self._last_stats: Optional[MetaQueryStats] = None
        self._build_stats: Optional[MetaBuildStats] = None
        self._dev_cols: Dict[str, int] = {}
        self._str_codes: Dict[str, tuple] = {}
        self._group_ids: Dict[str, tuple] = {}   # distinct_by: column name -> (dense uint32 ids, n_groups), built once
        self._groups_on_device: Optional[tuple] = None  # (column, the vector store's group generation) of the ids this store uploaded last
        self._mask_lock = threading.RLock()  # build_row_mask_device + the query that reads the mask: one critical section

    # -- constructors --------------------------------------------------------------------------------
    @staticmethod
    def from_columns(columns: List[Column], device: Optional[int] = None, devices=None) -> MetaStoreBuilder:  # src/meta.rs:332-347
        return MetaStoreBuilder({c.name(): c.dtype() for c in columns}, {c.name(): c for c in columns}, device, devices)

    @staticmethod
    def from_schema(schema, device: Optional[int] = None, devices=None) -> MetaStoreBuilder:  # src/meta.rs:350-364
        return MetaStoreBuilder({n: DataType(d) for n, d in schema}, {n: Column(n, DataType(d)) for n, d in schema}, device, devices)

    # -- accessors --------------------------------------------------------------------------------------
    def schema(self):
        return self._schema

    def columns(self):
        return self._columns

    def n_chunks(self) -> int:
        return self._n_chunks

    def chunk_size(self) -> int:
        return self._chunk_size

    def set_tie_order(self, order: str) -> None:
        """ "canonical" (default) or "reference": at exact score ties keep what the reference's MetaQueryPlan::collect keeps —
        one TopKCollector per surviving chunk (src/meta_compute.rs:153-192), the per-chunk lists concatenated in chunk order,
        sorted by score and truncated (src/meta.rs:699-709).  Any chunk size (a chunk's 8-row blocks are counted from its own first row)."""
        if self._store is not None:
            self._store.set_tie_order({"canonical": "canonical", "reference": "reference_chunked"}[order])

    # deleted rows: the vector store's live mask joins every query's row mask on the device (VecStore.delete_rows); zonemaps
    # stay conservative and materialisation only ever sees returned rows, so nothing else changes here
    def delete_rows(self, ids) -> int:
        return self._store.delete_rows(ids) if self._store is not None else 0

    def restore_rows(self, ids) -> int:
        return self._store.restore_rows(ids) if self._store is not None else 0

    def live_len(self) -> int:
        return self._store.live_len() if self._store is not None else self._n_rows

    def last_query_stats(self) -> Optional[MetaQueryStats]:
        return self._last_stats

    def build_stats(self) -> Optional[MetaBuildStats]:
        return self._build_stats

    def head_n(self, n: int) -> str:  # src/meta.rs:371-374 -> metastore_head, display.rs:125-161; printed and returned
        names = sorted(self._schema)
        rows = [[str(i)] + [_fmt_cell(self._columns[c], i) for c in names] for i in range(min(n, self._n_rows))]
        out = ascii_table(["index"] + names, rows,
                          title=f"MetaStore \u2022 rows={self._n_rows} \u2022 chunks={self._n_chunks} \u2022 chunk_size={self._chunk_size}")
        print(out)
        return out

    def head(self, n: int = 5) -> str:  # src/meta.rs:366-369
        return self.head_n(n)

    def print_build_stats(self) -> None:  # src/meta.rs:546-552
        print(self._build_stats.format() if self._build_stats else "(no build stats)")

    def print_last_query_stats(self) -> None:  # src/meta.rs:554-560
        print(self._last_stats.format() if self._last_stats else "(no query stats)")

    def print_last_stats(self) -> None:  # src/meta.rs:562-566
        self.print_build_stats()
        self.print_last_query_stats()

    # -- queries ----------------------------------------------------------------------------------------
    def query(self, query, metric: Metric) -> "MetaQueryPlan":  # src/meta.rs:569-571
        return MetaQueryPlan(self, [np.asarray(query, dtype=np.float32).ravel()], metric)

    def query_batch(self, queries, metric: Metric) -> "MetaQueryPlan":  # src/meta.rs:574-576
        return MetaQueryPlan(self, [np.asarray(q, dtype=np.float32).ravel() for q in queries], metric)

    def discover(self, context, target=None, target_row=None, metric: Metric = Metric.Cosine) -> "MetaDiscoverPlan":
        """Discovery and context search (VecStore.discover; ott_query_discover) with a meta_filter: `context` is a sequence of
        (positive, negative) row id pairs counted from the store's first row."""
        return MetaDiscoverPlan(self, context, target, target_row, metric)

    def fuse(self, leg_sets, metric: Metric = Metric.Cosine) -> "MetaFusePlan":
        """Rank fusion (VecStore.fuse; ott_query_fuse) with a meta_filter: `leg_sets` is a sequence of [legs, dim] matrices, one per
        request; every leg is ranked under the same filter, then the legs of a request are fused."""
        return MetaFusePlan(self, leg_sets, metric)

    def hybrid(self, dense_sets, sparse_sets, metric: Metric = Metric.Cosine) -> "MetaHybridPlan":
        """Hybrid search (VecStore.hybrid; ott_query_hybrid) with a meta_filter: one mask for the dense and the sparse legs of every
        request; .meta_filter(expr).idf().sparse_filter(...).take(k).collect()."""
        return MetaHybridPlan(self, dense_sets, sparse_sets, metric)

    def binary_query(self, q_bits, n_bits: Optional[int] = None) -> "MetaBinaryPlan":
        """Exact Hamming search (VecStore.binary_query; ott_query_binary) with a meta_filter: `q_bits` is one bit vector or a matrix
        of them; .meta_filter(expr).take(k).collect() for one query, .collect_per_query() for a batch."""
        return MetaBinaryPlan(self, q_bits, n_bits)

    def sparse_query(self, q) -> "MetaSparsePlan":
        """Exact sparse dot search (VecStore.sparse_query; ott_query_sparse) with a meta_filter: `q` is one (indices, values) pair or
        a list of them; .meta_filter(expr).vec_filter(...).take(k).collect()."""
        return MetaSparsePlan(self, q)

    def recommend(self, positive, negative=(), metric: Metric = Metric.Cosine, strategy: RecommendStrategy = RecommendStrategy.BestScore) -> "MetaRecommendPlan":
        """Recommend by example rows (VecStore.recommend; ott_query_recommend, or ott_query_recommend_strategy for another `strategy`
        than BestScore) with a meta_filter: `positive` and `negative` are row ids of this store."""
        return MetaRecommendPlan(self, positive, negative, metric, strategy)

    # -- zonemap prune: build_chunk_mask_for_plan, src/meta.rs:407-428 ----------------------------------
    def build_chunk_mask_for_plan(self, compiled: CompiledFilter) -> np.ndarray:
        n = self._n_chunks
        if n == 0:
            return np.zeros(0, bool)
        acc = np.ones(n, bool)
        for clause in compiled.clauses:
            cm = np.zeros(n, bool)
            for leaf in clause:
                if leaf.kind == "Numeric":
                    cm |= self._numeric_leaf_chunk_mask(leaf)
                else:
                    cm |= self._string_leaf_chunk_mask(leaf)
            acc &= cm
        return acc

    def _numeric_leaf_chunk_mask(self, leaf: ColumnFilter) -> np.ndarray:  # src/meta.rs:431-521
        n = self._n_chunks
        z = self._zones.get(leaf.column)
        dt = self._schema.get(leaf.column)
        none = np.zeros(n, bool)
        if z is None:
            return none
        rhs = leaf.rhs
        if rhs.kind == "F64":
            if dt == DataType.Float32 and z.kind == "f32":
                with np.errstate(over="ignore"):
                    thr = np.float32(rhs.value)
            elif dt == DataType.Float64 and z.kind == "f64":
                thr = np.float64(rhs.value)
            elif z.kind == "i64":
                thr = np.int64(_sat_i(rhs.value, I64_MIN, I64_MAX))
            else:
                return none
        else:
            if dt == DataType.Int32 and z.kind == "i32":
                thr = np.int32(_wrap_i32(rhs.value))
            elif dt in (DataType.Int64, DataType.DateTime) and z.kind == "i64":
                thr = np.int64(rhs.value)
            else:
                return none
        return _range_sat(z.min, z.max, leaf.cmp, thr) & (z.non_null > 0)

    def _string_leaf_chunk_mask(self, leaf: ColumnFilter) -> np.ndarray:  # src/meta.rs:523-544
        n = self._n_chunks
        out = np.zeros(n, bool)
        bl = self._blooms.get(leaf.column)
        if bl is None:
            return np.ones(n, bool)  # conservatively keep when unknown
        nn = np.asarray(self._str_nonnull[leaf.column])
        if leaf.cmp == CmpOp.Neq:
            return nn > 0
        if leaf.cmp != CmpOp.Eq:
            return out
        # the literal is hashed ONCE and the filters of one shape (all chunks but a ragged last one) are tested together: their
        # words sit in one [chunks][words] matrix, built on first use (per chunk and query this loop was 3.3 us x 489 chunks)
        hp = Bloom.hash_pair(leaf.rhs)
        mats = self.__dict__.setdefault("_bloom_mats", {})
        if leaf.column not in mats:
            groups = {}
            for i, b in enumerate(bl):
                groups.setdefault((b.m, b.k), []).append(i)
            mats[leaf.column] = [(m, k, np.array(idx), np.stack([bl[i].bits for i in idx])) for (m, k), idx in groups.items()]
        for m, k, idx, words in mats[leaf.column]:
            keep = np.ones(idx.size, bool)
            for j in range(k):
                pos = (hp[0] + j * hp[1]) % m
                keep &= ((words[:, pos >> 6] >> np.uint64(pos & 63)) & np.uint64(1)).astype(bool)
            out[idx] = keep
        out &= nn > 0
        return out

    def row_mask_is_all_true(self, compiled: CompiledFilter, chunk_mask: np.ndarray) -> bool:
        """True when the zone statistics alone prove that build_row_mask_for_chunk (src/meta_compute.rs:194-232) would return
        an all-ones mask for EVERY surviving chunk: per chunk and clause some leaf on an integer / datetime column has no NULL
        in the chunk and bounds that satisfy the row test wholesale (row-level literal coercion).  The row mask can then be
        skipped — the result is the reference's, without evaluating 1 bit per row.  Float columns never qualify (their
        bounds ignore NaN rows, which fail every comparison but !=), nor do string leaves."""
        n = self._n_chunks
        if n == 0 or chunk_mask is None:
            return False
        lens = np.minimum(self._chunk_size, self._n_rows - np.arange(n, dtype=np.int64) * self._chunk_size)
        for clause in compiled.clauses:
            full = np.zeros(n, bool)
            for leaf in clause:
                z = self._zones.get(leaf.column)
                dt = self._schema.get(leaf.column)
                if leaf.kind != "Numeric" or z is None or z.kind not in ("i32", "i64") or dt not in (DataType.Int32, DataType.Int64, DataType.DateTime):
                    continue
                thr = self._row_literal(dt, leaf.rhs)
                full |= _range_all(z.min, z.max, leaf.cmp, thr) & (z.non_null.astype(np.int64) == lens)
            if not full[chunk_mask].all():
                return False
        return True

    # -- row masks: build_row_mask_for_chunk, src/meta_compute.rs:194-318 -----------------------------------
    @staticmethod
    def _row_literal(dt: DataType, rhs):
        """literal coercions of src/meta_compute.rs:249-283"""
        if dt == DataType.Float32:
            with np.errstate(over="ignore"):
                return np.float32(rhs.value)
        if dt == DataType.Float64:
            return np.float64(rhs.value)
        if dt == DataType.Int32:
            return np.int32(_wrap_i32(rhs.value) if rhs.kind == "I64" else _sat_i(rhs.value, I32_MIN, I32_MAX))
        return np.int64(rhs.value if rhs.kind == "I64" else _sat_i(rhs.value, I64_MIN, I64_MAX))

    def build_row_mask_host(self, compiled: CompiledFilter) -> np.ndarray:
        """All rows at once on the host: the checker of the GPU evaluator in the tests, and the path for plans the GPU
        evaluator does not take (a leaf naming an unknown column or one of the wrong kind)."""
        n = self._n_rows
        acc = np.ones(n, bool)
        for clause in compiled.clauses:
            cm = np.zeros(n, bool)
            for leaf in clause:
                c = self._columns.get(leaf.column)
                if c is None:
                    continue
                live = ~c.null_mask()
                if leaf.kind == "Numeric":
                    if c.dtype() == DataType.String:
                        continue
                    cm |= _row_sat(c.values(), leaf.cmp, self._row_literal(c.dtype(), leaf.rhs)) & live
                else:
                    vals = np.array(c.values(), dtype=object)
                    if leaf.cmp == CmpOp.Eq:
                        cm |= (vals == leaf.rhs) & live
                    elif leaf.cmp == CmpOp.Neq:
                        cm |= (vals != leaf.rhs) & live
            acc &= cm
        return acc

    def _string_codes(self, name: str):
        """Dictionary encoding of a string column, built once: ({value: code}, int32 codes).  The reference compares the
        strings row by row inside every surviving chunk (src/meta_compute.rs:291-318); `==` / `!=` on the strings is
        `==` / `!=` on the codes, so the row predicate runs on the GPU over a resident Int32 column like a numeric one."""
        if name not in self._str_codes:
            c = self._columns[name]
            vals = np.asarray(c.values(), dtype=object)
            uniq, inv = np.unique(vals.astype(str), return_inverse=True) if vals.size else (np.zeros(0, str), np.zeros(0, np.int64))
            self._str_codes[name] = ({u: i for i, u in enumerate(uniq.tolist())}, inv.astype(np.int32))
        return self._str_codes[name]

    def _distinct_ids(self, name: str):
        """Dense group ids of a column for distinct_by, built once per column name: (uint32[n_rows], n_groups).  Int32, Int64
        and DateTime columns group by value, String columns through _string_codes; every NULL row is a group of its own (a
        fresh id behind the values' ids).  Pure host logic."""
        if name not in self._group_ids:
            c = self._columns.get(name)
            if c is None:
                raise OttersError(f"distinct_by: unknown column '{name}'")
            dt = c.dtype()
            if dt in (DataType.Float32, DataType.Float64):
                raise OttersError(f"distinct_by: column '{name}' is a Float column; group by an Int32, Int64, DateTime or String column")
            vals = self._string_codes(name)[1] if dt == DataType.String else np.asarray(c.values())
            nulls = np.asarray(c.null_mask(), dtype=bool)
            ids = np.zeros(self._n_rows, dtype=np.int64)
            live = ~nulls
            n_val = 0
            if live.any():
                uniq, inv = np.unique(np.asarray(vals)[live], return_inverse=True)
                ids[live] = inv.reshape(-1)
                n_val = int(uniq.size)
            n_null = int(nulls.sum())
            ids[nulls] = n_val + np.arange(n_null, dtype=np.int64)
            self._group_ids[name] = (np.ascontiguousarray(ids.astype(np.uint32)), n_val + n_null)
        return self._group_ids[name]

    def _ensure_groups(self, name: str) -> int:
        """The vector store holds the ids of column `name`: uploaded once per column name and reused while they are still what
        the store holds (its group generation tells: a set_groups / clear_groups on the VecStore in between, or another
        column's distinct_by, makes this upload them again)."""
        ids, n_groups = self._distinct_ids(name)
        if self._groups_on_device != (name, self._store._groups_gen):
            self._groups_on_device = (name, self._store._set_dense_groups(ids, n_groups))
        return n_groups

    def _device_column(self, name: str) -> int:
        if name not in self._dev_cols:
            c = self._columns[name]
            if c.dtype() == DataType.String:
                vals, dt = np.ascontiguousarray(self._string_codes(name)[1]), int(DataType.Int32)
            else:
                vals, dt = np.ascontiguousarray(c.values()), int(c.dtype())
            nulls = N.pack_bits(c.null_mask()) if c.null_mask().any() else None
            cid = C.c_uint32(0)
            N.check(N.lib().ott_store_add_column(self._store._handle(), dt, N.ptr(vals), N.ptr(nulls), vals.size, C.byref(cid)))
            self._dev_cols[name] = cid.value
        return self._dev_cols[name]

    def zone_stats_device(self, name: str):
        """build_zone_stat_for_range for every chunk on the GPU (src/meta_compute.rs:41-98, 117-130), packed like
        src/meta.rs:237-271.  Returns a _Zone equal to the host-built one."""
        c = self._columns[name]
        dt = c.dtype()
        cid = self._device_column(name)
        is_f = dt in (DataType.Float32, DataType.Float64)
        mn = np.zeros(self._n_chunks, dtype=np.float64 if is_f else np.int64)
        mx = np.zeros_like(mn)
        nn = np.zeros(self._n_chunks, dtype=np.uint64)
        N.check(N.lib().ott_store_zone_stats(self._store._handle(), cid, self._chunk_size, N.ptr(mn), N.ptr(mx), N.ptr(nn)))
        if dt == DataType.Float32:
            with np.errstate(over="ignore"):
                return _Zone("f32", mn.astype(np.float32), mx.astype(np.float32), nn)
        if dt == DataType.Float64:
            return _Zone("f64", mn, mx, nn)
        if dt == DataType.Int32:
            return _Zone("i32", mn.astype(np.int32), mx.astype(np.int32), nn)
        return _Zone("i64", mn, mx, nn)

    def _device_mask_ok(self, compiled: CompiledFilter) -> bool:
        """Every leaf names a known column of a kind the GPU evaluator takes (a Numeric leaf on a String column or
        an unknown column matches nothing in the host builder: those plans stay there)."""
        for cl in compiled.clauses:
            for leaf in cl:
                c = self._columns.get(leaf.column)
                if c is None or (leaf.kind == "Numeric") == (c.dtype() == DataType.String):
                    return False
        return True

    def build_row_mask_device(self, compiled: CompiledFilter, fetch: bool = False, slot: Optional[int] = None):
        """CNF evaluated on the GPU over HBM-resident columns (numeric, datetime, dictionary-coded strings): into the store's one
        evaluated mask, or, with `slot`, into that device mask slot (ott_store_eval_row_mask_slot; the one mask is not touched)."""
        leaves = []
        for ci, clause in enumerate(compiled.clauses):
            for leaf in clause:
                c = self._columns[leaf.column]
                lf = N.Leaf()
                lf.column, lf.op, lf.clause = self._device_column(leaf.column), int(leaf.cmp), ci
                if leaf.kind == "String":
                    # src/meta_compute.rs:291-318: Eq / Neq on the non-null rows, every other operator matches nothing.
                    # A literal absent from the dictionary gets code -1 (no row has it); "matches nothing" is Eq -1.
                    code = self._string_codes(leaf.column)[0].get(leaf.rhs, -1)
                    if leaf.cmp not in (CmpOp.Eq, CmpOp.Neq):
                        lf.op, code = int(CmpOp.Eq), -1
                    lf.lit_i64 = int(code)
                elif c.dtype() in (DataType.Float32, DataType.Float64):
                    lf.lit_f64 = float(self._row_literal(c.dtype(), leaf.rhs))
                else:
                    lf.lit_i64 = int(self._row_literal(c.dtype(), leaf.rhs))
                leaves.append(lf)
            if not clause:  # an empty clause is an OR over nothing: no row passes
                raise OttersError("empty clause in compiled filter")
        arr = (N.Leaf * max(len(leaves), 1))(*leaves)
        out = np.zeros(max((self._n_rows + 63) // 64, 1), dtype=np.uint64) if fetch else None
        if slot is None:
            N.check(N.lib().ott_store_eval_row_mask(self._store._handle(), arr, len(leaves), len(compiled.clauses), N.ptr(out)))
        else:
            N.check(N.lib().ott_store_eval_row_mask_slot(self._store._handle(), int(slot), arr, len(leaves), len(compiled.clauses), N.ptr(out)))
        return N.unpack_bits(out, self._n_rows) if fetch else None


class _MetaFiltered:
    """A plan over a MetaStore (`store`) with a meta_filter: `_meta_filter` is the compiled filter, `meta_error` what collect() raises."""

    def meta_filter(self, expr: Expr):  # src/meta.rs:605-616 (error deferred to collect)
        try:
            self._meta_filter = expr.compile(self.store._schema)
            self.meta_error = None
        except ExprError as e:
            self.meta_error = f"meta_filter compile error: {e}"
        return self


class MetaQueryPlan(_MetaFiltered):  # src/meta.rs:579-830
    def __init__(self, store: MetaStore, queries, metric: Metric):
        self.store = store
        self.queries = queries
        self.metric = Metric(metric)
        self._meta_filter: Optional[CompiledFilter] = None
        self.meta_error: Optional[str] = None
        self._vec_filter = None
        self.take_type: Optional[TakeType] = None
        self.take_count: Optional[int] = None
        self._path = Path.Auto
        self._row_ids = None
        self._distinct: Optional[str] = None
        self._keep = 1  # distinct_by(name, keep=m): rows per distinct value
        self._mmr = None  # mmr(): (lambda_mult, fetch_k or None)
        self._meta_filters = None  # meta_filters(): one CompiledFilter or None per query of the batch
        self._boosts: list = []    # boost_by / boost_decay / boost_where, in the caller's order (checked at resolve(), lowered at collect())
        self._boost_combine = None  # boost_combine(): (combine, score_weight); None = (Sum, 1.0)

    def meta_filters(self, exprs) -> "MetaQueryPlan":
        """A metadata filter per query of a query_batch (a filter per request; ott_query_masks): `exprs` holds one Expr or None per
        query.  collect_per_query() then returns one MetaQueryResults per query, each exactly what
        store.query(q).meta_filter(e).take(k).collect() returns for that query alone.  Exclusive with meta_filter; not together
        with with_row_ids, distinct_by or mmr.  Errors are deferred to collect_per_query()."""
        try:
            # (an entry may be a CompiledFilter already: a server compiles a tenant's filter once)
            self._meta_filters = [e if e is None or isinstance(e, CompiledFilter) else e.compile(self.store._schema) for e in exprs]
            self.meta_error = None
        except ExprError as e:
            self.meta_error = f"meta_filter compile error: {e}"
        except TypeError:
            self.meta_error = "meta_filters takes a sequence with one Expr or None per query"
        return self

    # -- score boosting (VecQueryPlan.boost; ott_query_boost): rank by a formula of the score and the columns ---------------------------
    def boost_by(self, name: str, weight: float, origin=0, missing: float = 0.0) -> "MetaQueryPlan":
        """Adds weight x (column `name` - origin) to the ranking score; a NULL row contributes weight x missing.  Int32, Int64,
        Float32, Float64 and DateTime columns (a DateTime origin may be a datetime string); a String column is refused at
        collect(): its dictionary codes are not values.  The terms add up in the order they were given."""
        self._boosts.append(("boost_by", str(name), weight, origin, None, missing))
        return self

    def boost_decay(self, name: str, origin, scale: float, weight: float = 1.0, missing: float = 0.0) -> "MetaQueryPlan":
        """Adds weight x max(0, 1 - |column `name` - origin| / scale): 1 at the origin, 0 from `scale` away (for a DateTime column
        origin may be a datetime string and scale is in milliseconds); a NULL row contributes weight x missing."""
        self._boosts.append(("boost_decay", str(name), weight, origin, scale, missing))
        return self

    def boost_where(self, expr, weight: float) -> "MetaQueryPlan":
        """Adds `weight` for the rows that match `expr` (an Expr or a CompiledFilter).  The filter is evaluated on the GPU into a
        device mask slot where the evaluator takes it, on the host otherwise.  Exclusive with meta_filters, which uses the
        slots; not on a multi-GPU store.  A compile error surfaces at collect()."""
        try:
            compiled = expr if isinstance(expr, CompiledFilter) else expr.compile(self.store._schema)
            self._boosts.append(("boost_where", compiled, weight, None, None, None))
        except ExprError as e:
            self._boosts.append(("boost_where", f"boost_where compile error: {e}", weight, None, None, None))
        except AttributeError:
            self._boosts.append(("boost_where", "boost_where takes an Expr", weight, None, None, None))
        return self

    def boost_combine(self, combine: BoostCombine, score_weight: float = 1.0) -> "MetaQueryPlan":
        """How the boost terms' sum B joins the score S: BoostCombine.Sum (default) ranks by score_weight x S + B, BoostCombine.Mult
        by score_weight x S x (1 + B).  vec_filter then acts on that final score."""
        self._boost_combine = (combine, score_weight)
        return self

    def _boosted(self) -> bool:
        return bool(self._boosts) or self._boost_combine is not None

    def vec_filter(self, score: float, cmp: Cmp) -> "MetaQueryPlan":  # src/meta.rs:618-621
        self._vec_filter = (float(np.float32(score)), Cmp(cmp))
        return self

    def take(self, k: int) -> "MetaQueryPlan":  # src/meta.rs:623-630
        self.take_count = int(k)
        self.take_type = infer_default_take_type(self.metric)
        return self

    def with_path(self, path: Path) -> "MetaQueryPlan":
        self._path = Path(path)
        return self

    def with_row_ids(self, ids) -> "MetaQueryPlan":
        """Rank only the rows `ids` (VecQueryPlan.with_row_ids): ANDed with meta_filter and vec_filter.  Ids of chunks the zone
        maps prune are dropped on the host before the call."""
        self._row_ids = ids
        return self

    def distinct_by(self, name: str, keep: int = 1) -> "MetaQueryPlan":
        """The best `keep` rows (default: one) per distinct value of column `name`, top-k over the values
        (VecQueryPlan.one_per_group / per_group): Int32, Int64 and DateTime columns by value, String columns by string; every
        NULL row is a group of its own.  meta_filter, vec_filter and deleted rows apply before grouping; the default take becomes
        the number of groups.  With keep > 1 a value's rows come out together, best first, the values in the order of their best
        row.  Float columns, unknown columns, a batch of queries, with_row_ids and a keep outside 1 .. 16 raise OttersError at
        collect()."""
        self._distinct = str(name)
        self._keep = keep
        return self

    def mmr(self, lambda_mult: float = 0.5, fetch_k: Optional[int] = None) -> "MetaQueryPlan":
        """MMR diversity re-ranking (VecQueryPlan.mmr): of the best `fetch_k` rows that pass meta_filter and vec_filter, take(k)
        picked greedily by relevance and dissimilarity to the rows already picked; the result rows come out in pick order.  Needs
        take(k); one query, not a batch; not together with distinct_by.  Refused at collect()."""
        self._mmr = (lambda_mult, fetch_k)
        return self

    def resolve(self):
        """Host-side part of collect (src/meta.rs:632-669): k / take defaults, zonemap prune.
        Returns (ResolvedQuery, chunk_mask or None, compiled filter or None)."""
        if self.meta_error is not None:
            raise OttersError(self.meta_error)
        if self._meta_filters is not None:
            raise OttersError("meta_filters returns one result per query: use collect_per_query()")
        st = self.store
        n_groups = 0
        if self._distinct is not None:
            if len(self.queries) > 1:
                raise OttersError("distinct_by takes one query, not a batch (a merged list over several queries would need one winner per group across queries)")
            if self._row_ids is not None:
                raise OttersError("distinct_by cannot be combined with with_row_ids in this version")
            if isinstance(self._keep, bool) or not isinstance(self._keep, (int, np.integer)) or not 1 <= int(self._keep) <= GROUP_SIZE_MAX:
                raise OttersError(f"distinct_by: keep must be an integer 1 .. {GROUP_SIZE_MAX}, not {self._keep!r}")
            n_groups = st._distinct_ids(self._distinct)[1]
        mmr = None
        if self._mmr is not None:
            if self._distinct is not None:
                raise OttersError("mmr cannot be combined with distinct_by in this version")
            if len(self.queries) > 1:
                raise OttersError("mmr takes one query, not a batch")
            mmr = mmr_args(self._mmr[0], self._mmr[1], self.take_count)
        if self._boosted():
            for what, on in (("with_row_ids", self._row_ids is not None), ("distinct_by", self._distinct is not None), ("mmr", self._mmr is not None)):
                if on:
                    raise OttersError(f"boost cannot be combined with {what} in this version")
            if len(self.queries) > 1:
                raise OttersError("boost takes one query, not a batch (a merged list over several boosted queries is not served)")
            if self._path == Path.Mfma:
                raise OttersError("boost cannot be combined with Path.Mfma: a boosted score has no certified bound; use Path.Auto or Path.Exact")
            if st._store is not None and st._store.devices is not None:
                raise OttersError("boost: a multi-GPU store is not served (the columns and mask slots of a boost live on one GPU)")
            _check_boosts(self)
        k = self.take_count if self.take_count is not None else (n_groups if self._distinct is not None else st._n_rows)  # src/meta.rs:638-640
        take = self.take_type if self.take_type is not None else (infer_default_take_type(self.metric))
        for q in self.queries:
            if st._n_rows and q.size != st._dim:
                raise OttersError(f"Query vector length {q.size} does not match expected dimension {st._dim}")
        chunk_mask = st.build_chunk_mask_for_plan(self._meta_filter) if self._meta_filter is not None else None
        fc, ft = (0, 0.0) if self._vec_filter is None else (int(self._vec_filter[1]), self._vec_filter[0])
        q = np.ascontiguousarray(np.stack(self.queries)) if self.queries else np.zeros((0, st._dim), np.float32)
        rq = ResolvedQuery(queries=q, metric=int(self.metric), take=int(take), k=max(int(k), 0), filter_cmp=fc, filter_thr=ft,
                           row_mask=None, mode=int(Mode.Merged), path=int(self._path), grouped=self._distinct is not None,
                           group_size=int(self._keep) if self._distinct is not None and int(self._keep) > 1 else 0)  # (keep = 1: ott_query_groups, as before)
        rq.mmr = mmr
        if self._row_ids is not None:
            ids = as_row_ids(self._row_ids)
            if chunk_mask is not None and ids.size:  # (an id past the store's end stays: the library names it)
                inside = ids < np.uint64(st._n_rows)
                keep = np.ones(ids.size, dtype=bool)
                keep[inside] = chunk_mask[(ids[inside] // np.uint64(st._chunk_size)).astype(np.int64)]
                ids = np.ascontiguousarray(ids[keep])
            rq.row_ids = ids
        return rq, chunk_mask, self._meta_filter

    def collect_per_query(self) -> List[MetaQueryResults]:
        """One MetaQueryResults per query of a meta_filters() plan, in query order (one ott_query_masks call)."""
        if self._meta_filters is None and self.meta_error is None:
            raise OttersError("collect_per_query needs meta_filters(): one Expr or None per query")
        return _collect_per_query(self)

    def collect(self) -> MetaQueryResults:  # src/meta.rs:632-829
        t0 = time.perf_counter()
        rq, chunk_mask, compiled = self.resolve()
        st = self.store
        prune = time.perf_counter() - t0
        total_chunks = st._n_chunks
        hits = np.zeros(0, dtype=N.HIT_DTYPE)
        gstats = None
        if not self.queries:
            raise OttersError("No queries provided")
        if st._store is not None and st._n_rows and (chunk_mask is None or chunk_mask.any()):
            use_dev = False
            # the device row mask is store-global state (ott_store_eval_row_mask writes it, the query reads it): building it and
            # querying with it are one critical section per MetaStore, so two threads filtering one store cannot score with
            # each other's mask (the reference's MetaStore is !Sync, src/meta.rs:54: there the compiler forbids the race)
            with st._mask_lock:
                if self._distinct is not None:
                    st._ensure_groups(self._distinct)
                if compiled is not None and st.row_mask_is_all_true(compiled, chunk_mask):
                    pass  # the zone statistics already decide every row of every surviving chunk: no row mask needed
                elif compiled is not None:
                    if st._device_mask_ok(compiled):
                        st.build_row_mask_device(compiled)  # numeric, datetime and (dictionary-coded) string leaves alike
                        use_dev = True
                    else:
                        rq.row_mask = st.build_row_mask_host(compiled)
                if self._boosted():  # (the slots are store-global state, like the one evaluated mask: filled and read under the lock)
                    rq.boost = boost_args(_lower_boosts(self), *(self._boost_combine or (BoostCombine.Sum, 1.0)))
                hits, _, gstats = st._store._run(rq, chunk_mask=chunk_mask, use_device_row_mask=use_dev)
            st._store.last_stats = gstats
        evaluated = int(chunk_mask.sum()) if chunk_mask is not None else total_chunks
        if gstats is not None:
            compared, score_d, merge_d = gstats["vectors_compared"], gstats["score_ns"] / 1e9, gstats["merge_ns"] / 1e9
        else:
            cs, n = st._chunk_size, st._n_rows
            lens = np.minimum(cs, n - np.arange(total_chunks) * cs) if total_chunks else np.zeros(0, int)
            compared = int((lens[chunk_mask] if chunk_mask is not None else lens).sum()) * len(self.queries)
            score_d = merge_d = 0.0
        total = time.perf_counter() - t0
        st._last_stats = MetaQueryStats(total_chunks, total_chunks - evaluated, evaluated, int(compared), prune,
                                        max(total - prune - merge_d, 0.0), merge_d, total,
                                        bytes_scanned=gstats["bytes_scanned"] if gstats else 0,
                                        path_used=gstats["path_used"] if gstats else 0, gpu_score_ms=score_d * 1e3)
        return _materialise(st, hits)


def _check_boosts(plan: "MetaQueryPlan"):
    """The host-side refusals of boost_by / boost_decay / boost_where, and every origin as a number: [(kind, column name or
    CompiledFilter, weight, origin as float, scale, missing)] in the caller's order.  Pure host logic."""
    st = plan.store
    out = []
    if len(plan._boosts) > N.BOOST_MAX_TERMS:
        raise OttersError(f"boost: {len(plan._boosts)} terms are above the {N.BOOST_MAX_TERMS} one formula takes")
    if plan._boost_combine is not None:
        boost_args([], *plan._boost_combine)
    for kind, what, weight, origin, scale, missing in plan._boosts:
        if kind == "boost_where":
            if isinstance(what, str):
                raise OttersError(what)
            out.append((kind, what, weight, 0.0, None, 0.0))
            continue
        c = st._columns.get(what)
        if c is None:
            raise OttersError(f"{kind}: unknown column '{what}'")
        if c.dtype() == DataType.String:
            raise OttersError(f"{kind}: column '{what}' is a String column; its dictionary codes are not values (boost_where takes string predicates)")
        if isinstance(origin, str):
            if c.dtype() != DataType.DateTime:
                raise OttersError(f"{kind}: a datetime string is an origin for a DateTime column; '{what}' is {c.dtype().name}")
            ms = parse_datetime_millis(origin)
            if ms is None:
                raise OttersError(f"{kind}: origin '{origin}' is not a datetime string")
            origin = ms
        out.append((kind, what, weight, float(origin), scale, missing))
    # the numbers, checked as VecQueryPlan.boost checks them (the sources are filled in by _lower_boosts)
    boost_args([BoostTerm.mask_slot(0, w) if kind == "boost_where" else BoostTerm.value(0, w, o, m) if kind == "boost_by" else BoostTerm.lin_decay(0, o, sc, w, m)
                for kind, _, w, o, sc, m in out], *(plan._boost_combine or (BoostCombine.Sum, 1.0)))
    return out


def _lower_boosts(plan: "MetaQueryPlan", column_id=None, fill_slot=None):
    """boost_by / boost_decay / boost_where as the BoostTerms of VecQueryPlan.boost: a column name becomes the id of its HBM-resident
    column (column_id, default MetaStore._device_column), the i-th boost_where becomes device mask slot i, filled by
    fill_slot(slot, compiled) -- by default evaluated on the GPU (build_row_mask_device) where _device_mask_ok accepts the filter,
    evaluated on the host and written otherwise.  The caller holds the store's mask lock."""
    st = plan.store
    column_id = column_id or st._device_column

    def default_fill(slot, compiled):
        if st._device_mask_ok(compiled):
            st.build_row_mask_device(compiled, slot=slot)
        else:
            st._store.write_row_mask_slot(slot, st.build_row_mask_host(compiled))

    fill_slot = fill_slot or default_fill
    terms, n_slots = [], 0
    for kind, what, weight, origin, scale, missing in _check_boosts(plan):
        if kind == "boost_where":
            fill_slot(n_slots, what)
            terms.append(BoostTerm.mask_slot(n_slots, weight))
            n_slots += 1
        elif kind == "boost_by":
            terms.append(BoostTerm.value(column_id(what), weight, origin, missing))
        else:
            terms.append(BoostTerm.lin_decay(column_id(what), origin, scale, weight, missing))
    return terms


def _same_filter(a: CompiledFilter, b: CompiledFilter) -> bool:
    key = lambda f: [[(l.column, l.kind, int(l.cmp), repr(l.rhs)) for l in cl] for cl in f.clauses]  # noqa: E731
    return key(a) == key(b)


def _resolve_filters(plan: "MetaQueryPlan"):
    """Host-side part of MetaQueryPlan.collect_per_query: the refusals, k / take as resolve() infers them, the distinct compiled
    filters and each one's chunk mask, and the chunk mask the batch shares -- the OR of the per-filter chunk masks (None = every
    chunk: some query has no filter).  Returns (ResolvedQuery in PerQuery mode, shared chunk mask or None, distinct filters,
    their chunk masks, filter_of_query: index into the distinct filters or -1)."""
    if plan.meta_error is not None:
        raise OttersError(plan.meta_error)
    st = plan.store
    if plan._meta_filter is not None:
        raise OttersError("meta_filters cannot be combined with meta_filter: put the common condition into every filter")
    if plan._row_ids is not None:
        raise OttersError("meta_filters cannot be combined with with_row_ids in this version")
    if plan._distinct is not None:
        raise OttersError("meta_filters cannot be combined with distinct_by in this version")
    if plan._mmr is not None:
        raise OttersError("meta_filters cannot be combined with mmr in this version")
    if plan._boosted():
        raise OttersError("meta_filters cannot be combined with boost_by, boost_decay or boost_where in this version (boost_where uses the mask slots too)")
    if not plan.queries:
        raise OttersError("No queries provided")
    if len(plan._meta_filters) != len(plan.queries):
        raise OttersError(f"meta_filters: {len(plan._meta_filters)} filters for {len(plan.queries)} queries")
    if len(plan.queries) > N.MASKS_MAX_QUERIES:
        raise OttersError(f"meta_filters: {len(plan.queries)} queries are above the {N.MASKS_MAX_QUERIES} one call takes")
    for q in plan.queries:
        if st._n_rows and q.size != st._dim:
            raise OttersError(f"Query vector length {q.size} does not match expected dimension {st._dim}")
    distinct, of_query = [], []
    for f in plan._meta_filters:
        if f is None:
            of_query.append(-1)
            continue
        at = next((i for i, g in enumerate(distinct) if g is f or _same_filter(g, f)), None)
        if at is None:
            distinct.append(f)
            at = len(distinct) - 1
        of_query.append(at)
    chunk_masks = [st.build_chunk_mask_for_plan(f) for f in distinct]
    shared = None
    if distinct and -1 not in of_query:
        shared = np.zeros(st._n_chunks, dtype=bool)
        for cm in chunk_masks:
            shared |= cm
    k = plan.take_count if plan.take_count is not None else st._n_rows
    take = plan.take_type if plan.take_type is not None else infer_default_take_type(plan.metric)
    fc, ft = (0, 0.0) if plan._vec_filter is None else (int(plan._vec_filter[1]), plan._vec_filter[0])
    rq = ResolvedQuery(queries=np.ascontiguousarray(np.stack(plan.queries)), metric=int(plan.metric), take=int(take), k=max(int(k), 0), filter_cmp=fc,
                       filter_thr=ft, row_mask=None, mode=int(Mode.PerQuery), path=int(plan._path))
    return rq, shared, distinct, chunk_masks, of_query


def _collect_per_query(plan: "MetaQueryPlan"):
    """MetaQueryPlan.collect_per_query (meta_filters): every distinct filter becomes ONE mask of ott_query_masks -- evaluated on the
    GPU into a device mask slot where the evaluator takes the filter and the store is a single-GPU one (the mask never travels),
    a host mask otherwise (and for what does not fit the slots) -- and the batch runs as one call, all under the store's mask lock."""
    t0 = time.perf_counter()
    rq, shared, distinct, chunk_masks, of_query = _resolve_filters(plan)
    st = plan.store
    nq = len(plan.queries)
    prune = time.perf_counter() - t0
    hits, counts, gstats = np.zeros(0, dtype=N.HIT_DTYPE), [0] * nq, None
    if st._store is not None and st._n_rows and (shared is None or shared.any()):
        single_gpu = len(st._store.shards()) <= 1
        with st._mask_lock:  # the slots are store-global state, like the one evaluated mask: filled and read in one critical section
            mask_id, host_masks, n_slots = [], [], 0
            for f, cm in zip(distinct, chunk_masks):
                if st.row_mask_is_all_true(f, cm):
                    # the zone statistics decide every row of the filter's own surviving chunks; the chunk mask the batch shares
                    # is wider than that, so the filter's chunk mask goes as its row mask
                    host_masks.append(np.repeat(cm, st._chunk_size)[: st._n_rows])
                    mask_id.append(len(host_masks) - 1)
                elif single_gpu and n_slots < N.MASK_SLOTS and st._device_mask_ok(f):
                    st.build_row_mask_device(f, slot=n_slots)
                    mask_id.append(N.MASK_SLOT_BASE + n_slots)
                    n_slots += 1
                else:
                    host_masks.append(st.build_row_mask_host(f))
                    mask_id.append(len(host_masks) - 1)
            rq.mask_of_query = np.asarray([N.NO_MASK if i < 0 else mask_id[i] for i in of_query], dtype=np.uint32)
            rq.query_masks = np.stack(host_masks) if host_masks else np.ones((0, 0), dtype=bool)
            hits, counts, gstats = st._store._run(rq, chunk_mask=shared)
        st._store.last_stats = gstats
    total_chunks = st._n_chunks
    evaluated = int(shared.sum()) if shared is not None else total_chunks
    compared = gstats["vectors_compared"] if gstats is not None else 0
    merge_d = gstats["merge_ns"] / 1e9 if gstats is not None else 0.0
    total = time.perf_counter() - t0
    st._last_stats = MetaQueryStats(total_chunks, total_chunks - evaluated, evaluated, int(compared), prune, max(total - prune - merge_d, 0.0), merge_d, total,
                                    bytes_scanned=gstats["bytes_scanned"] if gstats else 0, path_used=gstats["path_used"] if gstats else 0,
                                    gpu_score_ms=(gstats["score_ns"] / 1e6) if gstats else 0.0)
    return _materialise(st, hits, counts)


def _materialise(st: "MetaStore", hits, counts=None):
    """The hits' rows as MetaQueryResults (src/meta.rs:722-828); with `counts`, a list of them: the hits split by the per-query
    counts."""
    names = sorted(st._schema)  # src/meta.rs:723-724

    def rows(part):
        indices = [int(i) for i in part["index"]]
        return MetaQueryResults(names, {name: st._columns[name].take(indices) for name in names}, indices, [float(s) for s in part["score"]])

    if counts is None:
        return rows(hits)
    out, at = [], 0
    for c in counts:
        out.append(rows(hits[at:at + int(c)]))
        at += int(c)
    return out


def _run_filtered(st: "MetaStore", compiled: Optional[CompiledFilter], resolved, kind: str, run):
    """The meta filter stage of the extension plans: the zone maps prune chunks, the row mask is evaluated on the device where the
    evaluator takes the filter and on the host otherwise (there ANDed with the caller's own mask, rows behind its end kept), then
    `run(resolved, chunk_mask=, use_device_row_mask=)` -- one of VecStore._run_* -- returns (a, b, stats).  Returns (a, b), or
    None when no chunk survives (nothing runs).  `kind`: the word the refusal names."""
    chunk_mask = st.build_chunk_mask_for_plan(compiled) if compiled is not None else None
    if chunk_mask is not None and not chunk_mask.any():
        return None
    with st._mask_lock:  # the device row mask is store-global state: built and read in one critical section (MetaQueryPlan.collect)
        use_dev = False
        if compiled is not None and not st.row_mask_is_all_true(compiled, chunk_mask):
            if st._device_mask_ok(compiled):
                if resolved.row_mask is not None:
                    raise OttersError(f"{kind}: with_row_mask cannot be combined with a meta_filter that needs a row mask of its own")
                st.build_row_mask_device(compiled)
                use_dev = True
            else:
                host = st.build_row_mask_host(compiled)
                if resolved.row_mask is not None:
                    m = np.ones(host.size, bool)
                    m[: min(resolved.row_mask.size, host.size)] = resolved.row_mask[: host.size]
                    host &= m
                resolved.row_mask = host
        a, b, gstats = run(resolved, chunk_mask=chunk_mask, use_device_row_mask=use_dev)
    st._store.last_stats = gstats
    return a, b


class _MetaWrapper(_MetaFiltered):
    """What the extension plans over a MetaStore share: a meta_filter, and the builder calls of the VecStore plan
    underneath (`_plan`; None where the store holds no vectors: the calls then do nothing, and collect() names the fault)."""

    def __init__(self, store: MetaStore, plan):
        self.store = store
        self._meta_filter: Optional[CompiledFilter] = None
        self.meta_error: Optional[str] = None
        self._plan = plan

    def _forward(self, name, *args):
        if self._plan is not None:
            getattr(self._plan, name)(*args)
        return self

    def vec_filter(self, score: float, cmp: Cmp):
        return self._forward("filter", score, cmp)

    filter = vec_filter

    def take(self, k: int):
        return self._forward("take", k)

    def take_min(self, k: int):
        return self._forward("take_min", k)

    def take_max(self, k: int):
        return self._forward("take_max", k)

    def with_row_mask(self, mask):
        return self._forward("with_row_mask", mask)

    def with_path(self, path: Path):
        return self._forward("with_path", path)


class MetaRecommendPlan(_MetaWrapper):
    """Recommend by example rows over a MetaStore (MetaStore.recommend; VecStore.recommend's contract): meta_filter prunes chunks
    by their zone maps and masks rows on the device, as for MetaQueryPlan.mmr; vec_filter acts on a row's best positive score (the strategy
    BestScore), on the sum S (SumScores) or on the query's score (AverageVector), as RecommendPlan.filter.  An
    example need not pass the filter: stored data is read.  Errors surface at collect()."""

    def __init__(self, store: MetaStore, positive, negative, metric: Metric, strategy: RecommendStrategy = RecommendStrategy.BestScore):
        super().__init__(store, RecommendPlan(store._store, positive, negative, metric, strategy))
        self.metric = Metric(metric)

    def fill_negative_side(self, fill: bool = True) -> "MetaRecommendPlan":
        return self._forward("fill_negative_side", fill)

    def collect_arrays(self):
        """(hits, sides), as RecommendPlan.collect_arrays returns them."""
        if self.meta_error is not None:
            raise OttersError(self.meta_error)
        st = self.store
        if st._store is None:
            raise OttersError("recommend: the store holds no vectors, so no row can be an example")
        got = _run_filtered(st, self._meta_filter, self._plan.resolve(), "recommend", st._store._run_recommend)
        return got if got is not None else (np.zeros(0, dtype=N.HIT_DTYPE), np.zeros(0, dtype=np.uint32))

    def collect(self):
        """(MetaQueryResults, sides): the hits' rows materialised as MetaQueryPlan.collect does, and their sides as a list."""
        hits, sides = self.collect_arrays()
        return _materialise(self.store, hits), sides.tolist()


class MetaFusePlan(_MetaWrapper):
    """Rank fusion over a MetaStore (MetaStore.fuse; VecStore.fuse's contract): meta_filter prunes chunks by their zone maps and
    masks rows on the device, as for MetaRecommendPlan; it and vec_filter act on every leg before the fusion.  Errors surface at
    collect()."""

    kind = "fuse"  # the word the refusals name, and the VecStore._run_* underneath

    def __init__(self, store: MetaStore, leg_sets, metric: Metric):
        super().__init__(store, FusePlan(store._store, leg_sets, metric))
        self.metric = Metric(metric)

    def rrf(self, k: float = 60.0) -> "MetaFusePlan":
        return self._forward("rrf", k)

    def dbsf(self) -> "MetaFusePlan":
        return self._forward("dbsf")

    def min_max(self) -> "MetaFusePlan":
        return self._forward("min_max")

    def weights(self, list_of_lists) -> "MetaFusePlan":
        return self._forward("weights", list_of_lists)

    def fetch(self, n: int) -> "MetaFusePlan":
        return self._forward("fetch", n)

    def validate(self) -> None:
        if self.meta_error is not None:
            raise OttersError(self.meta_error)
        if self.store._store is None:
            raise OttersError(self.kind + ": the store holds no vectors")
        self._plan.validate()

    def collect_arrays(self):
        """(hits, counts), as FusePlan.collect_arrays (HybridPlan.collect_arrays) returns them."""
        self.validate()
        st = self.store
        rf = self._plan.resolve()
        got = _run_filtered(st, self._meta_filter, rf, self.kind, getattr(st._store, "_run_" + self.kind))
        return got if got is not None else (np.zeros(0, dtype=N.HIT_DTYPE), [0] * self._plan.n_requests())

    def collect(self):
        """One MetaQueryResults per request: the hits' rows materialised as MetaQueryPlan.collect does, scores = the fused scores."""
        return _materialise(self.store, *self.collect_arrays())


class MetaHybridPlan(MetaFusePlan):
    """Hybrid search over a MetaStore (MetaStore.hybrid; VecStore.hybrid's contract): meta_filter prunes chunks by their zone maps
    and masks rows on the device, as for MetaFusePlan — ONE mask for both kinds of leg, so the same rows vanish from the dense and
    the sparse lists; vec_filter acts on the dense legs, sparse_filter on the sparse ones.  Errors surface at collect()."""

    kind = "hybrid"

    def __init__(self, store: MetaStore, dense_sets, sparse_sets, metric: Metric):
        _MetaWrapper.__init__(self, store, HybridPlan(store._store, dense_sets, sparse_sets, metric))
        self.metric = Metric(metric)

    def idf(self, on: bool = True) -> "MetaHybridPlan":
        return self._forward("idf", on)

    def sparse_filter(self, score: float, cmp: Cmp) -> "MetaHybridPlan":
        return self._forward("sparse_filter", score, cmp)


class MetaSparsePlan(_MetaWrapper):
    """Sparse search over a MetaStore (MetaStore.sparse_query; VecStore.sparse_query's contract): meta_filter prunes chunks by their
    zone maps and masks rows on the device, exactly as the dense meta query does.  Errors surface at collect()."""

    def __init__(self, store: MetaStore, q):
        super().__init__(store, SparseQueryPlan(store._store, q))

    def idf(self, on: bool = True) -> "MetaSparsePlan":
        """The query weights times idf(index) (SparseQueryPlan.idf): the collection's statistic, whatever the meta_filter keeps."""
        return self._forward("idf", on)

    def collect_arrays(self):
        """(hits, counts), as SparseQueryPlan.collect_arrays returns them."""
        if self.meta_error is not None:
            raise OttersError(self.meta_error)
        st = self.store
        if st._store is None:
            raise OttersError("sparse_query: the store holds no vectors")
        self._plan.vector_store = st._store
        rs = self._plan.resolve()
        got = _run_filtered(st, self._meta_filter, rs, "sparse_query", st._store._run_sparse)
        return got if got is not None else (np.zeros(0, dtype=N.HIT_DTYPE), [0] * int(rs.indptr.size - 1))

    def collect_per_query(self):
        """One MetaQueryResults per query: the hits' rows materialised as MetaQueryPlan.collect does, scores = S."""
        return _materialise(self.store, *self.collect_arrays())

    def collect(self):
        """The MetaQueryResults of ONE query; a batch needs collect_per_query()."""
        if len(self._plan.queries) != 1:
            raise OttersError("ott_query_sparse: a batch needs OTT_MODE_PER_QUERY (a merged list over several sparse queries is not served)")
        return self.collect_per_query()[0]


class MetaBinaryPlan(_MetaWrapper):
    """Hamming search over a MetaStore (MetaStore.binary_query; VecStore.binary_query's contract): meta_filter prunes chunks by their
    zone maps and masks rows on the device, exactly as the dense meta query does.  Errors surface at collect()."""

    def __init__(self, store: MetaStore, q_bits, n_bits=None):
        super().__init__(store, BinaryQueryPlan(store._store, q_bits, n_bits))

    def collect_arrays(self):
        """(hits, counts), as BinaryQueryPlan.collect_arrays returns them."""
        if self.meta_error is not None:
            raise OttersError(self.meta_error)
        st = self.store
        if st._store is None:
            raise OttersError("binary_query: the store holds no vectors")
        self._plan.vector_store = st._store
        rb = self._plan.resolve()
        got = _run_filtered(st, self._meta_filter, rb, "binary_query", st._store._run_binary)
        return got if got is not None else (np.zeros(0, dtype=N.HIT_DTYPE), [0] * int(rb.words.shape[0]))

    def collect_per_query(self):
        """One MetaQueryResults per query: the hits' rows materialised as MetaQueryPlan.collect does, scores = the distances."""
        return _materialise(self.store, *self.collect_arrays())

    def collect(self):
        """The MetaQueryResults of ONE query; a batch needs collect_per_query()."""
        res = self.collect_per_query()
        if len(res) != 1:
            raise OttersError("ott_query_binary: a batch needs OTT_MODE_PER_QUERY (a merged list over several binary queries is not served)")
        return res[0]


class MetaDiscoverPlan(_MetaWrapper):
    """Discovery and context search over a MetaStore (MetaStore.discover; VecStore.discover's contract): meta_filter prunes chunks
    by their zone maps and masks rows on the device, as for MetaRecommendPlan; vec_filter acts on the hit's score.  An example or
    the target row need not pass the filter: stored data is read.  Errors surface at collect()."""

    def __init__(self, store: MetaStore, context, target, target_row, metric: Metric):
        super().__init__(store, DiscoverPlan(store._store, context, target, target_row, metric) if store._store is not None else None)
        self.metric = Metric(metric)

    def min_wins(self, n: int) -> "MetaDiscoverPlan":
        return self._forward("min_wins", n)

    def collect_arrays(self):
        """(hits, wins), as DiscoverPlan.collect_arrays returns them."""
        if self.meta_error is not None:
            raise OttersError(self.meta_error)
        st = self.store
        if st._store is None or self._plan is None:
            raise OttersError("discover: the store holds no vectors, so no row can be an example")
        got = _run_filtered(st, self._meta_filter, self._plan.resolve(), "discover", st._store._run_discover)
        return got if got is not None else (np.zeros(0, dtype=N.HIT_DTYPE), np.zeros(0, dtype=np.uint32))

    def collect(self):
        """(MetaQueryResults, wins): the hits' rows materialised as MetaQueryPlan.collect does, and the pairs each hit wins as a list."""
        hits, wins = self.collect_arrays()
        return _materialise(self.store, hits), wins.tolist()
