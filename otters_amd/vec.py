"""Host-side mirror of otters' `vec` module (src/vec.rs) over the MI355X backend.

Same names, argument meaning and error strings as the reference:

    store = VecStore(3)
    store.add_vectors([[1, 0, 0], [0, 1, 0]])
    hits = store.query([1, 0, 0], Metric.Cosine).filter(0.5, Cmp.Gt).take(5).collect()

`collect()` raises `OttersError(msg)` where the reference returns `Err(msg)`.  The vectors
live in HBM behind libotters_hip.so; the scoring loop, filter and top-k run there
(ott_query).  There is no CPU path in this package.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _native as N
from ._native import OttersError


class Metric(enum.IntEnum):  # src/vec.rs:11-16
    Cosine = 0
    Euclidean = 1
    DotProduct = 2
    Manhattan = 3   # extension: L1, sum of |q[i] - v[i]| in the other metrics' order; Path.Exact only (Path.Auto sends it there)


class TakeType(enum.IntEnum):  # src/vec.rs:18-22
    Min = 0
    Max = 1


class Cmp(enum.IntEnum):  # src/vec.rs:24-31 (0 is reserved for "no filter" in the ABI)
    Lt = 1
    Gt = 2
    Lte = 3
    Gte = 4
    Eq = 5


class Mode(enum.IntEnum):
    Merged = 0     # reference semantics: one top-k over all (query, row) pairs, src/vec.rs:217-219
    PerQuery = 1   # extension


class Path(enum.IntEnum):
    Auto = 0
    Exact = 1
    Mfma = 2


@dataclass(frozen=True)
class SearchResult:  # src/vec.rs:34-38
    index: int
    score: float

    def __str__(self) -> str:  # src/vec.rs:40-44
        return f"#{self.index} score={self.score:.6f}"


class QueryBatch:
    """src/vec.rs:320-336: a single vector or a batch of vectors."""

    def __init__(self, queries):
        self.queries: list = []
        if isinstance(queries, QueryBatch):
            self.queries = list(queries.queries)
            return
        if isinstance(queries, np.ndarray):
            if queries.ndim == 1:
                self.queries = [np.asarray(queries, dtype=np.float32)]
            else:  # a batch given as a matrix stays one (a sequence of row vectors): no per-row objects, no re-stacking
                self.queries = np.ascontiguousarray(queries, dtype=np.float32)
            return
        seq = list(queries)
        if len(seq) == 0:  # Vec<Vec<f32>>::new(): an empty batch
            self.queries = []
        elif isinstance(seq[0], (list, tuple, np.ndarray)):
            self.queries = [np.asarray(q, dtype=np.float32).ravel() for q in seq]
        else:
            self.queries = [np.asarray(seq, dtype=np.float32)]


@dataclass
class ResolvedQuery:
    """What `collect()` hands to ott_query once the plan is validated."""
    queries: np.ndarray            # [nq, dim] f32
    metric: int
    take: int
    k: int
    filter_cmp: int                # 0 = none
    filter_thr: float
    row_mask: Optional[np.ndarray]  # bool[<=n] or None
    mode: int = Mode.Merged
    path: int = Path.Auto
    row_ids: Optional[np.ndarray] = None  # uint64[n_ids] (with_row_ids): only these rows are ranked, or None
    grouped: bool = False                 # one_per_group: one best hit per group, top-k over the groups (ott_query_groups)
    max_sim: bool = False                 # max_sim: the query vectors are one query's tokens, top-k groups by the sum of their best scores (ott_query_maxsim)
    group_size: int = 0                   # per_group(m): up to m hits per group (ott_query_groups_top); 0 = not a per_group plan
    group_list: Optional[np.ndarray] = None    # with_groups: uint32[n listed] dense group ids, in the caller's order, duplicates kept (ott_query_maxsim_groups), or None
    group_of_hit: Optional[np.ndarray] = None  # OUTPUT of VecStore._run for a per_group plan: uint32[n hits], the dense group id of every hit
    mmr: Optional[tuple] = None                # mmr: (lambda as float32, fetch_k) -- the picks of ott_query_mmr instead of the top-k
    mmr_values: Optional[np.ndarray] = None    # OUTPUT of VecStore._run for an mmr plan: float32[n hits], the value of every pick
    mask_of_query: Optional[np.ndarray] = None  # with_row_masks: uint32[nq] -- an index into query_masks, N.MASK_SLOT_BASE + slot, or N.NO_MASK (ott_query_masks)
    query_masks: Optional[np.ndarray] = None    # with_row_masks: bool[n distinct masks, mask bits], every mask padded with True to the longest
    boost: Optional[tuple] = None               # boost: (N.BoostTerm array or None, n_terms, combine, score_weight) -- ranked by the formula (ott_query_boost)


def as_row_ids(ids) -> np.ndarray:
    """A candidate id list as uint64[n]: any integer sequence or array; a negative or non-integer id raises OttersError."""
    a = np.asarray(ids)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint64)
    a = a.ravel()
    if a.dtype == bool or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise OttersError(f"row ids must be integers, not {a.dtype}")
    if np.issubdtype(a.dtype, np.floating):
        if not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
            raise OttersError("row ids must be integers")
        if a.min() < 0:
            raise OttersError(f"row id {int(a.min())} is negative")
        if a.max() >= 2.0 ** 64:
            raise OttersError("row ids must fit 64 bits")
        return np.ascontiguousarray(a.astype(np.uint64))
    if np.issubdtype(a.dtype, np.signedinteger) and int(a.min()) < 0:
        raise OttersError(f"row id {int(a.min())} is negative")
    return np.ascontiguousarray(a.astype(np.uint64))


def dense_group_ids(ids):
    """Group labels -> (uint32[n] dense ids, n_groups): any integer array; equal labels share an id, ids are 0 .. n_groups - 1 in
    the labels' sorted order (np.unique).  Pure host logic."""
    a = np.asarray(ids)
    if a.ndim != 1:
        a = a.ravel()
    if a.size == 0:
        return np.zeros(0, dtype=np.uint32), 0
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise OttersError(f"group ids must be integers, not {a.dtype}")
    uniq, inv = np.unique(a, return_inverse=True)
    if uniq.size >= 2 ** 32:
        raise OttersError("more than 2^32 - 1 groups")
    return np.ascontiguousarray(inv.reshape(-1).astype(np.uint32)), int(uniq.size)


def dense_listed_groups(store: "VecStore", listed) -> np.ndarray:
    """with_groups' labels as uint32 dense group ids of `store`, in the caller's order, duplicates kept (the library sorts and dedupes
    them); a label no row carries raises OttersError.  Pure host logic."""
    a = np.asarray(listed)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint32)
    a = a.ravel()
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise OttersError(f"group labels must be integers, not {a.dtype}")
    labels = store.group_labels()
    if labels is None:  # the ids were set dense: a label is an id
        bad = (a < 0) | (a >= store.group_count()) if np.issubdtype(a.dtype, np.signedinteger) else (a >= store.group_count())
        if bad.any():
            raise OttersError(f"with_groups: group {int(a[bad][0])} is not one of the store's {store.group_count()} groups")
        return np.ascontiguousarray(a.astype(np.uint32))
    at = np.searchsorted(labels, a)  # labels: sorted and duplicate-free (np.unique)
    at_c = np.minimum(at, labels.size - 1)
    bad = labels[at_c] != a
    if bad.any():
        raise OttersError(f"with_groups: no row carries the group label {int(a[bad][0])}")
    return np.ascontiguousarray(at_c.astype(np.uint32))


GROUP_SIZE_MAX = 16  # include/otters_hip.h: OTT_GROUP_SIZE_MAX
MAXSIM_BATCH_MAX = 4096  # include/otters_hip.h: OTT_MAXSIM_BATCH_MAX
MMR_MAX_FETCH = 1024  # include/otters_hip.h: OTT_MMR_MAX_FETCH


def lower_row_masks(masks):
    """with_row_masks' entries as (mask_of_query uint32[nq], query_masks bool[n distinct, bits]): entries that are the same object
    or equal arrays share one mask (it is uploaded once), None becomes N.NO_MASK, shorter masks are padded with True to the
    longest (rows at or beyond a mask's length are kept)."""
    arrays, of_query, by_id = [], [], {}
    for m in masks:
        if m is None:
            of_query.append(N.NO_MASK)
            continue
        if id(m) in by_id:
            of_query.append(by_id[id(m)])
            continue
        a = np.asarray(m, dtype=bool).ravel()
        at = next((i for i, b in enumerate(arrays) if b.size == a.size and np.array_equal(a, b)), None)
        if at is None:
            arrays.append(a)
            at = len(arrays) - 1
        by_id[id(m)] = at
        of_query.append(at)
    bits = max((a.size for a in arrays), default=0)
    if bits == 0:  # only empty masks: every row is at or beyond their length, so every row is kept
        return np.full(len(of_query), N.NO_MASK, dtype=np.uint32), np.ones((0, 0), dtype=bool)
    qm = np.ones((len(arrays), bits), dtype=bool)
    for i, a in enumerate(arrays):
        qm[i, : a.size] = a
    return np.asarray(of_query, dtype=np.uint32), qm


def mmr_default_fetch_k(k: int) -> int:
    """mmr()'s candidate count when the caller names none: five times the picks, at least 20, at most OTT_MMR_MAX_FETCH"""
    return min(MMR_MAX_FETCH, max(20, 5 * int(k)))


def mmr_args(lam, fetch_k, take_count):
    """mmr()'s arguments checked against the plan's take: (lambda as float32, fetch_k).  Pure host logic."""
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not 0.0 <= float(lam) <= 1.0:
        raise OttersError(f"mmr: lambda_mult must be a number in [0, 1], not {lam!r}")
    if take_count is None:
        raise OttersError("mmr needs an explicit take: the number of picks (take, take_min or take_max)")
    k = int(take_count)
    if k < 1:
        raise OttersError(f"mmr: take must be at least 1, not {k}")
    if fetch_k is None:
        fetch_k = mmr_default_fetch_k(k)
    elif isinstance(fetch_k, bool) or not isinstance(fetch_k, (int, np.integer)):
        raise OttersError(f"mmr: fetch_k must be an integer, not {fetch_k!r}")
    fetch_k = int(fetch_k)
    if fetch_k > MMR_MAX_FETCH:
        raise OttersError(f"mmr: fetch_k {fetch_k} is above the limit of {MMR_MAX_FETCH} candidates")
    if k > fetch_k:
        raise OttersError(f"mmr: take({k}) asks for more picks than fetch_k = {fetch_k} candidates")
    return np.float32(lam), fetch_k


class BoostCombine(enum.IntEnum):  # include/otters_hip.h: ott_boost_combine
    Sum = 0   # F = score_weight * S + B
    Mult = 1  # F = score_weight * S * (1 + B)


@dataclass(frozen=True)
class BoostTerm:
    """One term of a boost formula (VecQueryPlan.boost; include/otters_hip.h: ott_boost_term).  `source` is a column id of
    VecStore.add_column (value, lin_decay) or a device mask slot (mask_slot)."""
    kind: int
    source: int
    weight: float
    scale: float = 0.0
    origin: float = 0.0
    missing: float = 0.0

    @staticmethod
    def value(column: int, weight: float, origin: float = 0.0, missing: float = 0.0) -> "BoostTerm":
        """weight x (the column's value - origin); a NULL row contributes weight x missing"""
        return BoostTerm(N.BOOST_VALUE, int(column), float(weight), 0.0, float(origin), float(missing))

    @staticmethod
    def lin_decay(column: int, origin: float, scale: float, weight: float = 1.0, missing: float = 0.0) -> "BoostTerm":
        """weight x max(0, 1 - |value - origin| / scale); a NULL row contributes weight x missing"""
        return BoostTerm(N.BOOST_LIN_DECAY, int(column), float(weight), float(scale), float(origin), float(missing))

    @staticmethod
    def mask_slot(slot: int, weight: float) -> "BoostTerm":
        """weight for the rows device mask slot `slot` keeps (and the rows behind its end), 0 for the others"""
        return BoostTerm(N.BOOST_MASK, int(slot), float(weight))


def boost_args(terms, combine, score_weight):
    """boost()'s arguments checked as ott_query_boost checks them: (ctypes array of N.BoostTerm or None, n_terms, combine, score
    weight as float32).  Pure host logic."""
    try:
        terms = list(terms)
    except TypeError:
        raise OttersError("boost takes a sequence of BoostTerm") from None
    if any(not isinstance(t, BoostTerm) for t in terms):
        raise OttersError("boost takes a sequence of BoostTerm (BoostTerm.value, BoostTerm.lin_decay, BoostTerm.mask_slot)")
    if len(terms) > N.BOOST_MAX_TERMS:
        raise OttersError(f"boost: {len(terms)} terms are above the {N.BOOST_MAX_TERMS} one formula takes")
    try:
        combine = BoostCombine(combine)
    except ValueError:
        raise OttersError(f"boost: combine must be BoostCombine.Sum or BoostCombine.Mult, not {combine!r}") from None
    if not np.isfinite(np.float32(score_weight)):
        raise OttersError("boost: score_weight is not finite")
    arr = (N.BoostTerm * max(len(terms), 1))()
    for j, t in enumerate(terms):
        if not 0 <= t.source < 2 ** 32:
            raise OttersError(f"boost: term {j}: {t.source} is no column id or slot")
        with np.errstate(over="ignore"):
            w, sc, ms = np.float32(t.weight), np.float32(t.scale), np.float32(t.missing)
        if not (np.isfinite(w) and np.isfinite(ms) and np.isfinite(t.origin)):
            raise OttersError(f"boost: term {j}: weight, origin and missing must be finite")
        if t.kind == N.BOOST_LIN_DECAY and not (np.isfinite(sc) and sc > 0):
            raise OttersError(f"boost: term {j}: scale must be finite and above 0")
        arr[j].kind, arr[j].source, arr[j].weight, arr[j].scale, arr[j].origin, arr[j].missing = t.kind, t.source, w, sc, float(t.origin), ms
    return (arr if terms else None), len(terms), int(combine), float(np.float32(score_weight))


def infer_default_take_type(metric: Metric) -> TakeType:  # src/vec.rs:92-98
    return TakeType.Min if metric in (Metric.Euclidean, Metric.Manhattan) else TakeType.Max


def split_results(hits, counts, index=None) -> list:
    """Hits and per-query counts -> one list of SearchResult per query.  `index`: what a result reports in place of hits["index"]
    (the caller's group labels)."""
    # .tolist() first: building the objects from Python scalars is several times faster than indexing a record array
    idx, sc = (hits["index"] if index is None else index).tolist(), hits["score"].tolist()
    out, o = [], 0
    for c in counts:
        out.append([SearchResult(i, x) for i, x in zip(idx[o:o + c], sc[o:o + c])])
        o += c
    return out


class _ScorePlan:
    """What the extension plans share: the score filter, the take and the caller's row mask, and how they lower.  A plan sets
    `search_metric`, which decides the take type of a take(n) that names none."""

    def __init__(self):
        self.filter_criteria: Optional[tuple] = None
        self.take_type: Optional[TakeType] = None
        self.take_count: Optional[int] = None
        self.row_mask: Optional[np.ndarray] = None

    def with_row_mask(self, mask):  # bit i = row i, True = keep
        self.row_mask = np.asarray(mask, dtype=bool).ravel()
        return self

    def filter(self, score: float, cmp: Cmp):
        self.filter_criteria = (float(np.float32(score)), Cmp(cmp))
        return self

    def _take_with_options(self, count: int, take_type: Optional[TakeType]):
        self.take_count = int(count)
        if take_type is not None:
            self.take_type = take_type
        elif self.take_type is None:
            self.take_type = infer_default_take_type(self.search_metric)
        return self

    def take(self, count: int):
        return self._take_with_options(count, None)

    def take_min(self, count: int):
        return self._take_with_options(count, TakeType.Min)

    def take_max(self, count: int):
        return self._take_with_options(count, TakeType.Max)

    def _lowered(self, default_k: int, default_take: Optional[TakeType] = None):
        """(take, k, filter_cmp, filter_thr) as a resolved record carries them; a plan without a take returns `default_k` hits,
        ranked by `default_take` (default: what the metric infers)."""
        k = self.take_count if self.take_count is not None else default_k
        take = self.take_type if self.take_type is not None else default_take if default_take is not None else infer_default_take_type(self.search_metric)
        fc, ft = (0, 0.0) if self.filter_criteria is None else (int(self.filter_criteria[1]), self.filter_criteria[0])
        return int(take), max(int(k), 0), fc, ft


class _PathScorePlan(_ScorePlan):
    """A _ScorePlan whose caller may name the path."""

    def __init__(self):
        super().__init__()
        self.path = Path.Auto

    def with_path(self, path: Path):
        self.path = Path(path)
        return self


class VecQueryPlan:
    """src/vec.rs:55-312: lazy builder; errors surface at collect()."""

    def __init__(self):  # VecQueryPlan::new, src/vec.rs:70-82
        self.query_vectors: Optional[list] = None
        self.search_metric: Optional[Metric] = None
        self.filter_criteria: Optional[tuple] = None
        self.take_type: Optional[TakeType] = None
        self.take_count: Optional[int] = None
        self.vector_store: Optional["VecStore"] = None
        self.error: Optional[str] = None
        self.row_mask: Optional[np.ndarray] = None
        self.row_ids = None  # with_row_ids: the list as the caller gave it (checked at validate())
        self._mode = Mode.Merged
        self._path = Path.Auto
        self._grouped = False
        self._max_sim = False
        self._per_group = None  # per_group(m): m as the caller gave it (checked at validate())
        self.group_list = None  # with_groups: the labels as the caller gave them (mapped at validate())
        self._mmr = None        # mmr(): (lambda_mult, fetch_k or None) as the caller gave them (checked at validate())
        self.row_masks = None   # with_row_masks: one boolean array or None per query, as the caller gave them (checked at validate())
        self._boost = None      # boost(): (terms, combine, score_weight) as the caller gave them (checked at validate())

    @staticmethod
    def new() -> "VecQueryPlan":
        return VecQueryPlan()

    # -- builder -------------------------------------------------------------------------------
    def with_vector_store(self, store: "VecStore") -> "VecQueryPlan":  # src/vec.rs:118-121
        if self.error is None:
            self.vector_store = store
        return self

    def with_query_vectors(self, queries) -> "VecQueryPlan":  # src/vec.rs:123-138
        if self.error is None:
            self.query_vectors = QueryBatch(queries).queries
        return self

    def with_metric(self, metric: Metric) -> "VecQueryPlan":  # src/vec.rs:140-143
        if self.error is None:
            self.search_metric = Metric(metric)
        return self

    def with_row_mask(self, mask) -> "VecQueryPlan":  # src/vec.rs:145-148; bit i = row i, True = keep
        if self.error is None:
            self.row_mask = np.asarray(mask, dtype=bool).ravel()
        return self

    def filter(self, score: float, cmp: Cmp) -> "VecQueryPlan":  # src/vec.rs:150-153
        if self.error is None:
            self.filter_criteria = (float(np.float32(score)), Cmp(cmp))
        return self

    def _take_with_options(self, count: int, take_type: Optional[TakeType]) -> "VecQueryPlan":  # src/vec.rs:103-116
        if self.error is not None:
            return self
        self.take_count = int(count)
        if take_type is not None:
            self.take_type = take_type
        elif self.take_type is None and self.search_metric is not None:
            self.take_type = infer_default_take_type(self.search_metric)
        return self

    def take(self, count: int) -> "VecQueryPlan":  # src/vec.rs:155-158
        return self._take_with_options(count, None)

    def take_min(self, count: int) -> "VecQueryPlan":  # src/vec.rs:160-163
        return self._take_with_options(count, TakeType.Min)

    def take_max(self, count: int) -> "VecQueryPlan":  # src/vec.rs:165-168
        return self._take_with_options(count, TakeType.Max)

    # -- extensions (not in the reference) -----------------------------------------------------
    def per_query(self) -> "VecQueryPlan":
        """Return k hits for every query instead of one merged list (collect() then returns a list of lists)."""
        self._mode = Mode.PerQuery
        return self

    def with_path(self, path: Path) -> "VecQueryPlan":
        self._path = Path(path)
        return self

    def with_row_ids(self, ids) -> "VecQueryPlan":
        """Rank only the rows `ids` (counted from the store's first row; any integer sequence or array, any order, duplicates
        allowed): the hits of the same plan with a row mask that keeps just these rows, ANDed with with_row_mask and the
        deleted rows (ott_query_ids).  The work follows the list, not the store.  A negative or non-integer id raises at
        validate(), an id >= len() when the query runs."""
        if self.error is None:
            self.row_ids = ids
        return self

    def with_row_masks(self, masks) -> "VecQueryPlan":
        """A row mask per query (a metadata filter per request; ott_query_masks): `masks` holds one entry per query of the batch, a
        boolean array (True = keep; rows at or beyond its length are kept) or None.  Query b's hits are exactly the hits of the
        same plan for that query alone with with_row_mask(common & masks[b]); with_row_mask stays the mask common to all.
        Entries that are the same object or equal arrays are uploaded once, and their queries share batch passes.  Needs
        per_query(); not together with with_row_ids, one_per_group, per_group, max_sim or mmr in this version."""
        if self.error is None:
            self.row_masks = masks
        return self

    def boost(self, terms, combine: BoostCombine = BoostCombine.Sum, score_weight: float = 1.0) -> "VecQueryPlan":
        """Score boosting (ott_query_boost): rank by F = score_weight x S + B (Sum) or score_weight x S x (1 + B) (Mult), S the
        row's score and B the sum, in the given order, of the `terms` (BoostTerm.value / lin_decay / mask_slot over the columns of
        VecStore.add_column and the slots of VecStore.write_row_mask_slot; at most 8).  Every surviving row is ranked by F, not
        just the best by S; filter() acts on F, a row whose F is NaN is dropped, collect() and collect_arrays() return F as the
        score.  All of it in f32, one rounded operation at a time.  A batch needs per_query(); not together with with_row_ids,
        with_row_masks, one_per_group, per_group, max_sim, mmr or Path.Mfma; not on a multi-GPU store."""
        if self.error is None:
            self._boost = (terms, combine, score_weight)
        return self

    def one_per_group(self) -> "VecQueryPlan":
        """One best hit per group, top-k over the groups (VecStore.set_groups; ott_query_groups): the hits of the same plan with
        the default take after dropping every hit whose group occurred earlier, cut at take(k); the default take becomes
        group_count().  Row mask, deleted rows and filter apply before grouping; ties are always in the canonical order.  A
        batch needs per_query().  Not together with with_row_ids in this version."""
        if self.error is None:
            self._grouped = True
        return self

    def per_group(self, m: int) -> "VecQueryPlan":
        """Up to `m` best hits per group, top-k over the groups (VecStore.set_groups; ott_query_groups_top): of the hits of the same
        plan with the default take, a hit is kept iff fewer than m earlier hits have its group; the groups rank by their first hit
        (one_per_group's ranking), take(k) keeps the first k groups, and each group's hits come out contiguous, best first.  It
        implies grouping — per_group(1) returns one_per_group's hits — and the default take is group_count().  collect_arrays()
        returns (hits, counts, groups) with the dense group id of every hit; collect() the SearchResults in output order (one
        list per query with per_query()); collect_groups() [(label, [SearchResult, ...]), ...].  m is 1 .. 16; not together with
        with_row_ids or max_sim; a batch needs per_query(); not on a multi-GPU store."""
        if self.error is None:
            self._grouped = True
            self._per_group = m
        return self

    def max_sim(self) -> "VecQueryPlan":
        """Late-interaction (MaxSim) search (VecStore.set_groups; ott_query_maxsim): the plan's query vectors are the TOKENS of one
        query; a group's score is the sum over the tokens, in token order, of the token's best score among the group's surviving
        rows, and the hits are the top groups by that sum (then lower group id).  take(k) infers Min / Max from the metric as
        usual (Euclidean / Manhattan: the sum of minimum distances); a plan without take ranks by Max and returns every group
        (the default take becomes group_count()).  filter() applies to the sum.  collect_arrays() returns hits whose `index` is
        the dense group id; collect() returns SearchResult(label, score) with the caller's own group label.  Not together with
        with_row_ids, one_per_group or per_query; not on a multi-GPU store.  with_groups(labels) re-ranks only the listed groups."""
        if self.error is None:
            self._max_sim = True
        return self

    def with_groups(self, labels) -> "VecQueryPlan":
        """Re-rank only the listed groups (ott_query_maxsim_groups): the hits of the same max_sim() plan with a row mask that keeps
        just the rows whose group is listed, ANDed with with_row_mask and the deleted rows.  The work follows the list, not the
        store.  `labels` are the caller's own group labels as set_groups got them (dense ids where the ids were set dense), any
        integer sequence or array, any order, duplicates allowed; a label no row carries raises at validate().  The default take
        becomes the number of distinct listed groups.  Only with max_sim() in this version."""
        if self.error is None:
            self.group_list = labels
        return self

    def mmr(self, lambda_mult: float = 0.5, fetch_k: Optional[int] = None) -> "VecQueryPlan":
        """MMR diversity re-ranking (maximal marginal relevance; ott_query_mmr): of the plan's best `fetch_k` hits -- exactly the
        hits of the same plan with take(fetch_k) -- pick take(k) greedily, each pick the one that maximises lambda_mult x relevance
        - (1 - lambda_mult) x its largest similarity to a row already picked (for a Min take both terms change sign).  Similarity
        is the plan's own metric between the stored rows.  lambda_mult = 1 returns the plain top-k, 0 ranks by diversity alone.
        fetch_k defaults to min(1024, max(20, 5 k)).  The hits come out in pick order; collect_mmr() also returns every pick's
        value.  Needs an explicit take / take_min / take_max; combines with filter, with_row_mask, with_row_ids, per_query (one
        MMR per query) and with_path; not with one_per_group, per_group or max_sim; not on a multi-GPU store."""
        if self.error is None:
            self._mmr = (lambda_mult, fetch_k)
        return self

    def _mmr_args(self):
        return mmr_args(self._mmr[0], self._mmr[1], self.take_count)

    def _dense_group_list(self) -> np.ndarray:
        """with_groups' labels as uint32 dense group ids, in the caller's order (the library sorts and dedupes them)"""
        return dense_listed_groups(self.vector_store, self.group_list)

    # -- execution -----------------------------------------------------------------------------
    def validate(self) -> None:  # src/vec.rs:170-203
        if self.error is not None:
            raise OttersError(self.error)
        if self.query_vectors is None:
            raise OttersError("Query vectors or their norms are not set")
        if self.search_metric is None:
            raise OttersError("Search metric is not set")
        if self.vector_store is None:
            raise OttersError("Vector store is not set")
        if len(self.query_vectors) == 0:
            raise OttersError("No queries provided")
        if self.row_ids is not None:
            as_row_ids(self.row_ids)
        if self._per_group is not None:
            m = self._per_group
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= GROUP_SIZE_MAX:
                raise OttersError(f"per_group: the group size must be an integer 1 .. {GROUP_SIZE_MAX}, not {m!r}")
            if self.row_ids is not None:
                raise OttersError("per_group cannot be combined with with_row_ids in this version; use with_row_mask")
            if self._max_sim:
                raise OttersError("max_sim cannot be combined with per_group: a hit of max_sim is a group already")
        if self._grouped and self.row_ids is not None:
            raise OttersError("one_per_group cannot be combined with with_row_ids in this version; use with_row_mask")
        if self._max_sim and self.row_ids is not None:
            raise OttersError("max_sim cannot be combined with with_row_ids in this version; use with_row_mask")
        if self._max_sim and self._grouped:
            raise OttersError("max_sim cannot be combined with one_per_group: a hit of max_sim is a group already")
        if self._max_sim and self._mode == Mode.PerQuery:
            raise OttersError("max_sim cannot be combined with per_query: the query vectors are the tokens of one query")
        if self.group_list is not None:
            if self._per_group is not None:
                raise OttersError("with_groups cannot be combined with per_group in this version; use with_row_mask")
            if self._grouped:
                raise OttersError("with_groups cannot be combined with one_per_group in this version; use with_row_mask")
            if self.row_ids is not None:
                raise OttersError("with_groups cannot be combined with with_row_ids in this version; use with_row_mask")
            if not self._max_sim:
                raise OttersError("with_groups needs max_sim in this version; use with_row_mask")
            self._dense_group_list()
        if self._mmr is not None:
            if self._per_group is not None:
                raise OttersError("mmr cannot be combined with per_group in this version")
            if self._grouped:
                raise OttersError("mmr cannot be combined with one_per_group in this version")
            if self._max_sim:
                raise OttersError("mmr cannot be combined with max_sim: a hit of max_sim is a group, not a row")
            if len(self.query_vectors) > 1 and self._mode != Mode.PerQuery:
                raise OttersError("mmr takes one query; a batch needs per_query() (one MMR per query)")
            self._mmr_args()
        if self.row_masks is not None:
            if self.row_ids is not None:
                raise OttersError("with_row_masks cannot be combined with with_row_ids in this version; put the ids into the masks")
            if self._per_group is not None:
                raise OttersError("with_row_masks cannot be combined with per_group in this version")
            if self._grouped:
                raise OttersError("with_row_masks cannot be combined with one_per_group in this version")
            if self._max_sim:
                raise OttersError("with_row_masks cannot be combined with max_sim: the query vectors are the tokens of one query")
            if self._mmr is not None:
                raise OttersError("with_row_masks cannot be combined with mmr in this version")
            if self._mode != Mode.PerQuery:
                raise OttersError("with_row_masks needs per_query(): a merged list over differently masked queries is not served")
            try:
                n_given = len(self.row_masks)
            except TypeError:
                raise OttersError("with_row_masks takes a sequence with one boolean array or None per query") from None
            if n_given != len(self.query_vectors):
                raise OttersError(f"with_row_masks: {n_given} masks for {len(self.query_vectors)} queries")
            if len(self.query_vectors) > N.MASKS_MAX_QUERIES:
                raise OttersError(f"with_row_masks: {len(self.query_vectors)} queries are above the {N.MASKS_MAX_QUERIES} one call takes")
        if self._boost is not None:
            for what, on in (("with_row_ids", self.row_ids is not None), ("with_row_masks", self.row_masks is not None),
                             ("per_group", self._per_group is not None), ("one_per_group", self._grouped), ("max_sim", self._max_sim),
                             ("mmr", self._mmr is not None)):
                if on:
                    raise OttersError(f"boost cannot be combined with {what} in this version")
            if self._path == Path.Mfma:
                raise OttersError("boost cannot be combined with Path.Mfma: a boosted score has no certified bound; use Path.Auto or Path.Exact")
            if len(self.query_vectors) > 1 and self._mode != Mode.PerQuery:
                raise OttersError("boost takes one query; a batch needs per_query() (a merged list over several boosted queries is not served)")
            if len(self.query_vectors) > N.BOOST_MAX_QUERIES:
                raise OttersError(f"boost: {len(self.query_vectors)} queries are above the {N.BOOST_MAX_QUERIES} one call takes")
            if self.vector_store.devices is not None:
                raise OttersError("boost: a multi-GPU store is not served (the columns and mask slots of a boost live on one GPU)")
            boost_args(*self._boost)
        dim = self.vector_store.dim
        if isinstance(self.query_vectors, np.ndarray):  # a matrix: every row has the same length
            if self.query_vectors.shape[1] != dim:
                raise OttersError(f"Query vector length {self.query_vectors.shape[1]} does not match expected dimension {dim}")
            return
        for q in self.query_vectors:
            if len(q) != dim:
                raise OttersError(f"Query vector length {len(q)} does not match expected dimension {dim}")

    def resolve(self) -> ResolvedQuery:
        """Validate and lower the plan (src/vec.rs:207-214).  Pure host logic, no GPU."""
        self.validate()
        store = self.vector_store
        if isinstance(self.query_vectors, np.ndarray):
            queries = self.query_vectors
        else:
            queries = np.ascontiguousarray(np.stack(self.query_vectors).astype(np.float32, copy=False))
        group_list = None if self.group_list is None else self._dense_group_list()
        if self.take_count is not None:
            k = self.take_count
        elif group_list is not None:
            k = int(np.unique(group_list).size)
        else:
            k = store.group_count() if self._grouped or self._max_sim else store.len()  # src/vec.rs:213
        take = self.take_type if self.take_type is not None else TakeType.Max  # src/vec.rs:214
        fc, ft = (0, 0.0) if self.filter_criteria is None else (int(self.filter_criteria[1]), self.filter_criteria[0])
        moq, qm = (None, None) if self.row_masks is None else lower_row_masks(self.row_masks)
        return ResolvedQuery(queries=queries, metric=int(self.search_metric), take=int(take), k=max(int(k), 0),
                             filter_cmp=fc, filter_thr=ft, row_mask=self.row_mask, mode=int(self._mode), path=int(self._path),
                             row_ids=None if self.row_ids is None else as_row_ids(self.row_ids), grouped=self._grouped,
                             max_sim=self._max_sim, group_size=0 if self._per_group is None else int(self._per_group), group_list=group_list,
                             mmr=None if self._mmr is None else self._mmr_args(), mask_of_query=moq, query_masks=qm,
                             boost=None if self._boost is None else boost_args(*self._boost))

    def collect(self):  # src/vec.rs:205-311
        hits, counts = self.collect_arrays()[:2]  # (a per_group plan returns the hits' groups too)
        if self._max_sim:  # a hit is a group: the caller's own label where set_groups made the ids dense
            labels = self.vector_store.group_labels()
            idx = hits["index"].astype(np.int64)
            return [SearchResult(i, x) for i, x in zip((idx if labels is None else labels[idx]).tolist(), hits["score"].tolist())]
        if self._mode == Mode.PerQuery:
            return split_results(hits, counts)
        return split_results(hits, [int(hits.size)])[0]

    def collect_groups(self):
        """A per_group plan's hits by group: [(label, [SearchResult, ...]), ...] in the groups' rank order, each group's hits best
        first; `label` is the caller's own group label (VecStore.group_labels()) or the dense id where there are none.  One such
        list per query with per_query()."""
        if self._per_group is None:
            raise OttersError("collect_groups needs a per_group(m) plan")
        hits, counts, groups = self.collect_arrays()
        labels = self.vector_store.group_labels()
        lab = (groups.astype(np.int64) if labels is None else labels[groups.astype(np.int64)]).tolist()
        idx, sc = hits["index"].tolist(), hits["score"].tolist()

        def by_group(lo, hi):  # a group's hits are contiguous: a new group starts where the id changes
            out = []
            for i in range(lo, hi):
                if i == lo or groups[i] != groups[i - 1]:
                    out.append((lab[i], []))
                out[-1][1].append(SearchResult(idx[i], sc[i]))
            return out

        if self._mode == Mode.PerQuery:
            out, o = [], 0
            for c in counts:
                out.append(by_group(o, o + c))
                o += c
            return out
        return by_group(0, len(idx))

    def collect_mmr(self):
        """An mmr() plan's picks with their values: (hits, counts, values) -- collect_arrays()'s hits and counts, in pick order, and
        `values[i]` (f32) = lambda x relevance - (1 - lambda) x redundancy of hits[i] at the moment it was picked."""
        if self._mmr is None:
            raise OttersError("collect_mmr needs an mmr() plan")
        rq = self.resolve()
        store = self.vector_store
        hits, counts, stats = store._run(rq)
        store.last_stats = stats
        if rq.mode != Mode.PerQuery:
            counts = np.bincount(hits["query"], minlength=rq.queries.shape[0]).tolist()
        return hits, counts, rq.mmr_values if rq.mmr_values is not None else np.zeros(0, dtype=np.float32)

    def collect_arrays(self):
        """collect() without the per-hit Python objects: (hits, counts) where `hits` is a NumPy record array
        (`index` u64, `score` f32, `query` u32 = which query of the batch scored it) sorted best-first -- per query,
        concatenated in query order, in per_query() mode -- and `counts[q]` is the number of hits of query q.  A per_group(m) plan
        returns (hits, counts, groups): `groups[i]` (u32) is the dense group id of hits[i]."""
        rq = self.resolve()
        store = self.vector_store
        hits, counts, stats = store._run(rq)
        store.last_stats = stats
        if rq.max_sim:  # one list of groups; the tokens have no hits of their own
            return hits, [int(hits.size)]
        if rq.mode != Mode.PerQuery:  # merged: how many of the k hits each query of the batch contributed
            counts = np.bincount(hits["query"], minlength=rq.queries.shape[0]).tolist()
        if rq.group_size:
            return hits, counts, rq.group_of_hit if rq.group_of_hit is not None else np.zeros(0, dtype=np.uint32)
        return hits, counts


@dataclass
class ResolvedMaxSimBatch:
    """What MaxSimBatchPlan hands to ott_query_maxsim_groups_batch once it is validated."""
    queries: np.ndarray            # [sum of tokens, dim] f32: the tokens of query 0, then of query 1, ...
    tokens_per_query: np.ndarray   # uint32[B]
    listed_per_query: np.ndarray   # uint64[B]
    groups: np.ndarray             # uint32[sum of listed]: the lists back to back, dense ids in the caller's order, duplicates kept
    distinct_per_query: list       # [B] distinct listed groups of every query
    metric: int
    take: int
    k: int
    filter_cmp: int
    filter_thr: float
    row_mask: Optional[np.ndarray]


class MaxSimBatchPlan(_ScorePlan):
    """MaxSim re-ranking in batches (VecStore.max_sim_batch; ott_query_maxsim_groups_batch): B queries, each with its own tokens and
    its own list of groups, through one call.  Query b's result is exactly that of
    store.query(token_sets[b], metric).max_sim().with_groups(lists[b]) with the same take, filter and row mask.  Lazy like
    VecQueryPlan: errors surface at validate() / collect()."""

    def __init__(self, store: "VecStore", token_sets, metric: Metric):
        super().__init__()
        self.vector_store = store
        self.token_sets = [QueryBatch(t).queries for t in token_sets]
        self.search_metric = Metric(metric)
        self.group_lists = None

    def with_groups(self, lists_of_labels) -> "MaxSimBatchPlan":
        """One list of group labels per token set, mapped as VecQueryPlan.with_groups maps them: any order, duplicates allowed, two
        queries may list the same group, an empty list is a query with no hits.  Required in this version."""
        self.group_lists = list(lists_of_labels)
        return self

    def validate(self) -> None:
        n = len(self.token_sets)
        if n == 0:
            raise OttersError("max_sim_batch: no token sets provided")
        if n > MAXSIM_BATCH_MAX:
            raise OttersError(f"max_sim_batch: {n} token sets; a batch holds at most {MAXSIM_BATCH_MAX}")
        if self.group_lists is None:
            raise OttersError("max_sim_batch needs with_groups in this version: one list of groups per token set")
        if len(self.group_lists) != n:
            raise OttersError(f"max_sim_batch: with_groups got {len(self.group_lists)} lists for {n} token sets")
        dim = self.vector_store.dim
        for b, t in enumerate(self.token_sets):
            if len(t) == 0:
                raise OttersError(f"max_sim_batch: token set {b} is empty")
            for q in ([t[0]] if isinstance(t, np.ndarray) else t):
                if len(q) != dim:
                    raise OttersError(f"Query vector length {len(q)} does not match expected dimension {dim}")
        for listed in self.group_lists:
            dense_listed_groups(self.vector_store, listed)

    def resolve(self) -> ResolvedMaxSimBatch:
        """Validate and lower the plan.  Pure host logic, no GPU."""
        self.validate()
        sets = [t if isinstance(t, np.ndarray) else np.stack(t).astype(np.float32, copy=False) for t in self.token_sets]
        lists = [dense_listed_groups(self.vector_store, listed) for listed in self.group_lists]
        distinct = [int(np.unique(g).size) for g in lists]
        take, k, fc, ft = self._lowered(max(distinct), TakeType.Max)  # the default take: the largest number of distinct listed groups
        return ResolvedMaxSimBatch(queries=np.ascontiguousarray(np.concatenate(sets), dtype=np.float32),
                                   tokens_per_query=np.array([t.shape[0] for t in sets], dtype=np.uint32),
                                   listed_per_query=np.array([g.size for g in lists], dtype=np.uint64),
                                   groups=np.ascontiguousarray(np.concatenate(lists), dtype=np.uint32), distinct_per_query=distinct,
                                   metric=int(self.search_metric), take=take, k=k, filter_cmp=fc, filter_thr=ft, row_mask=self.row_mask)

    def collect_arrays(self):
        """(hits, counts): `hits` as VecQueryPlan.collect_arrays returns them for a max_sim plan — `index` the dense group id, `score`
        the sum — every query's list best first, back to back in query order, `query` = the query of the batch; counts[b] = the number
        of hits of query b."""
        store = self.vector_store
        hits, counts, stats = store._run_maxsim_batch(self.resolve())
        store.last_stats = stats
        return hits, counts

    def collect(self):
        """One list of SearchResult(label, score) per query, with the caller's own group labels."""
        hits, counts = self.collect_arrays()
        labels = self.vector_store.group_labels()
        idx = hits["index"].astype(np.int64)
        return split_results(hits, counts, idx if labels is None else labels[idx])


RECOMMEND_MAX_EXAMPLES = 64  # include/otters_hip.h: OTT_RECOMMEND_MAX_EXAMPLES
RECOMMEND_FILL = 1           # include/otters_hip.h: OTT_RECOMMEND_FILL


class RecommendStrategy(enum.IntEnum):  # include/otters_hip.h: ott_recommend_strategy (Qdrant's three recommend strategies)
    BestScore = 0      # ott_query_recommend: a row's best positive score against its best negative one
    AverageVector = 1  # one ordinary query with mean(positives) [+ mean(positives) - mean(negatives)]
    SumScores = 2      # the sum of a row's scores against the positives minus those against the negatives


def recommend_examples(positive, negative, n_rows: int, who: str = "ott_query_recommend"):
    """recommend()'s example lists checked as ott_query_recommend checks them, with its messages: (uint64 positives, uint64
    negatives) as listed.  `who`: the call the messages name (ott_query_recommend_strategy for the other strategies).  Pure host logic."""
    pos, neg = as_row_ids(positive), as_row_ids(negative)
    if pos.size == 0:
        raise OttersError(f"{who}: at least one positive example is needed")
    # the library's walk (ott_recommend_plan.h: rec_examples), id by id, the positives first: the first fault it meets is the one named
    seen_pos, seen = set(), set()
    for ids, is_neg in ((pos, False), (neg, True)):
        for i in ids.tolist():
            if i >= n_rows:
                raise OttersError(f"{who}: example id {i} is not below the store's length {n_rows}")
            if is_neg and i in seen_pos:
                raise OttersError(f"{who}: row {i} is listed as both a positive and a negative example")
            if i in seen:
                continue
            if len(seen) == RECOMMEND_MAX_EXAMPLES:
                raise OttersError(f"{who}: more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples")
            seen.add(i)
        if not is_neg:
            seen_pos = set(seen)
    return pos, neg


@dataclass
class ResolvedRecommend:
    """What RecommendPlan hands to ott_query_recommend once it is validated."""
    positive: np.ndarray  # uint64[n_positive], as listed
    negative: np.ndarray  # uint64[n_negative], as listed
    metric: int
    take: int
    k: int
    filter_cmp: int
    filter_thr: float
    row_mask: Optional[np.ndarray]
    path: int
    flags: int
    strategy: int = 0  # RecommendStrategy; 0 lowers to ott_query_recommend, the others to ott_query_recommend_strategy with flags 0


class RecommendPlan(_PathScorePlan):
    """Recommend by example rows (VecStore.recommend; ott_query_recommend, Qdrant's recommend with the best_score strategy): rank the
    rows by their best score against the `positive` rows of the store; a row at least as close to a `negative` row as to its best
    positive leaves the positive side and follows it — least like its nearest negative first — unless fill_negative_side(False).
    With strategy AverageVector the hits are those of store.query(q) for q = mean(positives), or mean(positives) +
    mean(positives) - mean(negatives), with the examples masked out; with SumScores the rows are ranked by the sum of their scores
    against the positives minus the sum of those against the negatives (ott_query_recommend_strategy).  Both have the positive side
    only: fill_negative_side() does not reach them.  Lazy like VecQueryPlan: errors surface at validate() / collect()."""

    def __init__(self, store: "VecStore", positive, negative, metric: Metric, strategy: RecommendStrategy = RecommendStrategy.BestScore):
        super().__init__()
        self.vector_store = store
        self.positive, self.negative = positive, negative
        self.search_metric = Metric(metric)
        self.strategy = RecommendStrategy(strategy)
        self.fill = True

    def filter(self, score: float, cmp: Cmp) -> "RecommendPlan":
        """The score filter acts on the hit's score: with BestScore on a row's best POSITIVE score BP, on both sides; with SumScores
        on the sum S; with AverageVector on the query's score, as VecQueryPlan.filter does."""
        return super().filter(score, cmp)

    def fill_negative_side(self, fill: bool = True) -> "RecommendPlan":
        """True (default): when the positive side has fewer than take(k) rows, the negative-side rows follow it.  False: they never
        come out."""
        self.fill = bool(fill)
        return self

    def _who(self) -> str:
        return "ott_query_recommend" if self.strategy == RecommendStrategy.BestScore else "ott_query_recommend_strategy"

    def validate(self) -> None:
        st = self.vector_store
        recommend_examples(self.positive, self.negative, len(st), self._who())
        if self.path == Path.Mfma:
            if self.strategy == RecommendStrategy.BestScore:
                raise OttersError("ott_query_recommend: the MFMA path does not serve recommend queries; use path AUTO or EXACT")
            if self.strategy == RecommendStrategy.SumScores:
                raise OttersError("ott_query_recommend_strategy: the MFMA path does not serve sum_scores; use path AUTO or EXACT")
            if self.search_metric == Metric.Manhattan:
                raise OttersError("ott_query_recommend_strategy: the MFMA path does not score the Manhattan metric; use path AUTO or EXACT")
        if st.devices is not None:
            raise OttersError(f"{self._who()}: a multi-GPU store is not served (the examples' rows lie on different shards)")

    def resolve(self) -> ResolvedRecommend:
        """Validate and lower the plan.  Pure host logic, no GPU."""
        self.validate()
        pos, neg = recommend_examples(self.positive, self.negative, len(self.vector_store), self._who())
        take, k, fc, ft = self._lowered(len(self.vector_store))
        return ResolvedRecommend(positive=pos, negative=neg, metric=int(self.search_metric), take=take, k=k, filter_cmp=fc, filter_thr=ft,
                                 row_mask=self.row_mask, path=int(self.path),
                                 flags=(RECOMMEND_FILL if self.fill else 0) if self.strategy == RecommendStrategy.BestScore else 0, strategy=int(self.strategy))

    def collect_arrays(self):
        """(hits, sides): `hits` a NumPy record array (`index` u64, `score` f32 — the best positive score on the positive side, the
        best negative score on the negative side —, `query` = 0) in the call's order, `sides[i]` (u32) 1 = positive side, 0 =
        negative side (all 1 with the strategies AverageVector and SumScores, whose score is the query's score and the sum S)."""
        store = self.vector_store
        hits, sides, stats = store._run_recommend(self.resolve())
        store.last_stats = stats
        return hits, sides

    def collect(self):
        """(results, sides): one SearchResult(index, score) per hit, and the hits' sides as a list."""
        hits, sides = self.collect_arrays()
        return [SearchResult(i, s) for i, s in zip(hits["index"].tolist(), hits["score"].tolist())], sides.tolist()


DISCOVER_MAX_PAIRS = 32     # include/otters_hip.h: OTT_DISCOVER_MAX_PAIRS
NO_ROW = 2 ** 64 - 1        # include/otters_hip.h: OTT_NO_ROW


def discover_context(context, target_row, n_rows: int):
    """discover()'s context pairs and target row checked as ott_query_discover checks them, with its messages, in its order:
    (uint64 positives, uint64 negatives).  Pure host logic."""
    pairs = [tuple(p) for p in context]
    if any(len(p) != 2 for p in pairs):
        raise OttersError("discover: the context is a sequence of (positive, negative) row id pairs")
    if not 1 <= len(pairs) <= DISCOVER_MAX_PAIRS:
        raise OttersError("ott_query_discover: between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed")
    pos, neg = as_row_ids([p[0] for p in pairs]), as_row_ids([p[1] for p in pairs])
    # the library's walk (ott_discover_plan.h: disc_slots), pair by pair, the target row last: the first fault it meets is the one named
    for a, b in zip(pos.tolist(), neg.tolist()):
        for i in (a, b):
            if i >= n_rows:
                raise OttersError(f"ott_query_discover: row id {i} is not below the store's length {n_rows}")
        if a == b:
            raise OttersError(f"ott_query_discover: row {a} is both the positive and the negative of a pair")
    if target_row is not None and target_row >= n_rows:
        raise OttersError(f"ott_query_discover: row id {target_row} is not below the store's length {n_rows}")
    return pos, neg


@dataclass
class ResolvedDiscover:
    """What DiscoverPlan hands to ott_query_discover once it is validated."""
    positive: np.ndarray           # uint64[n_pairs]
    negative: np.ndarray           # uint64[n_pairs]
    target: Optional[np.ndarray]   # float32[dim], or None
    target_row: int                # NO_ROW = none
    min_wins: int
    metric: int
    take: int
    k: int
    filter_cmp: int
    filter_thr: float
    row_mask: Optional[np.ndarray]
    path: int


@dataclass
class DiscoverResult:
    """One hit of a discovery or context search: the row, its score (the target score, or the loss without a target), the pairs it wins."""
    index: int
    score: float
    wins: int


class DiscoverPlan(_PathScorePlan):
    """Discovery and context search (VecStore.discover; ott_query_discover, Qdrant's Discovery API).  `context` is a sequence of
    (positive, negative) row id pairs; a row WINS a pair when it is closer to the pair's positive than to its negative.  With a
    target — a vector (`target`) or a stored row (`target_row`) — the rows are ranked by the pairs they win, then by their score
    against the target; without one (context search) by a loss that is zero where every pair is won and falls with every violated
    pair.  Lazy like VecQueryPlan: errors surface at validate() / collect()."""

    def __init__(self, store: "VecStore", context, target, target_row, metric: Metric):
        super().__init__()
        self.vector_store = store
        self.context = list(context)
        self.target = target
        self.target_row = target_row
        self.search_metric = Metric(metric)
        self.min_wins_count = 0

    def filter(self, score: float, cmp: Cmp) -> "DiscoverPlan":
        """The score filter acts on the hit's score: the target score with a target, the loss without one."""
        return super().filter(score, cmp)

    def min_wins(self, n: int) -> "DiscoverPlan":
        """Only rows that win at least `n` of the pairs come out (n = the number of pairs: only rows inside the fenced region)."""
        self.min_wins_count = int(n)
        return self

    def _target_vector(self) -> Optional[np.ndarray]:
        if self.target is None:
            return None
        t = np.asarray(self.target, dtype=np.float32)
        if t.ndim == 2 and t.shape[0] != 1:
            raise OttersError("ott_query_discover: at most one target vector (d->nq <= 1)")
        t = np.ascontiguousarray(t.ravel())
        if t.size != self.vector_store.dim:
            raise OttersError(f"Query vector length {t.size} does not match expected dimension {self.vector_store.dim}")
        return t

    def resolve(self) -> ResolvedDiscover:
        """Validate and lower the plan.  Pure host logic, no GPU.  The library's refusals in the library's order."""
        st = self.vector_store
        pairs = [tuple(p) for p in self.context]
        if not 1 <= len(pairs) <= DISCOVER_MAX_PAIRS:
            raise OttersError("ott_query_discover: between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed")
        tv = self._target_vector()
        trow = None
        if self.target_row is not None:
            trow = int(as_row_ids([self.target_row])[0])
        if tv is not None and trow is not None:
            raise OttersError("ott_query_discover: a target vector and a target row are both given")
        if self.min_wins_count < 0 or self.min_wins_count > len(pairs):
            raise OttersError("ott_query_discover: min_wins is above the number of pairs" if self.min_wins_count > 0 else "discover: min_wins is negative")
        if self.path == Path.Mfma:
            raise OttersError("ott_query_discover: the MFMA path does not serve discovery queries; use path AUTO or EXACT")
        if st.devices is not None:
            raise OttersError("ott_query_discover: a multi-GPU store is not served (the examples' rows lie on different shards)")
        pos, neg = discover_context(pairs, trow, len(st))
        take, k, fc, ft = self._lowered(len(st))
        return ResolvedDiscover(positive=pos, negative=neg, target=tv, target_row=NO_ROW if trow is None else trow, min_wins=self.min_wins_count,
                                metric=int(self.search_metric), take=take, k=k, filter_cmp=fc, filter_thr=ft, row_mask=self.row_mask,
                                path=int(self.path))

    def validate(self) -> None:
        self.resolve()

    def collect_arrays(self):
        """(hits, wins): `hits` a NumPy record array (`index` u64, `score` f32 — the target score, or the loss without a target —,
        `query` = 0) in the call's order, `wins[i]` (u32) the pairs hit i wins."""
        store = self.vector_store
        hits, wins, stats = store._run_discover(self.resolve())
        store.last_stats = stats
        return hits, wins

    def collect(self):
        """One DiscoverResult(index, score, wins) per hit."""
        hits, wins = self.collect_arrays()
        return [DiscoverResult(i, s, w) for i, s, w in zip(hits["index"].tolist(), hits["score"].tolist(), wins.tolist())]


class Fusion(enum.IntEnum):  # include/otters_hip.h: ott_fusion
    Rrf = 0      # reciprocal rank fusion: weight / (k + rank)
    Dbsf = 1     # distribution-based score fusion: scores normalised by mean +- 3 sigma of the leg's list
    MinMax = 2   # min-max ("relative score") fusion: scores normalised by the leg's worst and best


def fuse_default_fetch(k: int) -> int:
    """Hits a leg contributes when the plan does not say: max(4 x take, 32), cut at OTT_FUSE_MAX_FETCH."""
    return min(max(4 * int(k), 32), N.FUSE_MAX_FETCH)


def fuse_args(legs_per_request, nq: int, fetch: int, fusion: int, rrf_k: float, weights, k: int) -> None:
    """ott_query_fuse's argument refusals (ott_fuse_plan.h: fuse_check_args), in its order and with its texts, before any native call."""
    who = "ott_query_fuse: "
    n = len(legs_per_request)
    if n == 0:
        raise OttersError(who + "n_requests must be at least 1")
    if n > N.FUSE_MAX_REQUESTS:
        raise OttersError(who + f"{n} requests are above OTT_FUSE_MAX_REQUESTS ({N.FUSE_MAX_REQUESTS})")
    if not 1 <= fetch <= N.FUSE_MAX_FETCH:
        raise OttersError(who + f"fetch must lie between 1 and OTT_FUSE_MAX_FETCH ({N.FUSE_MAX_FETCH})")
    for b, l in enumerate(legs_per_request):
        if not 1 <= l <= N.FUSE_MAX_LEGS:
            raise OttersError(who + f"request {b} has {l} legs; a request takes 1 to OTT_FUSE_MAX_LEGS ({N.FUSE_MAX_LEGS})")
        if l * fetch > N.FUSE_MAX_ENTRIES:
            raise OttersError(who + f"request {b} has {l * fetch} entries (legs x fetch), above OTT_FUSE_MAX_ENTRIES ({N.FUSE_MAX_ENTRIES})")
    if sum(legs_per_request) != nq:
        raise OttersError(who + f"legs_per_request adds up to {sum(legs_per_request)}, not to d->nq")
    if fusion not in (0, 1, 2):
        raise OttersError(who + "unknown fusion (OTT_FUSE_RRF, OTT_FUSE_DBSF or OTT_FUSE_MINMAX)")
    if fusion == int(Fusion.Rrf) and not (np.isfinite(np.float32(rrf_k)) and rrf_k >= 0):
        raise OttersError(who + "rrf_k must be finite and at least 0")
    if weights is not None:
        for l, w in enumerate(weights):
            if not np.isfinite(np.float32(w)):
                raise OttersError(who + f"the weight of leg {l} is not finite")
    if k == 0:
        raise OttersError(who + "k must be at least 1")


@dataclass
class ResolvedFuse:
    """What FusePlan hands to ott_query_fuse once it is validated."""
    queries: np.ndarray            # [sum of legs, dim] f32: the legs of request 0, then of request 1, ...
    legs_per_request: np.ndarray   # uint32[B]
    fusion: int
    rrf_k: float
    weights: Optional[np.ndarray]  # f32[sum of legs], or None = all 1
    fetch: int
    metric: int
    take: int
    k: int
    filter_cmp: int
    filter_thr: float
    row_mask: Optional[np.ndarray]
    path: int


class _FusionPlan(_PathScorePlan):
    """What the fusion plans (FusePlan, HybridPlan) share: the fusion and its parameter, the weights, the fetch, the default take."""

    def __init__(self, store: "VecStore", metric: Metric):
        super().__init__()
        self.vector_store = store
        self.search_metric = Metric(metric)
        self.fusion = Fusion.Rrf
        self.rrf_k = 60.0
        self.leg_weights = None
        self.fetch_count: Optional[int] = None

    def rrf(self, k: float = 60.0):
        """Reciprocal rank fusion: the entry at position r (0 based) of a leg with weight w contributes w / (k + (r + 1))."""
        self.fusion, self.rrf_k = Fusion.Rrf, float(k)
        return self

    def dbsf(self):
        """Distribution-based score fusion: a leg's scores are normalised by mean -+ 3 sigma of its list (no clamp), times its weight."""
        self.fusion = Fusion.Dbsf
        return self

    def min_max(self):
        """Min-max fusion: a leg's scores are normalised to [0, 1] by its list's worst and best score, times its weight."""
        self.fusion = Fusion.MinMax
        return self

    def weights(self, list_of_lists):
        """One list of weights per request, one weight per leg in the request's leg order (default: all 1)."""
        self.leg_weights = [list(w) for w in list_of_lists]
        return self

    def fetch(self, n: int):
        """Hits every leg contributes (default: max(4 x take, 32), at most 512)."""
        self.fetch_count = int(n)
        return self

    def _k(self) -> int:
        return max(int(self.take_count), 0) if self.take_count is not None else max(len(self.vector_store), 1)

    def _fetch(self) -> int:
        return self.fetch_count if self.fetch_count is not None else fuse_default_fetch(self._k())

    def _flat_weights_for(self, legs_per_request, what: str):
        if self.leg_weights is None:
            return None
        if len(self.leg_weights) != len(legs_per_request) or any(len(w) != n for w, n in zip(self.leg_weights, legs_per_request)):
            raise OttersError(what)
        return [float(x) for w in self.leg_weights for x in w]

    def collect(self):
        """One list of SearchResult(index, fused score) per request."""
        return split_results(*self.collect_arrays())


class FusePlan(_FusionPlan):
    """Rank fusion (VecStore.fuse; ott_query_fuse): every request brings several query vectors ("legs"); each leg's best `fetch` hits
    — exactly what store.query(leg, metric).per_query().take(fetch) returns under the same filter, masks and path — are merged into
    one ranking per request by reciprocal rank fusion (.rrf(k), the default), distribution-based score fusion (.dbsf()) or min-max
    score fusion (.min_max()).  A row's fused score F is the f32 sum, in leg order, of its contribution in every leg that lists it;
    the hits are ranked by F descending, equal F by the lower row, whatever the take type is (it ranks the legs).  Lazy like
    VecQueryPlan: errors surface at validate() / collect()."""

    def __init__(self, store: "VecStore", leg_sets, metric: Metric):
        super().__init__(store, metric)
        self.leg_sets = [QueryBatch(t).queries for t in leg_sets]

    def filter(self, score: float, cmp: Cmp) -> "FusePlan":
        """The score filter acts on a leg's own score: it is part of the leg, as VecQueryPlan.filter."""
        return super().filter(score, cmp)

    def n_requests(self) -> int:
        return len(self.leg_sets)

    def _flat_weights(self):
        return self._flat_weights_for([len(t) for t in self.leg_sets], "fuse: weights takes one list per request with one weight per leg")

    def validate(self) -> None:
        st = self.vector_store
        legs = [len(t) for t in self.leg_sets]
        fuse_args(legs, sum(legs), self._fetch(), int(self.fusion), self.rrf_k, self._flat_weights(), self._k())
        for t in self.leg_sets:
            for q in ([t[0]] if isinstance(t, np.ndarray) else t):
                if len(q) != st.dim:
                    raise OttersError(f"Query vector length {len(q)} does not match expected dimension {st.dim}")
        if self.path == Path.Mfma and self.search_metric == Metric.Manhattan:
            raise OttersError("ott_query: the MFMA path does not score the Manhattan metric; use path AUTO or EXACT")
        if st.devices is not None:
            raise OttersError("ott_query_fuse: a multi-GPU store is not served (the legs' lists lie on different GPUs)")

    def resolve(self) -> ResolvedFuse:
        """Validate and lower the plan.  Pure host logic, no GPU."""
        self.validate()
        sets = [t if isinstance(t, np.ndarray) else np.stack(t).astype(np.float32, copy=False) for t in self.leg_sets]
        w = self._flat_weights()
        take, k, fc, ft = self._lowered(max(len(self.vector_store), 1))  # (k: what _k() says)
        return ResolvedFuse(queries=np.ascontiguousarray(np.concatenate(sets), dtype=np.float32),
                            legs_per_request=np.array([t.shape[0] for t in sets], dtype=np.uint32), fusion=int(self.fusion), rrf_k=float(self.rrf_k),
                            weights=None if w is None else np.array(w, dtype=np.float32), fetch=self._fetch(), metric=int(self.search_metric),
                            take=take, k=k, filter_cmp=fc, filter_thr=ft, row_mask=self.row_mask, path=int(self.path))

    def collect_arrays(self):
        """(hits, counts): `hits` a NumPy record array (`index` u64, `score` f32 = the fused score F, `query` = the request), every
        request's list best first, back to back in request order; counts[b] = the hits of request b."""
        store = self.vector_store
        hits, counts, stats = store._run_fuse(self.resolve())
        store.last_stats = stats
        return hits, counts


SPARSE_MAX_VOCAB = 1 << 20      # include/otters_hip.h: OTT_SPARSE_MAX_VOCAB
SPARSE_MAX_QUERIES = 1024       # include/otters_hip.h: OTT_SPARSE_MAX_QUERIES


def sparse_csr(rows):
    """A list of (indices, values) pairs -> (indptr uint64[n + 1], indices uint32[nnz], values float32[nnz]).  Nothing is sorted
    or merged: ott_store_set_sparse and ott_query_sparse check what they are given."""
    idx, val, ptr = [], [], [0]
    for r, (i, v) in enumerate(rows):
        i = np.asarray(i).ravel()
        v = np.asarray(v, dtype=np.float32).ravel()
        if i.size != v.size:
            raise OttersError(f"sparse vector {r}: {i.size} indices for {v.size} values")
        if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
            raise OttersError(f"sparse vector {r}: an index is not a 32-bit unsigned integer")
        idx.append(i.astype(np.uint32))
        val.append(v)
        ptr.append(ptr[-1] + int(i.size))
    return (np.array(ptr, dtype=np.uint64), np.concatenate(idx) if idx else np.zeros(0, np.uint32),
            np.concatenate(val) if val else np.zeros(0, np.float32))


def is_one_sparse_query(q) -> bool:
    """whether `q` is ONE (indices, values) pair, not a sequence of them"""
    return isinstance(q, tuple) and len(q) == 2 and not (len(q[0]) and isinstance(q[0][0], (tuple, list, np.ndarray)))


@dataclass
class ResolvedSparse:
    """What SparseQueryPlan hands to ott_query_sparse once it is validated."""
    indptr: np.ndarray   # uint64[nq + 1]
    indices: np.ndarray  # uint32[]
    values: np.ndarray   # float32[]
    take: int
    k: int
    filter_cmp: int
    filter_thr: float
    row_mask: Optional[np.ndarray]
    path: int
    metric: int = int(Metric.DotProduct)  # a sparse score is a dot product
    idf: bool = False                     # ott_query_sparse_idf: the weights times idf(index)


class SparseQueryPlan(_PathScorePlan):
    """Exact sparse dot search over the store's sparse rows (VecStore.sparse_query; ott_query_sparse): a row is a hit iff it shares
    an index with the query; its score adds value x weight over the shared indices in the row's index order, one rounded f32
    operation at a time.  Lazy like VecQueryPlan: errors surface at collect()."""

    def __init__(self, store: "VecStore", q):
        super().__init__()
        self.vector_store = store
        self.search_metric = Metric.DotProduct  # a sparse score is a dot product: it decides the default take
        self.queries = [q] if is_one_sparse_query(q) else list(q)
        self.use_idf = False

    def idf(self, on: bool = True) -> "SparseQueryPlan":
        """Scale every query weight by idf(index) = log(1 + (n_docs - df + 0.5) / (df + 0.5)) over the store's live rows
        (ott_query_sparse_idf; VecStore.sparse_df returns df and n_docs)."""
        self.use_idf = bool(on)
        return self

    def resolve(self) -> ResolvedSparse:
        """Lower the plan.  Pure host logic, no GPU; the library checks the queries against the store's vocab."""
        if not self.queries:
            raise OttersError("No queries provided")
        ptr, idx, val = sparse_csr(self.queries)
        take, k, fc, ft = self._lowered(len(self.vector_store))
        return ResolvedSparse(indptr=ptr, indices=idx, values=val, take=take, k=k, filter_cmp=fc, filter_thr=ft, row_mask=self.row_mask,
                              path=int(self.path), idf=self.use_idf)

    def collect_arrays(self):
        """(hits, counts): `hits` a NumPy record array (`index` u64, `score` f32 = S, `query`), every query's list best first, back
        to back in query order; counts[b] = the hits of query b."""
        store = self.vector_store
        hits, counts, stats = store._run_sparse(self.resolve())
        store.last_stats = stats
        return hits, counts

    def collect_per_query(self):
        """One list of SearchResult(index, score) per query."""
        return split_results(*self.collect_arrays())

    def collect(self):
        """The hits of ONE query as a list of SearchResult(index, score); a batch needs collect_per_query()."""
        if len(self.queries) != 1:
            raise OttersError("ott_query_sparse: a batch needs OTT_MODE_PER_QUERY (a merged list over several sparse queries is not served)")
        return self.collect_per_query()[0]


BINARY_MAX_BITS = 16384         # include/otters_hip.h: OTT_BINARY_MAX_BITS
BINARY_MAX_QUERIES = 1024       # include/otters_hip.h: OTT_BINARY_MAX_QUERIES


def binary_words(bits, n_bits: Optional[int] = None, who: str = "set_binary"):
    """Bit rows as the library takes them: (words uint64[n, ceil(n_bits / 64)], n_bits).  `bits` is a bool / 0-1 matrix [n, n_bits]
    (bit j of a row goes to bit j % 64 of word j // 64) or packed uint64 words [n, W] with `n_bits` named (W == ceil(n_bits / 64);
    without n_bits: 64 W).  One row may be given as a vector.  Padding bits are not touched: the library refuses a set one."""
    a = np.asarray(bits)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2:
        raise OttersError(f"{who}: bits must be a matrix (rows x bits, or rows x uint64 words)")
    if a.dtype == np.uint64:
        nb = 64 * a.shape[1] if n_bits is None else int(n_bits)
        if a.shape[1] != (nb + 63) // 64:
            raise OttersError(f"{who}: {a.shape[1]} words per row for n_bits = {nb}")
        return np.ascontiguousarray(a), nb
    if a.dtype != np.bool_:
        if a.size and not np.isin(a, (0, 1)).all():
            raise OttersError(f"{who}: a bit matrix holds only 0 and 1 (packed words are uint64)")
        a = a.astype(bool)
    nb = a.shape[1] if n_bits is None else int(n_bits)
    if nb != a.shape[1]:
        raise OttersError(f"{who}: {a.shape[1]} bits per row for n_bits = {nb}")
    W = (nb + 63) // 64
    packed = np.zeros((a.shape[0], W * 8), dtype=np.uint8)
    if nb:
        packed[:, : (nb + 7) // 8] = np.packbits(a, axis=1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u8").reshape(a.shape[0], W), nb


def sign_bits(x) -> np.ndarray:
    """ott_store_set_binary_sign's rule on the host: bit j = x[j] > 0.0 in f32 (NaN, -0.0 and +0.0 give 0; +denormals give 1)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(x, dtype=np.float32) > np.float32(0.0)


@dataclass
class ResolvedBinary:
    """What BinaryQueryPlan hands to ott_query_binary once it is validated."""
    words: np.ndarray    # uint64[nq, ceil(n_bits / 64)]
    n_bits: int
    take: int
    k: int
    filter_cmp: int
    filter_thr: float
    row_mask: Optional[np.ndarray]
    path: int
    metric: int = int(Metric.Manhattan)  # the Hamming distance is the L1 distance of the bit vectors


class BinaryQueryPlan(_PathScorePlan):
    """Exact Hamming search over the store's bit rows (VecStore.binary_query; ott_query_binary): every row the masks leave is a
    candidate, its score is popcount(q XOR v) as a float, the default take is Min.  Lazy like VecQueryPlan: errors surface at
    collect()."""

    def __init__(self, store: "VecStore", q_bits, n_bits: Optional[int] = None):
        super().__init__()
        self.vector_store = store
        self.search_metric = Metric.Manhattan  # decides the default take: Min
        self.q_bits = q_bits
        self.n_bits = n_bits

    def resolve(self) -> ResolvedBinary:
        """Lower the plan.  Pure host logic, no GPU; the library checks the queries against the store's n_bits."""
        words, nb = binary_words(self.q_bits, self.n_bits, "binary_query")
        if words.shape[0] == 0:
            raise OttersError("No queries provided")
        take, k, fc, ft = self._lowered(len(self.vector_store))
        return ResolvedBinary(words=words, n_bits=nb, take=take, k=k, filter_cmp=fc, filter_thr=ft, row_mask=self.row_mask, path=int(self.path))

    def collect_arrays(self):
        """(hits, counts): `hits` a NumPy record array (`index` u64, `score` f32 = the distance, `query`), every query's list best
        first, back to back in query order; counts[b] = the hits of query b."""
        store = self.vector_store
        hits, counts, stats = store._run_binary(self.resolve())
        store.last_stats = stats
        return hits, counts

    def collect_per_query(self):
        """One list of SearchResult(index, score) per query."""
        return split_results(*self.collect_arrays())

    def collect(self):
        """The hits of ONE query as a list of SearchResult(index, score); a batch needs collect_per_query()."""
        hits, counts = self.collect_arrays()
        if len(counts) != 1:
            raise OttersError("ott_query_binary: a batch needs OTT_MODE_PER_QUERY (a merged list over several binary queries is not served)")
        return split_results(hits, counts)[0]

    def rescore(self, q_dense, metric: Metric, k: int):
        """The binary-quantisation pipeline: this plan's take(fetch) is the oversampled first stage; for each query its ids are
        re-scored by store.query(q_dense[b], metric).with_row_ids(ids).take(k) — the hits are by definition those of that call.
        Runs on the host, ONE second-stage call per query.  Returns one list of SearchResult per query."""
        q = np.asarray(q_dense, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        hits, counts = self.collect_arrays()
        if q.shape[0] != len(counts):
            raise OttersError(f"rescore: {q.shape[0]} dense queries for {len(counts)} binary queries")
        store, out, o = self.vector_store, [], 0
        for b, c in enumerate(counts):
            ids = hits["index"][o:o + c]
            o += c
            out.append(store.query(q[b:b + 1], metric).with_row_ids(ids).take(k).collect() if c else [])
        return out


def hybrid_args(dense_per, sparse_per, fetch: int, fusion: int, rrf_k: float, weights, k: int) -> None:
    """ott_query_hybrid's argument refusals that the plan can raise (ott_hybrid_plan.h: hybrid_check_args), in its order and with
    its texts, before any native call."""
    who = "ott_query_hybrid: "
    n = len(dense_per)
    if n == 0:
        raise OttersError(who + "n_requests must be at least 1")
    if n > N.FUSE_MAX_REQUESTS:
        raise OttersError(who + f"{n} requests are above OTT_FUSE_MAX_REQUESTS ({N.FUSE_MAX_REQUESTS})")
    if not 1 <= fetch <= N.FUSE_MAX_FETCH:
        raise OttersError(who + f"fetch must lie between 1 and OTT_FUSE_MAX_FETCH ({N.FUSE_MAX_FETCH})")
    for b, (nd, ns) in enumerate(zip(dense_per, sparse_per)):
        l = nd + ns
        if not 1 <= l <= N.FUSE_MAX_LEGS:
            raise OttersError(who + f"request {b} has {l} legs (dense plus sparse); a request takes 1 to OTT_FUSE_MAX_LEGS ({N.FUSE_MAX_LEGS})")
        if l * fetch > N.FUSE_MAX_ENTRIES:
            raise OttersError(who + f"request {b} has {l * fetch} entries (legs x fetch), above OTT_FUSE_MAX_ENTRIES ({N.FUSE_MAX_ENTRIES})")
    if fusion not in (0, 1, 2):
        raise OttersError(who + "unknown fusion (OTT_FUSE_RRF, OTT_FUSE_DBSF or OTT_FUSE_MINMAX)")
    if fusion == int(Fusion.Rrf) and not (np.isfinite(np.float32(rrf_k)) and rrf_k >= 0):
        raise OttersError(who + "rrf_k must be finite and at least 0")
    if weights is not None:
        for l, w in enumerate(weights):
            if not np.isfinite(np.float32(w)):
                raise OttersError(who + f"the weight of leg {l} is not finite")
    if k == 0:
        raise OttersError(who + "k must be at least 1")
    if sum(sparse_per) > N.SPARSE_MAX_QUERIES:
        raise OttersError(who + f"{sum(sparse_per)} sparse legs are above OTT_SPARSE_MAX_QUERIES ({N.SPARSE_MAX_QUERIES})")


@dataclass
class ResolvedHybrid:
    """What HybridPlan hands to ott_query_hybrid once it is validated."""
    queries: Optional[np.ndarray]    # [sum of dense legs, dim] f32, or None when no request has one
    dense_per_request: np.ndarray    # uint32[B]
    sparse_per_request: np.ndarray   # uint32[B]
    sq_indptr: np.ndarray            # uint64[n_sparse + 1]
    sq_indices: np.ndarray           # uint32[]
    sq_values: np.ndarray            # float32[]
    sparse_cmp: int
    sparse_thr: float
    sparse_flags: int
    fusion: int
    rrf_k: float
    weights: Optional[np.ndarray]    # f32[legs] in a request's own leg order (dense, then sparse), or None = all 1
    fetch: int
    metric: int
    take: int
    k: int
    filter_cmp: int
    filter_thr: float
    row_mask: Optional[np.ndarray]
    path: int


class HybridPlan(_FusionPlan):
    """Hybrid search (VecStore.hybrid; ott_query_hybrid): every request brings dense query vectors and sparse queries; each dense
    leg's best `fetch` hits are what store.query(leg, metric).take(fetch) returns, each sparse leg's what
    store.sparse_query(q).take(fetch) returns (take Max, under .sparse_filter, with .idf() the weights times idf), all under the
    same masks; a request's lists — its dense legs first, then its sparse legs — are merged as FusePlan merges them, except that
    min-max and DBSF normalise every leg under its own take: the metric's take for a dense leg, Max for a sparse one.  filter()
    acts on the dense legs only.  Lazy like VecQueryPlan: errors surface at validate() / collect()."""

    def __init__(self, store: "VecStore", dense_sets, sparse_sets, metric: Metric):
        super().__init__(store, metric)
        dense_sets = [] if dense_sets is None else list(dense_sets)
        sparse_sets = [] if sparse_sets is None else list(sparse_sets)
        n = max(len(dense_sets), len(sparse_sets))
        dense_sets += [None] * (n - len(dense_sets))    # a side that is shorter has no leg in the requests it does not name
        sparse_sets += [None] * (n - len(sparse_sets))
        self.dense_sets = [[] if t is None or len(t) == 0 else QueryBatch(t).queries for t in dense_sets]
        self.sparse_sets = [[] if t is None else [t] if is_one_sparse_query(t) else list(t) for t in sparse_sets]
        self.use_idf = False
        self.sparse_filter_criteria: Optional[tuple] = None

    def idf(self, on: bool = True) -> "HybridPlan":
        """The sparse queries' weights times idf(index) over the store's live rows (OTT_HYBRID_IDF)."""
        self.use_idf = bool(on)
        return self

    def sparse_filter(self, score: float, cmp: Cmp) -> "HybridPlan":
        """The filter on a sparse leg's score; filter() acts on the dense legs only."""
        self.sparse_filter_criteria = (float(np.float32(score)), Cmp(cmp))
        return self

    def n_requests(self) -> int:
        return len(self.dense_sets)

    def _legs(self):
        return [len(t) for t in self.dense_sets], [len(t) for t in self.sparse_sets]

    def _flat_weights(self):
        nd, ns = self._legs()
        return self._flat_weights_for([a + b for a, b in zip(nd, ns)],
                                      "hybrid: weights takes one list per request with one weight per leg (its dense legs, then its sparse legs)")

    def validate(self) -> None:
        st = self.vector_store
        nd, ns = self._legs()
        hybrid_args(nd, ns, self._fetch(), int(self.fusion), self.rrf_k, self._flat_weights(), self._k())
        for t in self.dense_sets:
            for q in ([t[0]] if isinstance(t, np.ndarray) else t):
                if len(q) != st.dim:
                    raise OttersError(f"Query vector length {len(q)} does not match expected dimension {st.dim}")
        if self.path == Path.Mfma and self.search_metric == Metric.Manhattan and sum(nd):
            raise OttersError("ott_query: the MFMA path does not score the Manhattan metric; use path AUTO or EXACT")
        if st.devices is not None:
            raise OttersError("ott_query_hybrid: a multi-GPU store is not served (the legs' lists lie on different GPUs, sparse rows on one)")

    def resolve(self) -> ResolvedHybrid:
        """Validate and lower the plan.  Pure host logic, no GPU."""
        self.validate()
        sets = [t if isinstance(t, np.ndarray) else np.stack(t).astype(np.float32, copy=False) for t in self.dense_sets if len(t)]
        nd, ns = self._legs()
        ptr, idx, val = sparse_csr([q for t in self.sparse_sets for q in t])
        w = self._flat_weights()
        take, k, fc, ft = self._lowered(max(len(self.vector_store), 1))
        sc, sthr = (0, 0.0) if self.sparse_filter_criteria is None else (int(self.sparse_filter_criteria[1]), self.sparse_filter_criteria[0])
        return ResolvedHybrid(queries=np.ascontiguousarray(np.concatenate(sets), dtype=np.float32) if sets else None,
                              dense_per_request=np.array(nd, dtype=np.uint32), sparse_per_request=np.array(ns, dtype=np.uint32),
                              sq_indptr=ptr, sq_indices=idx, sq_values=val, sparse_cmp=sc, sparse_thr=sthr,
                              sparse_flags=N.HYBRID_IDF if self.use_idf else 0, fusion=int(self.fusion), rrf_k=float(self.rrf_k),
                              weights=None if w is None else np.array(w, dtype=np.float32), fetch=self._fetch(), metric=int(self.search_metric),
                              take=take, k=k, filter_cmp=fc, filter_thr=ft, row_mask=self.row_mask, path=int(self.path))

    def collect_arrays(self):
        """(hits, counts): `hits` a NumPy record array (`index` u64, `score` f32 = the fused score F, `query` = the request), every
        request's list best first, back to back in request order; counts[b] = the hits of request b."""
        store = self.vector_store
        hits, counts, stats = store._run_hybrid(self.resolve())
        store.last_stats = stats
        return hits, counts


def query_desc(r, queries: Optional[np.ndarray], nq: int, mode: int, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
    """The ott_query_desc of a resolved record: `r` supplies metric, take, filter_cmp, filter_thr, k, row_mask and, where it has
    one, path (else Path.Auto); `queries` is the query matrix or None.  Returns (desc, keep): the descriptor holds bare addresses
    into the arrays of `keep`, which the caller keeps referenced until the native call has returned.  The evaluated device row
    mask takes precedence over the record's; a row mask of size 0 is not sent."""
    d = N.QueryDesc()
    keep = [queries]
    d.queries = None if queries is None else queries.ctypes.data
    d.nq = nq
    d.metric, d.take, d.filter_cmp, d.filter_thr = r.metric, r.take, r.filter_cmp, r.filter_thr
    d.mode, d.k, d.path = int(mode), r.k, getattr(r, "path", int(Path.Auto))
    if chunk_mask is not None:
        cm = N.pack_bits(chunk_mask)
        keep.append(cm)
        d.chunk_mask = cm.ctypes.data
    if use_device_row_mask:
        d.use_device_row_mask = 1
    elif r.row_mask is not None and r.row_mask.size:
        rm = N.pack_bits(r.row_mask)
        keep.append(rm)
        d.row_mask = rm.ctypes.data
        d.row_mask_bits = int(r.row_mask.size)
    return d, keep


class VecStore:
    """src/vec.rs:338-412: row-major f32 vectors + per-row inverse norms, resident in HBM."""

    def __init__(self, dim: int, device: Optional[int] = None, devices: Optional[Sequence[int]] = None):  # VecStore::new, src/vec.rs:348-355
        """`devices`: a list of HIP device ordinals makes this ONE store over several GPUs of this process
        (ott_store_create_multi): one shard per entry, contiguous chunk ranges in row order; every method below and
        `.query(...).take(k).collect()` work unchanged and return the same bits as a single-GPU store.  An ordinal may
        repeat (several shards on one GPU).  Default, when the caller names NEITHER `device` nor `devices` and the process
        is not one rank of a multi-process job (WORLD_SIZE > 1: there every rank's shard is a single-GPU store on its own
        GPU): the environment variable OTTERS_HIP_DEVICES ("0,1,2,3"), else GPU 0.  A shard is brought in per 32768 rows (`set_option("multi_min_shard_rows", n)`; 0 = always split
        evenly): smaller stores stay on the first GPU and are answered by that shard's own query."""
        self.dim = int(dim)
        if (devices is None and device is None and os.environ.get("OTTERS_HIP_DEVICES")
                and int(os.environ.get("WORLD_SIZE", "1") or "1") <= 1):
            devices = [int(x) for x in os.environ["OTTERS_HIP_DEVICES"].split(",") if x.strip() != ""]
        self.devices = [int(x) for x in devices] if devices is not None else None
        self.device = int(self.devices[0]) if self.devices else int(device or 0)
        self._h = None        # ott_store*, created on first append
        self._n = 0
        self._chunk_size = None
        self._base_offset = 0
        self._reduce = None
        self._options: dict = {}
        self._n_groups = 0
        self._groups_gen = 0  # changes with every set_groups / clear_groups
        self._group_labels: Optional[np.ndarray] = None  # set_groups: np.unique's sorted labels, [dense id] = label
        self.last_stats: Optional[dict] = None
        # OTTERS_TIE_ORDER=reference: this mirror then returns, like the Rust patch and the C++ mirror do by default, the
        # reference's own outcome at exact score ties (one TopKCollector over the store); default here: the canonical order
        if os.environ.get("OTTERS_TIE_ORDER") == "reference":
            self._options["tie_order"] = 1

    @staticmethod
    def new(dim: int, device: Optional[int] = None, devices: Optional[Sequence[int]] = None) -> "VecStore":
        return VecStore(dim, device, devices)

    # -- native handle -------------------------------------------------------------------------
    def _handle(self):
        if self._h is None:
            h = C.c_void_p()
            if self.devices is not None:
                ids = (C.c_int * len(self.devices))(*self.devices)
                N.check(N.lib().ott_store_create_multi(self.dim, len(self.devices), ids, C.byref(h)))
            else:
                N.check(N.lib().ott_store_create(self.dim, self.device, C.byref(h)))
            self._h = h
            if self._chunk_size is not None:
                N.check(N.lib().ott_store_set_chunk_size(h, self._chunk_size))
            if self._base_offset:
                N.check(N.lib().ott_store_set_base_offset(h, self._base_offset))
            if self._reduce is not None:
                N.check(N.lib().ott_store_set_reduce_order(h, self._reduce))
            for name, value in self._options.items():
                N.check(N.lib().ott_store_set_option(h, name.encode(), value))
        return self._h

    def close(self) -> None:
        if self._h is not None:
            N.lib().ott_store_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ingest --------------------------------------------------------------------------------
    def add_vector(self, vector) -> None:  # src/vec.rs:357-371
        v = np.asarray(vector, dtype=np.float32).ravel()
        if v.size != self.dim:
            raise OttersError(f"Input vector length {v.size} does not match expected dimension {self.dim}")
        self._append(v[None, :])

    def add_vectors(self, vectors) -> None:  # src/vec.rs:373-376 (try_for_each: rows before a bad one stay added)
        if isinstance(vectors, np.ndarray) and vectors.ndim == 2:
            if vectors.shape[1] != self.dim:
                if vectors.shape[0]:
                    raise OttersError(f"Input vector length {vectors.shape[1]} does not match expected dimension {self.dim}")
                return
            self._append(vectors)
            return
        good = []
        for v in vectors:
            a = np.asarray(v, dtype=np.float32).ravel()
            if a.size != self.dim:
                if good:
                    self._append(np.stack(good))
                raise OttersError(f"Input vector length {a.size} does not match expected dimension {self.dim}")
            good.append(a)
        if good:
            self._append(np.stack(good))

    def _append(self, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.shape[0] == 0:
            return
        N.check(N.lib().ott_store_append(self._handle(), N.ptr(rows), rows.shape[0]))
        self._n += rows.shape[0]

    # extensions used by benchmarks / tests
    def reserve(self, n_rows: int) -> None:
        N.check(N.lib().ott_store_reserve(self._handle(), int(n_rows)))

    def append_random(self, n_rows: int, seed: int) -> None:
        """Synthetic uniform [-1,1) rows generated on the GPU (examples/demo.rs:4-7 distribution)."""
        N.check(N.lib().ott_store_append_random(self._handle(), int(n_rows), int(seed)))
        self._n += int(n_rows)

    def append_clustered(self, n_rows: int, seed: int, n_clusters: int, spread: float, aniso: float = 0.0) -> None:
        """Synthetic clustered rows generated on the GPU (ott_store_append_clustered): centres uniform [-1,1), members
        centre + spread * uniform noise, optionally shrinking along the dimensions (aniso)."""
        N.check(N.lib().ott_store_append_clustered(self._handle(), int(n_rows), int(seed), int(n_clusters), float(spread), float(aniso)))
        self._n += int(n_rows)

    def append_device(self, dev_ptr: int, n_rows: int) -> None:
        N.check(N.lib().ott_store_append_device(self._handle(), C.c_void_p(dev_ptr), int(n_rows)))
        self._n += int(n_rows)

    def write_rows(self, first_row: int, rows) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.dim)
        N.check(N.lib().ott_store_write_rows(self._handle(), int(first_row), N.ptr(rows), rows.shape[0]))

    # -- deleted rows (include/otters_hip.h: ott_store_delete_rows) ------------------------------------
    def _set_live(self, fn, ids) -> int:
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).ravel())
        if ids.size and int(ids.min()) < 0:
            raise OttersError(f"row {int(ids.min())} is out of range (the store holds {self._n} rows)")
        ids = ids.astype(np.uint64)
        changed = C.c_uint64(0)
        N.check(fn(self._handle(), N.ptr(ids), ids.size, C.byref(changed)))
        return int(changed.value)

    def delete_rows(self, ids) -> int:
        """Rows `ids` (counted from the store's first row) no longer appear in any result; indices stay stable and `len()`
        keeps counting them.  Returns how many rows changed state (duplicates and repeats are not errors)."""
        return self._set_live(N.lib().ott_store_delete_rows, ids)

    def restore_rows(self, ids) -> int:
        """Brings deleted rows back exactly as they were.  Returns how many rows changed state."""
        return self._set_live(N.lib().ott_store_restore_rows, ids)

    def live_len(self) -> int:
        """`len()` minus the deleted rows."""
        return int(N.lib().ott_store_live_len(self._handle())) if self._h is not None else self._n

    def live_mask(self) -> np.ndarray:
        """bool[len()]: True = live."""
        if self._n == 0:
            return np.zeros(0, dtype=bool)
        words = np.zeros((self._n + 63) // 64, dtype="<u8")
        N.check(N.lib().ott_store_read_live_mask(self._handle(), N.ptr(words)))
        return N.unpack_bits(words, self._n)

    def compact(self) -> np.ndarray:
        """Physically removes the deleted rows (order preserved): `len()` becomes `live_len()`.  Returns int64[old len]:
        every row's new index, -1 for a removed row.  Not on a multi-GPU store, nor while metadata columns are resident."""
        new_index = np.empty(self._n, dtype="<u8")
        N.check(N.lib().ott_store_compact(self._handle(), N.ptr(new_index)))
        self._n = int(N.lib().ott_store_len(self._handle()))
        return new_index.view(np.int64)  # (UINT64_MAX reads as -1)

    # -- grouped search (include/otters_hip.h: ott_query_groups) ---------------------------------------
    def set_groups(self, ids) -> None:
        """One group label per row (any integer array of length len()); the host makes them dense (dense_group_ids) and the
        store keeps them in HBM at 4 B per row.  A second call replaces the first; rows appended afterwards need a new call.
        While groups are set, compact() is refused and a multi-GPU store moves no rows."""
        a = np.asarray(ids)
        if a.size != self._n:
            raise OttersError(f"{a.size} group ids for a store of {self._n} rows")
        self._set_dense_groups(*dense_group_ids(a))
        self._group_labels = np.unique(a) if a.size else None

    def _set_dense_groups(self, dense: np.ndarray, n_groups: int) -> int:
        """uint32 ids that are dense already (MetaStore.distinct_by builds them per column).  Returns the store's group
        generation: it changes with every set_groups / clear_groups, so a caller that remembers it knows whether the ids
        it uploaded are still the ones the store holds."""
        N.check(N.lib().ott_store_set_groups(self._handle(), N.ptr(dense), dense.size, n_groups))
        self._n_groups = n_groups
        self._group_labels = None
        self._groups_gen += 1
        return self._groups_gen

    def clear_groups(self) -> None:
        if self._h is not None:
            N.check(N.lib().ott_store_clear_groups(self._h))
        self._n_groups = 0
        self._group_labels = None
        self._groups_gen += 1

    def group_labels(self) -> Optional[np.ndarray]:
        """The labels set_groups was given, sorted and duplicate-free: [dense group id] = label (what max_sim().collect() reports).
        None when no groups are set or the ids came dense already (_set_dense_groups)."""
        return self._group_labels

    def group_count(self) -> int:
        """Number of groups set_groups left (0 = none)."""
        return self._n_groups

    # -- metadata columns and device mask slots of a bare store (include/otters_hip.h: ott_store_add_column, ott_store_write_row_mask_slot)
    def add_column(self, values, dtype, nulls=None) -> int:
        """A metadata column resident in HBM beside the rows (ott_store_add_column): `values` holds len() elements of `dtype`
        (DataType.Int32 / Int64 / Float32 / Float64 / DateTime, or its number), `nulls` an optional boolean array, True = NULL.
        Returns the column id BoostTerm.value and BoostTerm.lin_decay name."""
        np_dtype = {0: np.int32, 1: np.int64, 2: np.float32, 3: np.float64, 5: np.int64}.get(int(dtype))
        if np_dtype is None:
            raise OttersError("ott_store_add_column: only numeric / datetime columns live on the GPU")
        vals = np.ascontiguousarray(np.asarray(values).ravel(), dtype=np_dtype)
        words = None
        if nulls is not None:
            nb = np.asarray(nulls, dtype=bool).ravel()
            if nb.size != vals.size:
                raise OttersError(f"add_column: {nb.size} NULL flags for {vals.size} values")
            words = N.pack_bits(nb)
        cid = C.c_uint32(0)
        N.check(N.lib().ott_store_add_column(self._handle(), int(dtype), N.ptr(vals), N.ptr(words), vals.size, C.byref(cid)))
        return int(cid.value)

    def write_row_mask_slot(self, slot: int, mask) -> None:
        """A boolean row mask (True = keep; rows at or beyond its length are kept) into device mask slot `slot`
        (ott_store_write_row_mask_slot); an empty mask empties the slot."""
        m = np.asarray(mask, dtype=bool).ravel()
        words = N.pack_bits(m)
        N.check(N.lib().ott_store_write_row_mask_slot(self._handle(), int(slot), N.ptr(words), int(m.size)))

    def clear_row_mask_slots(self) -> None:
        """Every device mask slot is emptied (ott_store_clear_row_mask_slots)."""
        if self._h is not None:
            N.check(N.lib().ott_store_clear_row_mask_slots(self._h))

    # -- sparse rows (include/otters_hip.h: ott_store_set_sparse, ott_query_sparse) --------------------------------------------
    def set_sparse(self, indptr, indices, values, vocab: int) -> None:
        """A sparse row per stored row, as CSR: indptr[len() + 1], ascending distinct indices below `vocab` inside a row, finite
        values.  The store keeps them in HBM as a sliced ELL layout.  A second call replaces the first; rows appended afterwards
        need a new call.  While sparse rows are set, compact() is refused.  Not on a multi-GPU store."""
        ptr = np.ascontiguousarray(np.asarray(indptr).ravel(), dtype=np.uint64)
        idx = np.asarray(indices).ravel()
        if idx.size and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
            raise OttersError("ott_store_set_sparse: an index is not a 32-bit unsigned integer")
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        val = np.ascontiguousarray(np.asarray(values).ravel(), dtype=np.float32)
        if ptr.size == 0 or idx.size != val.size or int(ptr[-1]) != idx.size:
            raise OttersError(f"ott_store_set_sparse: indptr ends at {int(ptr[-1]) if ptr.size else 0}, {idx.size} indices and {val.size} values were given")
        if not 0 <= int(vocab) <= 0xFFFFFFFF:
            raise OttersError(f"ott_store_set_sparse: vocab {vocab} is not in 1 .. OTT_SPARSE_MAX_VOCAB ({SPARSE_MAX_VOCAB}); remap the indices")
        N.check(N.lib().ott_store_set_sparse(self._handle(), N.ptr(ptr), N.ptr(idx), N.ptr(val), ptr.size - 1, int(vocab)))

    def set_sparse_rows(self, rows, vocab: int) -> None:
        """set_sparse for a list of (indices, values) pairs, one per stored row."""
        self.set_sparse(*sparse_csr(rows), vocab)

    def clear_sparse(self) -> None:
        if self._h is not None:
            N.check(N.lib().ott_store_clear_sparse(self._h))

    def sparse_info(self) -> Optional[dict]:
        """{vocab, nnz, padded_entries, bytes} of the sparse rows in HBM, None when none are set."""
        if self._h is None:
            return None
        vocab, nnz, padded, nbytes = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        N.check(N.lib().ott_store_sparse_info(self._h, C.byref(vocab), C.byref(nnz), C.byref(padded), C.byref(nbytes)))
        if vocab.value == 0:
            return None
        return {"vocab": int(vocab.value), "nnz": int(nnz.value), "padded_entries": int(padded.value), "bytes": int(nbytes.value)}

    def read_sparse(self, first: int = 0, n: Optional[int] = None):
        """(indptr, indices, values): the CSR of sparse rows [first, first + n), read back from the device layout bit for bit."""
        info = self.sparse_info()
        if info is None:
            raise OttersError("ott_store_read_sparse: no sparse rows are set (ott_store_set_sparse)")
        n = self._n - first if n is None else n
        ptr = np.zeros(max(n, 0) + 1, dtype=np.uint64)
        idx = np.zeros(max(info["nnz"], 1), dtype=np.uint32)
        val = np.zeros(max(info["nnz"], 1), dtype=np.float32)
        N.check(N.lib().ott_store_read_sparse(self._h, int(first), int(n), N.ptr(ptr), N.ptr(idx), N.ptr(val), info["nnz"]))
        nnz = int(ptr[-1])
        return ptr, idx[:nnz].copy(), val[:nnz].copy()

    def sparse_query(self, q) -> SparseQueryPlan:
        """Exact sparse dot search (ott_query_sparse): `q` is one (indices, values) pair or a list of them; indices distinct and
        below the store's vocab, in any order.  .take(k).collect() for one query, .collect_per_query() for a batch."""
        return SparseQueryPlan(self, q)

    def _run_sparse(self, rs: ResolvedSparse, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query_sparse (ott_query_sparse_idf where the plan asked for idf).  Returns (hits HIT_DTYPE array, per-query counts, stats dict)."""
        nq = int(rs.indptr.size - 1)
        cap = max(nq * min(rs.k, self._n), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)
        d, keep = query_desc(rs, None, nq, Mode.PerQuery if nq > 1 else Mode.Merged, chunk_mask, use_device_row_mask)
        n_out, per, st = C.c_uint64(0), (C.c_uint64 * max(nq, 1))(), N.Stats()
        fn = N.lib().ott_query_sparse_idf if rs.idf else N.lib().ott_query_sparse
        N.check(fn(self._handle(), C.byref(d), N.ptr(rs.indptr), N.ptr(rs.indices) if rs.indices.size else None,
                   N.ptr(rs.values) if rs.values.size else None, N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        return out[: n_out.value].copy(), list(per)[:nq], st.as_dict()

    def sparse_df(self):
        """(df, n_docs): df[i] (uint32[vocab]) = the live rows whose sparse row stores index i, n_docs = the live rows
        (ott_store_sparse_df).  Cached on the device; rebuilt after set_sparse, delete_rows, restore_rows."""
        info = self.sparse_info()
        if info is None:
            raise OttersError("ott_store_sparse_df: no sparse rows are set (ott_store_set_sparse)")
        df, n_docs = np.zeros(info["vocab"], dtype=np.uint32), C.c_uint64(0)
        N.check(N.lib().ott_store_sparse_df(self._h, N.ptr(df), C.byref(n_docs)))
        return df, int(n_docs.value)

    def sparse_df_builds(self) -> int:
        """How many times the document frequencies were built (ott_store_sparse_df_builds)."""
        return 0 if self._h is None else int(N.lib().ott_store_sparse_df_builds(self._h))

    # -- bit rows (include/otters_hip.h: ott_store_set_binary, ott_query_binary) ------------------------------------------------
    def set_binary(self, bits, n_bits: Optional[int] = None) -> None:
        """A bit row per stored row: a bool / 0-1 matrix [len(), n_bits], or packed uint64 words [len(), ceil(n_bits / 64)] (bit j in
        bit j % 64 of word j // 64, padding bits zero).  The store keeps them in HBM in slices of 64 transposed rows.  A second call
        replaces the first; rows appended afterwards need a new call.  While bit rows are set, compact() is refused.  Not on a
        multi-GPU store."""
        words, nb = binary_words(bits, n_bits, "ott_store_set_binary")
        if not 0 <= nb <= 0xFFFFFFFF:
            raise OttersError(f"ott_store_set_binary: n_bits {nb} is not in 1 .. OTT_BINARY_MAX_BITS ({BINARY_MAX_BITS})")
        N.check(N.lib().ott_store_set_binary(self._handle(), N.ptr(words) if words.size else None, int(words.shape[0]), nb))

    def set_binary_sign(self) -> None:
        """Bit rows from the dense rows, on the device: n_bits = dim, bit j of row r = (row[j] > 0.0) in f32 (NaN and both zeros
        give 0): binary quantisation (ott_store_set_binary_sign).  Refused where dim > 16384."""
        N.check(N.lib().ott_store_set_binary_sign(self._handle()))

    def clear_binary(self) -> None:
        if self._h is not None:
            N.check(N.lib().ott_store_clear_binary(self._h))

    def binary_info(self) -> Optional[dict]:
        """{n_bits, bytes} of the bit rows in HBM, None when none are set."""
        if self._h is None:
            return None
        nb, nbytes = C.c_uint32(0), C.c_uint64(0)
        N.check(N.lib().ott_store_binary_info(self._h, C.byref(nb), C.byref(nbytes)))
        if nb.value == 0:
            return None
        return {"n_bits": int(nb.value), "bytes": int(nbytes.value)}

    def read_binary(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """uint64[n, ceil(n_bits / 64)]: the words of bit rows [first, first + n), read back from the device layout bit for bit."""
        info = self.binary_info()
        if info is None:
            raise OttersError("ott_store_read_binary: no bit rows are set (ott_store_set_binary)")
        n = self._n - first if n is None else n
        out = np.zeros((max(n, 0), (info["n_bits"] + 63) // 64), dtype=np.uint64)
        N.check(N.lib().ott_store_read_binary(self._h, int(first), int(n), N.ptr(out) if out.size else None))
        return out

    def binary_counters(self) -> dict:
        """{gated_calls, pairs_emitted, overflows, table_calls}: running totals of this store's binary queries (ott_store_binary_counters)."""
        out = (C.c_uint64 * 4)()
        if self._h is not None:
            N.check(N.lib().ott_store_binary_counters(self._h, out))
        return dict(zip(("gated_calls", "pairs_emitted", "overflows", "table_calls"), (int(x) for x in out)))

    def binary_query(self, q_bits, n_bits: Optional[int] = None) -> BinaryQueryPlan:
        """Exact Hamming search (ott_query_binary): `q_bits` is one bit vector or a matrix of them (bool / 0-1), or packed uint64
        words with `n_bits`.  .take(k).collect() for one query, .collect_per_query() for a batch; the default take is Min."""
        return BinaryQueryPlan(self, q_bits, n_bits)

    def binary_query_sign(self, q_dense) -> BinaryQueryPlan:
        """binary_query for the sign bits of dense queries, packed on the host by set_binary_sign's rule."""
        return BinaryQueryPlan(self, sign_bits(q_dense))

    def _run_binary(self, rb: ResolvedBinary, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query_binary.  Returns (hits HIT_DTYPE array, per-query counts, stats dict)."""
        nq = int(rb.words.shape[0])
        cap = max(nq * min(rb.k, self._n), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)
        d, keep = query_desc(rb, None, nq, Mode.PerQuery if nq > 1 else Mode.Merged, chunk_mask, use_device_row_mask)
        n_out, per, st = C.c_uint64(0), (C.c_uint64 * max(nq, 1))(), N.Stats()
        N.check(N.lib().ott_query_binary(self._handle(), C.byref(d), N.ptr(rb.words), N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        return out[: n_out.value].copy(), list(per)[:nq], st.as_dict()

    def hybrid(self, dense_sets, sparse_sets, metric: Metric) -> HybridPlan:
        """Hybrid search (ott_query_hybrid): `dense_sets` a sequence of [legs, dim] matrices and `sparse_sets` a sequence of lists of
        (indices, values) pairs, one of each per request (None or empty = no leg of that kind);
        .rrf() / .dbsf() / .min_max(), .idf(), .sparse_filter(thr, cmp), .fetch(n), .take(k).collect() returns one fused ranking per
        request."""
        return HybridPlan(self, dense_sets, sparse_sets, metric)

    def _run_hybrid(self, rh: ResolvedHybrid, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query_hybrid.  Returns (hits HIT_DTYPE array, per-request counts, stats dict)."""
        B = int(rh.dense_per_request.size)
        if self._n == 0:  # an empty store: a valid call with no hits (no native store exists yet)
            return np.zeros(0, dtype=N.HIT_DTYPE), [0] * B, N.Stats().as_dict()
        stride = min(rh.fetch, self._n)
        cap = max(sum(min(rh.k, (int(a) + int(b)) * stride) for a, b in zip(rh.dense_per_request, rh.sparse_per_request)), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)
        nq = 0 if rh.queries is None else int(rh.queries.shape[0])
        d, keep = query_desc(rh, rh.queries, nq, Mode.PerQuery, chunk_mask, use_device_row_mask)
        n_out, per, st = C.c_uint64(0), (C.c_uint64 * B)(), N.Stats()
        n_sparse = int(rh.sq_indptr.size - 1)
        N.check(N.lib().ott_query_hybrid(self._handle(), C.byref(d), N.ptr(rh.dense_per_request), N.ptr(rh.sq_indptr),
                                         N.ptr(rh.sq_indices) if rh.sq_indices.size else None, N.ptr(rh.sq_values) if rh.sq_values.size else None,
                                         n_sparse, N.ptr(rh.sparse_per_request), rh.sparse_cmp, rh.sparse_thr, rh.sparse_flags, B, rh.fusion, rh.rrf_k,
                                         N.ptr(rh.weights) if rh.weights is not None else None, rh.fetch, N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        return out[: n_out.value].copy(), list(per), st.as_dict()

    def shards(self):
        """[(device, first_row, n_rows)] of the store's shards (one entry for a single-GPU store)."""
        h = self._handle()
        out = []
        for g in range(N.lib().ott_store_shard_count(h)):
            dev, first, cnt = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
            N.check(N.lib().ott_store_shard_info(h, g, C.byref(dev), C.byref(first), C.byref(cnt)))
            out.append((dev.value, first.value, cnt.value))
        return out

    def transport(self) -> str:
        """How a multi-GPU store's candidate blocks travel: "peer", "rccl", "undecided" (before the first query); "none" for one GPU."""
        return N.lib().ott_store_transport(self._handle()).decode()

    def set_chunk_size(self, chunk_size: int) -> None:
        self._chunk_size = max(int(chunk_size), 1)
        if self._h is not None:
            N.check(N.lib().ott_store_set_chunk_size(self._h, self._chunk_size))

    def set_base_offset(self, base: int) -> None:
        self._base_offset = int(base)
        if self._h is not None:
            N.check(N.lib().ott_store_set_base_offset(self._h, self._base_offset))

    def set_batch_image(self, enabled: bool) -> None:
        """Allow (default) or forbid the bf16 copies of the corpus the batch path keeps in HBM (the hi plane, half the size of
        the rows, built by the first batch query; the split image, the same size, built only when a batch needs the split
        pass).  Results never depend on them, only the speed of batches."""
        N.check(N.lib().ott_store_set_batch_image(self._handle(), 1 if enabled else 0))

    def prepare_batch(self) -> None:
        """Build the batch path's hi plane now (after loading / appending) rather than inside the first batch query."""
        if self._n:
            N.check(N.lib().ott_store_prepare_batch(self._handle()))

    def batch_ready(self) -> bool:
        """The batch path's hi plane exists and covers every row (built in the background after appends: option hi_prebuild)."""
        return bool(self._n) and bool(N.lib().ott_store_batch_ready(self._handle()))

    def exact_finished(self) -> int:
        """Rows the pruned exact sweeps of this store have finished in f32 so far (ott_store_exact_finished): a running total."""
        return int(N.lib().ott_store_exact_finished(self._handle()))

    def set_option(self, name: str, value: int) -> None:
        """Behaviour switch of this store (ott_store_set_option; the twenty-nine names are listed in include/otters_hip.h:
        "tie_order", "hi_fmt", "hi_prebuild", ..., "force_fallback").  Results never depend on any but "tie_order"."""
        self._options[name] = int(value)
        if self._h is not None:
            N.check(N.lib().ott_store_set_option(self._h, name.encode(), int(value)))

    def set_tie_order(self, order: str) -> None:
        """Which of several EQUAL-scoring (row, query) pairs survives the cut at take(k).  "canonical" (default): the
        library's total order — better score, lower row, lower query.  "reference": what the reference's TopKCollector
        keeps (strict-improvement inserts in visit order — 8-row block, query, row — at the position its binary search
        returns, src/vec_compute.rs:236-277; one collector over the store, src/vec.rs:217-219).  Signed zeros: the
        collector admits a pair by IEEE comparison (-0.0 == +0.0) but places it by total order (+0.0 above -0.0), so at a
        cut through the zeros the two orders may keep zeros of different signs.  Otherwise scores and every hit strictly
        better than the k-th score are the same either way."""
        self.set_option("tie_order", {"canonical": 0, "reference": 1, "reference_chunked": 2}[order])

    def set_reduce_order(self, order: int) -> None:
        self._reduce = int(order)
        if self._h is not None:
            N.check(N.lib().ott_store_set_reduce_order(self._h, self._reduce))

    def rows(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self._n - first if n is None else n
        out = np.empty((n, self.dim), dtype=np.float32)
        if n:
            N.check(N.lib().ott_store_read_rows(self._handle(), int(first), int(n), N.ptr(out)))
        return out

    def inv_norms(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self._n - first if n is None else n
        out = np.empty(n, dtype=np.float32)
        if n:
            N.check(N.lib().ott_store_read_inv_norms(self._handle(), int(first), int(n), N.ptr(out)))
        return out

    # -- reference API -------------------------------------------------------------------------
    def len(self) -> int:  # src/vec.rs:378-380
        return self._n

    def __len__(self) -> int:
        return self._n

    def is_empty(self) -> bool:  # src/vec.rs:382-384
        return self._n == 0

    def query(self, queries, metric: Metric) -> VecQueryPlan:  # src/vec.rs:386-411
        plan = VecQueryPlan()
        plan.query_vectors = QueryBatch(queries).queries
        plan.search_metric = Metric(metric)
        plan.vector_store = self
        return plan

    # -- execution -----------------------------------------------------------------------------
    def _run(self, rq: ResolvedQuery, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query (ott_query_ids when the plan carries an id list).  Returns (hits HIT_DTYPE array, per-query counts, stats dict)."""
        nq = rq.queries.shape[0]
        ids = rq.row_ids
        if self._n == 0 and (ids is None or ids.size == 0):  # nothing resident: VecQueryPlan::collect yields an empty Vec (src/vec.rs:222, 270)
            return np.zeros(0, dtype=N.HIT_DTYPE), [0] * nq, None
        perq = rq.mode == Mode.PerQuery
        rows = self._n if ids is None else int(np.unique(ids).size)  # the buffer is sized by the list, not by the store
        pool = rows if perq else rows * nq
        k_eff = min(rq.k, pool)
        cap = max(k_eff * (nq if perq else 1), 1)
        if rq.grouped:  # at most one hit per group and query
            cap = max(min(rq.k, self._n_groups) * nq, 1)
        if rq.group_size:  # at most group_size hits per group and query
            cap = max(min(rq.k, self._n_groups) * nq * rq.group_size, 1)
        if rq.max_sim:  # at most one hit per group
            cap = max(min(rq.k, self._n_groups), 1)
        if rq.group_list is not None:  # ... and per listed group
            cap = max(min(rq.k, int(np.unique(rq.group_list).size)), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)  # ott_query writes n_out entries; only those are returned
        d, keep = query_desc(rq, rq.queries, nq, rq.mode, chunk_mask, use_device_row_mask)
        n_out, per, st = C.c_uint64(0), (C.c_uint64 * nq)(), N.Stats()
        if rq.group_list is not None:
            gl = rq.group_list
            N.check(N.lib().ott_query_maxsim_groups(self._handle(), C.byref(d), N.ptr(gl) if gl.size else None, gl.size, N.ptr(out), cap, C.byref(n_out), C.byref(st)))
            per[0] = n_out.value
        elif rq.max_sim:
            N.check(N.lib().ott_query_maxsim(self._handle(), C.byref(d), N.ptr(out), cap, C.byref(n_out), C.byref(st)))
            per[0] = n_out.value
        elif rq.group_size:
            gids = np.empty(cap, dtype=np.uint32)
            N.check(N.lib().ott_query_groups_top(self._handle(), C.byref(d), rq.group_size, N.ptr(out), cap, C.byref(n_out), per, N.ptr(gids), C.byref(st)))
            rq.group_of_hit = gids[: n_out.value].copy()
        elif rq.grouped:
            N.check(N.lib().ott_query_groups(self._handle(), C.byref(d), N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        elif rq.mmr is not None:
            lam, fetch_k = rq.mmr
            vals = np.empty(cap, dtype=np.float32)
            N.check(N.lib().ott_query_mmr(self._handle(), C.byref(d), None if ids is None else N.ptr(ids), 0 if ids is None else ids.size, fetch_k,
                                          float(lam), N.ptr(out), cap, C.byref(n_out), per, N.ptr(vals), C.byref(st)))
            rq.mmr_values = vals[: n_out.value].copy()
        elif rq.mask_of_query is not None:  # a row mask per query: the distinct masks back to back, one word row each
            qm = rq.query_masks
            n_masks, bits = (0, 0) if qm is None else (int(qm.shape[0]), int(qm.shape[1]))
            words = np.zeros(0, dtype="<u8") if not n_masks or not bits else np.ascontiguousarray(np.stack([N.pack_bits(m) for m in qm]))
            moq = np.ascontiguousarray(rq.mask_of_query, dtype=np.uint32)
            N.check(N.lib().ott_query_masks(self._handle(), C.byref(d), N.ptr(words) if words.size else None, n_masks if words.size else 0, bits,
                                            N.ptr(moq), N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        elif rq.boost is not None:
            terms, n_terms, combine, score_weight = rq.boost
            N.check(N.lib().ott_query_boost(self._handle(), C.byref(d), combine, score_weight, terms, n_terms, N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        elif ids is None:
            N.check(N.lib().ott_query(self._handle(), C.byref(d), N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        else:
            N.check(N.lib().ott_query_ids(self._handle(), C.byref(d), N.ptr(ids), ids.size, N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        hits = out if n_out.value == cap else out[: n_out.value].copy()
        stats = st.as_dict()
        if rq.group_list is not None:  # how often this store has built its group-to-rows index so far
            stats["group_index_builds"] = int(N.lib().ott_store_group_index_builds(self._handle()))
        return hits, list(per), stats

    def max_sim_batch(self, token_sets, metric: Metric) -> MaxSimBatchPlan:
        """MaxSim re-ranking for many queries at once (ott_query_maxsim_groups_batch): `token_sets` is a sequence of token matrices,
        one per query; .with_groups(lists) gives every query its own candidate list."""
        return MaxSimBatchPlan(self, token_sets, metric)

    def _run_maxsim_batch(self, rb: ResolvedMaxSimBatch, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query_maxsim_groups_batch.  Returns (hits HIT_DTYPE array, per-query counts, stats dict)."""
        B = int(rb.tokens_per_query.size)
        cap = max(sum(min(rb.k, n) for n in rb.distinct_per_query), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)
        d, keep = query_desc(rb, rb.queries, int(rb.queries.shape[0]), Mode.Merged, chunk_mask, use_device_row_mask)  # (the record has no path: always Path.Auto)
        n_out, per, st = C.c_uint64(0), (C.c_uint64 * B)(), N.Stats()
        N.check(N.lib().ott_query_maxsim_groups_batch(self._handle(), C.byref(d), N.ptr(rb.tokens_per_query), N.ptr(rb.listed_per_query), B,
                                                      N.ptr(rb.groups) if rb.groups.size else None, N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        hits = out if n_out.value == cap else out[: n_out.value].copy()
        stats = st.as_dict()
        stats["group_index_builds"] = int(N.lib().ott_store_group_index_builds(self._handle()))
        return hits, list(per), stats

    def recommend(self, positive, negative=(), metric: Metric = Metric.Cosine, strategy: RecommendStrategy = RecommendStrategy.BestScore) -> RecommendPlan:
        """Recommend by example rows (ott_query_recommend; ott_query_recommend_strategy for another `strategy`): `positive` and
        `negative` are row ids counted from the store's first row (not shifted by the base offset); .take(k).collect() returns the
        hits and their sides."""
        return RecommendPlan(self, positive, negative, metric, strategy)

    def _run_recommend(self, rr: ResolvedRecommend, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query_recommend, or ott_query_recommend_strategy for another strategy than BestScore.  Returns (hits HIT_DTYPE array,
        sides uint32 array, stats dict)."""
        cap = max(min(rr.k, self._n), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)
        sides = np.empty(cap, dtype=np.uint32)
        d, keep = query_desc(rr, None, 0, Mode.Merged, chunk_mask, use_device_row_mask)
        n_out, st = C.c_uint64(0), N.Stats()
        neg = N.ptr(rr.negative) if rr.negative.size else None
        if rr.strategy == int(RecommendStrategy.BestScore):
            N.check(N.lib().ott_query_recommend(self._handle(), C.byref(d), N.ptr(rr.positive), rr.positive.size, neg, rr.negative.size, rr.flags, N.ptr(out), cap,
                                                C.byref(n_out), N.ptr(sides), C.byref(st)))
        else:
            N.check(N.lib().ott_query_recommend_strategy(self._handle(), C.byref(d), rr.strategy, N.ptr(rr.positive), rr.positive.size, neg, rr.negative.size, rr.flags,
                                                         N.ptr(out), cap, C.byref(n_out), N.ptr(sides), C.byref(st)))
        return out[: n_out.value].copy(), sides[: n_out.value].copy(), st.as_dict()

    def fuse(self, leg_sets, metric: Metric) -> FusePlan:
        """Rank fusion (ott_query_fuse): `leg_sets` is a sequence of [legs, dim] matrices, one per request;
        .rrf() / .dbsf() / .min_max(), .fetch(n), .take(k).collect() returns one fused ranking per request."""
        return FusePlan(self, leg_sets, metric)

    def _run_fuse(self, rf: ResolvedFuse, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query_fuse.  Returns (hits HIT_DTYPE array, per-request counts, stats dict)."""
        B = int(rf.legs_per_request.size)
        if self._n == 0:  # an empty store: a valid call with no hits (no native store exists yet)
            return np.zeros(0, dtype=N.HIT_DTYPE), [0] * B, N.Stats().as_dict()
        stride = min(rf.fetch, self._n)
        cap = max(sum(min(rf.k, int(l) * stride) for l in rf.legs_per_request), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)
        d, keep = query_desc(rf, rf.queries, int(rf.queries.shape[0]), Mode.PerQuery, chunk_mask, use_device_row_mask)
        n_out, per, st = C.c_uint64(0), (C.c_uint64 * B)(), N.Stats()
        N.check(N.lib().ott_query_fuse(self._handle(), C.byref(d), N.ptr(rf.legs_per_request), B, rf.fusion, rf.rrf_k,
                                       N.ptr(rf.weights) if rf.weights is not None else None, rf.fetch, N.ptr(out), cap, C.byref(n_out), per, C.byref(st)))
        return out[: n_out.value].copy(), list(per), st.as_dict()

    def discover(self, context, target=None, target_row=None, metric: Metric = Metric.Cosine) -> DiscoverPlan:
        """Discovery search (ott_query_discover): `context` is a sequence of (positive, negative) row id pairs counted from the
        store's first row (not shifted by the base offset); `target` a vector or `target_row` a stored row, or neither for a context
        search.  .take(k).collect() returns the hits with the pairs they win."""
        return DiscoverPlan(self, context, target, target_row, metric)

    def _run_discover(self, rd: ResolvedDiscover, chunk_mask: Optional[np.ndarray] = None, use_device_row_mask: bool = False):
        """ott_query_discover.  Returns (hits HIT_DTYPE array, wins uint32 array, stats dict)."""
        cap = max(min(rd.k, self._n), 1)
        out = np.empty(cap, dtype=N.HIT_DTYPE)
        wins = np.empty(cap, dtype=np.uint32)
        # the target vector, when there is one, is the call's one query
        d, keep = query_desc(rd, rd.target, 0 if rd.target is None else 1, Mode.Merged, chunk_mask, use_device_row_mask)
        n_out, st = C.c_uint64(0), N.Stats()
        N.check(N.lib().ott_query_discover(self._handle(), C.byref(d), rd.target_row, N.ptr(rd.positive), N.ptr(rd.negative), rd.positive.size, rd.min_wins, 0,
                                           N.ptr(out), cap, C.byref(n_out), N.ptr(wins), C.byref(st)))
        return out[: n_out.value].copy(), wins[: n_out.value].copy(), st.as_dict()

    def score_rows(self, queries, metric: Metric, ids) -> np.ndarray:
        """float32[nq, n_ids]: the score of every query against every row of `ids` (ott_store_score_rows) -- the exact path's bits,
        in the list's order, duplicates allowed, no filter and no top-k; a NaN score comes back as NaN.  Reads stored data: a
        deleted row is scored like any other."""
        qv = QueryBatch(queries).queries
        if len(qv) == 0:
            raise OttersError("No queries provided")
        q = qv if isinstance(qv, np.ndarray) else np.ascontiguousarray(np.stack(qv).astype(np.float32, copy=False))
        if q.shape[1] != self.dim:
            raise OttersError(f"Query vector length {q.shape[1]} does not match expected dimension {self.dim}")
        ids = as_row_ids(ids)
        out = np.empty((q.shape[0], ids.size), dtype=np.float32)
        N.check(N.lib().ott_store_score_rows(self._handle(), N.ptr(q), q.shape[0], int(Metric(metric)), N.ptr(ids), ids.size, N.ptr(out)))
        return out
