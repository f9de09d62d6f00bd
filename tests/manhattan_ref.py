"""Host reference for the Manhattan (L1) metric — TEST INFRASTRUCTURE ONLY.

The oracle (oracle/) has no L1, so this module restates the arithmetic contract ("The Manhattan metric") in numpy
f32, one IEEE operation at a time, and the selection rules the oracle applies to the other metrics:

    manhattan(q, v) = reduce_add(acc) + tail
      acc[l] = 0;  for each chunk j of chunks_exact(8), in order:  acc[l] = acc[l] + |q[8j+l] - v[8j+l]|
      tail   = 0;  for each remainder element i, in order:          tail   = tail + |q[i] - v[i]|

Every add is a separate rounded f32 add in that order (never np.sum, whose pairwise order is another one).  The same code with
the term swapped for d*d or q*v is held to oracle.l2sq / oracle.dot bit for bit (tests/test_manhattan_cpu.py), which anchors
the machinery to the pinned oracle.

Selection: the canonical total order (better score, lower row, lower query), the five filters, NaN dropped, merged and per-query
modes, row and chunk masks; the reference's tie outcomes through tests/test_tie_rule_model.py's closed form."""
from __future__ import annotations

import numpy as np

from test_tie_rule_model import collector_result, visit_rank

REDUCE_AVX, REDUCE_SEQ4 = 0, 1
TAKE_MIN, TAKE_MAX = 0, 1
CMP_NONE, CMP_LT, CMP_GT, CMP_LTE, CMP_GTE, CMP_EQ = 0, 1, 2, 3, 4, 5
HIT_DTYPE = np.dtype([("index", "<u8"), ("score", "<f4"), ("query", "<u4")])

TERMS = {
    "l1": lambda q, v: np.abs(q - v),
    "l2": lambda q, v: (q - v) * (q - v),
    "dot": lambda q, v: q * v,
}


def reduce8(acc: np.ndarray, mode: int) -> np.ndarray:
    """wide::f32x8::reduce_add over the last axis (8 lanes), in the store's order; f32 adds one at a time"""
    a = [acc[..., i] for i in range(8)]
    if mode == REDUCE_SEQ4:
        return (((a[0] + a[1]) + a[2]) + a[3]) + (((a[4] + a[5]) + a[6]) + a[7])
    return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]))


def scores(rows, queries, kind: str = "l1", reduce_mode: int = REDUCE_AVX, block: int = 1 << 16) -> np.ndarray:
    """[nq, n] f32 scores of every (query, row) pair under the contract, for the term `kind` ("l1", "l2" or "dot")"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    n, dim = rows.shape
    nq = queries.shape[0]
    term = TERMS[kind]
    full = dim // 8
    out = np.empty((nq, n), np.float32)
    with np.errstate(all="ignore"):
        for qi in range(nq):
            q = queries[qi]
            for b0 in range(0, n, block):
                v = rows[b0:b0 + block]
                t = term(q[None, :], v)                                   # one rounded op per element (abs is exact)
                assert t.dtype == np.float32
                acc = np.zeros((v.shape[0], 8), np.float32)
                tc = t[:, :full * 8].reshape(v.shape[0], full, 8)
                for j in range(full):                                     # chunks in order, eight independent chains
                    acc = acc + tc[:, j, :]
                tail = np.zeros(v.shape[0], np.float32)
                for i in range(full * 8, dim):                            # the remainder, sequentially
                    tail = tail + t[:, i]
                out[qi, b0:b0 + block] = reduce8(acc, reduce_mode) + tail
    return out


def ordkey(s: np.ndarray, take: int) -> np.ndarray:
    """ascending = better: the total order of the scores (f32 total_cmp), reversed for take Max"""
    bits = np.asarray(s, np.float32).view(np.uint32).astype(np.int64)
    key = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    return -key if take == TAKE_MAX else key


def passes(s: np.ndarray, cmp: int, thr: float) -> np.ndarray:
    """the filter (src/vec.rs:24-31) and the NaN drop (src/vec_compute.rs:237)"""
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        ok = {CMP_NONE: np.ones(s.shape, bool), CMP_LT: s < thr, CMP_GT: s > thr, CMP_LTE: s <= thr, CMP_GTE: s >= thr,
              CMP_EQ: s == thr}[int(cmp)]
    return ok & ~np.isnan(s)


def _pairs(S, take, cmp, thr, row_mask, row_ids=None):
    """(score, row, query) of every admitted pair; S: [nq, n]"""
    nq, n = S.shape
    ok = passes(S, cmp, thr)
    if row_mask is not None:
        m = np.ones(n, bool)
        rm = np.asarray(row_mask, bool)
        m[:min(n, rm.size)] = rm[:n]
        ok &= m[None, :]
    qq, rr = np.nonzero(ok)
    rows = rr if row_ids is None else np.asarray(row_ids)[rr]
    return S[qq, rr], rows.astype(np.int64), qq.astype(np.int64)


def _hits(sc, rows, qs):
    h = np.zeros(len(sc), HIT_DTYPE)
    h["score"], h["index"], h["query"] = sc, rows, qs
    return h


def select_canonical(S, take, k, cmp=CMP_NONE, thr=0.0, row_mask=None, perq=False, row_ids=None) -> np.ndarray:
    """The library's default order: best score, then lower row, then lower query.  perq: k per query, concatenated in query
    order (each with its query id)."""
    sc, rows, qs = _pairs(S, take, cmp, thr, row_mask, row_ids)
    order = np.lexsort((qs, rows, ordkey(sc, take)))
    if not perq:
        o = order[:max(int(k), 0)]
        return _hits(sc[o], rows[o], qs[o])
    parts = []
    for qi in range(S.shape[0]):
        o = order[qs[order] == qi][:max(int(k), 0)]
        parts.append(_hits(sc[o], rows[o], qs[o]))
    return np.concatenate(parts) if parts else _hits([], [], [])


def query(rows, queries, take, k, cmp=CMP_NONE, thr=0.0, row_mask=None, perq=False, reduce_mode=REDUCE_AVX) -> np.ndarray:
    """VecStore query under Manhattan, canonical order"""
    queries = np.asarray(queries, np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    return select_canonical(scores(rows, queries, "l1", reduce_mode), take, k, cmp, thr, row_mask, perq)


def select_reference(S, take, k, cmp=CMP_NONE, thr=0.0, row_mask=None):
    """What the reference's one TopKCollector keeps (src/vec.rs:222-303 visit order, strict-improvement inserts): the closed
    form of tests/test_tie_rule_model.py on these scores.  Returns hits in the collector's buffer order."""
    nq, n = S.shape
    sc, rows, qs = _pairs(S, take, cmp, thr, row_mask)
    if k <= 0 or sc.size == 0:
        return _hits([], [], [])
    ok = ordkey(sc, take)
    vis = visit_rank(rows, qs, n, nq)
    order = np.lexsort((vis, ok))
    cand = [(int(ok[i]), int(vis[i]), int(rows[i]), int(qs[i])) for i in order[:k + 1]]
    by_visit = np.argsort(vis, kind="stable")[:k]
    fill = {(int(rows[i]), int(qs[i])) for i in by_visit}
    res = collector_result(cand, k, fill)
    score_of = {(int(rows[i]), int(qs[i])): sc[i] for i in order[:k + 1]}
    return _hits([score_of[(r, q)] for _, _, r, q in res], [r for _, _, r, q in res], [q for _, _, r, q in res])


def select_reference_chunked(S, take, k, chunk_size, cmp=CMP_NONE, thr=0.0, chunk_mask=None):
    """The reference's MetaStore (src/meta.rs:678-709, src/meta_compute.rs:153-192): one collector per surviving chunk, each
    visiting ITS rows in blocks of eight from its first row; then concatenate, stable sort by score, truncate to k."""
    nq, n = S.shape
    parts = []
    for c0 in range(0, n, chunk_size):
        c = c0 // chunk_size
        if chunk_mask is not None and not chunk_mask[c]:
            continue
        h = select_reference(S[:, c0:c0 + chunk_size], take, k, cmp, thr)
        h["index"] += c0
        parts.append(h)
    if not parts:
        return _hits([], [], [])
    allh = np.concatenate(parts)
    o = np.argsort(ordkey(allh["score"], take), kind="stable")[:k]
    return allh[o]
