"""The expectation of hybrid search in NumPy (ott_query_hybrid, VecStore.hybrid; ott_store_sparse_df, ott_query_sparse_idf; DESIGN.md
3.1t).  THE NORMATIVE STATEMENT: the header comment, ott_hybrid_plan.h and the device code restate it.  Test infrastructure: numpy,
the CPU oracle and the two models underneath (tests/fuse_ref.py, tests/sparse_ref.py), no GPU.

LEGS of a request: its dense legs in the caller's order, then its sparse legs in the caller's order.
A DENSE LEG'S LIST is fuse_ref.leg_lists': ott_query's hits for that vector with k = min(fetch, rows), canonical order.
A SPARSE LEG'S LIST is sparse_ref.query's hits for that sparse query with k = min(fetch, rows) under take Max, its own filter, the same
row mask; with IDF the query's weights are scaled first (below).
CONTRIBUTION, FUSED SCORE, RANKING: fuse_ref's, word for word, except that MINMAX and DBSF normalise a leg under THAT LEG'S take:
the call's take for a dense leg, Max for a sparse leg.

DOCUMENT FREQUENCIES: df[i] = the live rows whose sparse row stores index i (a stored 0.0 counts), n_docs = the live rows.
idf(i) = f32(log(1.0 + (n_docs - df[i] + 0.5) / (df[i] + 0.5))): f64, every operation rounded, the C library's log (math.log), one
rounding to f32.  A query weight becomes f32(weight * idf(index)): one f32 multiplication."""
import math

import numpy as np

import fuse_ref as R
import sparse_ref as SR
from otters_amd._native import HIT_DTYPE

TAKE_MIN, TAKE_MAX = 0, 1


# ---- document frequencies and idf ---------------------------------------------------------------------------------------------------------

def df(indptr, indices, vocab, live=None):
    """(df uint32[vocab], n_docs) over the live rows (live: bool[n] or None = all)"""
    indptr = np.asarray(indptr, np.int64)
    n = indptr.size - 1
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    lens = np.diff(indptr)
    entry_live = np.repeat(live, lens)
    counts = np.bincount(np.asarray(indices, np.int64)[entry_live], minlength=vocab).astype(np.uint32)
    return counts, int(live.sum())


def idf(n_docs, d):
    """f32: the definition, one Python float (f64) operation at a time"""
    n_docs, d = int(n_docs), int(d)
    return np.float32(math.log(1.0 + (float(n_docs - d) + 0.5) / (float(d) + 0.5)))


def idf_queries(queries, counts, n_docs):
    """the queries with every weight times idf(index), one f32 multiplication"""
    out = []
    for q_idx, q_val in queries:
        w = np.asarray(q_val, np.float32)
        f = np.array([idf(n_docs, counts[int(i)]) for i in q_idx], np.float32)
        with np.errstate(all="ignore"):
            s = w * f
        assert s.dtype == np.float32
        out.append((np.asarray(q_idx), s))
    return out


# ---- the legs' lists ----------------------------------------------------------------------------------------------------------------------

def sparse_lists(indptr, indices, values, queries, vocab, fetch, cmp=0, thr=0.0, keep=None, base=0):
    """[(rows u64, scores f32)] — one list per sparse query: sparse_ref's hits under take Max with k = min(fetch, rows)"""
    n = len(indptr) - 1
    if not queries:
        return []
    hits = SR.query(indptr, indices, values, queries, vocab, TAKE_MAX, min(fetch, n), cmp, thr, keep)
    return [(h["index"].astype(np.uint64) + np.uint64(base), h["score"].astype(np.float32)) for h in hits]


# ---- one request, the whole call ------------------------------------------------------------------------------------------------------------

def fuse_request(lists, takes, fusion, k, rrf_k=60.0, weights=None, request=0, leg_order=None):
    """One request: `lists` = [(rows, scores)] per leg in leg order, takes[l] = the take leg l's list is best first under.  Returns its
    fused hits (HIT_DTYPE).  leg_order: a WRONG summation order (the sharpness tests compare with it); a wrong take per leg is a wrong
    `takes`."""
    order = range(len(lists)) if leg_order is None else leg_order
    F = {}
    with np.errstate(all="ignore"):
        for l in order:
            rows, scores = lists[l]
            c = R.contributions(fusion, int(takes[l]) == TAKE_MAX, rrf_k, 1.0 if weights is None else weights[l], scores)
            for row, cc in zip(np.asarray(rows, np.uint64).tolist(), c):
                F[row] = np.float32(F.get(row, np.float32(0.0)) + cc)
    rows = np.array(sorted(F), np.uint64)
    f = np.array([F[int(r)] for r in rows], np.float32)
    keep = ~np.isnan(f)
    rows, f = rows[keep], f[keep]
    o = np.lexsort((rows, -R.total_key(f).astype(np.int64)))[: int(k)]  # F descending (total order), equal F to the lower row
    out = np.zeros(o.size, HIT_DTYPE)
    out["index"], out["score"], out["query"] = rows[o], f[o], request
    return out


def hybrid(dense_lists, sparse_lists_, dense_per_request, sparse_per_request, dense_take, fusion, k, rrf_k=60.0, weights=None, **wrong):
    """The whole call: dense_lists holds the dense legs of request 0, then of request 1, ...; sparse_lists_ the sparse legs likewise;
    weights is flat, in every request's own leg order.  Returns (hits back to back, counts)."""
    hits, counts, di, si, wi = [], [], 0, 0, 0
    for b, (nd, ns) in enumerate(zip(dense_per_request, sparse_per_request)):
        nd, ns = int(nd), int(ns)
        lists = list(dense_lists[di:di + nd]) + list(sparse_lists_[si:si + ns])
        takes = [dense_take] * nd + [TAKE_MAX] * ns
        h = fuse_request(lists, takes, fusion, k, rrf_k, None if weights is None else weights[wi:wi + nd + ns], b, **wrong)
        hits.append(h)
        counts.append(h.size)
        di, si, wi = di + nd, si + ns, wi + nd + ns
    return (np.concatenate(hits) if hits else np.zeros(0, HIT_DTYPE)), counts
