"""The expectation of late-interaction (MaxSim) search in NumPy (ott_query_maxsim, VecQueryPlan.max_sim).  Test
infrastructure: numpy only, no GPU.

It starts from the FULL canonical ranking of all (row, token) pairs — one oracle call with k = n x nq and TIES_CANONICAL, or
tests/manhattan_ref.py for L1, the way tests/test_gpu_groups.py::ranking makes it (NaN pairs are not in it).  Restricted to the kept
rows, the first occurrence of every group among a token's pairs is that token's `best` for the group IN THE TOTAL ORDER (np.maximum
would not order signed zeros).  The sum is a float32 array add per token, in token order, started from best[0].  Groups that miss a
token, NaN sums and sums the filter rejects are dropped; the rest is sorted by (total-order key of the sum, group id) and cut at k."""
import numpy as np

import manhattan_ref as M
from otters_amd import Metric
from otters_amd._native import HIT_DTYPE


def ord_of(score, take_max) -> np.ndarray:
    """ott_internal.h: ord_of — "larger is better" 32-bit ordinal of an f32 in the total order, for the take type"""
    b = np.asarray(score, np.float32).view(np.uint32).astype(np.uint64)
    key = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    return key if take_max else (~key & np.uint64(0xFFFFFFFF))


def ranking(oracle, rows, q, metric, take):
    """every (row, token) pair that has a score, best first in the canonical order"""
    n, nq = rows.shape[0], q.shape[0]
    if metric == Metric.Manhattan:
        return M.select_canonical(M.scores(rows, q, "l1", 0), take, n * nq)
    return oracle.vec_query(rows, q, int(metric), take, n * nq, ties=oracle.TIES_CANONICAL)


def holds(score, cmp, thr):
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        return {0: np.ones(score.shape, bool), 1: score < thr, 2: score > thr, 3: score <= thr, 4: score >= thr, 5: score == thr}[int(cmp)]


def bests(full, gid, keep, nq, n_groups):
    """best[t][g] and whether it exists: per token the first pair of every group in the ranking restricted to the kept rows"""
    f = full[keep[full["index"].astype(np.int64)]]
    best = np.zeros((nq, n_groups), np.float32)
    have = np.zeros((nq, n_groups), bool)
    for t in range(nq):
        ft = f[f["query"] == t]
        g = gid[ft["index"].astype(np.int64)]
        ug, first = np.unique(g, return_index=True)
        best[t, ug] = ft["score"][first]
        have[t, ug] = True
    return best, have


def sums(best):
    acc = best[0].copy()
    with np.errstate(all="ignore"):
        for t in range(1, best.shape[0]):
            acc = acc + best[t]
    assert acc.dtype == np.float32
    return acc


def expected(full, gid, keep, k, nq, take, cmp=0, thr=0.0, n_groups=None):
    """the hits of ott_query_maxsim: index = dense group id, score = the sum, query = 0"""
    gid = np.asarray(gid).astype(np.int64)
    n_groups = int(gid.max()) + 1 if n_groups is None else n_groups
    best, have = bests(full, gid, np.asarray(keep, bool), nq, n_groups)
    acc = sums(best)
    cand = np.flatnonzero(have.all(axis=0) & ~np.isnan(acc) & holds(acc, cmp, thr))
    key = ord_of(acc[cand], take == 1).astype(np.int64)
    sel = cand[np.lexsort((cand, -key))][:max(int(k), 0)]
    h = np.zeros(sel.size, HIT_DTYPE)
    h["index"], h["score"], h["query"] = sel, acc[sel], 0
    return h
