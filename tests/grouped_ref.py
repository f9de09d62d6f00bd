"""The expectations of the grouped, per-group, plain and id-list queries in NumPy, shared by the GPU tests.  Test infrastructure: NumPy
and the oracle only, nothing is taken from the library.

Everything starts from ONE full canonical ranking per (store, metric, queries, take): every (row, query) pair that has a score, best
first — better score, lower row, lower query (one oracle call with k = n x nq and TIES_CANONICAL; Manhattan: tests/manhattan_ref.py).
A plain query's hits are the first k pairs of that ranking among the kept rows and the pairs the filter passes (per query in PER_QUERY
mode); an id list keeps the listed rows only; grouped and per-group queries follow the rule in tests/test_gpu_groups_top.py's header."""
import numpy as np

import manhattan_ref as M
from otters_amd import Metric


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), (where, got["query"][:12], ref["query"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def ranking(oracle, rows, q, metric, take):
    """every (row, query) pair that has a score (NaN pairs are dropped), best first in the canonical order"""
    n, nq = rows.shape[0], q.shape[0]
    if metric == Metric.Manhattan:
        return M.select_canonical(M.scores(rows, q, "l1", 0), take, n * nq)
    return oracle.vec_query(rows, q, int(metric), take, n * nq, ties=oracle.TIES_CANONICAL)


class Rankings:
    """the full canonical ranking per (metric, nq, take), made once and never changed"""

    def __init__(self, oracle, rows, q_pool):
        self.args, self.have = (oracle, rows, q_pool), {}

    def get(self, metric, nq, take):
        key = (metric, nq, take)
        if key not in self.have:
            oracle, rows, q_pool = self.args
            self.have[key] = ranking(oracle, rows, q_pool[:nq], metric, take)
            self.have[key].setflags(write=False)
        return self.have[key]


def holds(score, cmp, thr):
    thr = np.float32(thr)
    return {0: np.ones(score.shape, bool), 1: score < thr, 2: score > thr, 3: score <= thr, 4: score >= thr, 5: score == thr}[int(cmp)]


def expected(full, gid, keep, k, nq, m, cmp=0, thr=0.0):
    """(hits, per-query hit counts, group id per hit) by the rule of the module's header"""
    f = full[keep[full["index"].astype(np.int64)]]
    f = f[holds(f["score"], cmp, thr)]
    parts, groups = [], []
    for qi in range(nq):
        fq = f[f["query"] == qi]
        g = gid[fq["index"].astype(np.int64)]
        if g.size == 0:
            parts.append(fq)
            groups.append(g)
            continue
        order = np.argsort(g, kind="stable")  # a group's hits side by side, still in L's order
        gs = g[order]
        start = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
        occ = np.empty(g.size, np.int64)
        occ[order] = np.arange(g.size) - np.repeat(start, np.diff(np.r_[start, g.size]))  # how many earlier hits of L have its group
        fq, g = fq[occ < m], g[occ < m]
        ug, first = np.unique(g, return_index=True)
        winners = ug[np.argsort(first)][:k]  # groups by the position of their first hit
        rank = np.full(int(gid.max()) + 2, -1, np.int64)
        rank[winners] = np.arange(winners.size)
        sel = rank[g] >= 0
        o = np.argsort(rank[g[sel]], kind="stable")
        parts.append(fq[sel][o])
        groups.append(g[sel][o])
    return np.concatenate(parts), [p.size for p in parts], np.concatenate(groups).astype(np.uint32)


def dense(labels):
    return np.unique(labels, return_inverse=True)[1].reshape(-1)


def plain_expected(full, keep, k, nq, perq=False, cmp=0, thr=0.0):
    """(hits, per-query hit counts) of ott_query: the first k pairs of the ranking among the kept rows that pass the filter; perq: the
    first k of every query, in query order.  The counts are those of the hits returned (merged: how many each query contributed)."""
    f = full[np.asarray(keep, bool)[full["index"].astype(np.int64)]]
    f = f[holds(f["score"], cmp, thr)]
    k = max(int(k), 0)
    if not perq:
        f = f[:k]
        return f, np.bincount(f["query"].astype(np.int64), minlength=nq).tolist()
    parts = [f[f["query"] == qi][:k] for qi in range(nq)]
    return np.concatenate(parts), [p.size for p in parts]


def ids_expected(full, keep, ids, k, nq, perq=False, cmp=0, thr=0.0):
    """the same for ott_query_ids: only rows that are kept AND listed (duplicates in the list count once)"""
    listed = np.zeros(np.asarray(keep).size, bool)
    listed[np.asarray(ids).astype(np.int64)] = True
    return plain_expected(full, np.asarray(keep, bool) & listed, k, nq, perq, cmp, thr)
