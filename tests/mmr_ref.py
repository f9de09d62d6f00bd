"""The expectation of MMR diversity re-ranking in NumPy f32 (ott_query_mmr, VecQueryPlan.mmr).  Test
infrastructure: numpy and the CPU oracle only, no GPU.

candidates(): one query's first-stage list, oracle.vec_query in the canonical order (tests/manhattan_ref.py for L1).
pair_row(): P[s][.] — candidate s's stored row as the query against every candidate's stored row, one oracle call per pair
(oracle.dot / oracle.l2sq / oracle.cosine with the STORE's inverse norms; manhattan_ref.scores for L1).  Only the rows of P that a
pick reads are made.
select(): the greedy loop, one rounded f32 operation at a time:
    g(x) = x (take Max) / -x (take Min);  om = f32(1) - lam
    pick 0 = candidate 0, value lam * g(rel_0);  red = g(P[s_0]) after pick 0
    after a later pick s, x = g(P[s]):  x NaN -> red stays;  red NaN -> x;  else x where x > red
    value = (lam * g(rel)) - (om * red);  next pick: the largest ordinal of the value (total order, a NaN value ranks lowest),
    equal ordinals to the lower position;  min(k, n) picks;  a NaN value is reported as 0x7FC00000.
mmr(): both for one query or, per query, for a batch."""
import numpy as np

import manhattan_ref as M
from otters_amd import Metric
from otters_amd._native import HIT_DTYPE

CANON_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def candidates(oracle, rows, q, metric, take, fetch_k, cmp=0, thr=0.0, row_mask=None, reduce_mode=0, inv=None):
    """the hits of the same plan with take(fetch_k), one query, canonical order"""
    rows = np.ascontiguousarray(rows, np.float32)
    q = np.asarray(q, np.float32).reshape(1, -1)
    if int(metric) == int(Metric.Manhattan):
        return M.select_canonical(M.scores(rows, q, "l1", reduce_mode), take, fetch_k, cmp, thr, row_mask)
    return oracle.vec_query(rows, q, int(metric), take, fetch_k, cmp, thr, row_mask=row_mask, reduce_mode=reduce_mode,
                            ties=oracle.TIES_CANONICAL, inv=inv)


def pair_row(oracle, crow, cinv, s, metric, reduce_mode=0):
    """P[s][c] for every candidate c.  crow: [n, dim] the candidates' stored rows, cinv: [n] their stored inverse norms"""
    n, dim = crow.shape
    if int(metric) == int(Metric.Manhattan):
        return M.scores(crow, crow[s], "l1", reduce_mode)[0]
    L = oracle.lib()
    base, step = crow.ctypes.data, dim * 4
    out = np.empty(n, np.float32)
    a = base + s * step
    if int(metric) == int(Metric.Cosine):
        ia = float(cinv[s])
        for c in range(n):
            out[c] = L.otto_cosine(a, base + c * step, dim, ia, float(cinv[c]), reduce_mode)  # == oracle.cosine(row_s, row_c, inv_s, inv_c)
    elif int(metric) == int(Metric.Euclidean):
        for c in range(n):
            out[c] = L.otto_l2sq(a, base + c * step, dim, reduce_mode)                       # == oracle.l2sq(row_s, row_c)
    else:
        for c in range(n):
            out[c] = L.otto_dot(a, base + c * step, dim, reduce_mode)                        # == oracle.dot(row_s, row_c)
    return out


def total_key(v):
    """ott_internal.h: total_key — ascending unsigned == ascending total order of the f32 bits"""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def value_ord(v):
    """the ordinal a pick is chosen by: ord_of(value, take Max), and 0 for a NaN value"""
    return np.where(np.isnan(v), np.uint64(0), total_key(v))


def greedy(rel, pair_of, k, lam, take):
    """The selection over n candidates with relevances `rel` (f32[n]); pair_of(s) -> f32[n] = P[s].  Returns (positions, values)."""
    rel = np.asarray(rel, np.float32)
    n = rel.size
    rounds = min(int(k), n)
    lam = np.float32(lam)
    om = np.float32(1.0) - lam
    sign = np.float32(1.0) if int(take) == 1 else np.float32(-1.0)
    picks, values = [], []
    if rounds == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    with np.errstate(all="ignore"):
        lr = lam * (rel if int(take) == 1 else -rel)
        assert lr.dtype == np.float32
        picks.append(0)
        values.append(lr[0])
        open_ = np.ones(n, bool)
        open_[0] = False
        red = None
        for r in range(1, rounds):
            pv = np.asarray(pair_of(picks[-1]), np.float32)
            x = pv if sign > 0 else -pv
            if r == 1:
                red = x.copy()
            else:
                red = np.where(np.isnan(x), red, np.where(np.isnan(red), x, np.where(x > red, x, red)))
            t = om * red
            value = lr - t
            assert t.dtype == np.float32 and value.dtype == np.float32
            o = value_ord(value).astype(np.int64)
            o[~open_] = -1
            best = int(np.flatnonzero(o == o.max())[0])  # equal ordinals: the lower position
            picks.append(best)
            values.append(value[best])
            open_[best] = False
    vals = np.array(values, np.float32)
    vals[np.isnan(vals)] = CANON_NAN
    return np.array(picks, np.int64), vals


def select(oracle, rows, inv, cand, metric, take, k, lam, reduce_mode=0, base=0):
    """MMR over ONE query's first-stage list `cand` (HIT_DTYPE, best first).  rows / inv: the store's rows and stored inverse
    norms; base: the store's base offset (a hit's index minus it is the row).  Returns (hits in pick order, values)."""
    idx = cand["index"].astype(np.int64) - int(base)
    crow = np.ascontiguousarray(np.asarray(rows, np.float32)[idx])
    cinv = np.asarray(inv, np.float32)[idx] if inv is not None else np.zeros(idx.size, np.float32)
    picks, vals = greedy(cand["score"], lambda s: pair_row(oracle, crow, cinv, s, metric, reduce_mode), k, lam, take)
    return cand[picks], vals


def mmr(oracle, rows, queries, metric, take, k, fetch_k, lam, cmp=0, thr=0.0, row_mask=None, reduce_mode=0, inv=None):
    """The whole call for one query or a per_query() batch: (hits, per-query counts, values)."""
    rows = np.ascontiguousarray(rows, np.float32)
    queries = np.asarray(queries, np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    if inv is None:
        inv = oracle.inv_norms(rows) if rows.shape[0] else np.zeros(0, np.float32)
    hits, counts, vals = [], [], []
    for qi in range(queries.shape[0]):
        cand = candidates(oracle, rows, queries[qi], metric, take, fetch_k, cmp, thr, row_mask, reduce_mode, inv)
        h, v = select(oracle, rows, inv, cand, metric, take, k, lam, reduce_mode)
        h = h.copy()
        h["query"] = qi
        hits.append(h)
        counts.append(int(h.size))
        vals.append(v)
    return (np.concatenate(hits) if hits else np.zeros(0, HIT_DTYPE)), counts, (np.concatenate(vals) if vals else np.zeros(0, np.float32))


def same(got_hits, got_vals, exp_hits, exp_vals):
    """bit equality of indices, order, relevance bits and value bits"""
    assert got_hits["index"].tolist() == exp_hits["index"].tolist(), (got_hits["index"].tolist(), exp_hits["index"].tolist())
    assert np.array_equal(got_hits["score"].view(np.uint32), exp_hits["score"].view(np.uint32))
    assert got_hits["query"].tolist() == exp_hits["query"].tolist()
    gv, ev = np.asarray(got_vals, np.float32).view(np.uint32), np.asarray(exp_vals, np.float32).view(np.uint32)
    assert np.array_equal(gv, ev), (np.flatnonzero(gv != ev)[:8], gv[gv != ev][:8], ev[gv != ev][:8])
