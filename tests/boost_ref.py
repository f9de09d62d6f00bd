"""The numpy model of score boosting (ott_query_boost) — TEST INFRASTRUCTURE ONLY.

S comes from the oracle: oracle.vec_query with k = rows per query (Manhattan through tests/manhattan_ref.py); a row the oracle drops
(its score is NaN) has S = NaN here.  The formula is restated with explicit np.float32 / np.float64 operations, one IEEE operation
at a time, in the contract's order:

    Sw  = fl(score_weight * S)
    g_j = VALUE:     missing for a NULL row, else (float)((double)x - origin)
          LIN_DECAY: missing for a NULL row, else with t = VALUE's result, u = fl(|t| / scale): +0 if u >= 1 else fl(1 - u)
          MASK:      1 where the mask keeps the row (rows at or beyond its length are kept), else 0
    c_j = fl(weight_j * g_j);  B = c_0, B = fl(B + c_j)
    F   = Sw (no terms) | fl(Sw + B) (SUM) | fl(Sw * fl(1 + B)) (MULT)

then the NaN drop, the filter on F, and the order by (canonical key of F, row) — tests/manhattan_ref.py's selection, which is held
to the oracle's in tests/test_manhattan_cpu.py.

A term is a tuple: ("value", values, nulls or None, weight, origin, missing), ("decay", values, nulls or None, weight, origin,
scale, missing) or ("mask", bool mask, weight).  `values` is a typed numpy array (int32, int64, float32, float64; a DateTime
column is int64)."""
import numpy as np

import manhattan_ref as M

SUM, MULT = 0, 1
F32 = np.float32


def scores(oracle, rows, queries, metric):
    """S[nq, n] f32: the exact path's score of every (query, row) pair; NaN where the oracle drops the row"""
    rows = np.ascontiguousarray(rows, np.float32)
    queries = np.ascontiguousarray(queries, np.float32).reshape(-1, rows.shape[1])
    if int(metric) == 3:
        return M.scores(rows, queries, "l1")
    n = rows.shape[0]
    S = np.full((queries.shape[0], n), np.nan, np.float32)
    for b in range(queries.shape[0]):
        h = oracle.vec_query(rows, queries[b][None], int(metric), 1, n, ties=oracle.TIES_CANONICAL)
        S[b, h["index"].astype(np.int64)] = h["score"]
    return S


def value_g(values, nulls, origin, missing):
    with np.errstate(all="ignore"):
        t = (np.asarray(values).astype(np.float64) - np.float64(origin)).astype(np.float32)  # the subtraction in f64, one rounding
    if nulls is not None:
        t = np.where(np.asarray(nulls, bool), F32(missing), t).astype(np.float32)
    return t


def term_g(term, n):
    """g_j[n] f32"""
    kind = term[0]
    if kind == "mask":
        m = np.asarray(term[1], bool).ravel()
        keep = np.ones(n, bool)
        keep[:min(n, m.size)] = m[:n]
        return np.where(keep, F32(1.0), F32(0.0)).astype(np.float32)
    if kind == "value":
        _, values, nulls, _, origin, missing = term
        return value_g(values, nulls, origin, missing)
    assert kind == "decay", kind
    _, values, nulls, _, origin, scale, missing = term
    t = value_g(values, None, origin, 0.0)
    with np.errstate(all="ignore"):
        u = np.abs(t) / F32(scale)
        g = np.where(u >= F32(1.0), F32(0.0), F32(1.0) - u).astype(np.float32)  # a NaN u fails the comparison: 1 - NaN
    if nulls is not None:
        g = np.where(np.asarray(nulls, bool), F32(missing), g).astype(np.float32)
    return g


def term_weight(term):
    return F32(term[2] if term[0] == "mask" else term[3])


def boost_sum(terms, n, order=None):
    """B[n] f32 in the caller's order (or in `order`, a permutation: the mutation the chain-order case is sharp against)"""
    idx = list(range(len(terms))) if order is None else list(order)
    B = None
    with np.errstate(all="ignore"):
        for j in idx:
            c = term_weight(terms[j]) * term_g(terms[j], n)
            assert c.dtype == np.float32
            B = c if B is None else B + c
    return B


def final(S, terms, combine=SUM, score_weight=1.0, order=None):
    """F[nq, n] f32"""
    S = np.asarray(S, np.float32)
    with np.errstate(all="ignore"):
        Sw = F32(score_weight) * S
        if not terms:
            return Sw
        B = boost_sum(terms, S.shape[-1], order)
        F = Sw + B[None, :] if combine == SUM else Sw * (F32(1.0) + B)[None, :]
    assert F.dtype == np.float32
    return F


def select(F, take, k, cmp=0, thr=0.0, keep=None):
    """[hits of query b]: NaN dropped, the filter on F, ordered by (canonical key of F, row), cut at k; `query` = b"""
    out = []
    for b in range(F.shape[0]):
        h = M.select_canonical(F[b][None], take, k, cmp, thr, keep).copy()
        h["query"] = b
        out.append(h)
    return out


def expected(S, terms, take, k, combine=SUM, score_weight=1.0, cmp=0, thr=0.0, keep=None):
    return select(final(S, terms, combine, score_weight), take, k, cmp, thr, keep)
