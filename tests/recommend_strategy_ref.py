"""The expectation of the recommend strategies average_vector and sum_scores (ott_query_recommend_strategy, VecStore.recommend(...,
strategy=...)) in NumPy.  Test infrastructure: numpy and the CPU oracle only, no GPU.

sum_chain(): S per row from the pair scores P (recommend_ref.pair_scores over the distinct positives, then the distinct negatives):
S = P[0] itself, then one np.float32 addition per positive slot and one np.float32 subtraction per negative slot, in slot order.
sum_scores(): candidates (mask, not an example, S not NaN, the filter on S), order (ord_of(S, take) descending, then the lower row),
cut at min(k, rows); every side is 1.
average_vector(): per dim the positives' stored values added in slot order in np.float32, one np.float32 division by their number;
with negatives the same over them, and (mp + mp) - mn."""
import numpy as np

import recommend_ref as R
from otters_amd._native import HIT_DTYPE


def slots(positive, negative):
    """distinct positives in first-occurrence order, then the distinct negatives"""
    return list(dict.fromkeys(int(i) for i in positive)), list(dict.fromkeys(int(i) for i in negative))


def sum_chain(P, n_pos):
    """f32[n]: the chain over P's rows, the first n_pos of them positives"""
    P = np.asarray(P, np.float32)
    S = P[0].copy()  # the first score itself, not 0 + P: a -0.0 stays -0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(1, P.shape[0]):
            S = (S + P[e]).astype(np.float32) if e < n_pos else (S - P[e]).astype(np.float32)
    return S


def sum_scores(oracle, rows, inv, positive, negative, metric, take, k, keep=None, cmp=0, thr=0.0, reduce_mode=0, base=0, P=None):
    """(hits, sides).  keep: bool[n] rows that survive every mask (None = all).  P: pair_scores over the slots, when the caller
    shares it among cases."""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    pos_ex, neg_ex = slots(positive, negative)
    if P is None:
        P = R.pair_scores(oracle, rows, inv, pos_ex + neg_ex, metric, reduce_mode)
    S = sum_chain(P, len(pos_ex))
    cand = ~np.isnan(S)
    if keep is not None:
        cand &= np.asarray(keep, bool)
    cand[np.asarray(pos_ex + neg_ex, np.int64)] = False
    cand &= R.cmp_holds(S, cmp, thr)
    o = R.ordinals(S, take)
    r = np.arange(n)[cand]
    r = r[np.lexsort((r, -o[r].astype(np.int64)))][: min(int(k), n)]
    hits = np.zeros(r.size, HIT_DTYPE)
    hits["index"] = r + int(base)
    hits["score"] = R.decode(o[r], take)  # (== S[r], bit for bit: the ordinal is a bijection of the non-NaN bits)
    return hits, np.ones(r.size, np.uint32)


def average_vector(rows, positive, negative=()):
    """f32[dim]"""
    rows = np.asarray(rows, np.float32)
    pos_ex, neg_ex = slots(positive, negative)

    def mean(ex):
        s = rows[ex[0]].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for e in ex[1:]:
                s = (s + rows[e]).astype(np.float32)
            return (s / np.float32(len(ex))).astype(np.float32)  # one correctly rounded division, not a multiply by a reciprocal

    mp = mean(pos_ex)
    if not neg_ex:
        return mp
    with np.errstate(invalid="ignore", over="ignore"):
        return ((mp + mp).astype(np.float32) - mean(neg_ex)).astype(np.float32)


def keep_without(n, positive, negative, keep=None):
    """bool[n]: `keep` (None = all) with the examples cleared — the one more row mask of average_vector"""
    m = np.ones(n, bool) if keep is None else np.asarray(keep, bool).copy()
    m[np.asarray(list(positive) + list(negative), np.int64)] = False
    return m
