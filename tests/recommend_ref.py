"""The expectation of recommend-by-example (ott_query_recommend, VecStore.recommend) in NumPy.  Test
infrastructure: numpy and the CPU oracle only, no GPU.

pair_scores(): P[e][r] for every example e and EVERY row r — mmr_ref.pair_row, example e's stored row as the query, with the
store's inverse norms.
best(): a row's best ordinal over a set of examples, mmr_ref.total_key under the take (~key for Min); a NaN pair score offers
nothing; 0 = none.
recommend(): candidates (mask, not an example, bp != 0, the filter on BP), sides (positive: bn == 0 or bp > bn), order (positive
side by bp descending then the lower row; with fill the negative side by bn ASCENDING then the lower row), cut at min(k, rows)."""
import numpy as np

import mmr_ref as R
from otters_amd._native import HIT_DTYPE

FILL = 1


def pair_scores(oracle, rows, inv, examples, metric, reduce_mode=0):
    """f32[len(examples), n]"""
    rows = np.ascontiguousarray(rows, np.float32)
    inv = np.asarray(inv, np.float32) if inv is not None else np.zeros(rows.shape[0], np.float32)
    return np.stack([R.pair_row(oracle, rows, inv, int(e), metric, reduce_mode) for e in examples]) if len(examples) else np.zeros((0, rows.shape[0]), np.float32)


def ordinals(scores, take):
    """ord_of(score, take) as uint64, 0 for NaN"""
    k = R.total_key(scores)
    o = k if int(take) == 1 else (~k & np.uint64(0xFFFFFFFF))
    return np.where(np.isnan(scores), np.uint64(0), o)


def decode(o, take):
    """score_of(ordinal, take) as f32"""
    o = np.asarray(o, np.uint64)
    k = o if int(take) == 1 else (~o & np.uint64(0xFFFFFFFF))
    b = np.where(k & np.uint64(0x80000000), k & np.uint64(0x7FFFFFFF), ~k & np.uint64(0xFFFFFFFF))
    return b.astype(np.uint32).view(np.float32)


def best(P, take):
    n = P.shape[1]
    return ordinals(P, take).max(axis=0) if P.shape[0] else np.zeros(n, np.uint64)


def cmp_holds(s, cmp, thr):
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        return {0: np.ones(s.shape, bool), 1: s < thr, 2: s > thr, 3: s <= thr, 4: s >= thr, 5: s == thr}[int(cmp)]


def sides(P_pos, P_neg, take, examples, keep=None, cmp=0, thr=0.0):
    """(bp, bn, candidate, positive side) per row"""
    bp, bn = best(P_pos, take), best(P_neg, take)
    n = bp.size
    cand = bp != 0
    if keep is not None:
        cand &= np.asarray(keep, bool)
    cand[np.asarray(examples, np.int64)] = False
    cand &= cmp_holds(decode(bp, take), cmp, thr)
    pos = (bn == 0) | (bp > bn)
    assert n == bn.size
    return bp, bn, cand, pos


def recommend(oracle, rows, inv, positive, negative, metric, take, k, flags=FILL, keep=None, cmp=0, thr=0.0, reduce_mode=0, base=0, P=None):
    """(hits, sides).  keep: bool[n] rows that survive every mask (None = all).  P: pair_scores over positives then negatives
    (distinct, in that order), when the caller shares it among cases."""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    pos_ex = list(dict.fromkeys(int(i) for i in positive))
    neg_ex = list(dict.fromkeys(int(i) for i in negative))
    if P is None:
        P = pair_scores(oracle, rows, inv, pos_ex + neg_ex, metric, reduce_mode)
    bp, bn, cand, pos = sides(P[: len(pos_ex)], P[len(pos_ex):], take, pos_ex + neg_ex, keep, cmp, thr)
    r = np.arange(n)
    first = r[cand & pos]
    first = first[np.lexsort((first, -bp[first].astype(np.int64)))]
    second = r[cand & ~pos] if (int(flags) & FILL) else r[:0]
    second = second[np.lexsort((second, bn[second].astype(np.int64)))]
    k_eff = min(int(k), n)
    order = np.concatenate([first, second])[:k_eff]
    n1 = min(first.size, k_eff)
    hits = np.zeros(order.size, HIT_DTYPE)
    hits["index"] = order + int(base)
    hits["score"][:n1] = decode(bp[order[:n1]], take)
    hits["score"][n1:] = decode(bn[order[n1:]], take)
    side = np.zeros(order.size, np.uint32)
    side[:n1] = 1
    return hits, side


def same(got, exp, where=""):
    """bit equality of indices, order, score bits, query, sides and counts"""
    (gh, gs), (eh, es) = got, exp
    assert gh["index"].tolist() == eh["index"].tolist(), (where, gh["index"].tolist()[:12], eh["index"].tolist()[:12])
    assert np.array_equal(gh["score"].view(np.uint32), eh["score"].view(np.uint32)), where
    assert not gh["query"].any(), where
    assert np.asarray(gs).tolist() == np.asarray(es).tolist(), where
