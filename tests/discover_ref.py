"""The expectation of discovery and context search (ott_query_discover, VecStore.discover) in NumPy.  Test
infrastructure: numpy and the CPU oracle only, no GPU.

pair_scores(): P[e][r] for every listed example e and EVERY row r — mmr_ref.pair_row, example e's stored row as the query, with
the store's inverse norms.  The examples are the slots: pair i's positive at 2i, its negative at 2i + 1, nothing deduplicated.
target_scores(): a vector target's score of every row from the oracle's query (NaN where the oracle drops the pair), as the
plain-query tests take them; a target ROW's scores are a pair_row.
fold(): wins (ordinal comparisons under the take), the loss (f32, one subtraction and one addition per pair, in pair order, from
+0.0) and whether a pair score is NaN.
discover(): candidates, both orders and the cut."""
import numpy as np

import manhattan_ref as M
import mmr_ref as R
import recommend_ref as RR
from otters_amd import Metric
from otters_amd._native import HIT_DTYPE

ordinals = RR.ordinals    # ord_of(score, take) as uint64, 0 for NaN
cmp_holds = RR.cmp_holds


def pair_scores(oracle, rows, inv, context, metric, reduce_mode=0):
    """f32[2 * len(context), n]: slot 2i is pair i's positive, 2i + 1 its negative.  A row that fills several slots is scored once."""
    rows = np.ascontiguousarray(rows, np.float32)
    inv = np.asarray(inv, np.float32)
    have = {}
    out = []
    for p, g in context:
        for e in (int(p), int(g)):
            if e not in have:
                have[e] = R.pair_row(oracle, rows, inv, e, metric, reduce_mode)
            out.append(have[e])
    return np.stack(out)


def target_scores(oracle, rows, inv, target, metric, reduce_mode=0):
    """f32[n]: the exact path's score of the vector `target` against every row, NaN where there is none"""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    q = np.asarray(target, np.float32).reshape(1, -1)
    if int(metric) == int(Metric.Manhattan):
        return M.scores(rows, q, "l1", reduce_mode)[0]
    h = oracle.vec_query(rows, q, int(metric), 1, n, reduce_mode=reduce_mode, ties=oracle.TIES_CANONICAL, inv=inv)
    T = np.full(n, np.nan, np.float32)
    T[h["index"].astype(np.int64)] = h["score"]
    return T


def fold(P, take):
    """(wins int64[n], loss f32[n], has_nan bool[n], terms f32[n_pairs, n]) from the slots' scores"""
    n_pairs, n = P.shape[0] // 2, P.shape[1]
    wins = np.zeros(n, np.int64)
    loss = np.zeros(n, np.float32)  # +0.0f
    has_nan = np.isnan(P).any(axis=0)
    terms = np.zeros((n_pairs, n), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n_pairs):
            sp, sn = P[2 * i], P[2 * i + 1]
            wins += ordinals(sp, take) > ordinals(sn, take)
            d = (sp - sn) if int(take) == 1 else (sn - sp)  # one f32 subtraction
            t = np.where(d < 0, d, np.float32(0.0)).astype(np.float32)  # a NaN d gives 0
            terms[i] = t
            loss = (loss + t).astype(np.float32)  # one f32 addition
    return wins, loss, has_nan, terms


def discover(P, take, k, T=None, examples=(), min_wins=0, keep=None, cmp=0, thr=0.0, base=0):
    """(hits, wins of the hits).  P: pair_scores; T: the target's scores (None: context search); examples: every row that is an
    example or the target row; keep: bool[n] rows that survive every mask (None = all)."""
    n = P.shape[1]
    wins, loss, has_nan, _ = fold(P, take)
    cand = ~has_nan & (wins >= int(min_wins))
    if keep is not None:
        cand &= np.asarray(keep, bool)
    cand[np.asarray(list(examples), np.int64)] = False
    score = loss if T is None else np.asarray(T, np.float32)
    if T is not None:
        cand &= ~np.isnan(score)
    cand &= cmp_holds(score, cmp, thr)
    r = np.arange(n)[cand]
    if T is None:
        o = ordinals(score[r], 1).astype(np.int64)  # take Max's ordinal of the loss, whatever the take
        order = r[np.lexsort((r, -o))]
    else:
        o = ordinals(score[r], take).astype(np.int64)
        order = r[np.lexsort((r, -o, -wins[r]))]
    order = order[: min(int(k), n)]
    hits = np.zeros(order.size, HIT_DTYPE)
    hits["index"] = order + int(base)
    hits["score"] = score[order]
    return hits, wins[order].astype(np.uint32)


def same(got, exp, where=""):
    """bit equality of indices, order, score bits, query, wins and counts"""
    (gh, gw), (eh, ew) = got, exp
    assert gh["index"].tolist() == eh["index"].tolist(), (where, gh["index"].tolist()[:12], eh["index"].tolist()[:12])
    assert np.array_equal(gh["score"].view(np.uint32), eh["score"].view(np.uint32)), where
    assert not gh["query"].any(), where
    assert np.asarray(gw).tolist() == np.asarray(ew).tolist(), where
