"""The expectation of rank fusion in NumPy (ott_query_fuse, VecStore.fuse).  THE NORMATIVE STATEMENT: the header
comment, ott_fuse_plan.h and the device kernel restate it.  Test infrastructure: numpy and the CPU oracle only, no GPU.

A LEG'S LIST is what ott_query returns for that one query vector with k = min(fetch, rows), PER_QUERY: rows and f32 scores, best
first.  leg_lists(): the lists from the oracle in the canonical order (tests/manhattan_ref.py for L1).  Positions are r = 0, 1, ...

contribution of the entry at position r with score s of a leg with weight w (f32), one IEEE operation at a time:
    RRF     c = w / (rrf_k + f32(r + 1))                                   one f32 addition, one f32 division
    MINMAX  best = f64(list[0]), worst = f64(list[n - 1]); span = best - worst (take Max) or worst - best (take Min)
            !(span > 0): nrm = f32(0.5) for the whole list;  else nrm = f32(dist / span), dist = s - worst (Max) or worst - s (Min) in f64
            c = w * nrm                                                    one f32 multiplication
    DBSF    the same with lo = mean - 3 sigma, hi = mean + 3 sigma, worst = lo (Max) or hi (Min), span = hi - lo; no clamp.
            mean = sum64(s) / n, var = sum64((s - mean) * (s - mean)) / n, sigma = sqrt(var), all f64, each operation rounded.
            sum64: partial t (0 <= t < 64) adds the terms at t, t + 64, ... ascending from +0.0; then p[t] += p[t + h] for
            h = 32, 16, 8, 4, 2, 1; the sum is p[0].
fused score of a row: F = f32(+0.0); over the request's legs in ascending order, for every leg whose list holds the row, F = F + c
(one f32 addition each).
ranking: F descending whatever the take is, equal F to the lower row; a NaN F drops the row; min(k, rows left) hits, score = F,
query = the request."""
import numpy as np

import manhattan_ref as M
from otters_amd import Metric
from otters_amd._native import HIT_DTYPE

RRF, DBSF, MINMAX = 0, 1, 2


def leg_lists(oracle, rows, legs, metric, take, fetch, cmp=0, thr=0.0, row_mask=None, reduce_mode=0, inv=None, base=0):
    """[(rows u64, scores f32)] — one list per leg: the hits of the same plan with take(min(fetch, rows)), canonical order"""
    rows = np.ascontiguousarray(rows, np.float32)
    out = []
    for q in np.asarray(legs, np.float32).reshape(-1, rows.shape[1]):
        if int(metric) == int(Metric.Manhattan):
            h = M.select_canonical(M.scores(rows, q.reshape(1, -1), "l1", reduce_mode), take, fetch, cmp, thr, row_mask)
        else:
            h = oracle.vec_query(rows, q.reshape(1, -1), int(metric), take, fetch, cmp, thr, row_mask=row_mask, reduce_mode=reduce_mode,
                                 ties=oracle.TIES_CANONICAL, inv=inv)
        out.append((h["index"].astype(np.uint64) + np.uint64(base), h["score"].astype(np.float32)))
    return out


def sum64(terms):
    """the f64 sum in the contract's one order (64 strided partials, then a tree)"""
    terms = np.asarray(terms, np.float64)
    p = np.zeros(64, np.float64)
    for t in range(64):
        a = np.float64(0.0)
        for x in terms[t::64]:
            a = a + x
        p[t] = a
    h = 32
    while h:
        p[:h] = p[:h] + p[h:2 * h]
        h >>= 1
    return p[0]


def leg_stats(fusion, take_max, scores, mean_of=None):
    """(worst, span) in f64; mean_of: another way to sum (the sharpness tests swap it in)"""
    s = np.asarray(scores, np.float32).astype(np.float64)
    n = s.size
    if n == 0 or fusion == RRF:
        return np.float64(0.0), np.float64(0.0)
    with np.errstate(all="ignore"):
        if fusion == MINMAX:
            best, worst = s[0], s[-1]
            return worst, (best - worst) if take_max else (worst - best)
        total = sum64 if mean_of is None else mean_of
        mean = np.float64(total(s)) / np.float64(n)
        df = s - mean
        var = np.float64(total(df * df)) / np.float64(n)
        sd3 = np.float64(3.0) * np.sqrt(var)
        lo, hi = mean - sd3, mean + sd3
        return (lo if take_max else hi), hi - lo


def contributions(fusion, take_max, rrf_k, w, scores, mean_of=None, rank_from=1):
    """f32[n]: the contribution of every entry of one leg's list"""
    s32 = np.asarray(scores, np.float32)
    n = s32.size
    w = np.float32(w)
    with np.errstate(all="ignore"):
        if fusion == RRF:
            r = (np.arange(n) + rank_from).astype(np.float32)
            c = w / (np.float32(rrf_k) + r)
            assert c.dtype == np.float32
            return c
        worst, span = leg_stats(fusion, take_max, s32, mean_of)
        if not span > 0:
            nrm = np.full(n, 0.5, np.float32)
        else:
            s = s32.astype(np.float64)
            nrm = (((s - worst) if take_max else (worst - s)) / span).astype(np.float32)
        c = w * nrm
        assert c.dtype == np.float32
        return c


def total_key(v):
    """ott_internal.h: total_key — ascending unsigned == ascending total order of the f32 bits"""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def fuse_request(lists, fusion, take, k, rrf_k=60.0, weights=None, request=0, leg_order=None, mean_of=None, rank_from=1):
    """One request: `lists` = [(rows, scores)] per leg.  Returns its fused hits (HIT_DTYPE).  leg_order / mean_of / rank_from: the
    WRONG implementations the sharpness tests compare with (another summation order of the legs, another mean, r in place of r + 1)."""
    take_max = int(take) == 1
    order = range(len(lists)) if leg_order is None else leg_order
    F = {}
    with np.errstate(all="ignore"):
        for l in order:
            rows, scores = lists[l]
            c = contributions(fusion, take_max, rrf_k, 1.0 if weights is None else weights[l], scores, mean_of, rank_from)
            for row, cc in zip(np.asarray(rows, np.uint64).tolist(), c):
                F[row] = np.float32(F.get(row, np.float32(0.0)) + cc)
    rows = np.array(sorted(F), np.uint64)
    f = np.array([F[int(r)] for r in rows], np.float32)
    keep = ~np.isnan(f)
    rows, f = rows[keep], f[keep]
    o = np.lexsort((rows, -total_key(f).astype(np.int64)))[: int(k)]  # F descending (total order), equal F to the lower row
    out = np.zeros(o.size, HIT_DTYPE)
    out["index"], out["score"], out["query"] = rows[o], f[o], request
    return out


def fuse(lists, legs_per_request, fusion, take, k, rrf_k=60.0, weights=None, **wrong):
    """The whole call: `lists` holds the legs of request 0, then of request 1, ...  Returns (hits back to back, counts)."""
    hits, counts, at = [], [], 0
    for b, n in enumerate(legs_per_request):
        h = fuse_request(lists[at:at + n], fusion, take, k, rrf_k, None if weights is None else weights[at:at + n], b, **wrong)
        hits.append(h)
        counts.append(h.size)
        at += n
    return (np.concatenate(hits) if hits else np.zeros(0, HIT_DTYPE)), counts
