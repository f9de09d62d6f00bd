"""Recommend by example rows against the same sweep as late interaction and against doing it by hand (results in
profiles/recommend/README.md).

A store of 10M x 768 rows made on the device, cosine, take 10, (positives, negatives) in {(1, 0), (4, 0), (8, 8), (40, 24)}.  Per
call and end to end on the host clock, median of --reps calls after --warmup, with the kernels' own time from the call's stats:

  recommend  (a) store.recommend(positive, negative).take(10): ott_query_recommend;
  maxsim     (b) ott_query_maxsim on the same store with group id = row and the examples' rows as the tokens: the same streaming
             sweep at the same number of passes, with a 4-byte atomic maximum per (row, token) in the place of the 8-byte state,
             a reduce kernel in the place of the keys kernel, and the same top-k.  Its table holds every token's maxima at once and
             may take 2 GiB: with 10M groups that is 53 tokens, so the 64 examples of the last case are timed with 48 tokens (12
             passes against 16): compare the time PER PASS;
  by hand    (c) what a caller does without it: the examples' rows read back, ott_store_score_rows over every row once per example
             (rows x 4 bytes down per example), the two maxima, the sides and the top 10 in numpy.

    python benchmarks/recommend.py [--rows 10000000] [--dim 768] [--reps 5] [--warmup 1] [--no-hand]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Metric, VecStore  # noqa: E402

CASES = [(1, 0), (4, 0), (8, 8), (40, 24)]
MAXSIM_TOKENS_MAX = 48


def timed(fn, reps, warmup, stats_of):
    for _ in range(warmup):
        fn()
    ts, score, merge = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        st = stats_of()
        score.append(st["score_ns"] / 1e6)
        merge.append(st["merge_ns"] / 1e6)
    ts.sort()
    return {"ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "score_ms": round(float(np.median(score)), 3),
            "merge_ms": round(float(np.median(merge)), 3), "passes": int(stats_of()["passes"])}


def by_hand(store, pos, neg, ids, k):
    """the do-it-by-hand route for take Max; returns the top-k rows of the positive side (enough to time it)"""
    n = ids.size
    bp = np.full(n, -np.inf, np.float32)
    bn = np.full(n, -np.inf, np.float32)
    for e in pos:
        np.maximum(bp, store.score_rows(store.rows(e, 1), Metric.Cosine, ids)[0], out=bp)
    for e in neg:
        np.maximum(bn, store.score_rows(store.rows(e, 1), Metric.Cosine, ids)[0], out=bn)
    bp[np.asarray(pos + neg, np.int64)] = -np.inf
    bp[bp <= bn] = -np.inf
    top = np.argpartition(-bp, k)[:k]
    return top[np.argsort(-bp[top], kind="stable")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-hand", action="store_true", help="skip (c)")
    a = ap.parse_args()
    n, k = a.rows, 10
    store = VecStore(a.dim)
    store.reserve(n)
    store.append_random(n, 20261020)
    store.set_groups(np.arange(n, dtype=np.uint32))  # (b): one group per row
    rng = np.random.default_rng(3)
    ids = np.arange(n, dtype=np.uint64)
    for n_pos, n_neg in CASES:
        ex = rng.choice(n, n_pos + n_neg, replace=False).tolist()
        pos, neg = ex[:n_pos], ex[n_pos:]
        row = {"rows": n, "dim": a.dim, "k": k, "positives": n_pos, "negatives": n_neg}
        rec = lambda: store.recommend(pos, neg, Metric.Cosine).take(k).collect_arrays()  # noqa: E731
        hits, sides = rec()
        assert hits.size == k and sides.all() and not np.isin(hits["index"], ex).any()
        row["recommend"] = timed(rec, a.reps, a.warmup, lambda: store.last_stats)
        tokens = np.concatenate([store.rows(e, 1) for e in ex[:MAXSIM_TOKENS_MAX]])
        ms = lambda: store.query(tokens, Metric.Cosine).max_sim().take(k).collect_arrays()  # noqa: E731
        row["maxsim"] = dict(timed(ms, a.reps, a.warmup, lambda: store.last_stats), tokens=int(tokens.shape[0]))
        for name in ("recommend", "maxsim"):
            row[name]["score_ms_per_pass"] = round(row[name]["score_ms"] / row[name]["passes"], 3)
        if not a.no_hand:
            t0 = time.perf_counter()
            top = by_hand(store, pos, neg, ids, k)
            row["by_hand_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            # (the host's query norm is another quantity than the stored one: a last bit may differ, the rows should not)
            row["by_hand_same_rows"] = sorted(top.tolist()) == sorted(hits["index"].tolist())
        print(json.dumps(row), flush=True)
    store.close()


if __name__ == "__main__":
    main()
