"""The three recommend strategies against each other and against their yardsticks (results in
profiles/recommend_strategies/README.md).

A store of 1M x 768 rows made on the device, cosine, take 10, (positives, negatives) in {(1, 0), (4, 0), (16, 16)}.  Per call and
end to end on the host clock, median of --reps calls after --warmup, with the kernels' own time from the call's stats:

  best_score      store.recommend(positive, negative).take(10): ott_query_recommend, timed TWICE in the same run (before and after
                  the others) — the spread of its own timings is the margin sum_scores is held to;
  sum_scores      strategy=SumScores: the same sweep in the same passes over the same bytes, a running sum in the 8-byte state;
  average_vector  strategy=AverageVector: the vector built on the device, one copy of dim floats down, one wait, then ott_query;
  plain query     store.query(q).with_row_mask(every row but the examples).take(10) with the same vector made on the host: what
                  average_vector adds to it is the build kernel, the copy and the wait.

    python benchmarks/recommend_strategies.py [--rows 1000000] [--dim 768] [--reps 9] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Metric, RecommendStrategy, VecStore  # noqa: E402

CASES = [(1, 0), (4, 0), (16, 16)]


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


def average_vector(store, pos, neg):
    """the library's vector, step by step in f32 (include/otters_hip.h)"""
    def mean(ex):
        s = store.rows(ex[0], 1)[0]
        for e in ex[1:]:
            s = (s + store.rows(e, 1)[0]).astype(np.float32)
        return (s / np.float32(len(ex))).astype(np.float32)
    mp = mean(pos)
    return mp if not neg else ((mp + mp).astype(np.float32) - mean(neg)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    n, k = a.rows, 10
    store = VecStore(a.dim)
    store.reserve(n)
    store.append_random(n, 20261020)
    rng = np.random.default_rng(3)
    stats = lambda: store.last_stats  # noqa: E731
    for n_pos, n_neg in CASES:
        ex = rng.choice(n, n_pos + n_neg, replace=False).tolist()
        pos, neg = ex[:n_pos], ex[n_pos:]
        row = {"rows": n, "dim": a.dim, "k": k, "positives": n_pos, "negatives": n_neg}
        rec = lambda s: (lambda: store.recommend(pos, neg, Metric.Cosine, s).take(k).collect_arrays())  # noqa: E731
        best, summed, avg = rec(RecommendStrategy.BestScore), rec(RecommendStrategy.SumScores), rec(RecommendStrategy.AverageVector)
        q = average_vector(store, pos, neg)
        mask = np.ones(n, bool)
        mask[ex] = False
        plain = lambda: store.query(q, Metric.Cosine).with_row_mask(mask).take(k).collect_arrays()  # noqa: E731
        for fn in (best, summed, avg):
            hits, sides = fn()
            assert hits.size == k and sides.all() and not np.isin(hits["index"], ex).any()
        assert avg()[0].tobytes() == plain()[0].tobytes()
        row["best_score"] = timed(best, a.reps, a.warmup, stats)
        row["sum_scores"] = timed(summed, a.reps, a.warmup, stats)
        row["average_vector"] = timed(avg, a.reps, a.warmup, stats)
        row["plain_query"] = timed(plain, a.reps, a.warmup, stats)
        row["best_score_again"] = timed(best, a.reps, a.warmup, stats)
        print(json.dumps(row), flush=True)
    store.close()


if __name__ == "__main__":
    main()
