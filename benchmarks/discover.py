"""Discovery and context search against recommend's sweep at the same number of slots and against doing it by hand (DESIGN.md
3.1l; results in profiles/discover/README.md).

A store of 10M x 768 rows made on the device, cosine, take 10, (pairs, target) in {(1, yes), (2, yes), (8, yes), (8, no),
(32, yes)}.  Per call and end to end on the host clock, median of --reps calls after --warmup, with the kernels' own time from the
call's stats (score_ms: the gather, the sweeps and the kernels up to the top-k's select; merge_ms: the top-k's merge):

  discover   (a) store.discover(context, target).take(10): ott_query_discover;
  recommend  (b) ott_query_recommend with as many example slots (2 * pairs + 1 with a target; 64 at most): the same streaming
             sweep at the same number of passes with another epilogue on the same 8-byte state, a keys kernel and the same top-k:
             compare the time PER PASS;
  by hand    (c) what a caller does without it: the examples' rows read back, ott_store_score_rows over every row once per distinct
             example and for the target (rows x 4 bytes down each), the wins, the loss and the rank in numpy.

    python benchmarks/discover.py [--rows 10000000] [--dim 768] [--reps 5] [--warmup 1] [--no-hand]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Metric, VecStore  # noqa: E402

CASES = [(1, True), (2, True), (8, True), (8, False), (32, True)]
RECOMMEND_MAX = 64


def timed(fn, reps, warmup, stats_of):
    for _ in range(warmup):
        fn()
    ts, score, merge, total = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        st = stats_of()
        score.append(st["score_ns"] / 1e6)
        merge.append(st["merge_ns"] / 1e6)
        total.append(st["total_ns"] / 1e6)
    ts.sort()
    passes = int(stats_of()["passes"])
    return {"ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "score_ms": round(float(np.median(score)), 3),
            "merge_ms": round(float(np.median(merge)), 3), "call_ms": round(float(np.median(total)), 3), "passes": passes,
            "score_ms_per_pass": round(float(np.median(score)) / passes, 3)}


def by_hand(store, ctx, target, ids, k):
    """the do-it-by-hand route for take Max: (rows, wins) of the top k"""
    n = ids.size
    have = {}
    for e in {e for pair in ctx for e in pair}:
        have[e] = store.score_rows(store.rows(e, 1), Metric.Cosine, ids)[0]
    wins = np.zeros(n, np.int32)
    loss = np.zeros(n, np.float32)
    for p, g in ctx:
        d = have[p] - have[g]
        wins += d > 0
        loss += np.minimum(d, np.float32(0))
    score = store.score_rows(target[None, :], Metric.Cosine, ids)[0] if target is not None else loss
    key = wins.astype(np.float64) * 4.0 + score if target is not None else score.astype(np.float64)  # (cosines lie in [-1, 1])
    key[np.asarray(sorted(have), np.int64)] = -np.inf
    top = np.argpartition(-key, k)[:k]
    top = top[np.argsort(-key[top], kind="stable")]
    return top, wins[top]


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
    rng = np.random.default_rng(3)
    ids = np.arange(n, dtype=np.uint64)
    target = rng.uniform(-1, 1, a.dim).astype(np.float32)
    for n_pairs, has_target in CASES:
        ex = rng.choice(n, 2 * n_pairs, replace=False).tolist()
        ctx = list(zip(ex[0::2], ex[1::2]))
        tgt = target if has_target else None
        row = {"rows": n, "dim": a.dim, "k": k, "pairs": n_pairs, "target": has_target, "slots": 2 * n_pairs + has_target}
        disc = lambda: store.discover(ctx, target=tgt, metric=Metric.Cosine).take(k).collect_arrays()  # noqa: E731
        hits, wins = disc()
        assert hits.size == k and not np.isin(hits["index"], ex).any()
        assert not has_target or (np.diff(wins.astype(np.int64)) <= 0).all()
        row["discover"] = timed(disc, a.reps, a.warmup, lambda: store.last_stats)
        row["wins_of_hits"] = wins.tolist()
        slots = min(2 * n_pairs + has_target, RECOMMEND_MAX)
        pool = rng.choice(n, slots, replace=False).tolist()
        rec = lambda: store.recommend(pool[: (slots + 1) // 2], pool[(slots + 1) // 2:], Metric.Cosine).take(k).collect_arrays()  # noqa: E731
        row["recommend"] = dict(timed(rec, a.reps, a.warmup, lambda: store.last_stats), slots=slots)
        row["sweep_per_pass_vs_recommend"] = round(row["discover"]["score_ms_per_pass"] / row["recommend"]["score_ms_per_pass"], 4)
        if not a.no_hand:
            t0 = time.perf_counter()
            top, w = by_hand(store, ctx, tgt, ids, k)
            row["by_hand_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            # (the host's sums are numpy's, not the library's: a last bit may differ, the rows should not)
            row["by_hand_same_rows"] = sorted(top.tolist()) == sorted(hits["index"].tolist())
        print(json.dumps(row), flush=True)
    store.close()


if __name__ == "__main__":
    main()
