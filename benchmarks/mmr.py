"""MMR diversity re-ranking against doing it on the host (results in profiles/mmr/README.md).

Stores of 10k x 768 and 1M x 768 (uniform rows made on the host, so that the caller owns a copy as a caller does), cosine, one
query, k = 10, fetch_k in {50, 200, 1024}.  Per call and end to end on the host clock, median of --reps calls after --warmup:

  take    (a) store.query(q).take(fetch_k): the first stage alone;
  mmr     (b) store.query(q).take(k).mmr(0.5, fetch_k): ott_query_mmr;
  host    (c) what a caller does without it: take(fetch_k), score_rows with the candidates' own rows uploaded again as queries
          (fetch_k x dim floats up, fetch_k^2 scores down), then the greedy loop in numpy.

(b) - (a) is the price of the feature, (c) what a user pays without it.  kernels_us: the hipEvent time of the pair and the greedy
kernel together, the difference of the two calls' merge_ns (each kernel's own time comes from a kernel trace of this script).  (b)
and (c) are checked to pick the same rows before anything is timed.

    python benchmarks/mmr.py [--rows 10000 1000000] [--dim 768] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Metric, VecStore  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)


def host_greedy(rel, P, k, lam):
    """the selection of DESIGN.md 3.1j for take Max in numpy f32 (finite scores: the plain maximum)"""
    lam = np.float32(lam)
    om = np.float32(1.0) - lam
    lr = lam * rel
    picks = [0]
    open_ = np.ones(rel.size, bool)
    open_[0] = False
    red = P[0].copy()
    for _ in range(1, min(k, rel.size)):
        value = lr - om * red
        value[~open_] = -np.inf
        best = int(np.argmax(value))  # the first of equal values: the lower position
        picks.append(best)
        open_[best] = False
        red = np.maximum(red, P[best])
    return picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[10_000, 1_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fetch", type=int, nargs="*", default=[50, 200, 1024])
    ap.add_argument("--no-host", action="store_true", help="skip (c): a kernel trace wants the library's kernels only")
    a = ap.parse_args()
    k, lam = 10, 0.5
    for n in a.rows:
        rng = np.random.default_rng(n)
        host = np.empty((n, a.dim), np.float32)
        store = VecStore(a.dim)
        store.reserve(n)
        for r0 in range(0, n, 100_000):
            blk = rng.random((min(100_000, n - r0), a.dim), dtype=np.float32) * np.float32(2) - np.float32(1)
            host[r0:r0 + blk.shape[0]] = blk
            store.add_vectors(blk)
        q = rng.random(a.dim, dtype=np.float32) * np.float32(2) - np.float32(1)
        for fetch_k in a.fetch:
            take = lambda: store.query(q, Metric.Cosine).take(fetch_k).collect_arrays()  # noqa: E731
            mmr = lambda: store.query(q, Metric.Cosine).take(k).mmr(lam, fetch_k).collect_mmr()  # noqa: E731

            def host_pipeline():
                hits, _ = take()
                idx = hits["index"].astype(np.int64)
                P = store.score_rows(host[idx], Metric.Cosine, idx)
                return hits[host_greedy(hits["score"], P, k, lam)]

            row = {"rows": n, "dim": a.dim, "k": k, "fetch_k": fetch_k}
            if not a.no_host:
                assert mmr()[0]["index"].tolist() == host_pipeline()["index"].tolist(), (n, fetch_k)
            row["take_ms"] = median_ms(take, a.reps, a.warmup)
            t_merge = store.last_stats["merge_ns"]
            row["mmr_ms"] = median_ms(mmr, a.reps, a.warmup)
            row["kernels_us"] = round((store.last_stats["merge_ns"] - t_merge) / 1e3, 1)
            if not a.no_host:
                row["host_ms"] = median_ms(host_pipeline, a.reps, a.warmup)
            print(json.dumps(row), flush=True)
        store.close()
        del host


if __name__ == "__main__":
    main()
