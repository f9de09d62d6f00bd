"""Several hits per group against its alternatives (the table to fill in is in profiles/groups_top/README.md).

One store of synthetic uniform rows made on the GPU per shape, groups of 8 consecutive rows, one query, cosine, take(10), through
the Python API; host clock, end to end per call, median / min / max of --reps calls after --warmup calls.  For m in --ms:

  (a) per_group(m).take(10)      ott_query_groups_top; the kernels' own time is the stats' score_ns (sweeps + select) and merge_ns
  (b) one_per_group().take(10)   ott_query_groups on the same store: what the sweep costs with one slot per group
  (c) workaround                 the default take (every passing pair through the sort path and over PCIe) followed by a NumPy
                                 first-m-per-group and the cut at 10 groups: what a caller did before; checked against (a) first

    python benchmarks/group_size.py [--shapes 1000000x128 10000000x768] [--ms 1 3 8] [--reps 30] [--warmup 5]
                                    [--workaround-reps 3] [--no-workaround]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Metric, VecStore  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def first_m_per_group(hits, gid, m, k):
    """the contract in NumPy: a hit stays iff fewer than m earlier hits have its group; the first k groups, each contiguous"""
    g = gid[hits["index"].astype(np.int64)]
    order = np.argsort(g, kind="stable")
    gs = g[order]
    start = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
    occ = np.empty(g.size, np.int64)
    occ[order] = np.arange(g.size) - np.repeat(start, np.diff(np.r_[start, g.size]))
    hits, g = hits[occ < m], g[occ < m]
    ug, first = np.unique(g, return_index=True)
    winners = ug[np.argsort(first)][:k]
    rank = np.full(int(gid.max()) + 1, -1, np.int64)
    rank[winners] = np.arange(winners.size)
    sel = rank[g] >= 0
    return hits[sel][np.argsort(rank[g[sel]], kind="stable")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["1000000x128", "10000000x768"])
    ap.add_argument("--ms", nargs="*", type=int, default=[1, 3, 8])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workaround-reps", type=int, default=3)
    ap.add_argument("--no-workaround", action="store_true")
    a = ap.parse_args()
    k = 10
    for shape in a.shapes:
        rows, dim = (int(x) for x in shape.split("x"))
        store = VecStore(dim)
        store.reserve(rows)
        store.append_random(rows, 12345)
        gid = np.arange(rows, dtype=np.int64) // 8
        store.set_groups(gid)
        q = np.random.default_rng(0).uniform(-1, 1, dim).astype(np.float32)
        one = timed(lambda: store.query(q, Metric.Cosine).one_per_group().take(k).collect_arrays(), a.reps, a.warmup)
        print(json.dumps({"shape": shape, "n_groups": store.group_count(), "one_per_group": one}), flush=True)
        full = None
        for m in a.ms:
            plan = lambda: store.query(q, Metric.Cosine).per_group(m).take(k).collect_arrays()  # noqa: E731
            row = {"shape": shape, "m": m, "per_group": timed(plan, a.reps, a.warmup)}
            st = store.last_stats
            row["per_group"]["sweep_select_us"] = round(st["score_ns"] / 1e3, 1)
            row["per_group"]["merge_us"] = round(st["merge_ns"] / 1e3, 1)
            row["per_group_over_one"] = round(row["per_group"]["median_ms"] / one["median_ms"], 3)
            got = plan()[0]
            if not a.no_workaround:
                host_ms = []

                def workaround():
                    nonlocal full
                    full = store.query(q, Metric.Cosine).collect_arrays()[0]  # the default take: every row, ranked by Max
                    t0 = time.perf_counter()
                    workaround.top = first_m_per_group(full, gid, m, k)
                    host_ms.append((time.perf_counter() - t0) * 1e3)

                workaround()
                ref = workaround.top
                assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (shape, m)
                row["workaround"] = timed(workaround, a.workaround_reps, 0)
                row["workaround"]["host_part_median_ms"] = round(sorted(host_ms)[len(host_ms) // 2], 3)
                row["speedup_over_workaround"] = round(row["workaround"]["median_ms"] / row["per_group"]["median_ms"], 1)
            print(json.dumps(row), flush=True)
        store.close()


if __name__ == "__main__":
    main()
