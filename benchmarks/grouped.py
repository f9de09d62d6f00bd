"""Grouped search against its alternatives (results in profiles/groups/README.md).

One store of synthetic uniform rows made on the GPU, one query, cosine top-10, through the C ABI; host clock, end to end per
call, median / min / max of --reps calls after --warmup calls.  Group layouts: groups of 8 consecutive rows, 8 random rows per
group, and 7 groups over the whole store (the contention case: every row of the store aims at seven slots).

  (a) grouped    ott_query_groups, path EXACT, k = 10; the kernels' own time is the stats' score_ns (sweep + select) + merge_ns
  (b) plain      ott_query, path EXACT, k = 10, on the same store: what the sweep costs without a table
  (c) workaround the default take (k = rows: every passing pair through the sort path) followed by numpy first-per-group on
                 the host and the cut at 10 — what a caller did before; the host part is timed too (--workaround-reps calls)

(b) and (c) are NOT timed on a build of the commit before this feature: they are timed on this one, in the same process and
session as (a).  ott_query's paths are untouched by the feature (a store without groups allocates nothing and launches nothing
more; tests/test_gpu_groups.py holds the plain query's bits).

    python benchmarks/grouped.py [--rows 1000000] [--dim 128] [--reps 30] [--warmup 5] [--workaround-reps 3]
                                 [--layouts consecutive random seven] [--no-workaround]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import _native as N  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workaround-reps", type=int, default=3)
    ap.add_argument("--layouts", nargs="*", default=["consecutive", "random", "seven"], choices=["consecutive", "random", "seven"])
    ap.add_argument("--no-workaround", action="store_true", help="time (a) and (b) only (a kernel trace of the grouped query alone)")
    a = ap.parse_args()
    L = N.lib()
    h = C.c_void_p()
    N.check(L.ott_store_create(a.dim, 0, C.byref(h)))
    N.check(L.ott_store_reserve(h, a.rows))
    N.check(L.ott_store_append_random(h, a.rows, 12345))
    N.check(L.ott_store_sync(h))
    rng = np.random.default_rng(0)
    q = rng.uniform(-1, 1, (1, a.dim)).astype(np.float32)
    k = 10
    out = np.empty(k, dtype=N.HIT_DTYPE)
    big = np.empty(a.rows, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(0)
    st = N.Stats()

    def desc(kk):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, 1, 0, 1, 0, kk, 1
        return d

    def plain():
        d = desc(k)
        N.check(L.ott_query(h, C.byref(d), N.ptr(out), k, C.byref(n_out), None, C.byref(st)))

    def grouped():
        d = desc(k)
        N.check(L.ott_query_groups(h, C.byref(d), N.ptr(out), k, C.byref(n_out), None, C.byref(st)))

    res = {"rows": a.rows, "dim": a.dim, "reps": a.reps, "warmup": a.warmup, "plain_exact_top10": timed(plain, a.reps, a.warmup), "layouts": []}
    res["plain_exact_top10"]["kernel_us"] = round((st.score_ns + st.merge_ns) / 1e3, 1)
    print(json.dumps({"plain_exact_top10": res["plain_exact_top10"]}), flush=True)
    n8 = (a.rows + 7) // 8
    layouts = {"consecutive": ("8 consecutive rows per group", lambda: (np.arange(a.rows) // 8).astype(np.uint32), n8),
               "random": ("8 random rows per group", lambda: rng.permutation(a.rows).astype(np.uint32) // np.uint32(8), n8),
               "seven": ("7 groups", lambda: rng.integers(0, 7, a.rows).astype(np.uint32), 7)}
    for name, make, n_groups in (layouts[x] for x in a.layouts):
        gid = np.ascontiguousarray(make())
        N.check(L.ott_store_set_groups(h, N.ptr(gid), gid.size, n_groups))
        row = {"layout": name, "n_groups": n_groups, "grouped": timed(grouped, a.reps, a.warmup)}
        row["grouped"]["sweep_select_us"] = round(st.score_ns / 1e3, 1)
        row["grouped"]["merge_us"] = round(st.merge_ns / 1e3, 1)
        got = out[: n_out.value].copy()
        row["grouped_over_plain"] = round(row["grouped"]["median_ms"] / res["plain_exact_top10"]["median_ms"], 3)
        if a.no_workaround:
            res["layouts"].append(row)
            print(json.dumps(row), flush=True)
            continue
        host_ms = []

        def workaround():
            d = desc(a.rows)
            N.check(L.ott_query(h, C.byref(d), N.ptr(big), a.rows, C.byref(n_out), None, None))
            t0 = time.perf_counter()
            hits = big[: n_out.value]
            _, first = np.unique(gid[hits["index"].astype(np.int64)], return_index=True)
            workaround.top = hits[np.sort(first)[:k]]
            host_ms.append((time.perf_counter() - t0) * 1e3)

        row["workaround"] = timed(workaround, a.workaround_reps, 1)
        row["workaround"]["host_part_median_ms"] = round(sorted(host_ms[1:])[len(host_ms[1:]) // 2], 3)
        ref = workaround.top
        assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), name
        row["speedup_over_workaround"] = round(row["workaround"]["median_ms"] / row["grouped"]["median_ms"], 1)
        res["layouts"].append(row)
        print(json.dumps(row), flush=True)
    N.check(L.ott_store_clear_groups(h))
    res["plain_exact_top10_after"] = timed(plain, a.reps, a.warmup)
    print(json.dumps(res))
    L.ott_store_destroy(h)


if __name__ == "__main__":
    main()
