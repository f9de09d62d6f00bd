"""MaxSim re-ranking over a listed set of documents against the routes a caller has without the gather (results in
profiles/maxsim_rerank/README.md).

benchmarks/maxsim.py's store: synthetic uniform rows made on the GPU (ColBERT-sized token vectors) in documents of --per-group rows,
one query of --nq tokens, cosine, take(10), through the C ABI; host clock, end to end per call.  Two layouts of the SAME rows:
"contiguous" (a document's rows were appended together: gid = row // per_group) and "shuffled" (the same group sizes, ids permuted
over the rows).  Lists of --lists random documents.  Three timed rows per (layout, list):

  (a) gather     ott_query_maxsim_groups with option group_gather = 1: the listed groups' rows through the group-to-rows index;
                 the kernels' own time is the stats' score_ns (gather + reduce + select) and merge_ns
  (b) mask       ott_query_maxsim_groups with group_gather = 0: the list becomes row-mask words on the device, then the sweep
  (c) today      what a caller did before this call, timed whole: the row mask built from the list on the host (one lookup per row),
                 packed, and ott_query_maxsim with it

All three are checked for equal hits (group ids and score bits) before anything is timed.  The first gather query of a layout also
builds the index: that one call is timed on its own ("index_build_ms", a one-off per set_groups).  Medians with min / max over
--reps calls after --warmup calls.

    python benchmarks/maxsim_rerank.py [--rows 2000000] [--dim 128] [--per-group 20] [--nq 32] [--lists 100,1000,10000,50000]
                                       [--reps 20] [--warmup 3]
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
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--per-group", type=int, default=20)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--lists", type=str, default="100,1000,10000,50000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    L = N.lib()
    h = C.c_void_p()
    N.check(L.ott_store_create(a.dim, 0, C.byref(h)))
    N.check(L.ott_store_reserve(h, a.rows))
    N.check(L.ott_store_append_random(h, a.rows, 12345))
    N.check(L.ott_store_sync(h))
    rng = np.random.default_rng(0)
    q = np.ascontiguousarray(rng.uniform(-1, 1, (a.nq, a.dim)).astype(np.float32))
    k = 10
    n_groups = (a.rows + a.per_group - 1) // a.per_group
    sizes = [min(int(x), n_groups) for x in a.lists.split(",")]
    out = np.empty(k, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(0)
    st = N.Stats()

    def desc():
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, a.nq, 0, 1, 0, k, 1
        return d

    res = {"rows": a.rows, "dim": a.dim, "per_group": a.per_group, "n_groups": n_groups, "nq": a.nq, "reps": a.reps, "warmup": a.warmup, "results": []}
    contiguous = (np.arange(a.rows) // a.per_group).astype(np.uint32)
    for name, gid in (("contiguous", contiguous), ("shuffled", contiguous[rng.permutation(a.rows)])):
        gid = np.ascontiguousarray(gid)
        N.check(L.ott_store_set_groups(h, N.ptr(gid), gid.size, n_groups))
        first = True
        for n_listed in sizes:
            listed = np.ascontiguousarray(rng.choice(n_groups, n_listed, replace=False).astype(np.uint32))

            def listed_call():
                d = desc()
                N.check(L.ott_query_maxsim_groups(h, C.byref(d), N.ptr(listed), listed.size, N.ptr(out), k, C.byref(n_out), C.byref(st)))

            def today():
                in_list = np.zeros(n_groups, bool)
                in_list[listed] = True
                words = N.pack_bits(in_list[gid])
                d = desc()
                d.row_mask, d.row_mask_bits = words.ctypes.data, a.rows
                N.check(L.ott_query_maxsim(h, C.byref(d), N.ptr(out), k, C.byref(n_out), C.byref(st)))

            row = {"layout": name, "listed_groups": n_listed}
            N.check(L.ott_store_set_option(h, b"group_gather", 1))
            if first:  # this call builds the index
                t0 = time.perf_counter()
                listed_call()
                row["index_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                first = False
            listed_call()  # equal results first, then the clock
            got = out[: n_out.value].copy()
            row["listed_rows"] = int(st.vectors_compared // a.nq)
            N.check(L.ott_store_set_option(h, b"group_gather", 0))
            listed_call()
            assert np.array_equal(out[: n_out.value], got), (name, n_listed, "mask route")
            today()
            assert np.array_equal(out[: n_out.value], got), (name, n_listed, "today's route")
            N.check(L.ott_store_set_option(h, b"group_gather", 1))
            row["gather"] = timed(listed_call, a.reps, a.warmup)
            row["gather"].update(score_us=round(st.score_ns / 1e3, 1), merge_us=round(st.merge_ns / 1e3, 1), passes=int(st.passes))
            N.check(L.ott_store_set_option(h, b"group_gather", 0))
            row["mask"] = timed(listed_call, a.reps, a.warmup)
            row["mask"].update(score_us=round(st.score_ns / 1e3, 1), merge_us=round(st.merge_ns / 1e3, 1), passes=int(st.passes))
            row["today"] = timed(today, max(a.reps // 2, 3), 1)
            row["gather_over_mask"] = round(row["mask"]["median_ms"] / row["gather"]["median_ms"], 2)
            row["gather_over_today"] = round(row["today"]["median_ms"] / row["gather"]["median_ms"], 2)
            res["results"].append(row)
            print(json.dumps(row), flush=True)
        N.check(L.ott_store_set_option(h, b"group_gather", -1))
    print(json.dumps(res))
    L.ott_store_destroy(h)


if __name__ == "__main__":
    main()
