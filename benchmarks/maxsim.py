"""Late-interaction (MaxSim) search against the route a caller had before it (results in profiles/maxsim/README.md).

One store of synthetic uniform rows made on the GPU (ColBERT-sized token vectors), groups of --per-group rows, one query of --nq
tokens, cosine, take(10), through the C ABI; host clock, end to end per call.  Two layouts of the SAME rows: "contiguous" (a
document's rows were appended together: gid = row // per_group) and "shuffled" (the same group sizes, ids permuted over the rows).

  (a) maxsim      ott_query_maxsim, k = 10; the kernels' own time is the stats' score_ns (sweeps + reduce + select) and merge_ns
  (b) workaround  ott_query_groups in PER_QUERY mode with k = n_groups (a plan without take) for the nq tokens — nq x n_groups hits
                  through the radix sort and over PCIe — then the sum per group in NumPy and the cut at 10.  Checked against (a)
                  for equal results (group ids and score bits) before it is timed.
  (c) fold A/B    (a) with the sweep's run-length fold off and on, alternated round by round.  Needs the diagnostic build of the
                  library, which carries both epilogues behind option "maxsim_fold" (make OUT=libotters_hip_dbg.so
                  OBJDIR=_obj_dbg EXTRA=-DOTT_MFMA_DEBUG_BUILD, then OTT_LIB_PATH=.../libotters_hip_dbg.so); skipped otherwise.

Medians with min / max over --reps calls after --warmup calls; (c) reports the median of the rounds' medians and their spread.

    python benchmarks/maxsim.py [--rows 2000000] [--dim 128] [--per-group 20] [--nq 32] [--reps 20] [--warmup 3]
                                [--workaround-reps 3] [--rounds 5] [--no-workaround]
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


def total_key(score):
    b = np.asarray(score, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--per-group", type=int, default=20)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workaround-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-workaround", action="store_true")
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
    out = np.empty(k, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(0)
    st = N.Stats()

    def desc(kk, mode):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, a.nq, 0, 1, mode, kk, 1
        return d

    def maxsim():
        d = desc(k, 0)
        N.check(L.ott_query_maxsim(h, C.byref(d), N.ptr(out), k, C.byref(n_out), C.byref(st)))

    have_ab = L.ott_store_set_option(h, b"maxsim_fold", -1) == 0
    res = {"rows": a.rows, "dim": a.dim, "per_group": a.per_group, "n_groups": n_groups, "nq": a.nq, "reps": a.reps, "warmup": a.warmup,
           "fold_ab_available": have_ab, "layouts": []}
    contiguous = (np.arange(a.rows) // a.per_group).astype(np.uint32)
    for name, gid in (("contiguous", contiguous), ("shuffled", contiguous[rng.permutation(a.rows)])):
        gid = np.ascontiguousarray(gid)
        N.check(L.ott_store_set_groups(h, N.ptr(gid), gid.size, n_groups))
        row = {"layout": name, "maxsim": timed(maxsim, a.reps, a.warmup)}
        row["maxsim"].update(score_us=round(st.score_ns / 1e3, 1), merge_us=round(st.merge_ns / 1e3, 1), passes=int(st.passes))
        got = out[: n_out.value].copy()
        if not a.no_workaround:
            big = np.empty(a.nq * n_groups, dtype=N.HIT_DTYPE)
            per = (C.c_uint64 * a.nq)()
            host_ms = []

            def workaround():
                d = desc(n_groups, 1)
                N.check(L.ott_query_groups(h, C.byref(d), N.ptr(big), big.size, C.byref(n_out), per, None))
                t0 = time.perf_counter()
                hits = big[: n_out.value]
                best = np.full((a.nq, n_groups), np.nan, np.float32)
                best[hits["query"], gid[hits["index"].astype(np.int64)]] = hits["score"]
                acc = best[0].copy()
                for t in range(1, a.nq):
                    acc = acc + best[t]  # (a group that lacks a token sums to NaN and is dropped with the NaN sums)
                cand = np.flatnonzero(~np.isnan(acc))
                top = cand[np.lexsort((cand, -total_key(acc[cand])))][:k]
                workaround.top = (top, acc[top])
                host_ms.append((time.perf_counter() - t0) * 1e3)

            workaround()  # equal results first, then the clock
            top, sums = workaround.top
            assert np.array_equal(got["index"].astype(np.int64), top) and np.array_equal(got["score"].view(np.uint32), sums.view(np.uint32)), name
            host_ms.clear()
            row["workaround"] = timed(workaround, a.workaround_reps, 0)
            row["workaround"]["host_part_median_ms"] = round(sorted(host_ms)[len(host_ms) // 2], 3)
            row["workaround"]["hits"] = int(n_out.value)
            row["speedup_over_workaround"] = round(row["workaround"]["median_ms"] / row["maxsim"]["median_ms"], 1)
        if have_ab:
            ab = {0: {"ms": [], "score_us": []}, 1: {"ms": [], "score_us": []}}
            for _ in range(a.rounds):
                for fold in (0, 1):  # alternated: drift of the box lands on both
                    N.check(L.ott_store_set_option(h, b"maxsim_fold", fold))
                    t = timed(maxsim, max(a.reps // 2, 3), 1)
                    ab[fold]["ms"].append(t["median_ms"])
                    ab[fold]["score_us"].append(round(st.score_ns / 1e3, 1))
                    assert np.array_equal(out[: n_out.value], got), (name, fold)  # max is order-free: the same hits
            N.check(L.ott_store_set_option(h, b"maxsim_fold", -1))
            for fold in (0, 1):
                ms, us = sorted(ab[fold]["ms"]), sorted(ab[fold]["score_us"])
                row["fold_%d" % fold] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1],
                                         "score_us_median": us[len(us) // 2], "score_us_min": us[0], "score_us_max": us[-1]}
        res["layouts"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))
    L.ott_store_destroy(h)


if __name__ == "__main__":
    main()
