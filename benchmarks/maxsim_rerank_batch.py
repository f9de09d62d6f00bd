"""MaxSim re-ranking in batches against the same queries as single calls in a loop (results in
profiles/maxsim_rerank_batch/README.md).

benchmarks/maxsim_rerank.py's store: synthetic uniform rows made on the GPU (ColBERT-sized token vectors) in documents of --per-group
rows (contiguous layout), queries of --nq tokens, cosine, take(10), through the C ABI; host clock, end to end per call.  For every
B of --batches and every list size of --lists: B queries, each with its own tokens and its own list of random documents.  Two timed
rows per cell:

  (a) batch   ONE ott_query_maxsim_groups_batch with the B queries (option group_gather = 1: the batched gather); the kernels' own
              time is the stats' score_ns (gather + select) and merge_ns
  (b) loop    the same B queries as B ott_query_maxsim_groups calls, one after the other — what a caller has without the batch

Both are checked for equal hits (group ids and score bits, query = b) before anything is timed.  Medians with min / max over --reps
calls after --warmup calls; "pays" says whether the batch's maximum lies below the loop's minimum.

    python benchmarks/maxsim_rerank_batch.py [--rows 2000000] [--dim 128] [--per-group 20] [--nq 32] [--batches 1,8,64]
                                             [--lists 100,1000] [--reps 20] [--warmup 3]
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
    ap.add_argument("--batches", type=str, default="1,8,64")
    ap.add_argument("--lists", type=str, default="100,1000")
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
    k = 10
    n_groups = (a.rows + a.per_group - 1) // a.per_group
    gid = np.ascontiguousarray((np.arange(a.rows) // a.per_group).astype(np.uint32))
    N.check(L.ott_store_set_groups(h, N.ptr(gid), a.rows, n_groups))
    N.check(L.ott_store_set_option(h, b"group_gather", 1))
    st = N.Stats()
    n_out = C.c_uint64(0)

    def desc(q):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, q.shape[0], 0, 1, 0, k, 1
        return d

    res = {"rows": a.rows, "dim": a.dim, "per_group": a.per_group, "n_groups": n_groups, "nq": a.nq, "k": k, "reps": a.reps, "warmup": a.warmup, "results": []}
    for n_list in (min(int(x), n_groups) for x in a.lists.split(",")):
        for B in (int(x) for x in a.batches.split(",")):
            q = np.ascontiguousarray(rng.uniform(-1, 1, (B * a.nq, a.dim)).astype(np.float32))
            lists = np.ascontiguousarray(np.stack([rng.choice(n_groups, n_list, replace=False) for _ in range(B)]).astype(np.uint32))
            tokens = np.full(B, a.nq, np.uint32)
            listed = np.full(B, n_list, np.uint64)
            out_b, out_l = np.zeros(B * k, dtype=N.HIT_DTYPE), np.zeros(B * k, dtype=N.HIT_DTYPE)
            per = np.zeros(B, np.uint64)
            d_all = desc(q)
            d_one = [desc(q[b * a.nq:(b + 1) * a.nq]) for b in range(B)]

            def batch(stats=None):  # (timed without stats, as the loop is: asking for them adds the events and their read-back)
                N.check(L.ott_query_maxsim_groups_batch(h, C.byref(d_all), N.ptr(tokens), N.ptr(listed), B, N.ptr(lists), N.ptr(out_b), B * k, C.byref(n_out), N.ptr(per), stats))

            def loop():
                for b in range(B):
                    N.check(L.ott_query_maxsim_groups(h, C.byref(d_one[b]), N.ptr(lists[b]), n_list, N.ptr(out_l[b * k:]), k, C.byref(n_out), None))

            batch(C.byref(st))
            loop()
            assert per.tolist() == [k] * B and st.passes == 1, (per, st.passes)
            assert np.array_equal(out_b["index"], out_l["index"]) and np.array_equal(out_b["score"].view(np.uint32), out_l["score"].view(np.uint32))
            assert out_b["query"].tolist() == np.repeat(np.arange(B), k).tolist()
            r = {"B": B, "listed": n_list, "rows_read": int(B * n_list * a.per_group), "batch": timed(batch, a.reps, a.warmup), "loop": timed(loop, a.reps, a.warmup)}
            batch(C.byref(st))
            r["batch_score_us"], r["batch_merge_us"] = round(st.score_ns / 1e3, 1), round(st.merge_ns / 1e3, 1)
            r["batch_per_query_ms"] = round(r["batch"]["median_ms"] / B, 4)
            r["loop_per_query_ms"] = round(r["loop"]["median_ms"] / B, 4)
            r["pays"] = r["batch"]["max_ms"] < r["loop"]["min_ms"]
            res["results"].append(r)
            print(json.dumps(r), flush=True)
    N.check(L.ott_store_destroy(h))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
