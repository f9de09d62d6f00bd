"""Candidate id lists against the row-mask route (results in profiles/idlist/README.md).

One store (default 10M x 768, synthetic rows made on the GPU), cosine top-10, one query, through the C ABI.  For lists of
100 / 1000 / 10 000 / 65 536 random ids it times, per call and end to end on the host clock:

  mask    what a caller did before ott_query_ids: build the bit mask of the listed rows over the whole store (numpy), then
          ott_query with it (the upload is inside the call) — the mask build is timed as part of it, the caller pays it;
  gather  ott_query_ids with option id_gather = 1;
  auto    ott_query_ids with id_gather = -1 (what AUTO chose shows in vectors_compared);
  off     ott_query_ids with id_gather = 0 (the list turned into a mask on the device).

Each is the median of --reps calls after --warmup calls; the gather's kernel time is the stats' score_ns + merge_ns (hipEvent
time) and its launch count is fixed by the code path (passes x 1 scoring launch + 1 merge).  A plain query without a list is
timed as well, to show that it runs what it ran before.

    python benchmarks/id_list.py [--rows 10000000] [--dim 768] [--reps 30] [--warmup 5]
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


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[100, 1000, 10_000, 65_536])
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
    n_out = C.c_uint64(0)
    st = N.Stats()

    def desc(mask_words=None):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, 1, 0, 1, 0, k, 0
        if mask_words is not None:
            d.row_mask, d.row_mask_bits = mask_words.ctypes.data, a.rows
        return d

    def plain():
        d = desc()
        N.check(L.ott_query(h, C.byref(d), N.ptr(out), k, C.byref(n_out), None, C.byref(st)))

    res = {"rows": a.rows, "dim": a.dim, "reps": a.reps, "plain_ms": median_ms(plain, a.reps, a.warmup), "lists": []}
    for n_ids in a.sizes:
        ids = np.ascontiguousarray(rng.choice(a.rows, n_ids, replace=False).astype(np.uint64))

        def by_mask():
            keep = np.zeros(a.rows, dtype=bool)  # the caller's cost today: a mask over the whole store
            keep[ids.astype(np.int64)] = True
            words = N.pack_bits(keep)
            d = desc(words)
            N.check(L.ott_query(h, C.byref(d), N.ptr(out), k, C.byref(n_out), None, C.byref(st)))

        def by_ids():
            d = desc()
            N.check(L.ott_query_ids(h, C.byref(d), N.ptr(ids), n_ids, N.ptr(out), k, C.byref(n_out), None, C.byref(st)))

        row = {"n_ids": n_ids, "mask_ms": median_ms(by_mask, a.reps, a.warmup)}
        ref = out[: n_out.value].copy()
        for name, opt in (("gather", 1), ("auto", -1), ("off", 0)):
            N.check(L.ott_store_set_option(h, b"id_gather", opt))
            row[name + "_ms"] = median_ms(by_ids, a.reps, a.warmup)
            row[name + "_kernel_us"] = (st.score_ns + st.merge_ns) / 1e3
            row[name + "_vectors_compared"] = int(st.vectors_compared)
            row[name + "_launches"] = int(st.passes) + 1 if st.vectors_compared <= n_ids else None
            got = out[: n_out.value]
            assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (n_ids, name)
        N.check(L.ott_store_set_option(h, b"id_gather", -1))
        res["lists"].append(row)
        print(json.dumps(row), flush=True)
    res["plain_after_ms"] = median_ms(plain, a.reps, a.warmup)
    print(json.dumps(res))
    L.ott_store_destroy(h)


if __name__ == "__main__":
    main()
