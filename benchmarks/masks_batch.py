"""A batch of queries with a row mask per query (ott_query_masks): the masks sweep against the by-mask-group
route of the same process and the same build (results and the auto rule's constants: profiles/masks_batch/README.md).

Synthetic uniform rows made on the GPU, cosine, take(10), PER_QUERY, through the C ABI; host clock, end to end per call (the
upload of the masks included).  For every store of --shapes, every batch size of --nq, every sharing (each query a mask of its
own, or every mask shared by 8 queries) and every kind of mask — random masks of selectivity 100 %, 10 % and 1 %, and "tenant"
masks that each keep one contiguous 1/16 of the rows — two timed rows per cell:

  (a) sweep   option masks_sweep = 1: one upload, a union mask and one four-query sweep per pass, one top-k, one host wait
  (b) loop    option masks_sweep = 0: one PER_QUERY run per distinct mask — what answers these batches without the sweep

Both are checked for equal hits (rows, score bits, query) before anything is timed.  Medians and the interquartile spread over
--reps calls after --warmup calls; "wins" says whether the sweep's median lies below the loop's by more than the two spreads
together.

    python benchmarks/masks_batch.py [--shapes 10000x768,1000000x128,1000000x768] [--nq 16,64] [--share 1,8] [--reps 20] [--warmup 3] [--out FILE]
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
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return {"median_ms": round(q(0.5), 4), "iqr_ms": round(q(0.75) - q(0.25), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def make_masks(kind, n_masks, n, rng):
    if kind == "tenant":  # mask i keeps the i-th (mod 16) contiguous sixteenth of the rows
        out = np.zeros((n_masks, n), bool)
        for i in range(n_masks):
            lo = (i % 16) * (n // 16)
            out[i, lo:lo + n // 16] = True
        return out
    sel = {"100%": 1.0, "10%": 0.1, "1%": 0.01}[kind]
    if sel >= 1.0:
        return np.ones((n_masks, n), bool)
    return np.stack([rng.random(n, dtype=np.float32) < sel for _ in range(n_masks)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="10000x768,1000000x128,1000000x768")
    ap.add_argument("--nq", type=str, default="16,64")
    ap.add_argument("--share", type=str, default="1,8", help="queries per mask")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    L = N.lib()
    rng = np.random.default_rng(7)
    results = []
    for shape in a.shapes.split(","):
        n, dim = (int(x) for x in shape.split("x"))
        h = C.c_void_p()
        N.check(L.ott_store_create(dim, 0, C.byref(h)))
        N.check(L.ott_store_reserve(h, n))
        N.check(L.ott_store_append_random(h, n, 12345))
        N.check(L.ott_store_sync(h))
        for nq in (int(x) for x in a.nq.split(",")):
            q = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
            d = N.QueryDesc()
            d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, nq, 0, 1, 1, 10, 0
            out = {r: np.zeros(nq * 10, dtype=N.HIT_DTYPE) for r in (0, 1)}
            n_out, per = C.c_uint64(0), (C.c_uint64 * nq)()
            for share in (int(x) for x in a.share.split(",")):
                n_masks = nq // share
                moq = np.ascontiguousarray(np.arange(nq, dtype=np.uint32) // share)
                for kind in ("100%", "10%", "1%", "tenant"):
                    masks = make_masks(kind, n_masks, n, rng)
                    words = np.ascontiguousarray(np.stack([N.pack_bits(m) for m in masks]))

                    def call(route):
                        N.check(L.ott_query_masks(h, C.byref(d), N.ptr(words), n_masks, n, N.ptr(moq), N.ptr(out[route]), nq * 10, C.byref(n_out), per, None))
                        return n_out.value

                    cell = {"rows": n, "dim": dim, "nq": nq, "distinct_masks": n_masks, "masks": kind}
                    counts = {}
                    for route in (0, 1):
                        N.check(L.ott_store_set_option(h, b"masks_sweep", route))
                        counts[route] = call(route)
                    if counts[0] != counts[1] or out[0][:counts[0]].tobytes() != out[1][:counts[1]].tobytes():  # rows, score bits and query
                        raise SystemExit(f"the two routes disagree: {cell}")
                    for route, name in ((1, "sweep"), (0, "loop")):
                        N.check(L.ott_store_set_option(h, b"masks_sweep", route))
                        cell[name] = timed(lambda: call(route), a.reps, a.warmup)  # noqa: B023
                    s, lp = cell["sweep"], cell["loop"]
                    cell["speedup"] = round(lp["median_ms"] / s["median_ms"], 3)
                    cell["wins"] = bool(s["median_ms"] + s["iqr_ms"] + lp["iqr_ms"] < lp["median_ms"])
                    results.append(cell)
                    print(json.dumps(cell), flush=True)
        N.check(L.ott_store_destroy(h))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
