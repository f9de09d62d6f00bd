"""The Manhattan (L1) metric on the exact path against the other metrics, through the C ABI (ott_query, host output: every call
returns after the hits are in host memory, so a call's wall time includes the device synchronisation).  Prints ONE JSON object.

  --part single10m : 10M x 768, one query, top-10 — Manhattan, Euclidean and dot, all on Path.Exact, alternated in one process
  --part c1        : 1M x 128, one query, top-10 (config 1's shape), Path.Auto — Manhattan against dot
  --part batch     : 256 queries x top-100 on 1M x 768 and 10M x 768 — Manhattan's ms per batch and its corpus passes

Every shape is warmed up first; the timed reps of the metrics are interleaved.  Reported per case: median / min / max ms over the
reps, the kernel-event split of one extra call (score_ns, merge_ns), and for the streaming shapes the algorithmic bytes (n x dim
x 4 per pass) over the median time against 8 TB/s.  No background plane build runs (option hi_prebuild = 0), so nothing else
competes for HBM."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from otters_amd import Metric, Path, VecStore  # noqa: E402
from otters_amd import _native as N  # noqa: E402

PEAK = 8.0e12
TAKE = {Metric.Manhattan: 0, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Cosine: 1}


class Case:
    def __init__(self, store, q, metric, k, path):
        self.store, self.q, self.metric = store, np.ascontiguousarray(q, np.float32), metric
        self.d = N.QueryDesc()
        self.d.queries, self.d.nq, self.d.metric, self.d.take, self.d.k = self.q.ctypes.data, self.q.shape[0], int(metric), TAKE[metric], k
        self.d.path = int(path)
        self.cap = k
        self.buf = np.zeros(k, dtype=N.HIT_DTYPE)
        self.n_out = C.c_uint64(0)
        self.times = []

    def call(self, stats=None):
        t = time.perf_counter()
        N.check(N.lib().ott_query(self.store._handle(), C.byref(self.d), N.ptr(self.buf), self.cap, C.byref(self.n_out), None,
                                  C.byref(stats) if stats is not None else None))
        return time.perf_counter() - t

    def stats(self):
        st = N.Stats()
        self.call(st)
        return st.as_dict()


def summary(case, nbytes=None):
    t = np.array(case.times) * 1e3
    st = case.stats()
    out = {"metric": case.metric.name, "reps": len(t), "ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4),
           "ms_max": round(float(t.max()), 4), "score_ms": round(st["score_ns"] / 1e6, 4), "merge_ms": round(st["merge_ns"] / 1e6, 4),
           "path_used": int(st["path_used"]), "passes": int(st["passes"]), "bytes_scanned": int(st["bytes_scanned"])}
    if nbytes:
        gbs = nbytes / (np.median(t) / 1e3) / 1e9
        out["GB_per_s"] = round(float(gbs), 1)
        out["share_of_8TBps"] = round(float(gbs * 1e9 / PEAK), 3)
    return out


def interleaved(cases, warmup, reps):
    for c in cases:
        for _ in range(warmup):
            c.call()
    for _ in range(reps):
        for c in cases:
            c.times.append(c.call())


def make_store(n, dim, seed):
    s = VecStore(dim)
    s.set_option("hi_prebuild", 0)
    s.reserve(n)
    s.append_random(n, seed)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["single10m", "c1", "batch"], required=True)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"part": a.part}
    if a.part == "single10m":
        n, dim = 10_000_000, 768
        s = make_store(n, dim, 5)
        q = rng.uniform(-1, 1, (1, dim)).astype(np.float32)
        cases = [Case(s, q, m, 10, Path.Exact) for m in (Metric.Manhattan, Metric.Euclidean, Metric.DotProduct)]
        interleaved(cases, a.warmup, a.reps)
        res["shape"] = "10M x 768, 1 query, top-10, Path.Exact"
        res["algorithmic_GB"] = n * dim * 4 / 1e9
        res["cases"] = [summary(c, n * dim * 4) for c in cases]
    elif a.part == "c1":
        n, dim = 1_000_000, 128
        s = make_store(n, dim, 0x07735)
        q = rng.uniform(-1, 1, (1, dim)).astype(np.float32)
        cases = [Case(s, q, m, 10, Path.Auto) for m in (Metric.Manhattan, Metric.DotProduct)]
        interleaved(cases, a.warmup, a.reps)
        res["shape"] = "1M x 128, 1 query, top-10, Path.Auto"
        res["cases"] = [summary(c, n * dim * 4) for c in cases]
    else:
        res["cases"] = []
        for n in (1_000_000, 10_000_000):
            dim = 768
            s = make_store(n, dim, 9)
            q = rng.uniform(-1, 1, (256, dim)).astype(np.float32)
            c = Case(s, q, Metric.Manhattan, 100, Path.Auto)
            interleaved([c], 1, max(3, a.reps // 6))
            r = summary(c)
            r["shape"] = f"{n // 1_000_000}M x 768, 256 queries, top-100"
            r["ms_per_query"] = round(r["ms_median"] / 256, 4)
            res["cases"].append(r)
            s.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
