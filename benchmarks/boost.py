"""Score boosting (ott_query_boost) against the masks sweep with no mask at all (ott_query_masks, every query
OTT_NO_MASK, option masks_sweep = 1): the same tile loop and the same top-k, so the difference is the boost epilogue — two FLOAT32
VALUE terms, 8 bytes more per row and pass beside the row's 4 x dim (results: profiles/boost/README.md).

Synthetic uniform rows made on the GPU, cosine, take(10), PER_QUERY, through the C ABI; host clock, end to end per call.  Before
anything is timed the two calls are compared where they must agree: with no terms and score_weight 1 the boosted call returns the
masks sweep's hits (rows, score bits, query).  The two calls are timed in alternating rounds of --reps calls; per call the median
and the interquartile spread over all rounds, and the spread of the rounds' medians (the run-to-run figure).  "expected" is the
bytes ratio 1 + 8 / (4 dim [+ 4 for cosine]); "within" says whether the boosted median lies below the masks median times that
ratio plus the two spreads.

    python benchmarks/boost.py [--shapes 250000x128,250000x768,1000000x128,1000000x768] [--nq 1,16] [--reps 20] [--rounds 5] [--warmup 3] [--out FILE]
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


def quantiles(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return q(0.25), q(0.5), q(0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="250000x128,250000x768,1000000x128,1000000x768")
    ap.add_argument("--nq", type=str, default="1,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
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
        N.check(L.ott_store_set_option(h, b"masks_sweep", 1))
        terms = (N.BoostTerm * 2)()
        for j in range(2):
            vals = rng.random(n, dtype=np.float32)
            cid = C.c_uint32(0)
            N.check(L.ott_store_add_column(h, 2, N.ptr(vals), None, n, C.byref(cid)))
            terms[j].kind, terms[j].source, terms[j].weight, terms[j].origin = N.BOOST_VALUE, cid.value, (0.1, -0.05)[j], 0.5
        for nq in (int(x) for x in a.nq.split(",")):
            q = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
            d = N.QueryDesc()
            d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, nq, 0, 1, 1, 10, 0
            out = {w: np.zeros(nq * 10, dtype=N.HIT_DTYPE) for w in ("masks", "boost")}
            n_out, per = C.c_uint64(0), (C.c_uint64 * nq)()
            moq = np.full(nq, N.NO_MASK, dtype=np.uint32)

            def masks():
                N.check(L.ott_query_masks(h, C.byref(d), None, 0, 0, N.ptr(moq), N.ptr(out["masks"]), nq * 10, C.byref(n_out), per, None))
                return n_out.value

            def boost(n_terms=2):
                N.check(L.ott_query_boost(h, C.byref(d), N.BOOST_SUM, 1.0, terms, n_terms, N.ptr(out["boost"]), nq * 10, C.byref(n_out), per, None))
                return n_out.value

            cell = {"rows": n, "dim": dim, "nq": nq}
            if masks() != boost(0) or out["masks"].tobytes() != out["boost"].tobytes():  # no terms: the same rows, score bits and query
                raise SystemExit(f"the boosted call without terms and the masks sweep disagree: {cell}")
            st = N.Stats()
            N.check(L.ott_query_boost(h, C.byref(d), N.BOOST_SUM, 1.0, terms, 2, N.ptr(out["boost"]), nq * 10, C.byref(n_out), per, C.byref(st)))
            cell["bytes_scanned"], cell["passes"] = int(st.bytes_scanned), int(st.passes)
            for fn in (masks, boost):
                for _ in range(a.warmup):
                    fn()
            ts = {"masks": [], "boost": []}
            medians = {"masks": [], "boost": []}
            for _ in range(a.rounds):  # alternating rounds: whatever else the machine does is seen by both
                for name, fn in (("masks", masks), ("boost", boost)):
                    r = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        fn()
                        r.append((time.perf_counter() - t0) * 1e3)
                    ts[name] += r
                    medians[name].append(quantiles(r)[1])
            for name in ("masks", "boost"):
                lo, med, hi = quantiles(ts[name])
                cell[name] = {"median_ms": round(med, 4), "iqr_ms": round(hi - lo, 4), "min_ms": round(min(ts[name]), 4),
                              "round_medians_spread_ms": round(max(medians[name]) - min(medians[name]), 4)}
            m, b = cell["masks"], cell["boost"]
            cell["ratio"] = round(b["median_ms"] / m["median_ms"], 4)
            cell["expected"] = round(1.0 + 8.0 / (4.0 * dim + 4.0), 4)
            cell["boost_gbps"] = round(cell["bytes_scanned"] / (b["median_ms"] * 1e-3) / 1e9, 1)
            cell["within"] = bool(b["median_ms"] <= m["median_ms"] * cell["expected"] + m["iqr_ms"] + b["iqr_ms"])
            results.append(cell)
            print(json.dumps(cell), flush=True)
        N.check(L.ott_store_destroy(h))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
