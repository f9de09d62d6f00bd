"""Rank fusion (ott_query_fuse) against fusing on the host (results: profiles/fuse/README.md).

Synthetic uniform rows made on the GPU, cosine, 64 requests x 4 legs, fetch 100, k 10, through the C ABI; host clock, end to end per
call (every call ends in a device wait).  Five figures per shape:

  (a) ott_query, PER_QUERY, of the same 256 legs with k = 100: the yardstick and the floor (this code does not know about fusion)
  (b) (a) plus the numpy model vectorised as a user would write it (RRF: one scatter-add per request over the legs' hits)
  (c) ott_query_fuse on the device route (option fuse_device = 1)
  (d) ott_query_fuse on the host route   (option fuse_device = 0)
  (e) the fuse kernel's own event time (the median stats.merge_ns of the fused call on the host route minus that of ott_query with
      k = fetch, which is its first stage), for RRF, DBSF and MINMAX, and for one request of 16 legs x 512

Before anything is timed (c) and (d) are compared with each other (the same bytes) and with (b)'s ranking (the same rows per request;
numpy's sum order is its own, so scores are compared to 1e-6).  (a) .. (d) are timed in alternating rounds of --reps calls; per
figure the median and the interquartile spread over all calls, and the spread of the rounds' medians (the run-to-run figure).

    python benchmarks/fuse.py [--shapes 1000000x128,1000000x768] [--requests 64] [--path 0] [--reps 10] [--rounds 4] [--warmup 3] [--out FILE]
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

LEGS, FETCH, K = 4, 100, 10


def quantiles(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return q(0.25), q(0.5), q(0.75)


def numpy_rrf(hits, per, requests, rrf_k=60.0):
    """the host fusion a user writes today: per request, scatter-add 1 / (k + rank) over its legs' hits, then a top-k"""
    out = []
    starts = np.concatenate([[0], np.cumsum(per)])
    for b in range(requests):
        lo, hi = starts[b * LEGS], starts[(b + 1) * LEGS]
        idx = hits["index"][lo:hi]
        rank = np.concatenate([np.arange(1, n + 1, dtype=np.float32) for n in per[b * LEGS:(b + 1) * LEGS]])
        rows, inv = np.unique(idx, return_inverse=True)
        F = np.zeros(rows.size, np.float32)
        np.add.at(F, inv, np.float32(1.0) / (np.float32(rrf_k) + rank))
        o = np.lexsort((rows, -F))[:K]
        out.append((rows[o], F[o]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="1000000x128,1000000x768")
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--path", type=int, default=0, help="ott_path of every call: 0 AUTO, 1 EXACT, 2 MFMA")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    requests = a.requests  # (q holds 16 rows at least: the 16 x 512 figure reads them)
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
        nq = requests * LEGS
        q = rng.uniform(-1, 1, (max(nq, 16), dim)).astype(np.float32)
        legs = np.full(requests, LEGS, np.uint32)
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.mode, d.path = q.ctypes.data, nq, 0, 1, 1, a.path
        first = np.zeros(nq * FETCH, dtype=N.HIT_DTYPE)
        fused = {w: np.zeros(requests * K, dtype=N.HIT_DTYPE) for w in ("device", "host")}
        n_out, per, per_req = C.c_uint64(0), (C.c_uint64 * nq)(), (C.c_uint64 * requests)()

        def plain():
            d.k = FETCH
            N.check(L.ott_query(h, C.byref(d), N.ptr(first), first.size, C.byref(n_out), per, None))
            return first[: n_out.value], np.array(list(per), np.int64)

        def plain_numpy():
            return numpy_rrf(*plain(), requests)

        def route_is(route):
            N.check(L.ott_store_set_option(h, b"fuse_device", 1 if route == "device" else 0))

        def fuse(route, fusion=N.FUSE_RRF, stats=None):  # (route: which buffer; the option is set by route_is, outside the timed call)
            d.k = K
            N.check(L.ott_query_fuse(h, C.byref(d), N.ptr(legs), requests, fusion, 60.0, None, FETCH, N.ptr(fused[route]), fused[route].size,
                                     C.byref(n_out), per_req, None if stats is None else C.byref(stats)))
            return n_out.value

        cell = {"rows": n, "dim": dim, "path": a.path, "requests": requests, "legs": LEGS, "fetch": FETCH, "k": K}
        route_is("device")
        n_dev = fuse("device")
        route_is("host")
        if n_dev != fuse("host") or fused["device"].tobytes() != fused["host"].tobytes():
            raise SystemExit(f"the two routes disagree: {cell}")
        for b, (rows, F) in enumerate(plain_numpy()):  # numpy's scatter-add has its own summation order: the ranked scores to 1e-6
            got = fused["device"][b * K:(b + 1) * K]
            if not np.allclose(got["score"], F, rtol=1e-6, atol=0):
                raise SystemExit(f"ott_query_fuse and the numpy fusion disagree in request {b}: {cell}")
        timed = {"a_plain": plain, "b_plain_numpy": plain_numpy, "c_fuse_device": lambda: fuse("device"), "d_fuse_host": lambda: fuse("host")}
        before = {"c_fuse_device": lambda: route_is("device"), "d_fuse_host": lambda: route_is("host")}
        for w, fn in timed.items():
            before.get(w, lambda: None)()
            for _ in range(a.warmup):
                fn()
        calls = {w: [] for w in timed}
        medians = {w: [] for w in timed}
        for _ in range(a.rounds):
            for w, fn in timed.items():
                before.get(w, lambda: None)()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter_ns()
                    fn()
                    ts.append((time.perf_counter_ns() - t0) / 1e3)
                calls[w] += ts
                medians[w].append(quantiles(ts)[1])
        for w in timed:
            q1, med, q3 = quantiles(calls[w])
            cell[w] = {"median_us": round(med, 1), "iqr_us": round(q3 - q1, 1), "rounds_spread_us": round(max(medians[w]) - min(medians[w]), 1), "calls": len(calls[w])}
        # (e) the kernel's event time.  On the host route the first stage IS ott_query with k = fetch, so the median merge_ns of the fused
        # call minus the median merge_ns of that ott_query is the fuse kernel's share
        st = N.Stats()
        kern = {}
        route_is("host")

        def kernel_share(fused_call, plain_call):
            fused_ns, plain_ns = [], []
            for i in range(a.warmup + 30):
                fused_call()
                fused_ns.append(int(st.merge_ns) / 1e3)
                plain_call()
                plain_ns.append(int(st.merge_ns) / 1e3)
            (f1, fm, f3), (p1, pm, p3) = quantiles(fused_ns[a.warmup:]), quantiles(plain_ns[a.warmup:])
            return {"median_us": round(fm - pm, 1), "iqr_us": round((f3 - f1) + (p3 - p1), 1), "first_stage_merge_us": round(pm, 1)}

        def plain_stats():
            d.k = FETCH
            N.check(L.ott_query(h, C.byref(d), N.ptr(first), first.size, C.byref(n_out), per, C.byref(st)))

        for name, fusion in (("rrf", N.FUSE_RRF), ("dbsf", N.FUSE_DBSF), ("minmax", N.FUSE_MINMAX)):
            kern[name] = kernel_share(lambda: fuse("host", fusion, st), plain_stats)
        # one request of 16 legs x 512: the 8192-entry network
        legs16 = np.array([16], np.uint32)
        d16 = N.QueryDesc()
        d16.queries, d16.nq, d16.metric, d16.take, d16.mode, d16.path = q.ctypes.data, 16, 0, 1, 1, a.path
        out16 = np.zeros(K, dtype=N.HIT_DTYPE)
        first16 = np.zeros(16 * 512, dtype=N.HIT_DTYPE)
        per16, per1 = (C.c_uint64 * 16)(), (C.c_uint64 * 1)()

        def fuse16(fusion):
            d16.k = K
            N.check(L.ott_query_fuse(h, C.byref(d16), N.ptr(legs16), 1, fusion, 60.0, None, 512, N.ptr(out16), K, C.byref(n_out), per1, C.byref(st)))

        def plain16():
            d16.k = 512
            N.check(L.ott_query(h, C.byref(d16), N.ptr(first16), first16.size, C.byref(n_out), per16, C.byref(st)))

        for name, fusion in (("rrf_16x512", N.FUSE_RRF), ("dbsf_16x512", N.FUSE_DBSF), ("minmax_16x512", N.FUSE_MINMAX)):
            kern[name] = kernel_share(lambda: fuse16(fusion), plain16)
        cell["e_kernel"] = kern
        results.append(cell)
        print(json.dumps(cell), flush=True)
        N.check(L.ott_store_destroy(h))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
