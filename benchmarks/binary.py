"""Binary vectors (ott_query_binary): the two routes against each other — store option binary_gate = 0 (a key per
(query, row) in the key table, the shared top-k behind the sweep) and 1 (the selection fused into the sweep: histograms and gates in
LDS, candidate pairs, one sort) — against what a user without bit rows does (ott_query with Metric.Dot over the same rows as f32),
and against the exact kernel's stream rate MEASURED IN THE SAME RUN (results and the automatic rule that rests on them:
profiles/binary/README.md).

A store of `rows` x `bits` f32 rows made on the GPU (i.i.d. uniform, or clustered: 256 clusters); its bit rows are the signs
(ott_store_set_binary_sign).  Queries: the signs of random f32 vectors (i.i.d.), or of stored rows with a tenth of the bits flipped
(clustered: near neighbours exist).  take_min(k), through the C ABI; host clock end to end per call, and the sweep's own time from the
stream events (ott_stats.score_ns).  Before anything is timed the two routes are compared: they must return the same bytes.  Three
runs of --reps calls per route, alternating; per route the median of each run and the spread of the three.
"frac" = layout bytes per pass x passes / the sweep's time, over the dense exact sweep's bytes per second in this run.
"pairs" = candidate pairs the gated route emitted per call and query (ott_store_binary_counters), "overflows" how many calls overflowed.

    python benchmarks/binary.py [--rows 1000000,10000000] [--bits 1024] [--k 10,100] [--nq 1,4,64] [--reps 10] [--warmup 2] [--out FILE]
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
from otters_amd.vec import binary_words, sign_bits  # noqa: E402


def counters(L, h):
    out = (C.c_uint64 * 4)()
    N.check(L.ott_store_binary_counters(h, out))
    return [int(x) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=str, default="1000000,10000000")
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--k", type=str, default="10,100")
    ap.add_argument("--nq", type=str, default="1,4,64")
    ap.add_argument("--corpora", type=str, default="iid,clustered")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    L = N.lib()
    rng = np.random.default_rng(11)
    dim = a.bits
    results = []
    for n in (int(x) for x in a.rows.split(",")):
        for corpus in a.corpora.split(","):
            h = C.c_void_p()
            N.check(L.ott_store_create(dim, 0, C.byref(h)))
            N.check(L.ott_store_reserve(h, n))
            if corpus == "iid":
                N.check(L.ott_store_append_random(h, n, 1))
            else:
                N.check(L.ott_store_append_clustered(h, n, 1, 256, 0.5, 0.0))
            N.check(L.ott_store_sync(h))
            t0 = time.perf_counter()
            N.check(L.ott_store_set_binary_sign(h))
            sign_s = time.perf_counter() - t0
            nb, nbytes = C.c_uint32(0), C.c_uint64(0)
            N.check(L.ott_store_binary_info(h, C.byref(nb), C.byref(nbytes)))
            for nq in (int(x) for x in a.nq.split(",")):
                if corpus == "iid":
                    qf = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
                else:  # stored rows with a tenth of the signs flipped
                    qf = np.empty((nq, dim), np.float32)
                    for b in range(nq):
                        N.check(L.ott_store_read_rows(h, int(rng.integers(0, n)), 1, N.ptr(qf[b:b + 1])))
                    qf *= np.where(rng.random((nq, dim)) < 0.1, -1.0, 1.0).astype(np.float32)
                qw, _ = binary_words(sign_bits(qf))
                for k in (int(x) for x in a.k.split(",")):
                    d = N.QueryDesc()
                    d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = None, nq, 3, 0, 1, k, 0
                    out = {g: np.zeros(nq * k, dtype=N.HIT_DTYPE) for g in (0, 1)}
                    n_out, per, st = C.c_uint64(0), (C.c_uint64 * nq)(), N.Stats()

                    def call(g, stats=None):
                        N.check(L.ott_query_binary(h, C.byref(d), N.ptr(qw), N.ptr(out[g]), nq * k, C.byref(n_out), per, stats))
                        return n_out.value

                    # what a user does today: Metric.Dot over the f32 rows, the same k (take Max), the exact sweep
                    dd = N.QueryDesc()
                    dd.queries, dd.nq, dd.metric, dd.take, dd.mode, dd.k, dd.path = qf.ctypes.data, nq, 2, 1, 1, k, 1
                    dout = np.zeros(nq * k, dtype=N.HIT_DTYPE)

                    def dense(stats=None):
                        N.check(L.ott_query(h, C.byref(dd), N.ptr(dout), nq * k, C.byref(n_out), per, stats))

                    cell = {"rows": n, "bits": dim, "corpus": corpus, "nq": nq, "k": k, "layout_bytes": int(nbytes.value), "set_binary_sign_s": round(sign_s, 3)}
                    counts = []
                    for g in (0, 1):
                        N.check(L.ott_store_set_option(h, b"binary_gate", g))
                        counts.append(call(g, C.byref(st)))
                        cell[f"passes_{g}"], cell[f"bytes_scanned_{g}"] = int(st.passes), int(st.bytes_scanned)
                    if counts[0] != counts[1] or out[0].tobytes() != out[1].tobytes():
                        raise SystemExit(f"the two routes disagree: {cell}")
                    runs = {g: [] for g in (0, 1, "dense")}
                    sweep = {g: [] for g in (0, 1, "dense")}
                    for g in (0, 1):
                        N.check(L.ott_store_set_option(h, b"binary_gate", g))
                        for _ in range(a.warmup):
                            call(g)
                    for _ in range(a.warmup):
                        dense()
                    c0 = counters(L, h)
                    gated_calls = 0
                    for _ in range(3):  # three runs per route, alternating: whatever else the machine does is seen by all
                        for g in (0, 1, "dense"):
                            if g != "dense":
                                N.check(L.ott_store_set_option(h, b"binary_gate", g))
                            r, sw = [], []
                            for _ in range(a.reps):
                                t0 = time.perf_counter()
                                if g == "dense":
                                    dense(C.byref(st))
                                else:
                                    call(g, C.byref(st))
                                r.append((time.perf_counter() - t0) * 1e3)
                                sw.append(st.score_ns * 1e-6)
                            if g == "dense":
                                cell["dense_bytes_scanned"] = int(st.bytes_scanned)
                            gated_calls += a.reps if g == 1 else 0
                            runs[g].append(sorted(r)[len(r) // 2])
                            sweep[g].append(sorted(sw)[len(sw) // 2])
                    c1 = counters(L, h)
                    dense_sweep_ms = sorted(sweep["dense"])[1]
                    stream = cell["dense_bytes_scanned"] / (dense_sweep_ms * 1e-3)  # the exact kernel's bytes per second, this run
                    cell["dense_dot"] = {"median_ms": round(sorted(runs["dense"])[1], 4), "sweep_ms": round(dense_sweep_ms, 4), "stream_TBps": round(stream / 1e12, 3)}
                    for g in (0, 1):
                        name = "table" if g == 0 else "gated"
                        med, sw = sorted(runs[g])[1], sorted(sweep[g])[1]
                        cell[name] = {"run_medians_ms": [round(x, 4) for x in runs[g]], "median_ms": round(med, 4), "spread_ms": round(max(runs[g]) - min(runs[g]), 4),
                                      "sweep_ms": round(sw, 4), "layout_TBps": round(cell[f"bytes_scanned_{g}"] / (sw * 1e-3) / 1e12, 3),
                                      "frac_of_stream": round(cell[f"bytes_scanned_{g}"] / (sw * 1e-3) / stream, 3),
                                      "dense_over_this": round(cell["dense_dot"]["median_ms"] / med, 2)}
                    cell["pairs_per_query"] = round((c1[1] - c0[1]) / max(gated_calls, 1) / nq, 1)
                    cell["overflows"] = c1[2] - c0[2]
                    gap = cell["table"]["median_ms"] - cell["gated"]["median_ms"]
                    spread = max(cell["table"]["spread_ms"], cell["gated"]["spread_ms"])
                    cell["faster"] = "gated" if gap > spread else "table"  # within the spread: the table route, which serves every call
                    results.append(cell)
                    print(json.dumps(cell), flush=True)
            N.check(L.ott_store_destroy(h))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
