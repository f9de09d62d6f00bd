"""Sparse dot search (ott_query_sparse): the two forms of the weight lookup against each other — store option
sparse_table = 0 (the query's table in LDS, one query per pass; vocab <= 32768 only) and 1 (a device table, four queries per pass) —
on synthetic sparse rows (results and the automatic rule that rests on them: profiles/sparse/README.md).

Rows: `mean` entries on average, uniform lengths (mean/2 .. 3 mean/2) or skewed ones (geometric with that mean, cut at 16 mean);
distinct ascending indices spread over the vocab (entry j of a row of L entries lies in the j-th of L equal parts of the vocab),
values uniform in (0, 1).  Queries: 64 distinct random indices each, weights uniform in (0, 2).  take(10), through the C ABI; host
clock, end to end per call.  Before anything is timed the two forms are compared where both are eligible: they must return the
same rows and score bits.  Three runs of --reps calls per form, alternating; per form the median of each run, and the spread of
the three.  "frac" is layout bytes per pass x passes / time over the stream rate the exact kernel measured on this part (7.04 TB/s).
With scipy on the machine its CSR product on the host (one matrix-vector product per query, top-k not included) is printed as an
informational baseline.

    python benchmarks/sparse.py [--rows 250000,1000000] [--means 64,128] [--vocabs 30522,250002] [--nq 1,4,64] [--reps 10] [--warmup 2] [--out FILE]
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

STREAM_TBPS = 7.04  # README: the exact kernel's measured stream rate on this part


def make_rows(rng, n, mean, skew, vocab):
    """(indptr u64, indices u32, values f32)"""
    if skew:
        L = np.minimum(rng.geometric(1.0 / mean, n), 16 * mean)
    else:
        L = rng.integers(mean // 2, mean * 3 // 2 + 1, n)
    L = np.minimum(L, vocab).astype(np.int64)
    ptr = np.zeros(n + 1, np.uint64)
    ptr[1:] = np.cumsum(L)
    idx = np.empty(int(ptr[-1]), np.uint32)
    val = np.empty(int(ptr[-1]), np.float32)
    step = 1 << 16
    for r0 in range(0, n, step):  # in pieces: the position-in-row arithmetic needs 64-bit temporaries
        r1 = min(r0 + step, n)
        Lc = L[r0:r1]
        lo, hi = int(ptr[r0]), int(ptr[r1])
        row_len = np.repeat(Lc, Lc)
        j = np.arange(hi - lo, dtype=np.int64) - np.repeat(ptr[r0:r1].astype(np.int64) - lo, Lc)
        u = rng.random(hi - lo)
        idx[lo:hi] = np.minimum(((j + u) * vocab / row_len).astype(np.int64), vocab - 1)
        val[lo:hi] = rng.random(hi - lo, dtype=np.float32)
    # (part j of L equal parts of the vocab is at least one index wide while L <= vocab, but two neighbours may round to the same
    #  index: push duplicates up by one — rare, and strictly ascending afterwards because the parts are ordered)
    for _ in range(4):
        dup = np.flatnonzero(idx[1:] <= idx[:-1]) + 1
        dup = dup[~np.isin(dup, ptr[:-1].astype(np.int64))]  # a row's first entry has no predecessor
        if dup.size == 0:
            break
        idx[dup] = idx[dup - 1] + 1
    return ptr, idx, val


def make_queries(rng, nq, vocab, q_len=64):
    ptr = np.arange(nq + 1, dtype=np.uint64) * q_len
    idx = np.concatenate([rng.choice(vocab, q_len, replace=False) for _ in range(nq)]).astype(np.uint32)
    return ptr, idx, rng.uniform(0, 2, nq * q_len).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=str, default="250000,1000000")
    ap.add_argument("--means", type=str, default="64,128")
    ap.add_argument("--vocabs", type=str, default="30522,250002")
    ap.add_argument("--nq", type=str, default="1,4,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
        print("scipy is not on this machine: no host baseline", flush=True)
    L = N.lib()
    rng = np.random.default_rng(11)
    results = []
    for n in (int(x) for x in a.rows.split(",")):
        for mean in (int(x) for x in a.means.split(",")):
            for skew in (False, True):
                for vocab in (int(x) for x in a.vocabs.split(",")):
                    ptr, idx, val = make_rows(rng, n, mean, skew, vocab)
                    h = C.c_void_p()
                    N.check(L.ott_store_create(1, 0, C.byref(h)))  # a sparse-only collection: a store of dim 1
                    N.check(L.ott_store_reserve(h, n))
                    N.check(L.ott_store_append_random(h, n, 1))
                    N.check(L.ott_store_sync(h))
                    t0 = time.perf_counter()
                    N.check(L.ott_store_set_sparse(h, N.ptr(ptr), N.ptr(idx), N.ptr(val), n, vocab))
                    set_s = time.perf_counter() - t0
                    v, nnz, padded, nbytes = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
                    N.check(L.ott_store_sparse_info(h, C.byref(v), C.byref(nnz), C.byref(padded), C.byref(nbytes)))
                    csr = sp.csr_matrix((val, idx, ptr.astype(np.int64)), shape=(n, vocab)) if sp is not None else None
                    forms = (0, 1) if vocab <= 32768 else (1,)
                    for nq in (int(x) for x in a.nq.split(",")):
                        qptr, qidx, qval = make_queries(rng, nq, vocab)
                        d = N.QueryDesc()
                        d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = None, nq, 2, 1, 1, 10, 0
                        out = {f: np.zeros(nq * 10, dtype=N.HIT_DTYPE) for f in forms}
                        n_out, per, st = C.c_uint64(0), (C.c_uint64 * nq)(), N.Stats()

                        def call(form, stats=None):
                            N.check(L.ott_query_sparse(h, C.byref(d), N.ptr(qptr), N.ptr(qidx), N.ptr(qval), N.ptr(out[form]), nq * 10, C.byref(n_out), per, stats))
                            return n_out.value

                        cell = {"rows": n, "mean": mean, "skew": skew, "vocab": vocab, "nq": nq, "nnz": int(nnz.value), "padded_over_nnz": round(padded.value / nnz.value, 3),
                                "layout_bytes": int(nbytes.value), "set_sparse_s": round(set_s, 2)}
                        counts = []
                        for f in forms:
                            N.check(L.ott_store_set_option(h, b"sparse_table", f))
                            counts.append(call(f, C.byref(st)))
                            cell[f"passes_{f}"], cell[f"bytes_scanned_{f}"] = int(st.passes), int(st.bytes_scanned)
                        if len(forms) == 2 and (counts[0] != counts[1] or out[0].tobytes() != out[1].tobytes()):
                            raise SystemExit(f"the two forms disagree: {cell}")
                        runs = {f: [] for f in forms}
                        for f in forms:
                            N.check(L.ott_store_set_option(h, b"sparse_table", f))
                            for _ in range(a.warmup):
                                call(f)
                        for _ in range(3):  # three runs per form, alternating: whatever else the machine does is seen by both
                            for f in forms:
                                N.check(L.ott_store_set_option(h, b"sparse_table", f))
                                r = []
                                for _ in range(a.reps):
                                    t0 = time.perf_counter()
                                    call(f)
                                    r.append((time.perf_counter() - t0) * 1e3)
                                runs[f].append(sorted(r)[len(r) // 2])
                        for f in forms:
                            name = "lds" if f == 0 else "table"
                            med = sorted(runs[f])[1]
                            cell[name] = {"run_medians_ms": [round(x, 4) for x in runs[f]], "median_ms": round(med, 4), "spread_ms": round(max(runs[f]) - min(runs[f]), 4),
                                          "frac_of_stream": round(cell[f"bytes_scanned_{f}"] / (med * 1e-3) / (STREAM_TBPS * 1e12), 3)}
                        if len(forms) == 2:
                            gap = cell["lds"]["median_ms"] - cell["table"]["median_ms"]
                            spread = max(cell["lds"]["spread_ms"], cell["table"]["spread_ms"])
                            cell["faster"] = "lds" if gap <= spread else "table"  # within the spread: the LDS form, which keeps no table resident
                        if csr is not None and nq <= 4:
                            t0 = time.perf_counter()
                            for b in range(nq):
                                w = np.zeros(vocab, np.float32)
                                w[qidx[b * 64:(b + 1) * 64]] = qval[b * 64:(b + 1) * 64]
                                csr @ w
                            cell["scipy_csr_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                        results.append(cell)
                        print(json.dumps(cell), flush=True)
                    N.check(L.ott_store_destroy(h))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
