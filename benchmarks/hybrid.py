"""Hybrid search (ott_query_hybrid) against the composition available without it, and the document-frequency kernel
in its two forms (results: profiles/hybrid/README.md).

Stores of --rows x 128 uniform dense rows made on the GPU, with sparse rows of about 64 entries drawn from a Zipfian vocabulary of
30522 (index of rank r with probability ~ 1 / (r + 1): a handful of indices occur in most rows), values uniform in (0, 1).  Requests
of (1 dense + 1 sparse) legs, squared L2 (take Min) beside the sparse dot product (take Max), fetch 100, k 10, through the C ABI; host
clock, end to end per call (every call ends in a device wait).  Per shape, request count and fusion:

  (a) ott_query PER_QUERY with k = fetch + ott_query_sparse with k = fetch + the same fusion in vectorised numpy, a take per leg: what a
      user composes without the call
  (b) ott_query_hybrid

Before anything is timed (b) is compared with (a): the same rows per request wherever the ranked scores differ by more than the
tolerance, the scores to 1e-5 (numpy's sum order is its own, so rows whose scores tie within it may swap).  (a)
and (b) are timed in alternating rounds of --reps calls; per figure the median and the interquartile spread over all calls, and the
spread of the rounds' medians.

The df kernel: ott_store_sparse_df end to end (memset, kernel, the counts back, one wait) with the cache made stale before every call
(a row deleted or restored outside the timed region), under sparse_df_lds = 1 (a histogram in LDS) and 0 (a global atomic add per entry), in
alternating rounds; beside it one ott_query_sparse of one query on the same store (the sweep that streams indices AND values), so that
index bytes / time can be read against the rate that sweep reaches.

    python benchmarks/hybrid.py [--rows 250000,1000000] [--requests 1,64] [--reps 10] [--rounds 4] [--warmup 3] [--out FILE]
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

DIM, VOCAB, DRAWS, FETCH, K = 128, 30522, 81, 100, 10  # 81 draws on average leave about 64 distinct indices per row
EUCLIDEAN, DOT = 1, 2


def quantiles(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return q(0.25), q(0.5), q(0.75)


def zipf_rows(rng, n, mean, vocab):
    """(indptr u64, indices u32, values f32): rows of mean/2 .. 3 mean/2 draws (`mean` on average) from the Zipfian vocabulary, duplicates merged"""
    cdf = np.cumsum(1.0 / np.arange(1, vocab + 1))
    cdf /= cdf[-1]
    lens, parts = np.zeros(n, np.int64), []
    step = 1 << 15
    for r0 in range(0, n, step):
        r1 = min(r0 + step, n)
        draws = rng.integers(mean // 2, mean * 3 // 2 + 1, r1 - r0)
        row = np.repeat(np.arange(r1 - r0, dtype=np.int64), draws)
        idx = np.minimum(np.searchsorted(cdf, rng.random(row.size)), vocab - 1)
        key = np.unique(row * (1 << 20) + idx)  # ascending by (row, index), duplicates gone
        lens[r0:r1] = np.bincount(key >> 20, minlength=r1 - r0)
        parts.append((key & ((1 << 20) - 1)).astype(np.uint32))
    ptr = np.zeros(n + 1, np.uint64)
    ptr[1:] = np.cumsum(lens)
    idx = np.concatenate(parts)
    return ptr, idx, rng.random(idx.size, dtype=np.float32)


def zipf_queries(rng, nq, vocab, q_len=16):
    """queries of q_len distinct indices: half from the vocabulary's head, half from anywhere"""
    ptr = np.arange(nq + 1, dtype=np.uint64) * q_len
    idx = np.concatenate([np.concatenate([rng.choice(256, q_len // 2, replace=False), 256 + rng.choice(vocab - 256, q_len - q_len // 2, replace=False)])
                          for _ in range(nq)]).astype(np.uint32)
    return ptr, idx, rng.uniform(0, 2, nq * q_len).astype(np.float32)


def numpy_fuse(fusion, dense, dper, sparse, sper, requests, rrf_k=60.0):
    """the host fusion a user writes today, one request after the other: a take per leg (dense Min, sparse Max)"""
    out = []
    ds, ss = np.concatenate([[0], np.cumsum(dper)]), np.concatenate([[0], np.cumsum(sper)])

    def contributions(scores, take_max):
        n = scores.size
        if fusion == N.FUSE_RRF:
            return np.float32(1.0) / (np.float32(rrf_k) + np.arange(1, n + 1, dtype=np.float32))
        s = scores.astype(np.float64)
        if fusion == N.FUSE_MINMAX:
            lo, hi = (s[-1], s[0]) if take_max else (s[0], s[-1])
        else:
            m, sd3 = s.mean(), 3.0 * s.std()
            lo, hi = m - sd3, m + sd3
        if not hi - lo > 0:
            return np.full(n, 0.5, np.float32)
        return (((s - lo) if take_max else (hi - s)) / (hi - lo)).astype(np.float32)

    for b in range(requests):
        dh, sh = dense[ds[b]:ds[b + 1]], sparse[ss[b]:ss[b + 1]]
        idx = np.concatenate([dh["index"], sh["index"]])
        c = np.concatenate([contributions(dh["score"], False), contributions(sh["score"], True)]) if idx.size else np.zeros(0, np.float32)
        rows, inv = np.unique(idx, return_inverse=True)
        F = np.zeros(rows.size, np.float32)
        np.add.at(F, inv, c)
        o = np.lexsort((rows, -F))[:K]
        out.append((rows[o], F[o]))
    return out


def timed_rounds(timed, before, a):
    for w, fn in timed.items():
        for _ in range(a.warmup):
            before.get(w, lambda: None)()
            fn()
    calls, medians = {w: [] for w in timed}, {w: [] for w in timed}
    for _ in range(a.rounds):
        for w, fn in timed.items():
            ts = []
            for _ in range(a.reps):
                before.get(w, lambda: None)()
                t0 = time.perf_counter_ns()
                fn()
                ts.append((time.perf_counter_ns() - t0) / 1e3)
            calls[w] += ts
            medians[w].append(quantiles(ts)[1])
    out = {}
    for w in timed:
        q1, med, q3 = quantiles(calls[w])
        out[w] = {"median_us": round(med, 1), "iqr_us": round(q3 - q1, 1), "rounds_spread_us": round(max(medians[w]) - min(medians[w]), 1), "calls": len(calls[w])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=str, default="250000,1000000")
    ap.add_argument("--requests", type=str, default="1,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    L = N.lib()
    rng = np.random.default_rng(17)
    results = []
    for n in (int(x) for x in a.rows.split(",")):
        h = C.c_void_p()
        N.check(L.ott_store_create(DIM, 0, C.byref(h)))
        N.check(L.ott_store_reserve(h, n))
        N.check(L.ott_store_append_random(h, n, 12345))
        N.check(L.ott_store_sync(h))
        ptr, idx, val = zipf_rows(rng, n, DRAWS, VOCAB)
        N.check(L.ott_store_set_sparse(h, N.ptr(ptr), N.ptr(idx), N.ptr(val), n, VOCAB))
        v, nnz, padded, nbytes = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        N.check(L.ott_store_sparse_info(h, C.byref(v), C.byref(nnz), C.byref(padded), C.byref(nbytes)))
        head = np.bincount(idx, minlength=VOCAB)
        store_cell = {"rows": n, "dim": DIM, "vocab": VOCAB, "nnz": int(nnz.value), "padded_entries": int(padded.value), "layout_bytes": int(nbytes.value),
                      "rows_storing_the_most_common_index": round(float(head.max()) / n, 3), "indices_in_over_half_the_rows": int((head > n / 2).sum())}

        # ---- the df kernel, both forms
        df = {f: np.zeros(VOCAB, np.uint32) for f in (0, 1)}
        n_docs, one_row, changed, flip = C.c_uint64(0), np.array([n - 1], np.uint64), C.c_uint64(0), [False]

        def stale():
            fn = L.ott_store_restore_rows if flip[0] else L.ott_store_delete_rows
            N.check(fn(h, N.ptr(one_row), 1, C.byref(changed)))
            flip[0] = not flip[0]

        def df_call(form):
            N.check(L.ott_store_sparse_df(h, N.ptr(df[form]), C.byref(n_docs)))

        for f in (0, 1):
            N.check(L.ott_store_set_option(h, b"sparse_df_lds", f))
            stale()
            stale()  # (deleted and restored: every row is live, the counts are stale)
            df_call(f)
        live_counts = np.bincount(idx, minlength=VOCAB).astype(np.uint32)
        if not (np.array_equal(df[0], live_counts) and np.array_equal(df[1], live_counts) and n_docs.value == n):
            raise SystemExit(f"the df kernel disagrees with the host count: {store_cell}")
        sq1 = zipf_queries(rng, 1, VOCAB)
        d1 = N.QueryDesc()
        d1.queries, d1.nq, d1.metric, d1.take, d1.mode, d1.k, d1.path = None, 1, DOT, 1, 1, K, 0
        out1, n_out1, per1, st1 = np.zeros(K, dtype=N.HIT_DTYPE), C.c_uint64(0), (C.c_uint64 * 1)(), N.Stats()

        def sweep1():
            N.check(L.ott_query_sparse(h, C.byref(d1), N.ptr(sq1[0]), N.ptr(sq1[1]), N.ptr(sq1[2]), N.ptr(out1), K, C.byref(n_out1), per1, C.byref(st1)))

        def form_is(f):
            N.check(L.ott_store_set_option(h, b"sparse_df_lds", f))
            stale()

        t = timed_rounds({"df_lds": lambda: df_call(1), "df_global": lambda: df_call(0), "sparse_sweep_1q": sweep1},
                         {"df_lds": lambda: form_is(1), "df_global": lambda: form_is(0)}, a)
        idx_bytes = int(padded.value) * 4
        for w in ("df_lds", "df_global"):
            t[w]["idx_TBps"] = round(idx_bytes / (t[w]["median_us"] * 1e-6) / 1e12, 3)
        t["sparse_sweep_1q"]["layout_TBps"] = round(int(st1.bytes_scanned) / (t["sparse_sweep_1q"]["median_us"] * 1e-6) / 1e12, 3)
        store_cell["df"] = t
        if flip[0]:
            stale()
        N.check(L.ott_store_set_option(h, b"sparse_df_lds", -1))
        print(json.dumps(store_cell), flush=True)
        results.append(store_cell)

        # ---- the hybrid call against the composition
        for requests in (int(x) for x in a.requests.split(",")):
            q = rng.uniform(-1, 1, (requests, DIM)).astype(np.float32)
            sq = zipf_queries(rng, requests, VOCAB)
            ones = np.ones(requests, np.uint32)
            d = N.QueryDesc()
            d.queries, d.nq, d.metric, d.take, d.mode, d.path = q.ctypes.data, requests, EUCLIDEAN, 0, 1, 0
            ds = N.QueryDesc()
            ds.queries, ds.nq, ds.metric, ds.take, ds.mode, ds.k, ds.path = None, requests, DOT, 1, 1, FETCH, 0
            first_d, first_s = np.zeros(requests * FETCH, dtype=N.HIT_DTYPE), np.zeros(requests * FETCH, dtype=N.HIT_DTYPE)
            fused = np.zeros(requests * K, dtype=N.HIT_DTYPE)
            n_out, per_d, per_s, per_req = C.c_uint64(0), (C.c_uint64 * requests)(), (C.c_uint64 * requests)(), (C.c_uint64 * requests)()

            def composed(fusion):
                d.k = FETCH
                N.check(L.ott_query(h, C.byref(d), N.ptr(first_d), first_d.size, C.byref(n_out), per_d, None))
                nd = n_out.value
                N.check(L.ott_query_sparse(h, C.byref(ds), N.ptr(sq[0]), N.ptr(sq[1]), N.ptr(sq[2]), N.ptr(first_s), first_s.size, C.byref(n_out), per_s, None))
                return numpy_fuse(fusion, first_d[:nd], np.array(list(per_d), np.int64), first_s[: n_out.value], np.array(list(per_s), np.int64), requests)

            def hybrid(fusion):
                d.k = K
                N.check(L.ott_query_hybrid(h, C.byref(d), N.ptr(ones), N.ptr(sq[0]), N.ptr(sq[1]), N.ptr(sq[2]), requests, N.ptr(ones), 0, 0.0, 0, requests, fusion, 60.0,
                                           None, FETCH, N.ptr(fused), fused.size, C.byref(n_out), per_req, None))
                return n_out.value

            for name, fusion in (("rrf", N.FUSE_RRF), ("dbsf", N.FUSE_DBSF), ("minmax", N.FUSE_MINMAX)):
                cell = {"rows": n, "dim": DIM, "requests": requests, "legs": "1 dense + 1 sparse", "fetch": FETCH, "k": K, "fusion": name}
                hybrid(fusion)
                for b, (rows, F) in enumerate(composed(fusion)):
                    got = fused[b * K:(b + 1) * K]
                    # a rank holds the same row in both, unless a neighbour's score lies within the tolerance of its own (numpy's sum
                    # order is its own: such rows may swap)
                    gap = np.abs(np.diff(F)) if F.size > 1 else np.zeros(0, np.float32)
                    clear = np.concatenate([[True], gap > 1e-5]) & np.concatenate([gap > 1e-5, [True]]) if F.size else np.zeros(0, bool)
                    clear[-1:] = False  # (the last rank's lower neighbour was cut off)
                    if got.size != rows.size or not np.allclose(got["score"], F, rtol=1e-5, atol=1e-6) or not np.array_equal(got["index"][clear], rows[clear]):
                        raise SystemExit(f"ott_query_hybrid and the composed fusion disagree in request {b}: {cell}")
                cell.update(timed_rounds({"a_composed": lambda: composed(fusion), "b_hybrid": lambda: hybrid(fusion)}, {}, a))
                cell["hybrid_over_composed"] = round(cell["b_hybrid"]["median_us"] / cell["a_composed"]["median_us"], 3)
                results.append(cell)
                print(json.dumps(cell), flush=True)
        N.check(L.ott_store_destroy(h))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
