"""What deleted rows cost, one case per process so that two builds of the library can be run alternately:

  python benchmarks/deleted_rows.py a   no deletions: config 1 (1M x 128 dot top-10 through the C ABI) and the 10M x 768 cosine
                                        top-10 headline — medians of 3 x 400 / 3 x 100 calls; run on this build and on the parent
  python benchmarks/deleted_rows.py b   the headline with 1 % random rows out: through the store's live mask (no caller mask) and
                                        through the equivalent host row mask (what a host had to do before; the only form the
                                        parent build has)
  python benchmarks/deleted_rows.py c   10M x 768: time to delete 100k rows, to compact, and to append the survivors to a fresh
                                        store from host memory (1M-row pieces), the alternative to compacting

OTT_TREE=<root of another checkout of this project> measures that checkout (its Python package and its built library) instead
of this one; a checkout without ott_store_delete_rows runs the parts it can.  One JSON line per case on stdout."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

TREE = os.environ.get("OTT_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
from otters_amd import Metric, Path, VecStore  # noqa: E402
from otters_amd import _native as N  # noqa: E402

HAVE = hasattr(VecStore, "delete_rows")
N_BIG, DIM_BIG = int(os.environ.get("OTT_N", 10_000_000)), int(os.environ.get("OTT_DIM", 768))


def make(n, dim, seed=7):
    s = VecStore(dim)
    s.set_option("hi_prebuild", 0)  # (no background plane build beside the measurement)
    s.reserve(n)
    s.append_random(n, seed)
    return s


def c_abi_medians(store, qs, metric, take, k, reps, calls, mask=None):
    """per-call wall of ott_query without stats, path EXACT: medians of `reps` runs of `calls` calls, in microseconds"""
    d = N.QueryDesc()
    d.nq, d.metric, d.take, d.k, d.mode, d.path = 1, int(metric), take, k, 0, int(Path.Exact)
    keep = None
    if mask is not None:
        keep = N.pack_bits(mask)
        d.row_mask, d.row_mask_bits = keep.ctypes.data, int(mask.size)
    out = np.empty(k, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(0)
    h, lib = store._handle(), N.lib()
    for i in range(20):
        d.queries = qs[i % len(qs)].ctypes.data
        N.check(lib.ott_query(h, C.byref(d), N.ptr(out), k, C.byref(n_out), None, None))
    meds = []
    for _ in range(reps):
        per = []
        for i in range(calls):
            d.queries = qs[i % len(qs)].ctypes.data
            t = time.perf_counter()
            lib.ott_query(h, C.byref(d), N.ptr(out), k, C.byref(n_out), None, None)
            per.append(time.perf_counter() - t)
        meds.append(float(np.median(per) * 1e6))
    return meds, out.copy()


def case_a():
    res = {"case": "a", "tree": TREE}
    s = make(1_000_000, 128)
    qs = np.random.default_rng(3).uniform(-1, 1, (400, 128)).astype(np.float32)
    res["config1_us"], _ = c_abi_medians(s, qs, Metric.DotProduct, 1, 10, 3, 400)
    s.close()
    s = make(N_BIG, DIM_BIG)
    qs = np.random.default_rng(4).uniform(-1, 1, (100, DIM_BIG)).astype(np.float32)
    res["headline_us"], _ = c_abi_medians(s, qs, Metric.Cosine, 1, 10, 3, 100)
    s.close()
    return res


def case_b():
    res = {"case": "b", "tree": TREE}
    s = make(N_BIG, DIM_BIG)
    qs = np.random.default_rng(4).uniform(-1, 1, (100, DIM_BIG)).astype(np.float32)
    dead = np.random.default_rng(5).choice(N_BIG, N_BIG // 100, replace=False)
    mask = np.ones(N_BIG, bool)
    mask[dead] = False
    res["host_mask_us"], via_mask = c_abi_medians(s, qs, Metric.Cosine, 1, 10, 3, 100, mask=mask)
    if HAVE:
        s.delete_rows(dead)
        res["live_mask_us"], via_live = c_abi_medians(s, qs, Metric.Cosine, 1, 10, 3, 100)
        res["same_hits"] = bool(np.array_equal(via_mask, via_live))
    s.close()
    return res


def case_c():
    res = {"case": "c", "tree": TREE}
    if not HAVE:
        return res
    s = make(N_BIG, DIM_BIG)
    dead = np.random.default_rng(5).choice(N_BIG, 100_000, replace=False)
    t = time.perf_counter()
    s.delete_rows(dead)
    res["delete_100k_ms"] = (time.perf_counter() - t) * 1e3
    h, lib = s._handle(), N.lib()
    t = time.perf_counter()
    N.check(lib.ott_store_compact(h, None))
    res["compact_ms"] = (time.perf_counter() - t) * 1e3
    res["len_after"] = int(lib.ott_store_len(h))
    s.close()
    # the alternative: a fresh store, the survivors appended from host memory
    n_live = N_BIG - 100_000
    piece = np.random.default_rng(6).uniform(-1, 1, (1_000_000, DIM_BIG)).astype(np.float32)
    f = VecStore(DIM_BIG)
    f.set_option("hi_prebuild", 0)
    t = time.perf_counter()
    f.reserve(n_live)
    left = n_live
    while left:
        m = min(left, piece.shape[0])
        f.add_vectors(piece[:m])
        left -= m
    N.check(N.lib().ott_store_sync(f._handle()))
    res["reappend_ms"] = (time.perf_counter() - t) * 1e3
    res["compact_over_reappend"] = res["compact_ms"] / res["reappend_ms"]
    f.close()
    return res


if __name__ == "__main__":
    print(json.dumps({"a": case_a, "b": case_b, "c": case_c}[sys.argv[1]]()), flush=True)
