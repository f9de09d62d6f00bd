"""Pruned exact sweep: the head form of the four-bit sketch against the same store without a head, in one process.

    python benchmarks/exact_head_ab.py [rows] [dim] [k] [steps]      (default 10000000 768 10 30)

Two stores of the same random rows, exact_sketch_head = -1 (the default: a gated row reads no f32 stage) and 0 (stage 0 of every row
is read, as on a store without a head), queried in turn with the same queries; prints ms per step (wall, one query per step) and
`rescored` of each, three rounds.  With both stores resident the rows take twice their HBM: 10M x 768 needs 62 GB."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Metric, Path, VecStore  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
k = int(sys.argv[3]) if len(sys.argv) > 3 else 10
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
stores = {}
for name, head in (("head", -1), ("no head", 0)):
    s = VecStore(dim)
    s.set_option("exact_sketch_head", head)
    s.reserve(rows)
    t0 = time.perf_counter()
    s.append_random(rows, 0x07735)
    print(json.dumps({"store": name, "append_random_ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)
    stores[name] = s
rng = np.random.default_rng(0x07736)
q = rng.uniform(-1, 1, dim).astype(np.float32)
for rnd in range(3):
    for name, s in stores.items():
        plan = s.query(q, Metric.Cosine).take_max(k).with_path(Path.Exact)
        for _ in range(5):
            plan.collect_arrays()
        t0 = time.perf_counter()
        for _ in range(steps):
            plan.collect_arrays()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        st = s.last_stats
        print(json.dumps({"store": name, "round": rnd, "rows": rows, "dim": dim, "k": k, "ms_per_step": round(ms, 4), "score_ms": round(st["score_ns"] / 1e6, 4),
                          "rescored": st["rescored"]}), flush=True)
for s in stores.values():
    s.close()
