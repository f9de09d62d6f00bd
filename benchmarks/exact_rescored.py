"""Pruned exact sweep: the rows whose tails were finished (`rescored`) and the kernel times of one query on a large store.

    python benchmarks/exact_rescored.py [rows] [dim] [k] [exact_sketch_bits]      (default 10000000 768 10, the store's default form)

Prints last_stats of a few queries: `rescored` against the gated rows is the share of rows that survive the checkpoint."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Metric, Path, VecStore  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
k = int(sys.argv[3]) if len(sys.argv) > 3 else 10
store = VecStore(dim)
if len(sys.argv) > 4:
    store.set_option("exact_sketch_bits", int(sys.argv[4]))
store.reserve(rows)
store.append_random(rows, 0x07735)
rng = np.random.default_rng(0x07736)
for i in range(4):
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    store.query(q, Metric.Cosine).take_max(k).with_path(Path.Exact).collect_arrays()
    st = store.last_stats
    print(json.dumps({"rows": rows, "dim": dim, "k": k, "query": i, "rescored": st["rescored"], "share_of_rows": round(st["rescored"] / rows, 5),
                      "score_ms": round(st["score_ns"] / 1e6, 4), "merge_ms": round(st["merge_ns"] / 1e6, 4), "total_ms": round(st["total_ns"] / 1e6, 4)}))
store.close()
