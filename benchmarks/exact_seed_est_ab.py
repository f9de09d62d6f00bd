"""Pruned exact sweep: the seed as an estimate pass, one library build per process.

    OTT_LIB_PATH=<build> python benchmarks/exact_seed_est_ab.py [rows] [dim] [k] [steps] [filter]   (default 10000000 768 10 30 0)

The seed's form, its coverage and the rows a wave finishes are compile-time choices (ott_exact_plan.h), so builds are compared by
running this once per library and alternating them in one job:
    -DOTT_X_SEED_EST=0        the full seed (the parent's sweep)
    -DOTT_X_SEED_EST_DIV=64   the estimate pass over rows / 64 (16: rows / 16; default: the plan's seed, rows / 32)
    -DOTT_X_SEED_KEEP=4       a wave finishes 4 rows (16: sixteen; default: min(k, 16))
(make -C otters_amd/csrc OUT=libotters_hip_x.so OBJDIR=_obj_x EXTRA=-D...).  Prints one JSON line per round, three rounds: ms per
step (wall, one query per step), the score kernels' time by the library's own events, `rescored` and the first hit.  `filter` = 1
adds a score filter that every row passes: such a query keeps the full seed in every build."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otters_amd import Cmp, Metric, Path, VecStore  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
k = int(sys.argv[3]) if len(sys.argv) > 3 else 10
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
filt = int(sys.argv[5]) if len(sys.argv) > 5 else 0
s = VecStore(dim)
s.reserve(rows)
s.append_random(rows, 0x07735)
q = np.random.default_rng(0x07736).uniform(-1, 1, dim).astype(np.float32)
plan = s.query(q, Metric.Cosine)
if filt:
    plan = plan.filter(-2.0, Cmp.Gt)
plan = plan.take_max(k).with_path(Path.Exact)
for rnd in range(3):
    for _ in range(5):
        plan.collect_arrays()
    t0 = time.perf_counter()
    for _ in range(steps):
        hits = plan.collect_arrays()[0]
    ms = (time.perf_counter() - t0) * 1e3 / steps
    st = s.last_stats
    print(json.dumps({"lib": os.path.basename(os.environ.get("OTT_LIB_PATH", "libotters_hip.so")), "round": rnd, "rows": rows, "dim": dim, "k": k, "filter": filt,
                      "ms_per_step": round(ms, 4), "score_ms": round(st["score_ns"] / 1e6, 4), "rescored": st["rescored"],
                      "first": [int(hits["index"][0]), float(hits["score"][0])]}), flush=True)
s.close()
