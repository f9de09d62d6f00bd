"""Queries that stress the quantised query of the pruned sweep's integer decode (otters_amd/csrc/ott_prune.h: prune_query_quant), shared
by tests/test_exact_prune_sketchq_bound.py (CPU: the bound) and tests/test_gpu_exact_sketch4_int.py (GPU: the kernel).  The sketch
starts at dim 32 (stage 1); every kind fits dim >= 96."""
import numpy as np

QUERY_KINDS = ["one_big", "max_in_stage0", "max_in_tail", "half_integers", "zero_tail", "subnormals", "max_2^-126", "max_2^-100", "max_2^40", "max_under_2^50"]
REFUSED = {"max_2^-126"}


def stress_query(kind, dim, seed=0):
    rng = np.random.default_rng(1000 + seed)
    first = 32
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    if kind == "one_big":            # one element 2^20 times the rest: the rest quantises to 0 or +-1
        q[first + 5] = np.float32(2.0 ** 20)
    elif kind == "max_in_stage0":    # the scale comes from the prefix: the whole tail is small against it
        q *= np.float32(1e-3)
        q[3] = 1.0
    elif kind == "max_in_tail":
        q *= np.float32(1e-3)
        q[dim - 2] = -1.0
    elif kind == "half_integers":    # scale 2^0: every element sits exactly between two integers
        q = (rng.integers(-1800, 1800, dim) + 0.5).astype(np.float32)
        q[1] = 1900.5
    elif kind == "zero_tail":
        q[first:] = 0.0
    elif kind == "subnormals":
        q[first::3] = (rng.uniform(-1, 1, q[first::3].size) * 1e-40).astype(np.float32)
        q[7] = np.float32(1e-42)
    elif kind == "max_2^-126":
        q = (q / np.abs(q).max() * np.float32(2.0 ** -126)).astype(np.float32)
    elif kind == "max_2^-100":
        q = (q / np.abs(q).max() * np.float32(2.0 ** -100)).astype(np.float32)
    elif kind == "max_2^40":
        q = (q / np.abs(q).max() * np.float32(2.0 ** 40)).astype(np.float32)
    elif kind == "max_under_2^50":   # (||q|| stays under prune_query_bounds' 2^50: the other elements are 2^25 at most)
        q = (q * np.float32(2.0 ** 25)).astype(np.float32)
        q[first + 9] = np.float32(2.0 ** 50 * (1 - 2.0 ** -10))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(q, np.float32)
