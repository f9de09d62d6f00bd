"""The three sharp cases of score boosting, shared by tests/test_boost_cpu.py — which proves on the CPU that each
one tells the contract's arithmetic from the nearest wrong one — and tests/test_gpu_boost.py, which holds the device to the model
on them.  TEST INFRASTRUCTURE ONLY: numpy, no GPU.  Scores are integers (rows and queries in -2..2), so a boost of less than 1
decides only between rows of equal score, and there are many of those."""
import numpy as np

import boost_ref as BR


def int_corpus(n, dim, seed, nq=2):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    rows[np.all(rows == 0, axis=1), 0] = 1.0
    q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    q[np.all(q == 0, axis=1), 0] = 1.0
    return rng, rows, q


def chain_order(n=600, seed=71):
    """weights 1e8, 1 and -1e8: in the caller's order (1e8 + x) - 1e8 loses x (an ulp of 1e8 is 8), so B is 0 or 8; summed as
    (1e8 - 1e8) + x it is x.  Returns (terms, the permutation that is the wrong order)."""
    rng = np.random.default_rng(seed)
    one = np.ones(n, np.float32)
    x = rng.uniform(0.0, 3.0, n).astype(np.float32)
    terms = [("value", one, None, 1e8, 0.0, 0.0), ("value", x, None, 1.0, 0.0, 0.0), ("value", one, None, -1e8, 0.0, 0.0)]
    return terms, [0, 2, 1]


def datetime_decay(n=600, seed=72):
    """epoch milliseconds near 1.7e12 within 100 s of an origin beside them, and a scale of 200 s: the f64 subtraction is exact, an
    f32 one sees multiples of 131072 ms only (an ulp of f32 at 1.7e12), so every row is 0 or 131 s away.  Returns (terms, the
    f32-subtraction g of the term)."""
    rng = np.random.default_rng(seed)
    origin = 1_700_000_000_123
    ts = (origin + rng.integers(-100_000, 100_000, n)).astype(np.int64)
    scale = 200_000.0
    terms = [("decay", ts, None, 0.9, float(origin), scale, 0.0)]
    with np.errstate(all="ignore"):
        t32 = ts.astype(np.float32) - np.float32(origin)  # the wrong arithmetic: both operands rounded to f32 first
        u = np.abs(t32) / np.float32(scale)
        g32 = np.where(u >= np.float32(1.0), np.float32(0.0), np.float32(1.0) - u).astype(np.float32)
    return terms, g32


I64_EDGE = np.array([2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 3, np.iinfo(np.int64).max, np.iinfo(np.int64).min, 2 ** 24 + 1, 0, -1], dtype=np.int64)
# (double)x by the IEEE conversion, ties to even: 2^53 + 1 -> 2^53, 2^53 + 3 -> 2^53 + 4, i64::MAX -> 2^63
I64_EDGE_F64 = np.array([2.0 ** 53, -(2.0 ** 53), 2.0 ** 53 + 4.0, 2.0 ** 63, -(2.0 ** 63), 2.0 ** 24 + 1.0, 0.0, -1.0], dtype=np.float64)


def int64_edges(n=600, seed=73):
    """an Int64 column whose first rows are the edge values, the rest spread around 2^53 where f64 holds only even integers;
    origin 2^53.  Returns the terms."""
    rng = np.random.default_rng(seed)
    v = (2 ** 53 + rng.integers(-40, 40, n)).astype(np.int64)
    v[: I64_EDGE.size] = I64_EDGE
    return [("value", v, None, 0.01, 2.0 ** 53, 0.0)]


def topk_rows(F, k):
    return [h["index"].tolist() for h in BR.select(F, 1, k)]
