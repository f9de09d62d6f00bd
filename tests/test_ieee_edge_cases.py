"""CPU: the IEEE edge corpora of tests/ieee_edges.py hit the edges they name — proved with numpy and the oracle, so that the GPU
comparisons of tests/test_gpu_ieee_edges.py cannot pass by testing tame data."""
import numpy as np
import pytest

import ieee_edges as E


def _zero_signs(scores):
    z = scores[scores == 0]
    return set(np.signbit(z).tolist())


def test_family_a_gives_both_signed_zeros_and_the_literal_collector_differs(oracle):
    rng = np.random.default_rng(0)
    rows, q, info = E.signed_zero_cosines(rng)
    inv = oracle.inv_norms(rows)
    assert np.all(inv[info["huge_rows"]] == 0)                       # the rows' own norms overflow
    assert oracle.inv_norms(q[info["huge_query"]])[0] == 0          # so does the query's: every cosine is dot * 0
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(q))
    every = oracle.vec_query(rows, q[0], oracle.METRIC_COSINE, oracle.TAKE_MAX, rows.shape[0], ties=oracle.TIES_CANONICAL)
    assert _zero_signs(every["score"]) == {False, True}
    canon = oracle.vec_query(rows, q[0], oracle.METRIC_COSINE, oracle.TAKE_MAX, 3, ties=oracle.TIES_CANONICAL)
    lit = oracle.vec_query(rows, q[0], oracle.METRIC_COSINE, oracle.TAKE_MAX, 3, ties=oracle.TIES_LITERAL)
    assert not np.array_equal(canon["score"].view(np.uint32), lit["score"].view(np.uint32))
    assert np.signbit(lit["score"]).any() and not np.signbit(canon["score"]).any()
    # the issue's case: 40 rows of dim 8 uniform in [-1, 1), one query x 1e20, cosine top-3
    r = np.random.default_rng(5)
    for _ in range(20):
        rows2 = r.uniform(-1, 1, (40, 8)).astype(np.float32)
        q2 = (r.uniform(-1, 1, 8) * 1e20).astype(np.float32)
        c = oracle.vec_query(rows2, q2, oracle.METRIC_COSINE, oracle.TAKE_MAX, 3, ties=oracle.TIES_CANONICAL)
        l = oracle.vec_query(rows2, q2, oracle.METRIC_COSINE, oracle.TAKE_MAX, 3, ties=oracle.TIES_LITERAL)
        if c["index"].tolist() != l["index"].tolist():
            break
    else:
        pytest.fail("no query x 1e20 separates the literal collector from the canonical one")
    # the subnormal rows give +-0 and +-2^-149 cosines against a query of ordinary norm
    s = np.array([oracle.cosine(rows[i], q[1], inv[i], oracle.inv_norms(q[1])[0]) for i in info["subnormal_rows"]], np.float32)
    assert np.all(np.abs(s) <= 4 * E.TINY), s


def test_family_b_sums_of_squares_are_subnormal(oracle):
    rows, q, info = E.subnormal_sums(np.random.default_rng(1))
    b = info["blocks"]
    ss = E.seq_sumsq(rows)
    assert np.all(ss[:b] < E.MIN_NORMAL) and np.all(ss[:b] > 0)               # subnormal input to sqrtf
    assert np.all(ss[b:2 * b] < E.MIN_NORMAL)                                 # (subnormal squares underflow to 0)
    assert np.all(np.abs(rows[b:2 * b]) < E.MIN_NORMAL)                       # subnormal elements only
    sq = rows[2 * b:3 * b].astype(np.float32) ** 2
    assert np.all((sq == 0).sum(axis=1) > 0) and np.all(ss[2 * b:3 * b] >= E.MIN_NORMAL)  # some squares underflow, not the norm
    assert np.all(ss[3 * b:] == 0) and np.all(np.any(rows[3 * b:] != 0, axis=1))           # nonzero rows of norm 0
    inv = oracle.inv_norms(rows)
    assert np.all(inv[3 * b:] == 0)


def test_family_c_overflows(oracle):
    rows, q, _ = E.overflow(np.random.default_rng(2))
    dots = oracle.vec_query(rows, q[0], oracle.METRIC_DOT, oracle.TAKE_MAX, rows.shape[0], ties=oracle.TIES_CANONICAL)
    assert np.isposinf(dots["score"]).any() and np.isneginf(dots["score"]).any()
    assert dots.size < rows.shape[0]                                           # inf - inf = NaN, dropped
    l2 = oracle.vec_query(rows, q[2], oracle.METRIC_EUCLIDEAN, oracle.TAKE_MAX, rows.shape[0], ties=oracle.TIES_CANONICAL)
    assert np.isposinf(l2["score"]).sum() >= 16                                # many equal +inf scores


def test_family_d_is_exact_in_half_and_lives_on_subnormals():
    rows, q, info = E.half_subnormal_rows(np.random.default_rng(3))
    # exact in half after the plane's power-of-two factor (1: row 0 carries the largest norm)
    norms = np.sqrt(E.seq_sumsq(rows))
    assert norms.argmax() == 0 and norms[0] == 1.0
    for x in (rows, q):
        assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
    # hi_rows_kernel<true>'s loss measurement, restated: sum of |x - f32(half(x))| (gradual underflow) is 0 on every row
    loss = np.abs(rows - rows.astype(np.float16).astype(np.float32)).sum(axis=1)
    assert np.all(loss == 0)
    s = rows[info["s_rows"]]
    assert np.all((np.abs(s[:, 1:]) < 2.0 ** -14) & (s[:, 1:] != 0))       # half subnormals
    # what a unit that flushed them would score, against the exact score: the miss exceeds 3x the hi pass's accumulation
    # allowance (2.5 x dim x 2^-24 x sum |a b|; the loss terms are 0 here)
    dim = rows.shape[1]
    mag = np.abs(s.astype(np.float64)) @ np.abs(q[0].astype(np.float64))
    eps = 2.5 * dim * 2.0 ** -24 * mag
    miss = info["s_exact"] - info["s_flushed"]
    assert np.all(miss > 3 * eps), (miss.min(), eps.max())


def test_family_e_bf16_lo_parts_are_subnormal(oracle):
    rows, q, _ = E.bf16_lo_edges(np.random.default_rng(4))
    assert np.all(np.sqrt(E.seq_sumsq(rows).astype(np.float64)) >= 1e-18)
    assert np.all(oracle.inv_norms(rows) > 0)                                  # not flagged
    tail = rows[:, rows.shape[1] // 2:]
    lo = E.bf16_lo(tail)
    assert np.all(np.abs(lo) < E.MIN_NORMAL) and np.count_nonzero(lo) > lo.size // 2
