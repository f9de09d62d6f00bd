"""CPU: the seed of the pruned sweep as an estimate pass ("the seed by estimate") — the plan's rule
(otters_amd/csrc/ott_exact_plan.h: prune_plan_seed_est, prune_seed_keep) and the estimate that ranks the seed's rows
(otters_amd/csrc/ott_prune.h: prune_score_est_sketchq).  The headers are compiled on their own with the host compiler, as in
test_exact_plan_head_cpu.py and test_exact_prune_head_bound.py, whose driver and case families the estimate's half reuses.
  1. the rule: a table over head on / off, list entries per lane, filter or none, and stores around 1 310 720 rows;
  2. the estimate on the head bound's inputs, cosine and dot: in f32::total_cmp order at most the upper bound (Take Max) and at least
     the lower bound (Take Min: the mirror image), within the bound's half width of the oracle's score, and NaN exactly where the
     line claims no bound;
  3. a figure, not a gate: the share of the exact top-10 of 100k uniform rows that the top-10 by estimate holds.
The GPU half is tests/test_gpu_exact_seed_est.py; the sanitizer walk is tests/host/prune_seed_est_walk.cpp."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_exact_prune_head_bound as HB
from sketchq_queries import QUERY_KINDS, stress_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")
P, PU, PI = HB.P, HB.PU, HB.PI
FIRST = HB.FIRST

DRIVER = HB.DRIVER + r"""
#include "ott_exact_plan.h"
// the estimate of one row from its line and head, as the estimate pass forms it (the K of hd_bound_line)
extern "C" float hd_est_line(const float* q, const float* v, unsigned dim, const unsigned* line, float qinv, float vinv, int cosine) {
    const unsigned nst = stages(dim);
    unsigned codes[4];
    const float rho_all = hd_head(v, dim, line, codes);
    PruneQuant x;
    double qt, qn;
    if (!prune_query_bounds(q, dim, 0, &qt, &qn) || !prune_query_quant(q, dim, 0, &x)) return NAN;
    unsigned planes[12 * 64];
    planes_of(q, dim, x.inv_scale, nst, planes);
    int K[3] = {0, 0, 0};
    for (unsigned s = 0; s < nst; s++) {
        const unsigned* w = s ? line + 4 + 4 * (s - 1) : codes;
        for (unsigned i = 0; i < 4; i++)
            for (unsigned d = 0; d < 3; d++) K[d] = prune_dot8_i4(w[i], planes[s * 12 + d * 4 + i], K[d]);
    }
    return prune_score_est_sketchq(vinv, prune_u2f(line[0]), rho_all, 2 * (256 * K[2] + 16 * K[1] + K[0]) + x.qsum, x.scale, qinv, cosine != 0);
}
extern "C" void est_rows(const float* q, const float* rows, unsigned long long n, unsigned dim, float qinv, const float* vinv, float* out) {
    for (unsigned long long r = 0; r < n; r++) {
        unsigned line[4 + 4 * 64];
        hd_line(rows + r * dim, dim, line);
        out[r] = hd_est_line(q, rows + r * dim, dim, line, qinv, vinv[r], 1);
    }
}
// a four-bit store of `rows` rows x 768 with a head or none; o: the plan's seed, the rows of the estimate pass
extern "C" void seed_plan(unsigned long long rows, int head, int E, int filtered, int exact_prune, unsigned long long* o) {
    const PruneIn in{768, 768, OTT_METRIC_COSINE, false, true, false, 0, exact_prune, 1, SketchState{true, true, 4, 92, 1}, rows, E};
    const PrunePlan pp = prune_plan(in);
    o[0] = pp.seed;
    o[1] = prune_plan_seed_est(in, pp, head != 0 && prune_plan_head(in, pp, true, HeadState{true, true, -1}), filtered != 0);
}
extern "C" unsigned seed_keep(unsigned long long k) { return prune_seed_keep(k); }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("seedest")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    u, i, f = C.c_uint, C.c_int, C.c_float
    for name, args, res in (("hd_pitch", [u], u), ("hd_line", [P, u, PU], None), ("hd_custom", [P, u, f, PI, PU], None), ("hd_head", [P, u, PU, PU], f),
                            ("hd_bound_line", [P, P, u, PU, f, f, i, i, PI], f), ("hd_bound", [P, P, u, f, f, i, i], f),
                            ("hd_est_line", [P, P, u, PU, f, f, i], f), ("est_rows", [P, P, C.c_ulonglong, u, f, P, P], None),
                            ("seed_plan", [C.c_ulonglong, i, i, i, i, C.POINTER(C.c_ulonglong)], None), ("seed_keep", [C.c_ulonglong], u)):
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, res
    return L


# ---- 1. the rule --------------------------------------------------------------------------------------------------------------------
def test_the_rule(lib):
    """the estimate pass covers the plan's seed exactly when the head form runs, the list has one entry per lane (k <= 64), the query
    carries no filter and a tenth of the rows is at least 131 072 — stores from 1 310 720 rows; else 0, the full seed"""
    n = 0
    for head, E, filtered, rows in itertools.product((0, 1), (1, 2, 4, 8), (0, 1), (1_310_656, 1_310_719, 1_310_720, 1_310_784, 10_000_000)):
        o = (C.c_ulonglong * 2)()
        lib.seed_plan(rows, head, E, filtered, -1, o)
        seed = rows // 10  # (prune_plan: a tenth; k <= 64, once that is more than 131 072: a thirty-second, never fewer than 131 072)
        if E == 1 and seed > 131_072:
            seed = max(rows // 32, 131_072)
        seed = (seed + 63) // 64 * 64
        assert int(o[0]) == seed, (rows, E, int(o[0]))
        want = seed if (head and E == 1 and not filtered and rows >= 1_310_720) else 0
        assert int(o[1]) == want, (head, E, filtered, rows, int(o[1]))
        n += 1
    assert n == 80
    o = (C.c_ulonglong * 2)()
    lib.seed_plan(1_310_656, 1, 1, 0, -1, o)  # (its seed rounds UP to 131 072 rows: the rule reads the tenth itself)
    assert (int(o[0]), int(o[1])) == (131_072, 0)
    lib.seed_plan(40_320, 1, 1, 0, 1, o)  # a small store with the sweep forced on: the full seed, as before
    assert (int(o[0]), int(o[1])) == (4032, 0)
    lib.seed_plan(10_000_000, 1, 1, 0, 0, o)  # the sweep switched off: nothing
    assert (int(o[0]), int(o[1])) == (0, 0)


def test_rows_a_wave_finishes(lib):
    assert [lib.seed_keep(k) for k in (1, 4, 10, 16, 17, 64)] == [1, 4, 10, 16, 16, 16]


# ---- 2. the estimate on the head bound's inputs -----------------------------------------------------------------------------------------
def ulp(x):
    x = np.float32(abs(float(x)))
    return float(np.spacing(x)) if np.isfinite(x) else 0.0


def check_est(lib, oracle, q, rows, where, lines=None):
    """every row, cosine and dot.  Returns (rows with an estimate, rows without)"""
    q = np.ascontiguousarray(q, np.float32)
    rows = np.ascontiguousarray(rows, np.float32)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    n_est = n_none = 0
    for i in range(rows.shape[0]):
        line = HB.line_of(lib, rows[i]) if lines is None else lines[i]
        for cosine in (True, False):
            e = np.float32(lib.hd_est_line(q.ctypes.data_as(P), rows[i].ctypes.data_as(P), q.size, line.ctypes.data_as(PU), np.float32(inv_q), np.float32(inv_v[i]),
                                           int(cosine)))
            up = HB.bound(lib, q, rows[i], inv_q, inv_v[i], cosine, True, line)
            lo = HB.bound(lib, q, rows[i], inv_q, inv_v[i], cosine, False, line)
            # NaN — the row is not offered — exactly for a line that claims no bound
            assert np.isnan(e) == np.isnan(up) == np.isnan(lo), (where, i, cosine, e, lo, up)
            if np.isnan(e):
                n_none += 1
                continue
            n_est += 1
            # Take Max: the estimate's ordinal is at most the upper bound's; Take Min, the mirror image: at least the lower bound's
            assert HB.tkey(e) <= HB.tkey(up), (where, i, cosine, e, up)
            assert HB.tkey(e) >= HB.tkey(lo), (where, i, cosine, e, lo)
            s = np.float32(oracle.cosine(q, rows[i], inv_q, inv_v[i]) if cosine else oracle.dot(q, rows[i]))
            if np.isnan(s) or not (np.isfinite(up) and np.isfinite(lo) and np.isfinite(e)):
                continue
            # within the bound's half width of the score: the estimate is the interval's centre, rounded to f32 once (half an ulp);
            # cosine scales the centre and both ends by two f32 products each (an ulp each)
            half = (float(up) - float(lo)) / 2
            slack = 0.5 * ulp(e) + (ulp(e) + ulp(up) + ulp(lo) if cosine else 0.0)
            assert abs(float(e) - float(s)) <= half + slack, (where, i, cosine, e, s, lo, up)
    return n_est, n_none


@pytest.mark.parametrize("dim", HB.DIMS)
@pytest.mark.parametrize("kind", ["uniform", "gauss"])
def test_uniform_and_gaussian_rows(lib, oracle, dim, kind):
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (120, dim)) if kind == "uniform" else rng.normal(0, 1, (120, dim))).astype(np.float32)
    assert check_est(lib, oracle, q, rows, kind) == (240, 0)


@pytest.mark.parametrize("dim", [768, 773])
def test_clipped_outliers_and_lines_of_any_a(lib, oracle, dim):
    """the decoys of the GPU test are of this kind: an outlier makes the line coarse and the estimate poor — but it stays inside the bound"""
    rng = np.random.default_rng(dim + 5)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.normal(0, 1, (40, dim)).astype(np.float32)
    rows[:, FIRST + 7] = 40.0
    rows[::2, dim - 2] = -55.0
    rows[::3, 4] = 70.0
    lines = []
    for i in range(rows.shape[0]):
        tail = rows[i, FIRST:].astype(np.float64)
        delta = [np.quantile(np.abs(tail), 0.9) / 8, 1e-6, 1e6, np.abs(tail).max() / 8, 0.3][i % 5]
        code = np.clip(np.floor(tail / delta), HB.LO, HB.HI).astype(np.int32)
        if i % 7 == 3:
            code = rng.integers(HB.LO, HB.HI + 1, tail.size).astype(np.int32)
        lines.append(HB.custom(lib, rows[i], 0.0 if i % 11 == 10 else delta / 2, code))
    assert check_est(lib, oracle, q, rows, "custom", lines=lines) == (80, 0)
    assert check_est(lib, oracle, q, rows, "outliers") == (80, 0)


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-38, 1e-42, 1e10, 1e15, 1e18, 1e19, 3e20])
def test_subnormal_and_near_overflow_scales(lib, oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale) + 50))
    dim = 768
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (40, dim)) * scale).astype(np.float32)
    rows[::7, FIRST:] = 0.0
    check_est(lib, oracle, q, rows, scale)
    qs = (q * np.float32(scale)).astype(np.float32)  # (a query the quantiser or prune_query_bounds refuses: no estimate either)
    n_est, n_none = check_est(lib, oracle, qs, rng.uniform(-1, 1, (20, dim)).astype(np.float32), ("query", scale))
    assert (n_est > 0) == (1e-30 <= scale <= 1e10) and n_est + n_none == 40
    big = (rng.uniform(-1, 1, (8, dim)) * 3e38).astype(np.float32)  # rho_all = +inf
    assert check_est(lib, oracle, q, big, "overflow") == (0, 16)
    big0 = rng.uniform(-1, 1, (8, dim)).astype(np.float32)
    big0[:, :FIRST] = (rng.uniform(0.5, 1, (8, FIRST)) * 3e38).astype(np.float32)
    assert check_est(lib, oracle, q, big0, "overflow in stage 0") == (0, 16)


@pytest.mark.parametrize("dim", [768, 225])
def test_nan_inf_and_zero_rows(lib, oracle, dim):
    rng = np.random.default_rng(3)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (12, dim)).astype(np.float32)
    rows[0, 3] = np.nan
    rows[1, 0] = np.inf
    rows[2, 31] = -np.inf
    rows[3, FIRST + 3] = np.nan
    rows[4, dim - 1] = np.inf
    rows[5] = 0.0  # (a zero norm: no bound, no estimate)
    rows[6, :FIRST] = 0.0
    rows[7, :FIRST] = -0.0
    rows[8, FIRST:] = -0.0
    rows[9, FIRST:] = 0.0  # zero outside stage 0: a = 0, the estimate is 0
    assert check_est(lib, oracle, q, rows[:6], "no bound") == (0, 12)
    assert check_est(lib, oracle, q, rows[6:], "zeros") == (12, 0)
    inv_q = oracle.inv_norms(q[None, :])[0]
    line = HB.line_of(lib, rows[11])
    for vinv in (np.nan, np.inf, 0.0, 1e-30):
        assert np.isnan(lib.hd_est_line(q.ctypes.data_as(P), rows[11].ctypes.data_as(P), dim, line.ctypes.data_as(PU), np.float32(inv_q), np.float32(vinv), 1))


@pytest.mark.parametrize("dim", [768, 225])
def test_a_stage_0_that_holds_nearly_the_whole_norm(lib, oracle, dim):
    rng = np.random.default_rng(dim + 9)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    rows[:, :FIRST] *= np.geomspace(1e2, 1e12, 40, dtype=np.float32)[:, None]
    assert check_est(lib, oracle, q, rows, "stage 0 dominates") == (80, 0)


@pytest.mark.parametrize("kind", QUERY_KINDS)
def test_queries_that_stress_the_quantiser(lib, oracle, kind):
    dim = 773
    rng = np.random.default_rng(dim + 31)
    rows = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    n_est, n_none = check_est(lib, oracle, stress_query(kind, dim), rows, kind)
    assert n_est + n_none == 80 and (n_est == 0) == (kind in HB.REFUSED)


# ---- 3. the figure ------------------------------------------------------------------------------------------------------------------------
def test_share_of_the_top_10_that_the_estimate_finds(lib, oracle):
    """dim 768, cosine, Take Max, 100k uniform rows: how many of the exact top-10 the top-10 by estimate holds, and where the exact
    10th best of the rows chosen by estimate (the gate the estimate pass would hand on) ranks among all rows.  Printed, not held:
    nothing rests on the estimate's accuracy.  What IS held: ten rows chosen by estimate give a gate that is no better than the real
    10th best — any ten exactly scored rows do."""
    dim, n, k = 768, 100_000, 10
    rng = np.random.default_rng(2024)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = np.ascontiguousarray(oracle.inv_norms(rows), np.float32)
    est = np.empty(n, np.float32)
    lib.est_rows(q.ctypes.data_as(P), rows.ctypes.data_as(P), n, dim, np.float32(inv_q), inv_v.ctypes.data_as(P), est.ctypes.data_as(P))
    assert not np.isnan(est).any()
    top = oracle.vec_query(rows, q, oracle.METRIC_COSINE, oracle.TAKE_MAX, 100, 0, 0.0, ties=oracle.TIES_CANONICAL)
    by_est = np.argsort(-est.astype(np.float64), kind="stable")[:k]
    exact_of = {int(i): float(s) for i, s in zip(top["index"], top["score"])}
    shared = len(set(int(i) for i in by_est) & set(int(i) for i in top["index"][:k]))
    chosen = oracle.vec_query(np.ascontiguousarray(rows[np.sort(by_est)]), q, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, 0, 0.0, ties=oracle.TIES_CANONICAL)
    gate = float(chosen["score"][k - 1])
    rank = int(np.count_nonzero(top["score"].astype(np.float64) > gate))
    err = np.array([float(est[i]) - exact_of[i] for i in exact_of])
    print(f"dim {dim}, {n} uniform rows: the top-10 by estimate holds {shared} of the exact top-10; the exact 10th best of the ten rows "
          f"chosen by estimate ranks {rank + 1}{'+' if rank == 100 else ''} among all rows; |estimate - score| over the exact top-100: "
          f"mean {np.abs(err).mean():.2e}, max {np.abs(err).max():.2e} (sigma = 1/sqrt(dim) = {dim ** -0.5:.2e})")
    assert HB.tkey(np.float32(gate)) <= HB.tkey(top["score"][k - 1])
