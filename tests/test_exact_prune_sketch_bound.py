"""CPU: the tail sign sketch of the pruned exact sweep and its score bound (otters_amd/csrc/ott_prune.h) against
the oracle's bit-exact scores.  The header is compiled on its own with the host compiler, as in test_exact_prune_bound.py; a small
driver makes a row's sketch line with the library's own prune_sketch_row, computes the kernel's checkpoint state — the eight partial
chains after m dims (separate multiply and add) and the f32 sign dot q_t . s, one fma per dim — and asks for the bound.
  1. the sketch against a float64 restatement: signs = the f32 sign bits, rho >= ||v_t - a s||;
  2. every final score on the right side of its bound in f32::total_cmp order, and the strict gate decision;
  3. a floor on the prune rate, so that a bound that never prunes cannot pass.
The GPU half is tests/test_gpu_exact_sketch.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include <math.h>
#include "ott_prune.h"
extern "C" unsigned sk_stage0(unsigned nst) { return ott::prune_sketch_stage0(nst); }
extern "C" unsigned sk_pitch(unsigned n_words) { return ott::prune_sketch_pitch(n_words); }
extern "C" void sk_row(const float* v, unsigned dim, unsigned first, unsigned n_words, unsigned* line) {
    ott::prune_sketch_row(v, dim, first, n_words, line);
}
// the bound of one row at the checkpoint m >= first (both multiples of 32); NaN = no bound claimed
extern "C" float sk_bound(const float* q, const float* v, unsigned dim, unsigned first, unsigned m, float qinv, float vinv, int cosine, int upper) {
    const unsigned nst = ((dim + 3) / 4 * 4 + 31) / 32, n_words = nst - first / 32;
    uint32_t line[2 + 64 + 4];
    ott::prune_sketch_row(v, dim, first, n_words, line);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned c = 0; c < m; c += 8)
        for (int l = 0; l < 8; l++) {
            volatile float prod = q[c + l] * v[c + l];
            acc[l] = acc[l] + prod;
        }
    float D = 0.0f;  // the kernel's sign dot: +-1.0 from the sign bit, one fma per dim, dims past `dim` read a zero query
    for (unsigned s = m / 32; s < nst; s++) {
        const uint32_t w = line[2 + s - first / 32];
        for (unsigned b = 0; b < 32; b++) {
            const float sg = ott::prune_u2f(((w << (31 - b)) & 0x80000000u) | 0x3F800000u);
            const unsigned i = 32 * s + b;
            D = fmaf(sg, i < dim ? q[i] : 0.0f, D);
        }
    }
    double qt, qn;
    if (!ott::prune_query_bounds(q, dim, m, &qt, &qn)) return NAN;
    const double q1 = ott::prune_query_l1(q, dim, m);
    return ott::prune_score_bound_sketch(acc, vinv, ott::prune_u2f(line[0]), ott::prune_u2f(line[1]), D, m, dim, qt, q1, qn, qinv, cosine != 0,
                                         upper != 0);
}
extern "C" void sk_bound_rows(const float* q, const float* rows, unsigned long long n, unsigned dim, unsigned first, unsigned m, float qinv,
                              const float* vinv, int cosine, int upper, float* out) {
    for (unsigned long long r = 0; r < n; r++) out[r] = sk_bound(q, rows + r * dim, dim, first, m, qinv, vinv[r], cosine, upper);
}
"""

P = C.POINTER(C.c_float)
PU = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sketch")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.sk_stage0.argtypes = [C.c_uint]
    L.sk_stage0.restype = C.c_uint
    L.sk_pitch.argtypes = [C.c_uint]
    L.sk_pitch.restype = C.c_uint
    L.sk_row.argtypes = [P, C.c_uint, C.c_uint, C.c_uint, PU]
    L.sk_row.restype = None
    L.sk_bound.argtypes = [P, P, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.c_int, C.c_int]
    L.sk_bound.restype = C.c_float
    L.sk_bound_rows.argtypes = [P, P, C.c_ulonglong, C.c_uint, C.c_uint, C.c_uint, C.c_float, P, C.c_int, C.c_int, P]
    L.sk_bound_rows.restype = None
    return L


def tkey(x):
    """f32::total_cmp as an unsigned key (the library's total_key)"""
    b = int(np.float32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def geometry(lib, dim):
    """stages, the sketch's first dim (= the checkpoint), its sign words per row"""
    nst = ((dim + 3) // 4 * 4 + 31) // 32
    s0 = lib.sk_stage0(nst)
    assert s0 == nst - (nst + 3) // 4  # the last quarter of the stages, rounded up: stage 18 of 24 at dim 768
    return nst, 32 * s0, nst - s0


def sketch(lib, v, dim, first, n_words):
    v = np.ascontiguousarray(v, np.float32)
    line = np.zeros(lib.sk_pitch(n_words), np.uint32)
    lib.sk_row(v.ctypes.data_as(P), dim, first, n_words, line.ctypes.data_as(PU))
    return line


def bound(lib, q, v, first, m, qinv, vinv, cosine, upper):
    q = np.ascontiguousarray(q, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    return np.float32(lib.sk_bound(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, first, m, np.float32(qinv), np.float32(vinv),
                                   int(cosine), int(upper)))


def check_sketch(lib, rows):
    """part 1: every row's line against the float64 restatement"""
    dim = rows.shape[1]
    _, first, n_words = geometry(lib, dim)
    assert lib.sk_pitch(n_words) % 4 == 0 and lib.sk_pitch(n_words) >= n_words + 2  # whole 16-B lines
    for i in range(rows.shape[0]):
        line = sketch(lib, rows[i], dim, first, n_words)
        a, rho = line[:2].view(np.float32)
        tail = rows[i, first:]
        neg = (tail.view(np.uint32) >> 31).astype(bool)  # -0 counts as negative
        bits = np.zeros(32 * n_words, bool)
        bits[:tail.size] = neg
        want = np.packbits(bits.reshape(n_words, 32), axis=1, bitorder="little").view("<u4").ravel()
        assert np.array_equal(line[2:2 + n_words], want), i
        assert not line[2 + n_words:].any()
        if not np.isfinite(tail).all():
            assert np.isposinf(rho), (i, rho)
            continue
        with np.errstate(over="ignore"):
            t64 = tail.astype(np.float64)
            s = np.where(neg, -1.0, 1.0)
            exact = float(np.sqrt(np.sum((t64 - float(a) * s) ** 2)))
        assert a >= 0 and np.isfinite(a), (i, a)
        assert float(rho) >= exact, (i, rho, exact)
        if np.isfinite(rho) and exact > 0:  # ... and not by much: the bound is only as good as rho is close
            assert float(rho) <= exact * (1 + 1e-3) + 1e-4 * float(np.linalg.norm(t64)), (i, rho, exact)
        if np.isfinite(rho):  # a = the mean of |v_i|, rounded to f32
            mean = float(np.mean(np.abs(t64)))
            assert abs(float(a) - mean) <= 1.2e-7 * mean + 1.5e-45, (i, a, mean)


def check_rows(lib, oracle, q, rows, where, metrics=(True, False)):
    """part 2: every row, cosine and dot, Max and Min: the score inside its bound, and the gate decision at theta = the score's own
    ordinal and one on either side (prune iff ord(bound) < theta, strict) drops the row only when theta is above the row's ordinal"""
    dim = q.size
    _, first, _ = geometry(lib, dim)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    n_bounded = 0
    for i in range(rows.shape[0]):
        for cosine in metrics:
            s = np.float32(oracle.cosine(q, rows[i], inv_q, inv_v[i]) if cosine else oracle.dot(q, rows[i]))
            for upper in (True, False):
                b = bound(lib, q, rows[i], first, first, inv_q, inv_v[i], cosine, upper)
                if np.isnan(b) or np.isnan(s):
                    continue
                n_bounded += 1
                ks, kb = tkey(s), tkey(b)
                if upper:
                    assert ks <= kb, (where, i, cosine, s, b)
                    ords, ordb = ks, kb
                else:
                    assert ks >= kb, (where, i, cosine, s, b)
                    ords, ordb = 0xFFFFFFFF - ks, 0xFFFFFFFF - kb
                for theta in (ords - 1, ords, ords + 1):
                    assert not (ordb < theta) or theta > ords, (where, i, theta)
    return n_bounded


DIMS = [225, 768, 1000, 1536, 773]  # with (225, 773) and without a remainder of the chunks of eight


@pytest.mark.parametrize("dim", DIMS)
def test_uniform_rows(lib, oracle, dim):
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (200, dim)).astype(np.float32)
    check_sketch(lib, rows)
    assert check_rows(lib, oracle, q, rows, "uniform") == 4 * 200


@pytest.mark.parametrize("dim", DIMS)
def test_tails_that_are_exactly_a_times_s(lib, oracle, dim):
    """|v_i| the same over the whole tail: r = 0, rho ~ 0, and the bound is the score up to the rounding terms"""
    rng = np.random.default_rng(dim + 1)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, n_words = geometry(lib, dim)
    rows = rng.uniform(-1, 1, (120, dim)).astype(np.float32)
    for i, a in enumerate(np.geomspace(1e-3, 8.0, 120)):
        rows[i, first:] = np.float32(a) * rng.choice(np.array([-1, 1], np.float32), dim - first)
    check_sketch(lib, rows)
    check_rows(lib, oracle, q, rows, "exact a s")
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(0, 120, 7):
        line = sketch(lib, rows[i], dim, first, n_words)
        tnorm = float(np.linalg.norm(rows[i, first:].astype(np.float64)))
        assert float(line[:2].view(np.float32)[1]) <= 1e-4 * tnorm, (i, line[:2].view(np.float32))
        s = float(oracle.dot(q, rows[i]))
        scale = float(np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(rows[i].astype(np.float64)))
        up = float(bound(lib, q, rows[i], first, first, inv_q, inv_v[i], False, True))
        lo = float(bound(lib, q, rows[i], first, first, inv_q, inv_v[i], False, False))
        assert up - s <= 1e-3 * scale and s - lo <= 1e-3 * scale, (i, lo, s, up)


@pytest.mark.parametrize("dim", [768, 225])
@pytest.mark.parametrize("align", [1, -1])
def test_tails_aligned_with_and_against_the_query_signs(lib, oracle, dim, align):
    """s = +-sign(q_t): q_t . s = +-||q_t||_1, the extreme values of the sign dot"""
    rng = np.random.default_rng(11 + align)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, _ = geometry(lib, dim)
    rows = rng.uniform(-1, 1, (120, dim)).astype(np.float32)
    sgn = np.where(np.signbit(q[first:]), np.float32(-1), np.float32(1)) * np.float32(align)
    rows[:, first:] = np.abs(rows[:, first:]) * sgn
    rows[60:, first:] *= np.geomspace(1e-2, 30, 60, dtype=np.float32)[:, None]
    check_sketch(lib, rows)
    assert check_rows(lib, oracle, q, rows, ("aligned", align)) == 4 * 120


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-38, 1e-42, 1e10, 1e15, 1e18, 1e19, 3e20])
def test_subnormal_and_near_overflow_scales(lib, oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale) + 50))
    dim = 768
    _, first, _ = geometry(lib, dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (60, dim)) * scale).astype(np.float32)
    rows[::7, first:] = 0.0
    check_sketch(lib, rows)
    check_rows(lib, oracle, q, rows, scale)
    qs = (q * np.float32(scale)).astype(np.float32)
    check_rows(lib, oracle, qs, rng.uniform(-1, 1, (30, dim)).astype(np.float32), ("query", scale))
    big = (rng.uniform(-1, 1, (8, dim)) * 3e38).astype(np.float32)  # a tail whose sums leave the f32 range: rho = +inf, no bound
    check_sketch(lib, big)
    check_rows(lib, oracle, q, big, "overflow")


@pytest.mark.parametrize("dim", [768, 225])
def test_signed_zeros_nan_and_inf_in_the_tail(lib, oracle, dim):
    rng = np.random.default_rng(3)
    _, first, n_words = geometry(lib, dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (12, dim)).astype(np.float32)
    rows[0, first + 3] = np.nan
    rows[1, first + 3] = np.inf
    rows[2, dim - 1] = -np.inf
    rows[3] = 0.0                    # zero row: inverse norm 0
    rows[4, :first] = 3e38           # the prefix overflows
    rows[5, 5] = np.nan              # NaN in the prefix
    rows[6, first:] = 0.0            # a tail of +0 ...
    rows[7, first:] = -0.0           # ... and of -0: all sign bits set, a = 0, rho = 0
    rows[8, first::2] = -0.0         # zeros of both signs among finite values: |r_i| = a there
    rows[9, first + 1::2] = 0.0
    check_sketch(lib, rows)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(6):
        for cosine in (True, False):
            for upper in (True, False):
                assert np.isnan(bound(lib, q, rows[i], first, first, inv_q, inv_v[i], cosine, upper)), (i, cosine, upper)
    line = sketch(lib, rows[7], dim, first, n_words)
    assert line[0] == 0 and line[1] == 0 and line[2] == 0xFFFFFFFF
    assert check_rows(lib, oracle, q, rows[6:], "zeros") == 4 * 6
    # a query with a non-finite element, a zero query: no bound for any row; nor with a stored inverse norm NaN / inf / 0 / tiny
    for qq in (np.where(np.arange(dim) == 9, np.float32(np.inf), q), np.zeros(dim, np.float32)):
        assert np.isnan(bound(lib, qq.astype(np.float32), rows[10], first, first, 1.0, inv_v[10], False, True))
    for vinv in (np.nan, np.inf, 0.0, 1e-30):
        assert np.isnan(bound(lib, q, rows[10], first, first, inv_q, vinv, True, True)), vinv
    # scores that are +0 / -0: a query that only sees the tail, rows whose tail is a zero of either sign
    qz = np.zeros(dim, np.float32)
    qz[first:] = 1.0
    z = np.zeros((4, dim), np.float32)
    z[1, first:] = -0.0
    z[2, :first] = 1.0
    z[3, :first] = -1.0
    z[:, 0] = 1e-3
    check_rows(lib, oracle, qz, z, "signed zero scores")


def test_checkpoint_after_the_sketchs_first_stage(lib, oracle):
    """a checkpoint later than the sketch's first stage uses the same line: the remainder over fewer dims is no longer"""
    dim = 768
    rng = np.random.default_rng(5)
    _, first, _ = geometry(lib, dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (100, dim)).astype(np.float32)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(100):
        s = np.float32(oracle.dot(q, rows[i]))
        for m in (first + 32, first + 64):
            assert tkey(s) <= tkey(bound(lib, q, rows[i], first, m, inv_q, inv_v[i], False, True)), (i, m)
            assert tkey(s) >= tkey(bound(lib, q, rows[i], first, m, inv_q, inv_v[i], False, False)), (i, m)


def test_prune_rate_on_uniform_rows(lib, oracle):
    """part 3: 100k uniform rows at dim 768, the gate at the k-th best (k = 10) of the rows themselves: the bound drops at least half
    of them (a float64 model of the sketch gives 74-80 % at the weaker gate of a tenth of the rows)"""
    dim, n, k = 768, 100_000, 10
    rng = np.random.default_rng(2024)
    _, first, _ = geometry(lib, dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = np.ascontiguousarray(oracle.inv_norms(rows), np.float32)
    top = oracle.vec_query(rows, q, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, 0, 0.0, ties=oracle.TIES_CANONICAL)
    gate = tkey(top["score"][k - 1])
    out = np.empty(n, np.float32)
    lib.sk_bound_rows(q.ctypes.data_as(P), rows.ctypes.data_as(P), n, dim, first, first, np.float32(inv_q), inv_v.ctypes.data_as(P), 1, 1,
                      out.ctypes.data_as(P))
    assert not np.isnan(out).any()
    b = out.view(np.uint32).astype(np.int64)
    keys = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    dropped = int(np.count_nonzero(keys < gate))
    print(f"sketch bound at dim {first} of {dim}: {dropped} of {n} rows dropped ({100.0 * dropped / n:.1f} %)")
    assert set(int(i) for i in top["index"]).isdisjoint(np.flatnonzero(keys < gate).tolist())
    assert dropped >= n // 2, dropped
