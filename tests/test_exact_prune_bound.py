"""CPU: the score bound of the pruned exact sweep (otters_amd/csrc/ott_prune.h) against the oracle's bit-exact
scores.  The header is compiled on its own with the host compiler; a small driver computes the kernel's checkpoint state — the
eight partial chains after m dims (separate multiply and add) and the fmaf chain of the prefix squares — and asks for the bound.
Every final score must lie on the right side of its bound in f32::total_cmp order (the GPU half is tests/test_gpu_exact_prune.py)."""
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
extern "C" float prune_bound(const float* q, const float* v, unsigned dim, unsigned m, float qinv, float vinv, int cosine, int upper) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, vsq = 0.0f;
    for (unsigned c = 0; c < m; c += 8)
        for (int l = 0; l < 8; l++) {
            volatile float prod = q[c + l] * v[c + l];
            acc[l] = acc[l] + prod;
            vsq = fmaf(v[c + l], v[c + l], vsq);
        }
    double qt, qn;
    if (!ott::prune_query_bounds(q, dim, m, &qt, &qn)) return NAN;
    return ott::prune_score_bound(acc, vsq, vinv, m, dim, qt, qn, qinv, cosine != 0, upper != 0);
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("prune")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    P = C.POINTER(C.c_float)
    L.prune_bound.argtypes = [P, P, C.c_uint, C.c_uint, C.c_float, C.c_float, C.c_int, C.c_int]
    L.prune_bound.restype = C.c_float
    return L


def tkey(x):
    """f32::total_cmp as an unsigned key (the library's total_key)"""
    b = int(np.float32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def bound(lib, q, v, m, qinv, vinv, cosine, upper):
    P = C.POINTER(C.c_float)
    q = np.ascontiguousarray(q, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    return np.float32(lib.prune_bound(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, m, np.float32(qinv), np.float32(vinv),
                                      int(cosine), int(upper)))


def checkpoint(dim):
    nst = (dim + 3) // 4 * 4
    nst = (nst + 31) // 32
    c = nst * 7 // 8
    while c > 0 and c * 32 > dim - dim % 8:
        c -= 1
    return c * 32


def check_rows(lib, oracle, q, rows, where):
    """every row: score inside its bound both ways, and the gate decision at theta = the score's own ordinal and one on either
    side (prune iff ord(bound) < theta, strict) drops the row only when theta is above the row's ordinal"""
    dim = q.size
    m = checkpoint(dim)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    n_bounded = 0
    for i in range(rows.shape[0]):
        for cosine in (True, False):
            s = np.float32(oracle.cosine(q, rows[i], inv_q, inv_v[i]) if cosine else oracle.dot(q, rows[i]))
            for upper in (True, False):
                b = bound(lib, q, rows[i], m, inv_q, inv_v[i], cosine, upper)
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


@pytest.mark.parametrize("dim", [768, 769, 200, 64, 1030])
def test_uniform_rows(lib, oracle, dim):
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (300, dim)).astype(np.float32)
    assert check_rows(lib, oracle, q, rows, "uniform") == 4 * 300


@pytest.mark.parametrize("dim", [768, 200])
def test_tight_cauchy_schwarz_tails(lib, oracle, dim):
    """v_tail = alpha q_tail: Cauchy-Schwarz holds with equality — the bound must still hold, and stay close"""
    rng = np.random.default_rng(7)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    m = checkpoint(dim)
    rows = rng.uniform(-1, 1, (200, dim)).astype(np.float32)
    for i, alpha in enumerate(np.linspace(-3, 3, 200)):
        rows[i, m:] = (np.float32(alpha) * q[m:]).astype(np.float32)
    check_rows(lib, oracle, q, rows, "tight")
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(140, 200, 6):  # alpha >= 1.2: the upper bound is the tight one (a tail of little energy leaves the norm slack)
        s = oracle.dot(q, rows[i])
        b = bound(lib, q, rows[i], m, inv_q, inv_v[i], False, True)
        scale = float(np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(rows[i].astype(np.float64)))
        assert float(b) - float(s) <= 1e-3 * scale + 1e-3 * abs(float(s)), (i, s, b)


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-38, 1e-42, 1e10, 1e15, 1e18, 1e19, 3e20])
def test_subnormal_and_near_overflow_rows(lib, oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale) + 50))
    dim = 768
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (60, dim)) * scale).astype(np.float32)
    rows[::7, checkpoint(dim):] = 0.0
    check_rows(lib, oracle, q, rows, scale)
    qs = (q * np.float32(scale)).astype(np.float32)
    check_rows(lib, oracle, qs, rng.uniform(-1, 1, (30, dim)).astype(np.float32), ("query", scale))


def test_non_finite_inputs_claim_no_bound(lib, oracle):
    dim = 768
    m = checkpoint(dim)
    rng = np.random.default_rng(1)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (8, dim)).astype(np.float32)
    rows[0, 5] = np.nan           # NaN in the prefix
    rows[1, m + 3] = np.inf       # inf in the tail: the norm is inf, the inverse norm 0
    rows[2, m + 3] = np.nan       # NaN in the tail: the norm is NaN
    rows[3] = 0.0                 # zero row: inverse norm 0
    rows[4, :m] = 3e38            # the prefix overflows
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(5):
        for cosine in (True, False):
            for upper in (True, False):
                assert np.isnan(bound(lib, q, rows[i], m, inv_q, inv_v[i], cosine, upper)), (i, cosine, upper)
    # a query with a non-finite element, a zero query: no bound for any row
    for qq in (np.where(np.arange(dim) == 9, np.float32(np.inf), q), np.zeros(dim, np.float32)):
        qq = qq.astype(np.float32)
        assert np.isnan(bound(lib, qq, rows[5], m, 1.0, inv_v[5], False, True))
    # the stored inverse norm NaN / inf / 0
    for vinv in (np.nan, np.inf, 0.0, 1e-30):
        assert np.isnan(bound(lib, q, rows[5], m, inv_q, vinv, True, True)), vinv
    check_rows(lib, oracle, q, rows[5:], "finite")


def test_signed_zero_bounds(lib, oracle):
    """rows whose exact-order score is +0 or -0: the bound keeps the zero on the right side of total_cmp"""
    dim = 256
    m = checkpoint(dim)
    q = np.zeros(dim, np.float32)
    q[m:] = 1.0
    rows = np.zeros((4, dim), np.float32)
    rows[0, m] = 0.0
    rows[1, m] = -0.0
    rows[2, :m] = 1.0             # prefix energy, zero product with the query
    rows[3, :m] = -1.0
    rows[:, 0] = 1e-3
    check_rows(lib, oracle, q, rows, "zeros")
