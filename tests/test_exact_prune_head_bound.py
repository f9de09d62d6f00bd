"""CPU: the head of the four-bit tail sketch (otters_amd/csrc/ott_prune.h: prune_sketch4_head_row, DESIGN.md 3.1b, "no f32 stage in
front") — stage 0's codes with the line's cell width and rho_all over every stage — and the bound the head form of the sweep asks:
prune_score_bound_sketchq at m = 0, an all-zero acc, rho_all, K over all stages, against the oracle's bit-exact scores.  The header
is compiled on its own with the host compiler, as in test_exact_prune_sketchq_bound.py, whose case families these are.
  1. the head against a float64 restatement: the codes clamp, rho_all >= the true remainder over all stages (and is close to
     it), the line beside it is what it is without a head;
  2. every final score on the right side of its bound in f32::total_cmp order and the strict gate decision at the score's ordinal
     and one either side, Take Max and Take Min, cosine and dot;
  3. what only this form meets: NaN / inf / -0 in stage 0, a stage 0 that holds nearly the whole norm (every code clamps), a row
     that is zero outside stage 0, the queries that stress the quantiser;
  4. the prune rate at dim 768 against a float64 restatement of the new bound, the c = 1 form's rate beside it.
The GPU half is tests/test_gpu_exact_head.py; the sanitizer walk is tests/host/prune_head_walk.cpp."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from sketchq_queries import QUERY_KINDS, REFUSED, stress_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include <math.h>
#include "ott_prune.h"
using namespace ott;
static unsigned stages(unsigned dim) { return ((dim + 3) / 4 * 4 + 31) / 32; }
extern "C" unsigned hd_pitch(unsigned dim) { return prune_sketchb_pitch(stages(dim) - 1, 4); }
extern "C" void hd_line(const float* v, unsigned dim, unsigned* line) { prune_sketchb_row(v, dim, 32, stages(dim) - 1, 4, line); }
// a line of the caller's choosing: a and one code per tail dim; rho is the library's, for exactly these
extern "C" void hd_custom(const float* v, unsigned dim, float a, const int* codes, unsigned* line) {
    for (unsigned j = 0; j < hd_pitch(dim); j++) line[j] = 0u;
    PruneSketchSumsB t;
    for (unsigned i = 32; i < dim; i++) {
        line[4 + ((i - 32) >> 3)] |= ((unsigned)codes[i - 32] & 15u) << (4 * ((i - 32) & 7u));
        prune_sketchb_add(t, prune_f2u(v[i]), 2 * codes[i - 32] + 1);
    }
    float ao, rho;
    prune_sketchb_finish(t, a, &ao, &rho);
    line[0] = prune_f2u(ao);
    line[1] = prune_f2u(rho);
}
extern "C" float hd_head(const float* v, unsigned dim, const unsigned* line, unsigned* codes) {
    float rho_all;
    prune_sketch4_head_row(v, dim, stages(dim), line, codes, &rho_all);
    return rho_all;
}
static void planes_of(const float* q, unsigned dim, float inv_scale, unsigned nst, unsigned* planes) {
    for (unsigned i = 0; i < 4 * nst; i++) {
        float q8[8];
        for (unsigned j = 0; j < 8; j++) q8[j] = 8 * i + j < dim ? q[8 * i + j] : 0.0f;
        unsigned d3[3];
        prune_quant_word(q8, inv_scale, d3);
        for (unsigned d = 0; d < 3; d++) planes[(i >> 2) * 12 + d * 4 + (i & 3)] = d3[d];
    }
}
// the head form's bound of one row: the checkpoint in front of stage 0.  NaN = no bound claimed (or the query refused).  K_out: the kernel's K
extern "C" float hd_bound_line(const float* q, const float* v, unsigned dim, const unsigned* line, float qinv, float vinv, int cosine, int upper, int* K_out) {
    const unsigned nst = stages(dim);
    unsigned codes[4];
    const float rho_all = hd_head(v, dim, line, codes);
    double qt, qn;
    PruneQuant x;
    if (!prune_query_bounds(q, dim, 0, &qt, &qn) || !prune_query_quant(q, dim, 0, &x)) return NAN;
    unsigned planes[12 * 64];
    planes_of(q, dim, x.inv_scale, nst, planes);
    int K[3] = {0, 0, 0};
    for (unsigned s = 0; s < nst; s++) {
        const unsigned* w = s ? line + 4 + 4 * (s - 1) : codes;
        for (unsigned i = 0; i < 4; i++)
            for (unsigned d = 0; d < 3; d++) K[d] = prune_dot8_i4(w[i], planes[s * 12 + d * 4 + i], K[d]);
    }
    const int Kk = 2 * (256 * K[2] + 16 * K[1] + K[0]) + x.qsum;
    if (K_out) *K_out = Kk;
    const float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return prune_score_bound_sketchq(acc, vinv, prune_u2f(line[0]), rho_all, Kk, x.scale, dim, qt, x.qe1, qn, qinv, cosine != 0, upper != 0);
}
extern "C" float hd_bound(const float* q, const float* v, unsigned dim, float qinv, float vinv, int cosine, int upper) {
    unsigned line[4 + 4 * 64];
    hd_line(v, dim, line);
    return hd_bound_line(q, v, dim, line, qinv, vinv, cosine, upper, nullptr);
}
// the c = 1 form on the same line: stage 0 in f32, prune_score_bound_sketchq with m = 32 (the prune rate's companion figure)
extern "C" float c1_bound(const float* q, const float* v, unsigned dim, float qinv, float vinv, int cosine, int upper) {
    const unsigned nst = stages(dim), m = 32;
    unsigned line[4 + 4 * 64];
    hd_line(v, dim, line);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned c = 0; c < m; c += 8)
        for (int l = 0; l < 8; l++) {
            volatile float prod = q[c + l] * v[c + l];
            acc[l] = acc[l] + prod;
        }
    double qt, qn;
    PruneQuant x;
    if (!prune_query_bounds(q, dim, m, &qt, &qn) || !prune_query_quant(q, dim, m, &x)) return NAN;
    unsigned planes[12 * 64];
    planes_of(q, dim, x.inv_scale, nst, planes);
    int K[3] = {0, 0, 0};
    for (unsigned s = 1; s < nst; s++)
        for (unsigned i = 0; i < 4; i++)
            for (unsigned d = 0; d < 3; d++) K[d] = prune_dot8_i4(line[4 + 4 * (s - 1) + i], planes[s * 12 + d * 4 + i], K[d]);
    return prune_score_bound_sketchq(acc, vinv, prune_u2f(line[0]), prune_u2f(line[1]), 2 * (256 * K[2] + 16 * K[1] + K[0]) + x.qsum, x.scale, dim, qt, x.qe1, qn, qinv,
                                     cosine != 0, upper != 0);
}
// per row: the head form's bound, the c = 1 form's, and for the float64 restatement a, rho_all and K
extern "C" void rate_rows(const float* q, const float* rows, unsigned long long n, unsigned dim, float qinv, const float* vinv, float* out_h, float* out_c, float* a,
                          float* rho_all, int* K) {
    for (unsigned long long r = 0; r < n; r++) {
        const float* v = rows + r * dim;
        unsigned line[4 + 4 * 64], codes[4];
        hd_line(v, dim, line);
        out_h[r] = hd_bound_line(q, v, dim, line, qinv, vinv[r], 1, 1, K + r);
        out_c[r] = c1_bound(q, v, dim, qinv, vinv[r], 1, 1);
        a[r] = prune_u2f(line[0]);
        rho_all[r] = hd_head(v, dim, line, codes);
    }
}
// o: e, qsum; f: scale, inv_scale; d: qe1, qt, qn (m = 0)
extern "C" int hd_quant(const float* q, unsigned dim, int* o, float* f, double* d) {
    PruneQuant x;
    if (!prune_query_quant(q, dim, 0, &x) || !prune_query_bounds(q, dim, 0, d + 1, d + 2)) return 0;
    o[0] = x.e; o[1] = x.qsum; f[0] = x.scale; f[1] = x.inv_scale; d[0] = x.qe1;
    return 1;
}
"""

P = C.POINTER(C.c_float)
PU = C.POINTER(C.c_uint32)
PI = C.POINTER(C.c_int32)
LO, HI = -8, 7
DIMS = [225, 256, 768, 773, 896]
FIRST = 32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("head")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    u, i, f = C.c_uint, C.c_int, C.c_float
    for name, args, res in (("hd_pitch", [u], u), ("hd_line", [P, u, PU], None), ("hd_custom", [P, u, f, PI, PU], None), ("hd_head", [P, u, PU, PU], f),
                            ("hd_bound_line", [P, P, u, PU, f, f, i, i, PI], f), ("hd_bound", [P, P, u, f, f, i, i], f), ("c1_bound", [P, P, u, f, f, i, i], f),
                            ("rate_rows", [P, P, C.c_ulonglong, u, f, P, P, P, P, P, PI], None), ("hd_quant", [P, u, PI, P, C.POINTER(C.c_double)], i)):
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, res
    return L


def tkey(x):
    """f32::total_cmp as an unsigned key (the library's total_key)"""
    b = int(np.float32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def line_of(lib, v):
    v = np.ascontiguousarray(v, np.float32)
    line = np.zeros(lib.hd_pitch(v.size), np.uint32)
    lib.hd_line(v.ctypes.data_as(P), v.size, line.ctypes.data_as(PU))
    return line


def custom(lib, v, a, codes):
    v = np.ascontiguousarray(v, np.float32)
    codes = np.ascontiguousarray(codes, np.int32)
    assert codes.size == v.size - FIRST
    line = np.zeros(lib.hd_pitch(v.size), np.uint32)
    lib.hd_custom(v.ctypes.data_as(P), v.size, np.float32(a), codes.ctypes.data_as(PI), line.ctypes.data_as(PU))
    return line


def head_of(lib, v, line):
    v = np.ascontiguousarray(v, np.float32)
    codes = np.zeros(4, np.uint32)
    rho_all = lib.hd_head(v.ctypes.data_as(P), v.size, line.ctypes.data_as(PU), codes.ctypes.data_as(PU))
    return codes, np.float32(rho_all)


def unpack(words, n):
    f = (words.astype(np.int64)[:, None] >> (4 * np.arange(8))[None, :]) & 15
    return np.where(f >= 8, f - 16, f).reshape(-1)[:n]


def bound(lib, q, v, qinv, vinv, cosine, upper, line=None):
    q = np.ascontiguousarray(q, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    if line is None:
        return np.float32(lib.hd_bound(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, np.float32(qinv), np.float32(vinv), int(cosine), int(upper)))
    return np.float32(lib.hd_bound_line(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, line.ctypes.data_as(PU), np.float32(qinv), np.float32(vinv), int(cosine),
                                        int(upper), None))


def check_rows(lib, oracle, q, rows, where, metrics=(True, False), lines=None):
    """every row, cosine and dot, Max and Min: the score inside its bound, and the gate decision at theta = the score's own ordinal
    and one on either side (prune iff ord(bound) < theta, strict) drops the row only when theta is above the row's ordinal"""
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    n_bounded = 0
    for i in range(rows.shape[0]):
        for cosine in metrics:
            s = np.float32(oracle.cosine(q, rows[i], inv_q, inv_v[i]) if cosine else oracle.dot(q, rows[i]))
            for upper in (True, False):
                b = bound(lib, q, rows[i], inv_q, inv_v[i], cosine, upper, None if lines is None else lines[i])
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


# ---- 1. the head against a float64 restatement ------------------------------------------------------------------------------------------
def head64(v, line):
    """stage 0's codes with the line's cell width (f32 product, floor, clamp; the width from the tail's largest finite magnitude as
    prune_sketchb_scale takes it) and the true remainder over all stages for the stored a and codes, in float64"""
    dim = v.size
    a = float(line[:1].view(np.float32)[0])
    tail = np.abs(v[FIRST:])
    vmax = np.float32(tail[np.isfinite(tail)].max()) if np.isfinite(tail).any() and tail.size else np.float32(0)
    delta = np.float32(vmax / np.float32(8))
    with np.errstate(divide="ignore", over="ignore"):
        inv = np.float32(1) / delta if delta > 0 else np.float32(0)
    if not inv <= np.float32(3.4028234e38):
        inv = np.float32(3.4028234e38)
    n0 = min(FIRST, dim)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.floor((v[:n0] * inv).astype(np.float32))
    code0 = np.where(np.isnan(t), 0, np.clip(t, LO, HI)).astype(np.int64)
    nst = ((dim + 3) // 4 * 4 + 31) // 32
    codes = np.concatenate([code0, unpack(line[4:4 + 4 * (nst - 1)], dim - FIRST)])
    res = v.astype(np.float64) - a * (2 * codes + 1)
    return code0, float(np.sqrt(np.sum(res * res)))


@pytest.mark.parametrize("dim", DIMS)
def test_head_against_a_float64_restatement(lib, dim):
    rng = np.random.default_rng(dim + 40)
    rows = rng.uniform(-1, 1, (80, dim)).astype(np.float32)
    rows[20:40] = rng.normal(0, 1, (20, dim)).astype(np.float32)
    rows[40:50, :FIRST] *= np.geomspace(2, 1e4, 10, dtype=np.float32)[:, None]  # stage 0 beyond the tail's +-max: the codes clamp
    rows[50:55, FIRST:] = 0.0  # zero outside stage 0: a = 0, every kappa = 1 with nothing to scale
    rows[55, :] = 0.0
    rows[56, 3] = -0.0
    rows[57, :FIRST] = -0.0
    clamped = 0
    for i in range(rows.shape[0]):
        line = line_of(lib, rows[i])
        before = line.copy()
        codes, rho_all = head_of(lib, rows[i], line)
        assert np.array_equal(line, before) and np.array_equal(line, line_of(lib, rows[i]))  # the line beside it is unchanged
        code0, true = head64(rows[i], line)
        got = unpack(codes, 32)
        assert np.array_equal(got[:min(32, dim)], code0), (dim, i, got, code0)
        assert got.min() >= LO and got.max() <= HI
        clamped += int(np.count_nonzero(np.abs(rows[i, :FIRST]) > np.abs(rows[i, FIRST:]).max()))
        rho = float(line[1:2].view(np.float32)[0])
        assert np.isfinite(rho_all) and float(rho_all) >= true and float(rho_all) >= rho * (1 - 1e-6), (dim, i, rho_all, true, rho)
        # (the slack: 2^-34 of the magnitudes under the root, 2^-30 on it, one rounding up)
        mag = float(np.sqrt(np.sum(rows[i].astype(np.float64) ** 2) + dim * (15 * float(line[:1].view(np.float32)[0])) ** 2))
        assert float(rho_all) <= true * (1 + 1e-6) + mag * 2.0 ** -16, (dim, i, rho_all, true)
    assert clamped > 100


def test_head_past_dim_holds_code_zero(lib):
    """dim < 32 never reaches a four-bit store (two stages at least); dim 225: the tail's last stage is one dim, stage 0 is whole"""
    v = np.random.default_rng(5).uniform(-1, 1, 225).astype(np.float32)
    line = line_of(lib, v)
    codes, _ = head_of(lib, v, line)
    assert np.array_equal(unpack(codes, 32), head64(v, line)[0])


# ---- 2. the bound on the case families of the integer decode's file ---------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["uniform", "gauss"])
def test_uniform_and_gaussian_rows(lib, oracle, dim, kind):
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (120, dim)) if kind == "uniform" else rng.normal(0, 1, (120, dim))).astype(np.float32)
    assert check_rows(lib, oracle, q, rows, kind) == 4 * 120


@pytest.mark.parametrize("dim", DIMS)
def test_rows_on_the_reconstruction_levels(lib, oracle, dim):
    """every dim, stage 0 included, on a reconstruction level a kappa: rho_all ~ a, the bound is the score up to the half width"""
    rng = np.random.default_rng(dim + 1)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = np.empty((60, dim), np.float32)
    levels = np.arange(-15, 16, 2).astype(np.float32)
    for i, a in enumerate(np.geomspace(1e-3, 8.0, 60)):
        a = np.float32(2.0 ** np.round(np.log2(a)))
        rows[i] = a * rng.choice(levels, dim)
        rows[i, FIRST + 1] = np.float32(16) * a
    assert check_rows(lib, oracle, q, rows, "levels") == 4 * 60
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    o, f, d = (C.c_int32 * 2)(), (C.c_float * 2)(), (C.c_double * 3)()
    assert lib.hd_quant(q.ctypes.data_as(P), dim, o, f, d)
    for i in range(0, 60, 7):
        line = line_of(lib, rows[i])
        a = float(line[:1].view(np.float32)[0])
        rho_all = float(head_of(lib, rows[i], line)[1])
        s = float(oracle.dot(q, rows[i]))
        scale = float(np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(rows[i].astype(np.float64)))
        width = d[1] * rho_all + a * 15 * d[0]
        up = float(bound(lib, q, rows[i], inv_q, inv_v[i], False, True))
        lo = float(bound(lib, q, rows[i], inv_q, inv_v[i], False, False))
        assert up - s <= 2 * width + 1e-3 * scale and s - lo <= 2 * width + 1e-3 * scale, (i, lo, s, up)


@pytest.mark.parametrize("dim", [768, 225])
@pytest.mark.parametrize("align", [1, -1])
def test_rows_aligned_with_and_against_the_query_signs(lib, oracle, dim, align):
    rng = np.random.default_rng(11 + align)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (100, dim)).astype(np.float32)
    sgn = np.where(np.signbit(q), np.float32(-1), np.float32(1)) * np.float32(align)
    rows = np.abs(rows) * sgn
    rows[50:] *= np.geomspace(1e-2, 30, 50, dtype=np.float32)[:, None]
    rows[90:] = sgn * np.float32(0.999)  # every code at the range's edge: |kappa| = 15 throughout, stage 0 included
    line = line_of(lib, rows[95])
    assert np.all(np.abs(2 * unpack(head_of(lib, rows[95], line)[0], 32) + 1) == 15)
    assert check_rows(lib, oracle, q, rows, ("aligned", align)) == 4 * 100


@pytest.mark.parametrize("dim", [768, 773])
def test_clipped_outliers_and_any_a_with_its_own_rho(lib, oracle, dim):
    """lines of the test's choosing (any a, any codes): rho_all is taken for what is stored, so the bound holds whatever it is"""
    rng = np.random.default_rng(dim + 5)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.normal(0, 1, (40, dim)).astype(np.float32)
    rows[:, FIRST + 7] = 40.0
    rows[::2, dim - 2] = -55.0
    rows[::3, 4] = 70.0  # an outlier in stage 0 as well
    lines = []
    for i in range(rows.shape[0]):
        tail = rows[i, FIRST:].astype(np.float64)
        delta = [np.quantile(np.abs(tail), 0.9) / 8, 1e-6, 1e6, np.abs(tail).max() / 8, 0.3][i % 5]
        code = np.clip(np.floor(tail / delta), LO, HI).astype(np.int32)
        if i % 7 == 3:
            code = rng.integers(LO, HI + 1, tail.size).astype(np.int32)
        if i % 7 == 5:
            code = np.clip(code + 1, LO, HI).astype(np.int32)
        lines.append(custom(lib, rows[i], 0.0 if i % 11 == 10 else delta / 2, code))
    assert check_rows(lib, oracle, q, rows, "custom", lines=lines) == 4 * 40
    assert check_rows(lib, oracle, q, rows, "outliers") == 4 * 40


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-38, 1e-42, 1e10, 1e15, 1e18, 1e19, 3e20])
def test_subnormal_and_near_overflow_scales(lib, oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale) + 50))
    dim = 768
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (40, dim)) * scale).astype(np.float32)
    rows[::7, FIRST:] = 0.0
    check_rows(lib, oracle, q, rows, scale)
    qs = (q * np.float32(scale)).astype(np.float32)  # (a query the quantiser or prune_query_bounds refuses claims no bound)
    n = check_rows(lib, oracle, qs, rng.uniform(-1, 1, (20, dim)).astype(np.float32), ("query", scale))
    assert (n > 0) == (1e-30 <= scale <= 1e10), (scale, n)
    big = (rng.uniform(-1, 1, (8, dim)) * 3e38).astype(np.float32)  # sums that leave the f32 range: rho_all = +inf, no bound
    assert check_rows(lib, oracle, q, big, "overflow") == 0
    big0 = rng.uniform(-1, 1, (8, dim)).astype(np.float32)  # ... from stage 0 alone
    big0[:, :FIRST] = (rng.uniform(0.5, 1, (8, FIRST)) * 3e38).astype(np.float32)
    assert check_rows(lib, oracle, q, big0, "overflow in stage 0") == 0


# ---- 3. what only this form meets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [768, 225])
def test_nan_inf_and_signed_zeros_in_stage_0(lib, oracle, dim):
    rng = np.random.default_rng(3)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (14, dim)).astype(np.float32)
    rows[0, 3] = np.nan
    rows[1, 0] = np.inf
    rows[2, 31] = -np.inf
    rows[3, FIRST + 3] = np.nan  # (the tail's: the line has no bound, so the head has none)
    rows[4, dim - 1] = np.inf
    rows[5] = 0.0
    rows[6, :FIRST] = 0.0
    rows[7, :FIRST] = -0.0
    rows[8, :FIRST:2] = -0.0
    rows[9, 1:FIRST:2] = 0.0
    rows[10, FIRST:] = -0.0
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(6):
        if i < 5:
            assert head_of(lib, rows[i], line_of(lib, rows[i]))[1] == np.inf, i
        for cosine in (True, False):
            for upper in (True, False):
                assert np.isnan(bound(lib, q, rows[i], inv_q, inv_v[i], cosine, upper)), (i, cosine, upper)
    assert check_rows(lib, oracle, q, rows[6:], "zeros") == 4 * 8
    for qq in (np.where(np.arange(dim) == 9, np.float32(np.inf), q), np.where(np.arange(dim) == dim - 1, np.float32(np.nan), q), np.zeros(dim, np.float32)):
        assert np.isnan(bound(lib, qq.astype(np.float32), rows[11], 1.0, inv_v[11], False, True))
    for vinv in (np.nan, np.inf, 0.0, 1e-30):
        assert np.isnan(bound(lib, q, rows[11], inv_q, vinv, True, True)), vinv
    qz = np.zeros(dim, np.float32)  # scores that are +0 / -0: a query that only sees stage 0, rows whose stage 0 is a zero of either sign
    qz[:FIRST] = 1.0
    z = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    z[0, :FIRST] = 0.0
    z[1, :FIRST] = -0.0
    z[2, :FIRST:2] = -0.0
    z[2, 1:FIRST:2] = 0.0
    assert check_rows(lib, oracle, qz, z, "signed zero scores") == 4 * 3


@pytest.mark.parametrize("dim", [768, 773, 225])
def test_a_stage_0_that_holds_nearly_the_whole_norm(lib, oracle, dim):
    """stage 0 far beyond the tail's max: every code of the head clamps to -8 or 7, rho_all is nearly the row's norm, and the bound
    is a weak one — but a bound"""
    rng = np.random.default_rng(dim + 9)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    rows[:, :FIRST] *= np.geomspace(1e2, 1e12, 40, dtype=np.float32)[:, None]
    rows[:, :FIRST] += np.sign(rows[:, :FIRST]) * np.float32(100)
    for i in (0, 20, 39):
        line = line_of(lib, rows[i])
        codes, rho_all = head_of(lib, rows[i], line)
        assert set(unpack(codes, 32).tolist()) <= {LO, HI}
        n0 = float(np.linalg.norm(rows[i, :FIRST].astype(np.float64)))
        assert 0.9 * n0 <= float(rho_all) <= 1.001 * float(np.linalg.norm(rows[i].astype(np.float64)))
    assert check_rows(lib, oracle, q, rows, "stage 0 dominates") == 4 * 40


@pytest.mark.parametrize("dim", [768, 256])
def test_a_row_that_is_zero_outside_stage_0(lib, oracle, dim):
    """the tail's max is 0: the cell width is 0, a = 0, every code 0; rho_all is the row's norm"""
    rng = np.random.default_rng(dim + 13)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = np.zeros((30, dim), np.float32)
    rows[:, :FIRST] = rng.uniform(-1, 1, (30, FIRST)).astype(np.float32) * np.geomspace(1e-30, 1e15, 30, dtype=np.float32)[:, None]
    rows[3, FIRST:] = -0.0
    for i in (0, 3, 29):
        line = line_of(lib, rows[i])
        codes, rho_all = head_of(lib, rows[i], line)
        assert line[0] == 0 and not codes.any()
        n = float(np.linalg.norm(rows[i].astype(np.float64)))
        assert n <= float(rho_all) <= n * (1 + 1e-4) + 1e-37
    assert check_rows(lib, oracle, q, rows, "zero tail") > 0


@pytest.mark.parametrize("kind", QUERY_KINDS)
@pytest.mark.parametrize("dim", [256, 773])
def test_queries_that_stress_the_quantiser(lib, oracle, dim, kind):
    rng = np.random.default_rng(dim + 31)
    q = stress_query(kind, dim)
    rows = rng.uniform(-1, 1, (60, dim)).astype(np.float32)
    rows[40:] = rng.normal(0, 1, (20, dim)).astype(np.float32)
    o, f, d = (C.c_int32 * 2)(), (C.c_float * 2)(), (C.c_double * 3)()
    ok = lib.hd_quant(q.ctypes.data_as(P), dim, o, f, d)
    if kind in REFUSED:
        assert not ok and check_rows(lib, oracle, q, rows, kind) == 0
        return
    assert ok and d[1] == d[2]  # m = 0: qt is qn
    if kind == "zero_tail":  # (the tail is zero, stage 0 is not: the whole query's sum and error)
        assert o[1] != 0
    inv_q = float(oracle.inv_norms(q[None, :])[0])
    assert check_rows(lib, oracle, q, rows, kind) == (2 if kind == "max_2^-100" else 4) * 60


# ---- 4. the prune rate ------------------------------------------------------------------------------------------------------------------
def test_prune_rate_against_a_float64_restatement(lib, oracle):
    """dim 768, the gate at the 10th best of 100k uniform rows, cosine, Take Max.  The rate of the head form's bound is held to a
    float64 restatement of it — (a 2^e K + 15 a qe1 + ||q|| rho_all) / (||q|| ||v||) against the gate's score — with the allowance
    of the other bound files, 0.25 point.  The c = 1 form's rate on the same inputs (stage 0 in f32, prune_score_bound_sketchq
    with m = 32: 97.775 %) is printed beside it: the head form gives up the difference for reading no f32 stage."""
    dim, n, k = 768, 100_000, 10
    rng = np.random.default_rng(2024)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = np.ascontiguousarray(oracle.inv_norms(rows), np.float32)
    top = oracle.vec_query(rows, q, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, 0, 0.0, ties=oracle.TIES_CANONICAL)
    gate = tkey(top["score"][k - 1])
    out_h, out_c, a, rho_all = (np.empty(n, np.float32) for _ in range(4))
    K = np.empty(n, np.int32)
    lib.rate_rows(q.ctypes.data_as(P), rows.ctypes.data_as(P), n, dim, np.float32(inv_q), inv_v.ctypes.data_as(P), out_h.ctypes.data_as(P), out_c.ctypes.data_as(P),
                  a.ctypes.data_as(P), rho_all.ctypes.data_as(P), K.ctypes.data_as(PI))
    dropped = []
    for out in (out_h, out_c):
        assert not np.isnan(out).any()
        b = out.view(np.uint32).astype(np.int64)
        keys = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
        assert set(int(i) for i in top["index"]).isdisjoint(np.flatnonzero(keys < gate).tolist())
        dropped.append(int(np.count_nonzero(keys < gate)))
    o, f, d = (C.c_int32 * 2)(), (C.c_float * 2)(), (C.c_double * 3)()
    assert lib.hd_quant(q.ctypes.data_as(P), dim, o, f, d)
    qn = float(np.linalg.norm(q.astype(np.float64)))
    vn = np.linalg.norm(rows.astype(np.float64), axis=1)
    b64 = (a.astype(np.float64) * float(f[0]) * K + 15.0 * a.astype(np.float64) * d[0] + qn * rho_all.astype(np.float64)) / (qn * vn)
    dropped64 = int(np.count_nonzero(b64 < float(top["score"][k - 1])))
    print(f"dim {dim}, gate at the 10th best of {n}: the head form (checkpoint 0) drops {100.0 * dropped[0] / n:.3f} %, its float64 restatement "
          f"{100.0 * dropped64 / n:.3f} %, the c = 1 form {100.0 * dropped[1] / n:.3f} %")
    assert abs(dropped64 - dropped[0]) <= n * 25 // 10000, (dropped, dropped64)
