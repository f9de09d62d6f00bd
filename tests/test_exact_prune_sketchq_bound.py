"""CPU: the integer decode of the four-bit tail sketch (otters_amd/csrc/ott_prune.h, DESIGN.md 3.1b, "the integer decode") — the
quantised query, its base-16 digit planes, the signed 4-bit dot products and prune_score_bound_sketchq — against the oracle's
bit-exact scores.  The header is compiled on its own with the host compiler, as in test_exact_prune_sketch4_bound.py; a small
driver makes a row's line with the library's own prune_sketchb_row (or a line of the test's choosing), computes the kernel's
checkpoint state — the eight partial chains after m dims and K = 2 (256 K2 + 16 K1 + K0) + sum qhat from twelve nibble-wise dot
products per piece over the digit planes prune_quant_word packs — and asks prune_score_bound_sketchq.
  1. digits: every qhat in [-1911, 1911] has digits in [-8, 7] that reconstruct it;
  2. the dot restatement over packed words equals sum qhat_i kappa_i computed directly;
  3. every final score on the right side of its bound in f32::total_cmp order, and the strict gate decision, on the case families
     of the four-bit file and on queries that stress the quantiser;
  4. where the quantiser refuses a query the plan (ott_exact_plan.h) does not choose the four-bit form;
  5. the prune rate against prune_score_bound_sketchb's on the same inputs.
The GPU half is tests/test_gpu_exact_sketch4_int.py; the sanitizer walk is tests/host/prune_quant_walk.cpp."""
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
#include "ott_exact_plan.h"
#include "ott_prune.h"
using namespace ott;
extern "C" unsigned sq_pitch(unsigned n_stages) { return prune_sketchb_pitch(n_stages, 4); }
extern "C" void sq_row(const float* v, unsigned dim, unsigned first, unsigned n_stages, unsigned* line) { prune_sketchb_row(v, dim, first, n_stages, 4, line); }
// a line of the caller's choosing: a and one code per tail dim; rho is the library's, for exactly these
extern "C" void sq_custom(const float* v, unsigned dim, unsigned first, unsigned n_stages, float a, const int* codes, unsigned* line) {
    for (unsigned j = 0; j < prune_sketchb_pitch(n_stages, 4); j++) line[j] = 0u;
    PruneSketchSumsB t;
    for (unsigned i = first; i < dim; i++) {
        line[4 + ((i - first) >> 3)] |= ((unsigned)codes[i - first] & 15u) << (4 * ((i - first) & 7u));
        prune_sketchb_add(t, prune_f2u(v[i]), 2 * codes[i - first] + 1);
    }
    float ao, rho;
    prune_sketchb_finish(t, a, &ao, &rho);
    line[0] = prune_f2u(ao);
    line[1] = prune_f2u(rho);
}
extern "C" int sq_q(float q, float inv_scale) { return prune_quant_q(q, inv_scale); }
extern "C" void sq_digits(int qhat, int* d) { prune_quant_digits(qhat, d); }
// o: e, qsum; f: scale, inv_scale; d: qe1
extern "C" int sq_quant(const float* q, unsigned dim, unsigned m, int* o, float* f, double* d) {
    PruneQuant x;
    if (!prune_query_quant(q, dim, m, &x)) return 0;
    o[0] = x.e; o[1] = x.qsum; f[0] = x.scale; f[1] = x.inv_scale; d[0] = x.qe1;
    return 1;
}
// the digit planes as the kernel keeps them: [stage][digit][word], stages 0 .. nst - 1
extern "C" void sq_planes(const float* q, unsigned dim, float inv_scale, unsigned nst, unsigned* planes) {
    for (unsigned i = 0; i < 4 * nst; i++) {
        float q8[8];
        for (unsigned j = 0; j < 8; j++) q8[j] = 8 * i + j < dim ? q[8 * i + j] : 0.0f;
        unsigned d3[3];
        prune_quant_word(q8, inv_scale, d3);
        for (unsigned d = 0; d < 3; d++) planes[(i >> 2) * 12 + d * 4 + (i & 3)] = d3[d];
    }
}
// the kernel's K: per piece twelve dot products into three sums, then 2 (256 K2 + 16 K1 + K0) + qsum.  o: K0, K1, K2
extern "C" int sq_K(const unsigned* line, const unsigned* planes, unsigned first, unsigned m, unsigned nst, int qsum, int* o) {
    int K[3] = {0, 0, 0};
    for (unsigned s = m / 32; s < nst; s++) {
        const unsigned* w = line + 4 + 4 * (s - first / 32);
        for (unsigned i = 0; i < 4; i++)
            for (unsigned d = 0; d < 3; d++) K[d] = prune_dot8_i4(w[i], planes[s * 12 + d * 4 + i], K[d]);
    }
    if (o) { o[0] = K[0]; o[1] = K[1]; o[2] = K[2]; }
    return 2 * (256 * K[2] + 16 * K[1] + K[0]) + qsum;
}
// the bound of one row from its line at the checkpoint m >= first (both multiples of 32); NaN = no bound claimed (or the query refused)
extern "C" float sq_bound_line(const float* q, const float* v, unsigned dim, unsigned first, unsigned m, const unsigned* line, float qinv, float vinv,
                               int cosine, int upper) {
    const unsigned nst = ((dim + 3) / 4 * 4 + 31) / 32;
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
    sq_planes(q, dim, x.inv_scale, nst, planes);
    const int K = sq_K(line, planes, first, m, nst, x.qsum, nullptr);
    return prune_score_bound_sketchq(acc, vinv, prune_u2f(line[0]), prune_u2f(line[1]), K, x.scale, dim, qt, x.qe1, qn, qinv, cosine != 0, upper != 0);
}
extern "C" float sq_bound(const float* q, const float* v, unsigned dim, unsigned first, unsigned m, float qinv, float vinv, int cosine, int upper) {
    const unsigned nst = ((dim + 3) / 4 * 4 + 31) / 32;
    uint32_t line[4 + 4 * 64];
    prune_sketchb_row(v, dim, first, nst - first / 32, 4, line);
    return sq_bound_line(q, v, dim, first, m, line, qinv, vinv, cosine, upper);
}
// today's form on the same line: the f32 chain D and prune_score_bound_sketchb with kmax = 15 (the prune rate's reference)
extern "C" float sb_bound(const float* q, const float* v, unsigned dim, unsigned first, float qinv, float vinv, int cosine, int upper) {
    const unsigned nst = ((dim + 3) / 4 * 4 + 31) / 32, m = first;
    uint32_t line[4 + 4 * 64];
    prune_sketchb_row(v, dim, first, nst - first / 32, 4, line);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned c = 0; c < m; c += 8)
        for (int l = 0; l < 8; l++) {
            volatile float prod = q[c + l] * v[c + l];
            acc[l] = acc[l] + prod;
        }
    float D = 0.0f;
    for (unsigned s = m / 32; s < nst; s++)
        for (unsigned b = 0; b < 32; b++) {
            const int code = prune_sketchb_code(line + 4 + 4 * (s - first / 32), b, 4);
            const unsigned i = 32 * s + b;
            D = fmaf((float)(2 * code + 1), i < dim ? q[i] : 0.0f, D);
        }
    double qt, qn;
    if (!prune_query_bounds(q, dim, m, &qt, &qn)) return NAN;
    return prune_score_bound_sketchb(acc, vinv, prune_u2f(line[0]), prune_u2f(line[1]), D, 15.0, m, dim, qt, prune_query_l1(q, dim, m), qn, qinv, cosine != 0, upper != 0);
}
extern "C" void both_bound_rows(const float* q, const float* rows, unsigned long long n, unsigned dim, unsigned first, float qinv, const float* vinv, float* out_q,
                                float* out_b) {
    for (unsigned long long r = 0; r < n; r++) {
        out_q[r] = sq_bound(q, rows + r * dim, dim, first, first, qinv, vinv[r], 1, 1);
        out_b[r] = sb_bound(q, rows + r * dim, dim, first, qinv, vinv[r], 1, 1);
    }
}
// the plan of a four-bit store of `rows` rows x dim for this query, as plan_pruned_sweep (ott_api.hip) takes it.  o: c, sketch, seed, quantiser accepted
extern "C" void sq_plan(const float* q, unsigned dim, unsigned long long rows, unsigned long long* o) {
    const unsigned ld = (dim + 3) / 4 * 4, nst = (ld + 31) / 32;
    const PruneIn in{dim, ld, OTT_METRIC_COSINE, false, true, false, 0, 1, 1, SketchState{true, true, 4, 4 * (nst - 1), prune_sketchb_stage0(nst, 4)}, rows, 1};
    PrunePlan pp = prune_plan(in);
    PruneQuant x;
    bool ok = true;
    if (prune_plan_needs_quant(in, pp) && !(ok = prune_query_quant(q, dim, pp.c * 32, &x))) pp = prune_plan_quant_refused(in);
    o[0] = pp.c; o[1] = pp.sketch; o[2] = pp.seed; o[3] = ok;
}
"""

P = C.POINTER(C.c_float)
PU = C.POINTER(C.c_uint32)
PI = C.POINTER(C.c_int32)
QMAX = 1911
LO, HI = -8, 7


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sketchq")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    u, i, f = C.c_uint, C.c_int, C.c_float
    for name, args, res in (("sq_pitch", [u], u), ("sq_row", [P, u, u, u, PU], None), ("sq_custom", [P, u, u, u, f, PI, PU], None), ("sq_q", [f, f], i),
                            ("sq_digits", [i, PI], None), ("sq_quant", [P, u, u, PI, P, C.POINTER(C.c_double)], i), ("sq_planes", [P, u, f, u, PU], None),
                            ("sq_K", [PU, PU, u, u, u, i, PI], i), ("sq_bound_line", [P, P, u, u, u, PU, f, f, i, i], f),
                            ("sq_bound", [P, P, u, u, u, f, f, i, i], f), ("sb_bound", [P, P, u, u, f, f, i, i], f),
                            ("both_bound_rows", [P, P, C.c_ulonglong, u, u, f, P, P, P], None), ("sq_plan", [P, u, C.c_ulonglong, C.POINTER(C.c_ulonglong)], None)):
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, res
    return L


def tkey(x):
    """f32::total_cmp as an unsigned key (the library's total_key)"""
    b = int(np.float32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def geometry(dim):
    """stages, the sketch's first dim (= the checkpoint: stage 1), its sketched stages"""
    nst = ((dim + 3) // 4 * 4 + 31) // 32
    return nst, 32, nst - 1


def sketch(lib, v, dim):
    _, first, n_st = geometry(dim)
    v = np.ascontiguousarray(v, np.float32)
    line = np.zeros(lib.sq_pitch(n_st), np.uint32)
    lib.sq_row(v.ctypes.data_as(P), dim, first, n_st, line.ctypes.data_as(PU))
    return line


def custom(lib, v, a, codes):
    _, first, n_st = geometry(v.size)
    v = np.ascontiguousarray(v, np.float32)
    codes = np.ascontiguousarray(codes, np.int32)
    assert codes.size == v.size - first
    line = np.zeros(lib.sq_pitch(n_st), np.uint32)
    lib.sq_custom(v.ctypes.data_as(P), v.size, first, n_st, np.float32(a), codes.ctypes.data_as(PI), line.ctypes.data_as(PU))
    return line


def codes_of(line, n_st, n_dims):
    w = line[4:4 + 4 * n_st].astype(np.int64).reshape(n_st, 4)
    f = (w[:, :, None] >> (4 * np.arange(8))[None, None, :]) & 15
    return np.where(f >= 8, f - 16, f).reshape(-1)[:n_dims]


def quant(lib, q, m):
    """the host function: None where it refuses, else (e, qsum, scale, inv_scale, qe1)"""
    q = np.ascontiguousarray(q, np.float32)
    o, f, d = (C.c_int32 * 2)(), (C.c_float * 2)(), (C.c_double * 1)()
    if not lib.sq_quant(q.ctypes.data_as(P), q.size, m, o, f, d):
        return None
    return int(o[0]), int(o[1]), np.float32(f[0]), np.float32(f[1]), float(d[0])


def qhat_of(lib, q, inv_scale):
    return np.array([lib.sq_q(np.float32(x), np.float32(inv_scale)) for x in q], np.int64)


def bound(lib, q, v, qinv, vinv, cosine, upper, line=None):
    q = np.ascontiguousarray(q, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    _, first, _ = geometry(q.size)
    if line is None:
        return np.float32(lib.sq_bound(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, first, first, np.float32(qinv), np.float32(vinv), int(cosine), int(upper)))
    return np.float32(lib.sq_bound_line(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, first, first, line.ctypes.data_as(PU), np.float32(qinv), np.float32(vinv),
                                        int(cosine), int(upper)))


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


DIMS = [225, 256, 768, 773, 896]


# ---- 1. digits ------------------------------------------------------------------------------------------------------------------------
def test_every_qhat_has_balanced_digits(lib):
    d = (C.c_int32 * 3)()
    for qhat in range(-QMAX, QMAX + 1):
        lib.sq_digits(qhat, d)
        assert all(LO <= x <= HI for x in d), (qhat, list(d))
        assert 256 * d[2] + 16 * d[1] + d[0] == qhat, (qhat, list(d))
    assert QMAX == 7 * 256 + 7 * 16 + 7


def test_quantiser_scale_rounding_and_clamp(lib):
    """the smallest power of two with max |q| 2^-e <= 1911; round to nearest even; clamped; an underflowing product gives 0"""
    for mx, e in ((1.0, -10), (1911.0, 0), (1912.0, 1), (0.93310546875, -11), (0.9331055, -10), (2.0 ** -100, -110), (2.0 ** 40, 30), (2.0 ** 50 * (1 - 2.0 ** -10), 40)):
        q = np.array([0.25 * mx, -mx, 0.0, 0.5 * mx], np.float32)
        got = quant(lib, q, 0)
        assert got is not None and got[0] == e, (mx, e, got)
        assert got[2] == np.float32(2.0 ** e) and got[3] == np.float32(2.0 ** -e)
        assert abs(float(np.float32(mx)) * 2.0 ** -e) <= QMAX and abs(float(np.float32(mx)) * 2.0 ** -(e - 1)) > QMAX
    assert [lib.sq_q(x, 1.0) for x in (0.5, 1.5, 2.5, -0.5, -1.5, 3.49, 1e9, -1e9, float("nan"))] == [0, 2, 2, 0, -2, 3, QMAX, -QMAX, 0]
    assert lib.sq_q(np.float32(1e-40), np.float32(2.0 ** -20)) == 0 and lib.sq_q(np.float32(2.0 ** -126), np.float32(2.0 ** -30)) == 0
    for bad in ([0.0, 0.0], [1.0, np.inf], [np.nan, 1.0], [2.0 ** -126, 0.0], [1e-38, 1e-39], [2.0 ** -117, 0.0]):
        assert quant(lib, np.array(bad, np.float32), 0) is None, bad
    assert quant(lib, np.array([2.0 ** -115, 0.0], np.float32), 0)[0] == -125


# ---- 2. the dot restatement -------------------------------------------------------------------------------------------------------------
def K_both(lib, q, line, dim, codes):
    """K through the packed words and the dot restatement, and sum qhat_i kappa_i computed directly"""
    nst, first, n_st = geometry(dim)
    e, qsum, scale, inv_scale, qe1 = quant(lib, q, first)
    qh = qhat_of(lib, q, inv_scale)
    assert np.abs(qh).max() <= QMAX and int(qh[first:].sum()) == qsum
    err = float(np.sum(np.abs(q[first:].astype(np.float64) - float(scale) * qh[first:])))
    assert err <= qe1 <= err * (1 + 1e-8) + 1e-300
    planes = np.zeros(12 * nst, np.uint32)
    lib.sq_planes(np.ascontiguousarray(q, np.float32).ctypes.data_as(P), dim, inv_scale, nst, planes.ctypes.data_as(PU))
    k3 = (C.c_int32 * 3)()
    K = lib.sq_K(line.ctypes.data_as(PU), planes.ctypes.data_as(PU), first, first, nst, qsum, k3)
    assert all(abs(int(x)) < 2 ** 31 - 2 ** 20 for x in k3)
    direct = int(np.sum(qh[first:] * (2 * codes.astype(np.int64) + 1)))
    assert abs(direct) < 2 ** 25
    return K, direct


@pytest.mark.parametrize("dim", DIMS)
def test_dot_restatement_on_random_lines(lib, dim):
    rng = np.random.default_rng(dim + 70)
    _, first, n_st = geometry(dim)
    for t in range(20):
        q = (rng.uniform(-1, 1, dim) * 2.0 ** rng.integers(-30, 30)).astype(np.float32)
        v = rng.normal(0, 1, dim).astype(np.float32)
        codes = rng.integers(LO, HI + 1, dim - first).astype(np.int32)
        line = custom(lib, v, 0.1, codes) if t % 2 else sketch(lib, v, dim)
        K, direct = K_both(lib, q, line, dim, codes_of(line, n_st, dim - first))
        assert K == direct, (dim, t)


def test_dot_restatement_at_the_extremes_and_past_dim(lib):
    """all codes -8 / 7 against qhat = +-1911 over 896 dims: no i32 sum overflows; dim 773: the padded dims contribute nothing"""
    for dim in (896, 773):
        nst, first, n_st = geometry(dim)
        v = np.ones(dim, np.float32)
        for code in (LO, HI):
            for sign in (1, -1):
                q = np.full(dim, sign * 1911.0, np.float32)
                codes = np.full(dim - first, code, np.int32)
                line = custom(lib, v, 1.0, codes)
                K, direct = K_both(lib, q, line, dim, codes)
                assert K == direct == sign * 1911 * (2 * code + 1) * (dim - first)
                if dim == 773:  # whatever sits in the fields past dim meets a zero digit (and the library's own lines hold code 0 there)
                    dirty = line.copy()
                    dirty[4 + (dim - first) // 8] |= np.uint32(0xFFFFFFFF) << np.uint32(4 * ((dim - first) % 8))
                    dirty[4 + (dim - first) // 8 + 1:] = 0xFFFFFFFF
                    assert K_both(lib, q, dirty, dim, codes)[0] == direct


# ---- 3. the bound against the oracle: the four-bit file's case families ------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["uniform", "gauss"])
def test_uniform_and_gaussian_rows(lib, oracle, dim, kind):
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (120, dim)) if kind == "uniform" else rng.normal(0, 1, (120, dim))).astype(np.float32)
    assert check_rows(lib, oracle, q, rows, kind) == 4 * 120


@pytest.mark.parametrize("dim", DIMS)
def test_tails_on_the_reconstruction_levels(lib, oracle, dim):
    rng = np.random.default_rng(dim + 1)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, _ = geometry(dim)
    rows = rng.uniform(-1, 1, (60, dim)).astype(np.float32)
    levels = np.arange(-15, 16, 2).astype(np.float32)
    for i, a in enumerate(np.geomspace(1e-3, 8.0, 60)):
        a = np.float32(2.0 ** np.round(np.log2(a)))
        rows[i, first:] = a * rng.choice(levels, dim - first)
        rows[i, first + 1] = np.float32(16) * a
    assert check_rows(lib, oracle, q, rows, "levels") == 4 * 60
    # rho ~ a there, so the bound is the score up to one cell's half width, the quantisation term a 15 qe1 and the rounding terms
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    qe1 = quant(lib, q, first)[4]
    for i in range(0, 60, 7):
        a, rho = sketch(lib, rows[i], dim)[:2].view(np.float32)
        s = float(oracle.dot(q, rows[i]))
        scale = float(np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(rows[i].astype(np.float64)))
        width = float(np.linalg.norm(q[first:].astype(np.float64))) * float(rho) + float(a) * 15 * qe1
        up = float(bound(lib, q, rows[i], inv_q, inv_v[i], False, True))
        lo = float(bound(lib, q, rows[i], inv_q, inv_v[i], False, False))
        assert up - s <= 2 * width + 1e-3 * scale and s - lo <= 2 * width + 1e-3 * scale, (i, lo, s, up)


@pytest.mark.parametrize("dim", [768, 225])
@pytest.mark.parametrize("align", [1, -1])
def test_tails_aligned_with_and_against_the_query_signs(lib, oracle, dim, align):
    rng = np.random.default_rng(11 + align)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, n_st = geometry(dim)
    rows = rng.uniform(-1, 1, (100, dim)).astype(np.float32)
    sgn = np.where(np.signbit(q[first:]), np.float32(-1), np.float32(1)) * np.float32(align)
    rows[:, first:] = np.abs(rows[:, first:]) * sgn
    rows[50:, first:] *= np.geomspace(1e-2, 30, 50, dtype=np.float32)[:, None]
    rows[90:, first:] = sgn * np.float32(0.999)  # every code at the range's edge: |kappa| = 15 throughout
    assert np.all(np.abs(2 * codes_of(sketch(lib, rows[95], dim), n_st, dim - first) + 1) == 15)
    assert check_rows(lib, oracle, q, rows, ("aligned", align)) == 4 * 100


@pytest.mark.parametrize("dim", [768, 773])
def test_clipped_outliers_and_any_a_with_its_own_rho(lib, oracle, dim):
    rng = np.random.default_rng(dim + 5)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, n_st = geometry(dim)
    rows = rng.normal(0, 1, (40, dim)).astype(np.float32)
    rows[:, first + 7] = 40.0
    rows[::2, dim - 2] = -55.0
    lines = []
    for i in range(rows.shape[0]):
        tail = rows[i, first:].astype(np.float64)
        delta = [np.quantile(np.abs(tail), 0.9) / 8, 1e-6, 1e6, np.abs(tail).max() / 8, 0.3][i % 5]
        code = np.clip(np.floor(tail / delta), LO, HI).astype(np.int32)
        if i % 7 == 3:
            code = rng.integers(LO, HI + 1, tail.size).astype(np.int32)
        if i % 7 == 5:
            code = np.clip(code + 1, LO, HI).astype(np.int32)
        lines.append(custom(lib, rows[i], 0.0 if i % 11 == 10 else delta / 2, code))
        assert np.array_equal(codes_of(lines[-1], n_st, tail.size), code)
    assert check_rows(lib, oracle, q, rows, "custom", lines=lines) == 4 * 40
    assert check_rows(lib, oracle, q, rows, "outliers") == 4 * 40


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-38, 1e-42, 1e10, 1e15, 1e18, 1e19, 3e20])
def test_subnormal_and_near_overflow_scales(lib, oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale) + 50))
    dim = 768
    _, first, _ = geometry(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (40, dim)) * scale).astype(np.float32)
    rows[::7, first:] = 0.0
    check_rows(lib, oracle, q, rows, scale)
    qs = (q * np.float32(scale)).astype(np.float32)  # (a query the quantiser or prune_query_bounds refuses claims no bound)
    n = check_rows(lib, oracle, qs, rng.uniform(-1, 1, (20, dim)).astype(np.float32), ("query", scale))
    assert (n > 0) == (1e-30 <= scale <= 1e10), (scale, n)
    big = (rng.uniform(-1, 1, (8, dim)) * 3e38).astype(np.float32)  # a tail whose sums leave the f32 range: rho = +inf, no bound
    assert check_rows(lib, oracle, q, big, "overflow") == 0


@pytest.mark.parametrize("dim", [768, 225])
def test_signed_zeros_nan_and_inf_in_tail_and_query(lib, oracle, dim):
    rng = np.random.default_rng(3)
    _, first, _ = geometry(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (12, dim)).astype(np.float32)
    rows[0, first + 3] = np.nan
    rows[1, first + 3] = np.inf
    rows[2, dim - 1] = -np.inf
    rows[3] = 0.0
    rows[4, :first] = 3e38
    rows[5, 5] = np.nan
    rows[6, first:] = 0.0
    rows[7, first:] = -0.0
    rows[8, first::2] = -0.0
    rows[9, first + 1::2] = 0.0
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(6):
        for cosine in (True, False):
            for upper in (True, False):
                assert np.isnan(bound(lib, q, rows[i], inv_q, inv_v[i], cosine, upper)), (i, cosine, upper)
    assert check_rows(lib, oracle, q, rows[6:], "zeros") == 4 * 6
    for qq in (np.where(np.arange(dim) == 9, np.float32(np.inf), q), np.where(np.arange(dim) == dim - 1, np.float32(np.nan), q), np.zeros(dim, np.float32)):
        assert np.isnan(bound(lib, qq.astype(np.float32), rows[10], 1.0, inv_v[10], False, True))
    for vinv in (np.nan, np.inf, 0.0, 1e-30):
        assert np.isnan(bound(lib, q, rows[10], inv_q, vinv, True, True)), vinv
    qz = np.zeros(dim, np.float32)  # scores that are +0 / -0: a query that only sees the tail, rows whose tail is a zero of either sign
    qz[first:] = 1.0
    z = np.zeros((4, dim), np.float32)
    z[1, first:] = -0.0
    z[2, :first] = 1.0
    z[3, :first] = -1.0
    z[:, 0] = 1e-3
    check_rows(lib, oracle, qz, z, "signed zero scores")
    qm = q.copy()  # zeros of both signs in the query: qhat = 0 either way
    qm[first::2] = -0.0
    qm[first + 1::4] = 0.0
    assert check_rows(lib, oracle, qm, rows[6:], "query zeros") == 4 * 6


# ---- queries that stress the quantiser (tests/test_gpu_exact_sketch4_int.py runs the same kinds on the device) ---------------------------
@pytest.mark.parametrize("kind", QUERY_KINDS)
@pytest.mark.parametrize("dim", [256, 773])
def test_queries_that_stress_the_quantiser(lib, oracle, dim, kind):
    rng = np.random.default_rng(dim + 31)
    q = stress_query(kind, dim)
    rows = rng.uniform(-1, 1, (60, dim)).astype(np.float32)
    rows[40:] = rng.normal(0, 1, (20, dim)).astype(np.float32)
    got = quant(lib, q, 32)
    o = (C.c_ulonglong * 4)()
    lib.sq_plan(q.ctypes.data_as(P), dim, 1 << 21, o)
    nst = geometry(dim)[0]
    if kind in REFUSED:  # the plan of a store without a sketch: the 7/8 form, its checkpoint, the tenth as seed
        assert got is None and list(o) == [nst * 7 // 8, 0, ((1 << 21) // 10 + 63) // 64 * 64, 0]
        assert check_rows(lib, oracle, q, rows, kind) == 0
        return
    assert got is not None and list(o) == [1, 1, 131072, 1]
    e, qsum, scale, inv_scale, qe1 = got
    qh = qhat_of(lib, q, inv_scale)
    assert np.abs(qh).max() <= QMAX and np.abs(q).max() * float(inv_scale) > QMAX / 2  # the smallest power of two that fits
    if kind == "half_integers":
        assert e == 0 and np.all(qh % 2 == 0) and qe1 >= 0.5 * (dim - 32)
    if kind == "zero_tail":
        assert qsum == 0 and qe1 == 0.0
    if kind == "one_big":
        assert np.abs(qh[np.arange(dim) != 37]).max() <= 1
    inv_q = float(oracle.inv_norms(q[None, :])[0])  # (max 2^-100: the squares underflow, the reference's inverse norm is not finite: no cosine bound)
    assert (kind == "max_2^-100") == (not (0 < inv_q < np.inf))
    assert check_rows(lib, oracle, q, rows, kind) == (2 if kind == "max_2^-100" else 4) * 60


# ---- 5. the prune rate ------------------------------------------------------------------------------------------------------------------
def test_prune_rate_against_the_f32_chain_form(lib, oracle):
    """dim 768, checkpoint 32, the gate at the 10th best of 100k uniform rows.  Reference: the drop rate of prune_score_bound_sketchb
    (the f32 chain, kmax = 15) computed here on the same inputs, 97.85 %.  The integer decode pays a 15 qe1 for the quantised query
    and saves the chain's rounding term; it may drop at most 0.25 point fewer (the model: about 0.06)."""
    dim, n, k = 768, 100_000, 10
    rng = np.random.default_rng(2024)
    first = 32
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = np.ascontiguousarray(oracle.inv_norms(rows), np.float32)
    top = oracle.vec_query(rows, q, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, 0, 0.0, ties=oracle.TIES_CANONICAL)
    gate = tkey(top["score"][k - 1])
    out_q, out_b = np.empty(n, np.float32), np.empty(n, np.float32)
    lib.both_bound_rows(q.ctypes.data_as(P), rows.ctypes.data_as(P), n, dim, first, np.float32(inv_q), inv_v.ctypes.data_as(P), out_q.ctypes.data_as(P),
                        out_b.ctypes.data_as(P))
    dropped = []
    for out in (out_q, out_b):
        assert not np.isnan(out).any()
        b = out.view(np.uint32).astype(np.int64)
        keys = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
        assert set(int(i) for i in top["index"]).isdisjoint(np.flatnonzero(keys < gate).tolist())
        dropped.append(int(np.count_nonzero(keys < gate)))
    print(f"dim {dim}, checkpoint {first}: integer decode drops {100.0 * dropped[0] / n:.3f} %, f32 chain form {100.0 * dropped[1] / n:.3f} % of {n} rows")
    assert dropped[1] - dropped[0] <= n * 25 // 10000, dropped
