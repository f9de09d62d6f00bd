"""CPU: the four-bit tail sketch of the pruned exact sweep and its score bound (otters_amd/csrc/ott_prune.h, DESIGN.md 3.1b, "four
bits per dim") against the oracle's bit-exact scores.  The header is compiled on its own with the host compiler, as in
test_exact_prune_sketch3_bound.py; a small driver makes a row's line with the library's own prune_sketchb_row (or, for a sketch of
the test's choosing, with prune_sketchb_add / prune_sketchb_finish), computes the kernel's checkpoint state — the eight partial chains
after m dims (separate multiply and add) and D = sum q_i kappa_i, one fma per dim in dim order — and asks prune_score_bound_sketchb
with kmax = 15.
  1. the line against a float64 restatement: [a | rho | 0 | 0], piece 1 + j = stage j's four words, codes = floor(v / Delta) clamped
     to [-8, 7], a = Delta / 2, rho >= ||v_t - a kappa||;
  2. every final score on the right side of its bound in f32::total_cmp order, and the strict gate decision;
  3. b = 1 and b = 3 are what they were, bit for bit: the sign form against its own functions, both against digests of the lines
     and bounds taken before the four-bit form was added;
  4. the prune rate against a float64 restatement of the bound.
The GPU half is tests/test_gpu_exact_sketch4.py."""
import ctypes as C
import hashlib
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
extern "C" unsigned skb_stage0(unsigned nst, unsigned bits) { return ott::prune_sketchb_stage0(nst, bits); }
extern "C" unsigned skb_pitch(unsigned n_stages, unsigned bits) { return ott::prune_sketchb_pitch(n_stages, bits); }
extern "C" unsigned skb_word0(unsigned bits) { return ott::prune_sketchb_word0(bits); }
extern "C" void skb_row(const float* v, unsigned dim, unsigned first, unsigned n_stages, unsigned bits, unsigned* line) {
    ott::prune_sketchb_row(v, dim, first, n_stages, bits, line);
}
extern "C" int skb_code(const unsigned* w, unsigned i, unsigned bits) { return ott::prune_sketchb_code(w, i, bits); }
// a line of the caller's choosing: a and one code per tail dim; rho is the library's, for exactly these
extern "C" void skb_custom(const float* v, unsigned dim, unsigned first, unsigned n_stages, unsigned bits, float a, const int* codes, unsigned* line) {
    for (unsigned j = 0; j < ott::prune_sketchb_pitch(n_stages, bits); j++) line[j] = 0u;
    ott::PruneSketchSumsB t;
    for (unsigned i = first; i < dim; i++) {
        const unsigned pos = bits * ((i - first) & 31u), lo = pos & 31u;
        unsigned* w = line + ott::prune_sketchb_word0(bits) + bits * ((i - first) >> 5) + (pos >> 5);
        const unsigned f = (unsigned)codes[i - first] & ((1u << bits) - 1u);
        w[0] |= f << lo;
        if (lo + bits > 32u) w[1] |= f >> (32u - lo);
        ott::prune_sketchb_add(t, ott::prune_f2u(v[i]), 2 * codes[i - first] + 1);
    }
    float ao, rho;
    ott::prune_sketchb_finish(t, a, &ao, &rho);
    line[0] = ott::prune_f2u(ao);
    line[1] = ott::prune_f2u(rho);
}
// the bound of one row from its line at the checkpoint m >= first (both multiples of 32); NaN = no bound claimed
extern "C" float skb_bound_line(const float* q, const float* v, unsigned dim, unsigned first, unsigned m, unsigned bits, const unsigned* line,
                                float qinv, float vinv, int cosine, int upper) {
    const unsigned nst = ((dim + 3) / 4 * 4 + 31) / 32;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned c = 0; c < m; c += 8)
        for (int l = 0; l < 8; l++) {
            volatile float prod = q[c + l] * v[c + l];
            acc[l] = acc[l] + prod;
        }
    float D = 0.0f;  // the kernel's chain: kappa = 2 code + 1 as a float, one fma per dim, dims past `dim` read a zero query
    for (unsigned s = m / 32; s < nst; s++)
        for (unsigned b = 0; b < 32; b++) {
            const int code = ott::prune_sketchb_code(line + ott::prune_sketchb_word0(bits) + bits * (s - first / 32), b, bits);
            const unsigned i = 32 * s + b;
            D = fmaf((float)(2 * code + 1), i < dim ? q[i] : 0.0f, D);
        }
    double qt, qn;
    if (!ott::prune_query_bounds(q, dim, m, &qt, &qn)) return NAN;
    const double q1 = ott::prune_query_l1(q, dim, m);
    return ott::prune_score_bound_sketchb(acc, vinv, ott::prune_u2f(line[0]), ott::prune_u2f(line[1]), D, (double)((1u << bits) - 1u), m, dim, qt, q1,
                                          qn, qinv, cosine != 0, upper != 0);
}
extern "C" float skb_bound(const float* q, const float* v, unsigned dim, unsigned first, unsigned m, unsigned bits, float qinv, float vinv,
                           int cosine, int upper) {
    const unsigned nst = ((dim + 3) / 4 * 4 + 31) / 32;
    uint32_t line[2 + 8 * 64 + 8];
    ott::prune_sketchb_row(v, dim, first, nst - first / 32, bits, line);
    return skb_bound_line(q, v, dim, first, m, bits, line, qinv, vinv, cosine, upper);
}
extern "C" void skb_bound_rows(const float* q, const float* rows, unsigned long long n, unsigned dim, unsigned first, unsigned bits, float qinv,
                               const float* vinv, int cosine, int upper, float* out) {
    for (unsigned long long r = 0; r < n; r++) out[r] = skb_bound(q, rows + r * dim, dim, first, first, bits, qinv, vinv[r], cosine, upper);
}
// the sign form's own names, for part 3
extern "C" void sk_row(const float* v, unsigned dim, unsigned first, unsigned n_words, unsigned* line) { ott::prune_sketch_row(v, dim, first, n_words, line); }
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
    float D = 0.0f;
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
"""

P = C.POINTER(C.c_float)
PU = C.POINTER(C.c_uint32)
PI = C.POINTER(C.c_int32)
B = 4
LO, HI = -8, 7


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sketch4")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.skb_stage0.argtypes = [C.c_uint, C.c_uint]
    L.skb_stage0.restype = C.c_uint
    L.skb_pitch.argtypes = [C.c_uint, C.c_uint]
    L.skb_pitch.restype = C.c_uint
    L.skb_word0.argtypes = [C.c_uint]
    L.skb_word0.restype = C.c_uint
    L.skb_row.argtypes = [P, C.c_uint, C.c_uint, C.c_uint, C.c_uint, PU]
    L.skb_row.restype = None
    L.skb_code.argtypes = [PU, C.c_uint, C.c_uint]
    L.skb_code.restype = C.c_int
    L.skb_custom.argtypes = [P, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_float, PI, PU]
    L.skb_custom.restype = None
    L.skb_bound_line.argtypes = [P, P, C.c_uint, C.c_uint, C.c_uint, C.c_uint, PU, C.c_float, C.c_float, C.c_int, C.c_int]
    L.skb_bound_line.restype = C.c_float
    L.skb_bound.argtypes = [P, P, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.c_int, C.c_int]
    L.skb_bound.restype = C.c_float
    L.skb_bound_rows.argtypes = [P, P, C.c_ulonglong, C.c_uint, C.c_uint, C.c_uint, C.c_float, P, C.c_int, C.c_int, P]
    L.skb_bound_rows.restype = None
    L.sk_row.argtypes = [P, C.c_uint, C.c_uint, C.c_uint, PU]
    L.sk_row.restype = None
    L.sk_bound.argtypes = [P, P, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.c_int, C.c_int]
    L.sk_bound.restype = C.c_float
    return L


def tkey(x):
    """f32::total_cmp as an unsigned key (the library's total_key)"""
    b = int(np.float32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def geometry(lib, dim, bits=B):
    """stages, the sketch's first dim (= the checkpoint), its sketched stages"""
    nst = ((dim + 3) // 4 * 4 + 31) // 32
    s0 = lib.skb_stage0(nst, bits)
    if bits == 4:
        assert s0 == 1  # the committed rule: one stage of the row in front, every other stage sketched
    assert 1 <= s0 < nst and 32 * s0 <= dim - dim % 8
    return nst, 32 * s0, nst - s0


def sketch(lib, v, first, n_stages, bits=B):
    v = np.ascontiguousarray(v, np.float32)
    line = np.zeros(lib.skb_pitch(n_stages, bits), np.uint32)
    lib.skb_row(v.ctypes.data_as(P), v.size, first, n_stages, bits, line.ctypes.data_as(PU))
    return line


def custom(lib, v, first, n_stages, a, codes, bits=B):
    v = np.ascontiguousarray(v, np.float32)
    codes = np.ascontiguousarray(codes, np.int32)
    assert codes.size == v.size - first
    line = np.zeros(lib.skb_pitch(n_stages, bits), np.uint32)
    lib.skb_custom(v.ctypes.data_as(P), v.size, first, n_stages, bits, np.float32(a), codes.ctypes.data_as(PI), line.ctypes.data_as(PU))
    return line


def codes_of(line, n_stages, n_dims):
    """the four-bit fields read straight from the layout: piece 1 + j = stage j, field i of a stage at bits 4 (i % 8) of word i // 8"""
    w = line[4:4 + 4 * n_stages].astype(np.int64).reshape(n_stages, 4)
    f = (w[:, :, None] >> (4 * np.arange(8))[None, None, :]) & 15
    out = np.where(f >= 8, f - 16, f).reshape(-1)
    assert not out[n_dims:].any()  # dims past `dim` hold code 0
    return out[:n_dims]


def bound(lib, q, v, first, m, qinv, vinv, cosine, upper, line=None, bits=B):
    q = np.ascontiguousarray(q, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    if line is None:
        return np.float32(lib.skb_bound(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, first, m, bits, np.float32(qinv), np.float32(vinv),
                                        int(cosine), int(upper)))
    return np.float32(lib.skb_bound_line(q.ctypes.data_as(P), v.ctypes.data_as(P), q.size, first, m, bits, line.ctypes.data_as(PU),
                                         np.float32(qinv), np.float32(vinv), int(cosine), int(upper)))


def check_sketch(lib, rows, rho_tight=True):
    """part 1: every row's four-bit line against the float64 restatement"""
    dim = rows.shape[1]
    _, first, n_st = geometry(lib, dim)
    pitch = lib.skb_pitch(n_st, B)
    assert pitch == 4 * n_st + 4  # the header piece and one piece per sketched stage: the pitch did not grow
    for i in range(rows.shape[0]):
        line = sketch(lib, rows[i], first, n_st)
        a, rho = line[:2].view(np.float32)
        tail = rows[i, first:]
        assert line[2] == 0 and line[3] == 0, i
        if not np.isfinite(tail).all():
            assert np.isposinf(rho) and a == 0, (i, a, rho)
            continue
        code = codes_of(line, n_st, tail.size)
        assert code.min() >= LO and code.max() <= HI, i
        for d in (0, 7, 8, 31, 32, tail.size - 1):  # the layout agrees with the library's own field extract
            w = np.ascontiguousarray(line[lib.skb_word0(B) + 4 * (d // 32):lib.skb_word0(B) + 4 * (d // 32) + 4])
            assert lib.skb_code(w.ctypes.data_as(PU), d % 32, B) == code[d], (i, d)
        t64 = tail.astype(np.float64)
        delta = np.float32(np.abs(tail).max()) / np.float32(8)
        with np.errstate(over="ignore", invalid="ignore"):
            exact = float(np.sqrt(np.sum((t64 - float(a) * (2 * code + 1)) ** 2)))
        if not np.isfinite(rho):  # the sums left the f32 range: no sketch
            assert a == 0 and exact > 3e38, (i, a, exact)
            continue
        assert a == np.float32(delta * np.float32(0.5)), (i, a, delta)
        if delta > 1e-30:  # the cell of every value: floor(v / Delta) clamped; a value on a cell boundary may fall either way
            want = np.clip(np.floor(t64 / float(delta)), LO, HI)
            off = np.abs(t64 / float(delta) - np.round(t64 / float(delta))) < 1e-5
            assert np.all((code == want) | (off & (np.abs(code - want) <= 1))), i
        assert float(rho) >= exact, (i, rho, exact)
        if rho_tight and exact > 0:  # ... and not by much: the bound is only as good as rho is close
            assert float(rho) <= exact * (1 + 1e-3) + 1e-4 * float(np.linalg.norm(t64)), (i, rho, exact)


def check_rows(lib, oracle, q, rows, where, metrics=(True, False), lines=None):
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
                b = bound(lib, q, rows[i], first, first, inv_q, inv_v[i], cosine, upper, None if lines is None else lines[i])
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


DIMS = [225, 256, 768, 773, 896]  # with (225, 773) and without a remainder of the chunks of eight; 896: the widest query a launch carries


def test_geometry(lib):
    for nst, want in ((24, 1), (8, 1), (25, 1), (28, 1), (3, 1), (2, 1), (16, 1), (64, 1), (1, 0)):
        assert lib.skb_stage0(nst, 4) == want, nst
    assert lib.skb_word0(4) == 4 and lib.skb_word0(3) == 2 and lib.skb_word0(1) == 2
    assert lib.skb_pitch(23, 4) == 96  # dim 768: a 384-B line, the header and 23 stage pieces: 1/8 of the row
    assert lib.skb_pitch(27, 4) == 112  # 28 stages, the most a launch decodes: 28 pieces
    # the other forms' geometry is what it was
    for nst, want in ((24, 9), (8, 3), (25, 9), (28, 10), (3, 1), (2, 1)):
        assert lib.skb_stage0(nst, 3) == want, nst
    for nst in range(2, 40):
        assert lib.skb_stage0(nst, 1) == nst - (nst + 3) // 4
    assert lib.skb_pitch(15, 3) == 48 and lib.skb_pitch(18, 3) == 56 and lib.skb_pitch(6, 1) == 8


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["uniform", "gauss"])
def test_uniform_and_gaussian_rows(lib, oracle, dim, kind):
    rng = np.random.default_rng(dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (120, dim)) if kind == "uniform" else rng.normal(0, 1, (120, dim))).astype(np.float32)
    check_sketch(lib, rows)
    assert check_rows(lib, oracle, q, rows, kind) == 4 * 120


@pytest.mark.parametrize("dim", DIMS)
def test_tails_on_the_reconstruction_levels(lib, oracle, dim):
    """every tail value but one sits on a reconstruction level a (2 c + 1): rho ~ a, one cell's half width for the whole tail, and
    the bound is the score up to that and the rounding terms"""
    rng = np.random.default_rng(dim + 1)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, n_st = geometry(lib, dim)
    rows = rng.uniform(-1, 1, (60, dim)).astype(np.float32)
    levels = np.arange(-15, 16, 2).astype(np.float32)
    for i, a in enumerate(np.geomspace(1e-3, 8.0, 60)):
        a = np.float32(2.0 ** np.round(np.log2(a)))  # (a power of two: every product below is exact)
        rows[i, first:] = a * rng.choice(levels, dim - first)
        rows[i, first + 1] = np.float32(16) * a      # the largest magnitude: Delta = 2 a, so the levels are the odd multiples of a;
                                                     # this one value clips to the top cell, a away from its level
    check_sketch(lib, rows)
    check_rows(lib, oracle, q, rows, "levels")
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(0, 60, 7):
        line = sketch(lib, rows[i], first, n_st)
        a, rho = line[:2].view(np.float32)
        tnorm = float(np.linalg.norm(rows[i, first:].astype(np.float64)))
        assert float(rho) <= float(a) * 1.001 + 1e-4 * tnorm, (i, a, rho)  # (one value sits a away from its level)
        s = float(oracle.dot(q, rows[i]))
        scale = float(np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(rows[i].astype(np.float64)))
        up = float(bound(lib, q, rows[i], first, first, inv_q, inv_v[i], False, True))
        lo = float(bound(lib, q, rows[i], first, first, inv_q, inv_v[i], False, False))
        width = float(np.linalg.norm(q[first:].astype(np.float64))) * float(rho)
        assert up - s <= 2 * width + 1e-3 * scale and s - lo <= 2 * width + 1e-3 * scale, (i, lo, s, up)


@pytest.mark.parametrize("dim", [768, 225])
@pytest.mark.parametrize("align", [1, -1])
def test_tails_aligned_with_and_against_the_query_signs(lib, oracle, dim, align):
    """sign(v_t) = +-sign(q_t): q_t . kappa is as large in magnitude as the codes allow"""
    rng = np.random.default_rng(11 + align)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, n_st = geometry(lib, dim)
    rows = rng.uniform(-1, 1, (100, dim)).astype(np.float32)
    sgn = np.where(np.signbit(q[first:]), np.float32(-1), np.float32(1)) * np.float32(align)
    rows[:, first:] = np.abs(rows[:, first:]) * sgn
    rows[50:, first:] *= np.geomspace(1e-2, 30, 50, dtype=np.float32)[:, None]
    rows[90:, first:] = sgn * np.float32(0.999)  # every code at the range's edge: |kappa| = 15 throughout
    kap = 2 * codes_of(sketch(lib, rows[95], first, n_st), n_st, dim - first) + 1
    assert np.all(np.abs(kap) == 15)
    check_sketch(lib, rows)
    assert check_rows(lib, oracle, q, rows, ("aligned", align)) == 4 * 100


@pytest.mark.parametrize("dim", [768, 773])
def test_clipped_outliers_and_any_a_with_its_own_rho(lib, oracle, dim):
    """the bound holds for ANY a >= 0 and any codes, rho being taken for them: a cell width from the 90th percentile (the largest
    values clip), one far too small, one far too large, a = 0, random codes, and the codes of a neighbouring cell everywhere"""
    rng = np.random.default_rng(dim + 5)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    _, first, n_st = geometry(lib, dim)
    rows = rng.normal(0, 1, (40, dim)).astype(np.float32)
    rows[:, first + 7] = 40.0   # a few outliers far outside the other values
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
        a = 0.0 if i % 11 == 10 else delta / 2
        line = custom(lib, rows[i], first, n_st, a, code)
        got = line[:2].view(np.float32)
        exact = float(np.sqrt(np.sum((tail - float(got[0]) * (2 * code + 1)) ** 2)))
        assert got[0] == np.float32(a) and float(got[1]) >= exact and float(got[1]) <= exact * (1 + 1e-3) + 1e-4 * np.linalg.norm(tail), (i, got, exact)
        assert np.array_equal(codes_of(line, n_st, tail.size), code)
        lines.append(line)
    assert check_rows(lib, oracle, q, rows, "custom", lines=lines) == 4 * 40
    check_sketch(lib, rows)                       # the library's own rule on the same rows: the outlier sets the width
    assert check_rows(lib, oracle, q, rows, "outliers") == 4 * 40
    bad = custom(lib, rows[0], first, n_st, -1.0, np.zeros(dim - first, np.int32))  # a negative a is no sketch
    assert np.isposinf(bad[:2].view(np.float32)[1])


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-38, 1e-42, 1e10, 1e15, 1e18, 1e19, 3e20])
def test_subnormal_and_near_overflow_scales(lib, oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale) + 50))
    dim = 768
    _, first, _ = geometry(lib, dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = (rng.uniform(-1, 1, (40, dim)) * scale).astype(np.float32)
    rows[::7, first:] = 0.0
    check_sketch(lib, rows, rho_tight=scale > 1e-37)  # (subnormal values: Delta itself is rounded coarsely)
    check_rows(lib, oracle, q, rows, scale)
    qs = (q * np.float32(scale)).astype(np.float32)
    check_rows(lib, oracle, qs, rng.uniform(-1, 1, (20, dim)).astype(np.float32), ("query", scale))
    big = (rng.uniform(-1, 1, (8, dim)) * 3e38).astype(np.float32)  # a tail whose sums leave the f32 range: rho = +inf, no bound
    check_sketch(lib, big)
    check_rows(lib, oracle, q, big, "overflow")


@pytest.mark.parametrize("dim", [768, 225])
def test_signed_zeros_nan_and_inf_in_the_tail(lib, oracle, dim):
    rng = np.random.default_rng(3)
    _, first, n_st = geometry(lib, dim)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (12, dim)).astype(np.float32)
    rows[0, first + 3] = np.nan
    rows[1, first + 3] = np.inf
    rows[2, dim - 1] = -np.inf
    rows[3] = 0.0                    # zero row: inverse norm 0
    rows[4, :first] = 3e38           # the prefix overflows
    rows[5, 5] = np.nan              # NaN in the prefix
    rows[6, first:] = 0.0            # a tail of +0 ...
    rows[7, first:] = -0.0           # ... and of -0: a = 0, rho = 0 whatever the codes
    rows[8, first::2] = -0.0         # zeros of both signs among finite values
    rows[9, first + 1::2] = 0.0
    check_sketch(lib, rows)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(3):               # NaN / inf in the tail: rho = +inf, no bound is claimed
        assert np.isposinf(sketch(lib, rows[i], first, n_st)[:2].view(np.float32)[1])
    for i in range(6):
        for cosine in (True, False):
            for upper in (True, False):
                assert np.isnan(bound(lib, q, rows[i], first, first, inv_q, inv_v[i], cosine, upper)), (i, cosine, upper)
    for i in (6, 7):
        line = sketch(lib, rows[i], first, n_st)
        assert line[0] == 0 and line[1] == 0
    assert check_rows(lib, oracle, q, rows[6:], "zeros") == 4 * 6
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


def _old_forms_rows(dim):
    rng = np.random.default_rng(dim + 9)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.normal(0, 1, (60, dim)).astype(np.float32)
    return q, rows


@pytest.mark.parametrize("dim", [225, 768, 773, 1000])
def test_one_bit_is_the_sign_sketch_bit_for_bit(lib, oracle, dim):
    """part 3: b = 1 through the general functions: prune_sketch_row's line and prune_score_bound_sketch's value"""
    nst, first, n_st = geometry(lib, dim, bits=1)
    q, rows = _old_forms_rows(dim)
    rows[1, first:] = 0.0
    rows[2, first::3] = -0.0
    rows[3, dim - 1] = np.nan
    rows[4, first] = np.inf
    rows[5] *= np.float32(1e-41)
    rows[6] *= np.float32(3e37)
    rows[7, first:] = 0.25
    assert lib.skb_pitch(n_st, 1) == (n_st + 2 + 3) // 4 * 4
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    for i in range(rows.shape[0]):
        v = np.ascontiguousarray(rows[i])
        old = np.zeros(lib.skb_pitch(n_st, 1), np.uint32)
        lib.sk_row(v.ctypes.data_as(P), dim, first, n_st, old.ctypes.data_as(PU))
        assert np.array_equal(sketch(lib, v, first, n_st, bits=1), old), i
        for cosine in (True, False):
            for upper in (True, False):
                for m in (first, first + 32 if first + 32 < 32 * (nst - 1) else first):
                    new = bound(lib, q, v, first, m, inv_q, inv_v[i], cosine, upper, bits=1)
                    ref = np.float32(lib.sk_bound(q.ctypes.data_as(P), v.ctypes.data_as(P), dim, first, m, np.float32(inv_q), np.float32(inv_v[i]),
                                                  int(cosine), int(upper)))
                    assert new.view(np.uint32) == ref.view(np.uint32), (i, cosine, upper, m, new, ref)


# sha256 over the lines and the four bounds (cosine / dot x upper / lower) of 60 Gaussian rows and two edge rows per dim, taken with
# the header as it stood before the four-bit form was added (the same driver functions; inverse norms from the oracle)
OLD_FORM_DIGESTS = {
    (1, 768): "4619b89131d0c852f44116393449172cc4cc8aa2c60d56abc64099b190eebb32",
    (1, 773): "dce756b8b55dd65c8c075daa32f8b4c6609c9147be244566e6a52af14381db70",
    (3, 768): "06c787b60b9e3342cb79c8653842a58e79e232588c381ecedc4458f6d24bdfc4",
    (3, 773): "5f0a6df10d81f3417a64393b8bd259b0af43d00d05db1a5d1eb91bc47c3920dc",
}


def old_form_digest(lib, oracle, bits, dim):
    nst, first, n_st = geometry(lib, dim, bits=bits)
    q, rows = _old_forms_rows(dim)
    rows[1, first:] = 0.0
    rows[2, first::3] = -0.0
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = oracle.inv_norms(rows)
    h = hashlib.sha256()
    h.update(np.array([nst, first, n_st, lib.skb_pitch(n_st, bits)], np.uint32).tobytes())
    for i in range(rows.shape[0]):
        h.update(sketch(lib, rows[i], first, n_st, bits=bits).tobytes())
        for cosine in (True, False):
            for upper in (True, False):
                h.update(bound(lib, q, rows[i], first, first, inv_q, inv_v[i], cosine, upper, bits=bits).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("bits,dim", sorted(OLD_FORM_DIGESTS))
def test_one_and_three_bits_are_unchanged_bit_for_bit(lib, oracle, bits, dim):
    assert old_form_digest(lib, oracle, bits, dim) == OLD_FORM_DIGESTS[(bits, dim)]


def test_prune_rate_on_uniform_rows(lib, oracle):
    """part 4: 100k uniform rows at dim 768, checkpoint at the committed stage 1 (dim 32), the gate at the k-th best (k = 10) of the
    rows themselves.  The share the header's bound drops is within one percentage point of a float64 restatement (the same sketch
    rule, no rounding terms).  The byte model this form was chosen by puts that share at 97.7 %; a floor of 96.7 %, one point
    under it, is kept under both."""
    dim, n, k = 768, 100_000, 10
    rng = np.random.default_rng(2024)
    _, first, _ = geometry(lib, dim)
    assert first == 32
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    inv_q = oracle.inv_norms(q[None, :])[0]
    inv_v = np.ascontiguousarray(oracle.inv_norms(rows), np.float32)
    top = oracle.vec_query(rows, q, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, 0, 0.0, ties=oracle.TIES_CANONICAL)
    gate = tkey(top["score"][k - 1])
    out = np.empty(n, np.float32)
    lib.skb_bound_rows(q.ctypes.data_as(P), rows.ctypes.data_as(P), n, dim, first, B, np.float32(inv_q), inv_v.ctypes.data_as(P), 1, 1,
                       out.ctypes.data_as(P))
    assert not np.isnan(out).any()
    b = out.view(np.uint32).astype(np.int64)
    keys = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    dropped = int(np.count_nonzero(keys < gate))
    # the float64 restatement: S <= q_p . v_p + a (q_t . kappa) + ||q_t|| ||v_t - a kappa||, over ||q|| ||v||
    q64 = q.astype(np.float64)
    model = 0
    for lo in range(0, n, 10_000):
        r = rows[lo:lo + 10_000].astype(np.float64)
        t = r[:, first:]
        delta = np.abs(t).max(axis=1, keepdims=True) / 8
        kap = 2 * np.clip(np.floor(t / delta), LO, HI) + 1
        a = delta / 2
        rho = np.sqrt(np.sum((t - a * kap) ** 2, axis=1))
        ub = r[:, :first] @ q64[:first] + a[:, 0] * (kap @ q64[first:]) + np.linalg.norm(q64[first:]) * rho
        ub /= np.linalg.norm(q64) * np.linalg.norm(r, axis=1)
        model += int(np.count_nonzero(ub < float(top["score"][k - 1])))
    print(f"4-bit sketch bound at dim {first} of {dim}: {dropped} of {n} rows dropped ({100.0 * dropped / n:.2f} %), float64 model {100.0 * model / n:.2f} %")
    assert set(int(i) for i in top["index"]).isdisjoint(np.flatnonzero(keys < gate).tolist())
    assert abs(dropped - model) <= n // 100, (dropped, model)
    assert model >= n * 967 // 1000 and dropped >= n * 967 // 1000, (dropped, model)
