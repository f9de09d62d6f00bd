"""CPU: what the batch path's host side decides before it launches anything (otters_amd/csrc/ott_mfma_plan.h): tile geometry, the
candidate budget of a level, the bound on |approximate - exact| it certifies against, the query norms that bound is built from and
the layout of the query block.  The header is compiled on its own with the host compiler behind a small extern "C" driver, with
the library's -ffp-contract=off, as test_plane_policy_cpu.py does for ott_plane_policy.h: the code under test is the code
libotters_hip.so ships.
Expected values: transcriptions of the expressions run_mfma and run_i8_single carried before the header existed, in np.float32
scalars (every literal wrapped, so nothing is promoted to double) with the same operation order, compared bit for bit; and values
written out by hand where a case has an obvious answer.
The GPU half: test_gpu_mfma.py::test_first_level_rescores_its_documented_budget."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include "ott_mfma_plan.h"
using namespace ott;
extern "C" void mp_geometry(unsigned nq, int level, unsigned dim, long long* o) {
    const TileGeometry g = tile_geometry(nq, level, dim);
    o[0] = g.NB; o[1] = g.BN; o[2] = g.nq_pad; o[3] = g.qblk_max; o[4] = g.ldq; o[5] = g.ldh; o[6] = g.passes();
}
extern "C" void mp_budget(int level, unsigned k, unsigned t_min, unsigned long long rows_scored, int sweep, long long* o) {
    const Budget b = level_budget(level, k, t_min, rows_scored, sweep != 0);
    o[0] = b.T; o[1] = b.E; o[2] = b.wide; o[3] = b.cap; o[4] = b.k_too_large;
}
extern "C" int mp_hi_k_ok(unsigned long long k, int half) { return mfma_hi_k_ok(k, half != 0) ? 1 : 0; }
extern "C" void mp_wants(unsigned long long k, unsigned long long* o) { o[0] = t_want_split(k); o[1] = t_want_hi(k); o[2] = t_want_i8(k); o[3] = SWEEP_T; }
// o: eps_c, eps_r, qrel_cap, eps_scale, r_max, max_norm, eps_max, usable, then (flo, fhi) for filter_cmp = 0 .. 5
extern "C" void mp_model(int level, int hi_f16, unsigned dim, unsigned metric, int bf3, int ppm, float rel, float min_pos_inv, float qn_max, float thr, float* o) {
    const ErrorModel m = error_model(level, hi_f16 != 0, dim, metric, bf3 != 0, ppm, rel);
    o[0] = m.eps_c; o[1] = m.eps_r; o[2] = m.qrel_cap; o[3] = m.eps_scale; o[4] = m.r_max;
    o[5] = max_norm(min_pos_inv);
    o[6] = m.eps_max(metric, qn_max, o[5]);
    o[7] = o[6] < __builtin_inff() ? 1.0f : 0.0f;
    for (unsigned c = 0; c < 6; c++) {
        const FilterInterval f = relaxed_filter(c, thr, o[6]);
        o[8 + 2 * c] = f.flo;
        o[9 + 2 * c] = f.fhi;
    }
}
extern "C" int mp_query_regular(float qnorm) { return query_regular(qnorm) ? 1 : 0; }
extern "C" float mp_norms(const float* q, unsigned nq, unsigned dim, unsigned metric, int want_amax, float* qnorm, float* qinv, float* qamax) {
    return query_norms(q, nq, dim, metric, want_amax != 0, qnorm, qinv, qamax);
}
extern "C" void mp_layout(unsigned nq_pad, unsigned ldq, unsigned long long n_runs, unsigned long long n_prefix, int own, unsigned long long* o) {
    const QueryBlock b = query_block(nq_pad, ldq, n_runs, n_prefix, own != 0);
    const unsigned long long v[13] = {b.q_bytes, b.qinv, b.qnorm, b.tau, b.cntA, b.cntB, b.over, b.qrel, b.gate, b.runs, b.prefix, b.qraw, b.total};
    for (int i = 0; i < 13; i++) o[i] = v[i];
}
"""

f32, f64 = np.float32, np.float64
INF = f32(np.inf)
COSINE, EUCLIDEAN, DOT = 0, 1, 2
CMP_NONE, CMP_LT, CMP_GT, CMP_LTE, CMP_GTE, CMP_EQ = range(6)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("mfma_plan")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    fp, llp, ullp = C.POINTER(C.c_float), C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong)
    L.mp_geometry.argtypes = [C.c_uint, C.c_int, C.c_uint, llp]
    L.mp_budget.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_ulonglong, C.c_int, llp]
    L.mp_hi_k_ok.argtypes = [C.c_ulonglong, C.c_int]
    L.mp_wants.argtypes = [C.c_ulonglong, ullp]
    L.mp_model.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, fp]
    L.mp_query_regular.argtypes = [C.c_float]
    L.mp_norms.argtypes = [fp, C.c_uint, C.c_uint, C.c_uint, C.c_int, fp, fp, fp]
    L.mp_norms.restype = C.c_float
    L.mp_layout.argtypes = [C.c_uint, C.c_uint, C.c_ulonglong, C.c_ulonglong, C.c_int, ullp]
    return L


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ---- geometry and budget -----------------------------------------------------------------------------------------------------------
NQS = (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 520, 1030)
KS = (1, 10, 24, 25, 36, 100, 128, 228, 229, 363, 484, 512, 513)
T_MINS = (0, 128, 512, 4096)
ROWS = (1, 900, 2048, 16320, 16321, 10 ** 7)


def parent_geometry(nq, level, dim):
    """run_mfma's own lines (and run_i8_single's ld8 = 2 ldh, ldq)"""
    i8 = level == 2
    hi = level == 0 or i8
    NB = -1 if (nq <= 16 and not hi) else 0 if nq <= 32 else 1 if nq <= 64 else 2 if nq <= 128 else 4
    BN = 16 if NB == -1 else 32 if NB == 0 else 64 * NB
    nq_pad = (nq + BN - 1) // BN * BN
    qblk_max = min(4, nq_pad // BN) if NB == 4 else 1
    ldq = (dim + 32 - 1) // 32 * 32
    ldh = ((dim + 127) & ~127) // 2 if i8 else (dim + 63) & ~63
    passes = (nq_pad // BN + qblk_max - 1) // qblk_max
    return [NB, BN, nq_pad, qblk_max, ldq, ldh, passes]


def parent_budget(level, k, t_min, rows_scored, sweep):
    if sweep:  # run_i8_single
        t_want = t_min if t_min > 128 else (128 if k <= 24 else (4 * k + 88 if 4 * k + 88 < 512 else 512))
        E = 2
        while 64 * E < t_want and E < 8:
            E *= 2
        T = 64 * E
        return [T, E, 0, T, int(k > T)]  # (finalize's cap = T)
    i8 = level == 2
    hi = level == 0 or i8
    if i8:
        t_want = t_min if t_min > 4 * k + 88 else (4 * k + 88 if 4 * k + 88 < 512 else 512)
    elif hi:
        t_want = t_min if t_min > 2 * k + 56 else 2 * k + 56
    else:
        t_want = t_min if t_min > k + 28 else k + 28
    E = 1
    while 64 * E < min(t_want, 512) and E < 8:
        E *= 2
    wide = (not hi) and t_min > 512
    T = 4096 if wide else 64 * E
    if wide:
        E = 1
        while 64 * E < k and E < 8:
            E *= 2
    refused = k > T or k > 512
    cap_max = 65536 if wide else 16384
    want, c2 = rows_scored + 64, 1024
    while c2 < want and c2 < cap_max:
        c2 <<= 1
    return [T, E, int(wide), c2, int(refused)]


def test_tile_geometry_is_the_parents(lib):
    o = (C.c_longlong * 7)()
    for nq, level, dim in itertools.product(NQS, (0, 1, 2), (8, 31, 32, 33, 72, 128, 129, 768, 1030, 3072)):
        lib.mp_geometry(nq, level, dim, o)
        assert list(o) == parent_geometry(nq, level, dim), (nq, level, dim)
    # by hand: 300 queries on the hi pass = two 256-wide blocks in ONE pass over the plane; 1030 queries = five blocks, two passes
    lib.mp_geometry(300, 0, 72, o)
    assert list(o) == [4, 256, 512, 2, 96, 128, 1]
    lib.mp_geometry(1030, 1, 72, o)
    assert list(o) == [4, 256, 1280, 4, 96, 128, 2]
    lib.mp_geometry(5, 1, 72, o)  # the micro tile is the split pass's alone
    assert list(o)[:3] == [-1, 16, 16]
    lib.mp_geometry(5, 2, 72, o)  # int8: rows of 128 bytes = 64 16-bit units
    assert list(o) == [0, 32, 32, 1, 96, 64, 1]


def test_level_budget_is_the_parents(lib):
    o = (C.c_longlong * 5)()
    for level, k, t_min, rows, sweep in itertools.product((0, 1, 2), KS, T_MINS, ROWS, (0, 1)):
        lib.mp_budget(level, k, t_min, rows, sweep, o)
        assert list(o) == parent_budget(level, k, t_min, rows, sweep), (level, k, t_min, rows, sweep)
    # by hand (T, E, wide, cap, refused), 10M rows
    for args, want in {(1, 10, 0, 0): [64, 1, 0, 16384, 0], (1, 100, 0, 0): [128, 2, 0, 16384, 0],    # split: k + 28
                       (0, 10, 0, 0): [128, 2, 0, 16384, 0], (0, 100, 0, 0): [256, 4, 0, 16384, 0],   # hi: 2k + 56
                       (0, 10, 512, 0): [512, 8, 0, 16384, 0], (0, 363, 0, 0): [512, 8, 0, 16384, 0],
                       (2, 10, 0, 0): [128, 2, 0, 16384, 0], (2, 100, 0, 0): [512, 8, 0, 16384, 0],   # int8: min(4k + 88, 512)
                       (2, 10, 0, 1): [128, 2, 0, 128, 0], (2, 24, 0, 1): [128, 2, 0, 128, 0],        # the sweep: 128 while k <= 24
                       (2, 25, 0, 1): [256, 4, 0, 256, 0], (2, 10, 512, 1): [512, 8, 0, 512, 0],
                       (1, 10, 4096, 0): [4096, 1, 1, 65536, 0], (1, 100, 4096, 0): [4096, 2, 1, 65536, 0],
                       (0, 10, 4096, 0): [512, 8, 0, 16384, 0],                                          # (the hi pass has no wide level)
                       (1, 513, 4096, 0): [4096, 8, 1, 65536, 1], (1, 484, 0, 0): [512, 8, 0, 16384, 0],
                       (1, 513, 0, 0): [512, 8, 0, 16384, 1]}.items():
        lib.mp_budget(args[0], args[1], args[2], 10 ** 7, args[3], o)
        assert list(o) == want, args
    lib.mp_budget(1, 10, 0, 900, 0, o)  # a small store: slots for every row
    assert o[3] == 1024
    lib.mp_budget(1, 10, 0, 16321, 0, o)
    assert o[3] == 16384
    w = (C.c_ulonglong * 4)()
    for k in KS:
        lib.mp_wants(k, w)
        assert list(w) == [k + 28, 2 * k + 56, min(4 * k + 88, 512), 128]
    for k in list(KS) + [227, 362, 364, 2 ** 40]:
        assert bool(lib.mp_hi_k_ok(k, 0)) == (2 * k + 56 <= 512)        # ott_policy.h's formula before the header existed
        assert bool(lib.mp_hi_k_ok(k, 1)) == (k + k // 3 + 28 <= 512)
    assert [bool(lib.mp_hi_k_ok(k, h)) for k, h in ((228, 0), (229, 0), (363, 1), (364, 1))] == [True, False, True, False]


# ---- error model -------------------------------------------------------------------------------------------------------------------
def parent_i8_c_eps_units(dim):
    return f32(0.125) * f32(dim) + f32(32.0)


def parent_model(level, hi_f16, dim, metric, bf3, ppm, hi_rel, min_pos_inv, qn_max, thr):
    """run_mfma's lines between "error bound on |approx - exact|" and the buffers, in order"""
    i8 = level == 2
    hi = level == 0 or i8
    u = f32(5.9604645e-8)
    fmt_u = f32(0.015625) if i8 else f32(4.8828125e-4) if hi_f16 else f32(0.00390625)
    qrel_cap = f32(1.01) * fmt_u
    esc = f32(1.0) if ppm == 1000000 else f32(ppm) * f32(1e-6)
    if i8:
        inner = (f32(2.0) * f32(dim) + f32(32.0)) * u if metric == EUCLIDEAN else parent_i8_c_eps_units(dim) * u
    elif hi:
        inner = (f32(2.5) * f32(dim) + f32(32.0)) * u
    elif bf3:
        inner = (f32(3.75) * f32(dim) + f32(32.0)) * u + f32(3.03) * f32(1.52587890625e-5)
    else:
        inner = ((f32(2.0) if metric == EUCLIDEAN else f32(1.25)) * f32(dim) + f32(32.0)) * u
    c_eps = esc * inner
    eps_r = esc * (f32(1.001) * (f32(1.0) + fmt_u) * hi_rel) if hi else f32(0.0)
    r_max = eps_r + esc * (f32(1.001) * qrel_cap) if hi else f32(0.0)
    max_norm = (f32(1.0) / min_pos_inv) * f32(1.000001) if min_pos_inv < INF else f32(0.0)
    if metric == COSINE:
        eps_max = c_eps + r_max
    elif metric == DOT:
        eps_max = (c_eps + r_max) * max_norm * qn_max
    else:
        eps_max = c_eps * (qn_max + max_norm) * (qn_max + max_norm) + f32(2.0) * r_max * qn_max * max_norm
    out = [c_eps, eps_r, qrel_cap if hi else f32(0.0), esc, r_max, max_norm, eps_max, f32(1.0 if eps_max < INF else 0.0)]
    for cmp in range(6):
        flo, fhi = -INF, INF
        if cmp in (CMP_GT, CMP_GTE):
            flo = thr - eps_max
        elif cmp in (CMP_LT, CMP_LTE):
            fhi = thr + eps_max
        elif cmp == CMP_EQ:
            flo, fhi = thr - eps_max, thr + eps_max
        out += [flo, fhi]
    return out


def parent_sweep_model(dim, metric, ppm, i8_rel, min_pos_inv, qnorm):
    """run_i8_single's own copy ("as run_mfma's int8 level"): c_eps, eps_r, qrel_cap, esc, r_max, max_norm, eps_max"""
    u = f32(5.9604645e-8)
    esc = f32(1.0) if ppm == 1000000 else f32(ppm) * f32(1e-6)
    fmt_u = f32(0.015625)
    qrel_cap = f32(1.01) * fmt_u
    c_eps = esc * parent_i8_c_eps_units(dim) * u
    eps_r = esc * (f32(1.001) * (f32(1.0) + fmt_u) * i8_rel)
    r_max = eps_r + esc * (f32(1.001) * qrel_cap)
    max_norm = (f32(1.0) / min_pos_inv) * f32(1.000001) if min_pos_inv < INF else f32(0.0)
    eps_max = c_eps + r_max if metric == COSINE else (c_eps + r_max) * max_norm * qnorm
    return [c_eps, eps_r, qrel_cap, esc, r_max, max_norm, eps_max]


# every (level, hi_f16, bf3) the runners can produce: the hi pass on a bf16 or a half plane (bf3 = true with it), the split pass on
# split-bf16 operands or the f32 pipe, the int8 level (run_mfma level 2 and the sweep: no half, bf3 = true)
MODEL_KINDS = ((0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 0, 0), (2, 0, 1))
DIMS = (8, 72, 768, 1030, 3072)
PPMS = (1, 250000, 1000000)
RELS = (0.0, 1e-7, 3e-4, 4e-3, 0.5)
MIN_POS_INVS = (np.inf, 1e-6, 1.0, 1e3, 1e-30)  # (the last one and 3e38 below: norms at which the bound itself overflows and the level refuses)
QN_MAXS = (0.0, 1e-18, 1.0, 3e4, 1e18, 3e38)


def test_error_model_is_the_parents(lib):
    o = (C.c_float * 20)()
    refused = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for (level, hi_f16, bf3), metric, dim, ppm in itertools.product(MODEL_KINDS, (COSINE, EUCLIDEAN, DOT), DIMS, PPMS):
            for rel, mpi, qn, thr in itertools.product(RELS, MIN_POS_INVS, QN_MAXS, (0.25, -3e38)):
                lib.mp_model(level, hi_f16, dim, metric, bf3, ppm, rel, mpi, qn, thr, o)
                want = parent_model(level, hi_f16, dim, metric, bf3, ppm, f32(rel), f32(mpi), f32(qn), f32(thr))
                assert np.array_equal(bits(list(o)), bits(want)), (level, hi_f16, bf3, metric, dim, ppm, rel, mpi, qn, thr, list(o), want)
                refused += o[7] == 0.0
                if level == 2 and metric != EUCLIDEAN and thr == 0.25:
                    # the sweep's model and run_mfma's int8 level: one object for the same inputs (the sweep has one query: qn_max is its norm)
                    assert np.array_equal(bits(list(o)[:7]), bits(parent_sweep_model(dim, metric, ppm, f32(rel), f32(mpi), f32(qn))))
    assert refused > 0  # (the non-finite bound the level refuses is in the grid)


def test_error_model_by_hand(lib):
    o = (C.c_float * 20)()
    u = 2.0 ** -24
    # f32 pipe, cosine, 768 dims, unit norms: (1.25 * 768 + 32) * 2^-24 — every term exact in float32
    lib.mp_model(1, 0, 768, COSINE, 0, 1000000, 0.0, 1.0, 1.0, 0.5, o)
    assert o[0] == 992.0 * u and o[1] == 0.0 and o[2] == 0.0 and o[3] == 1.0 and o[4] == 0.0 and o[6] == o[0] and o[7] == 1.0
    assert (o[8 + 2 * CMP_NONE], o[9 + 2 * CMP_NONE]) == (-np.inf, np.inf)
    assert (o[8 + 2 * CMP_GT], o[9 + 2 * CMP_GT]) == (float(f32(0.5) - f32(992.0 * u)), np.inf) == (o[8 + 2 * CMP_GTE], o[9 + 2 * CMP_GTE])
    assert (o[8 + 2 * CMP_LT], o[9 + 2 * CMP_LT]) == (-np.inf, float(f32(0.5) + f32(992.0 * u))) == (o[8 + 2 * CMP_LTE], o[9 + 2 * CMP_LTE])
    assert (o[8 + 2 * CMP_EQ], o[9 + 2 * CMP_EQ]) == (o[8 + 2 * CMP_GT], o[9 + 2 * CMP_LT])
    # the same on squared L2: 2 * 768 + 32 units, times (1 + 1.000001)^2
    lib.mp_model(1, 0, 768, EUCLIDEAN, 0, 1000000, 0.0, 1.0, 1.0, 0.5, o)
    assert o[0] == 1568.0 * u and o[5] == float(f32(1.000001))
    # int8, cosine / dot: dim / 8 + 32 units; squared L2 2 dim + 32; a query may measure up to 1.01 * 2^-6
    lib.mp_model(2, 0, 768, DOT, 1, 1000000, 0.0, 1.0, 1.0, 0.5, o)
    assert o[0] == 128.0 * u and o[2] == float(f32(1.01) * f32(2.0 ** -6))
    lib.mp_model(2, 0, 768, EUCLIDEAN, 1, 1000000, 0.0, 1.0, 1.0, 0.5, o)
    assert o[0] == 1568.0 * u
    # hi pass: 2.5 dim + 32 units; the cap on a query's loss follows the plane's format (bf16 2^-8, half 2^-11)
    lib.mp_model(0, 0, 768, COSINE, 1, 1000000, 0.0, 1.0, 1.0, 0.5, o)
    assert o[0] == 1952.0 * u and o[2] == float(f32(1.01) * f32(2.0 ** -8))
    lib.mp_model(0, 1, 768, COSINE, 1, 1000000, 0.0, 1.0, 1.0, 0.5, o)
    assert o[2] == float(f32(1.01) * f32(2.0 ** -11))
    # a store without a regular row: max_norm 0; a dot bound is then 0 whatever the query
    lib.mp_model(1, 0, 768, DOT, 1, 1000000, 0.0, np.inf, 3e4, 0.5, o)
    assert o[5] == 0.0 and o[6] == 0.0
    # eps_scale_ppm = 250000: every term times float32(250000) * float32(1e-6)
    lib.mp_model(1, 0, 768, COSINE, 0, 250000, 0.0, 1.0, 1.0, 0.5, o)
    assert o[3] == float(f32(250000) * f32(1e-6)) and o[0] == float(f32(o[3]) * f32(992.0 * u))
    # huge norms on squared L2: the bound overflows, the level refuses
    lib.mp_model(0, 0, 768, EUCLIDEAN, 1, 1000000, 3e-4, 1e-30, 1e18, 0.5, o)
    assert o[6] == np.inf and o[7] == 0.0


def test_query_regular(lib):
    reg = lambda x: bool(lib.mp_query_regular(float(f32(x))))  # noqa: E731
    up, down = lambda x: np.nextafter(f32(x), INF), lambda x: np.nextafter(f32(x), -INF)  # noqa: E731
    assert reg(0.0) and reg(1.0) and reg(1e-18) and reg(1e18) and reg(3e4)
    assert not reg(up(1e18)) and reg(down(1e18))
    assert not reg(down(1e-18)) and reg(up(1e-18))
    assert not reg(1e-20) and not reg(1e-45) and not reg(1e19) and not reg(np.inf) and not reg(np.nan) and not reg(-1.0)


# ---- query norms -------------------------------------------------------------------------------------------------------------------
def parent_norms(rows, metric, want_amax):
    """per query what run_mfma's 8-at-a-time loop computed: the float sum of float squares in order, the f64 sum where the parent took it"""
    dim = rows.shape[1]
    qnorm, qinv, qamax = [], [], []
    for x in rows:
        fs = np.add.accumulate(x * x, dtype=f32)[-1]
        nrm = np.sqrt(fs)
        xd = x.astype(f64)
        ds = f64(0.0)
        if metric == EUCLIDEAN:
            ds = np.add.accumulate(xd * xd, dtype=f64)[-1]
            nd = np.sqrt(ds)
        elif nrm >= f32(1e-15) and nrm <= f32(1e18):
            nd = f64(nrm) * (f64(1.0) + f64(dim) * f64(5.9604644775390625e-8))
        else:
            ds = np.add.accumulate(xd * xd, dtype=f64)[-1]
            nd = np.sqrt(ds)
        qnorm.append(f32(nd * (f64(1.0) + f64(1e-6))))
        qinv.append(f32(ds) if metric == EUCLIDEAN else (f32(1.0) / nrm if nrm != 0 else f32(0.0)))
        qamax.append(np.fmax.reduce(np.abs(x), initial=f32(0.0)) if want_amax else f32(0.0))  # (fmaxf: a NaN element is passed over)
    qn_max = f32(0.0)
    for v in qnorm:
        if v > qn_max:
            qn_max = v
    return np.array(qnorm, f32), np.array(qinv, f32), np.array(qamax, f32), qn_max


def row_pool(dim, rng):
    """the awkward rows the issue lists, then ordinary ones"""
    unit = np.full(dim, 1.0 / np.sqrt(dim))
    pool = [np.zeros(dim), rng.uniform(-1, 1, dim), unit * 1e-20, unit * 1e19, rng.uniform(-1, 1, dim), rng.uniform(-1, 1, dim),
            rng.normal(0, 30, dim), rng.uniform(-1e-3, 1e-3, dim), rng.uniform(-1, 1, dim)]
    pool[1][dim // 2] = 1e-42  # one denormal element
    pool[4][dim - 1] = np.inf
    pool[5][0] = np.nan
    return [p.astype(f32) for p in pool]


def test_query_norms_are_the_parents(lib):
    rng = np.random.default_rng(5)
    fp = C.POINTER(C.c_float)
    seen_irregular = set()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        for dim in (1, 7, 8, 72, 1030):
            pool = row_pool(dim, rng)
            for nq in (1, 7, 8, 9, 17):
                for start in (range(len(pool)) if nq == 1 else (0, 3)):  # (one query: each kind of row on its own)
                    rows = np.ascontiguousarray(np.stack([pool[(start + i) % len(pool)] for i in range(nq)]))
                    for metric, want_amax in ((COSINE, 1), (DOT, 0), (EUCLIDEAN, 1)):
                        qnorm, qinv, qamax = np.full(nq, -7.0, f32), np.full(nq, -7.0, f32), np.zeros(nq, f32)
                        qn_max = lib.mp_norms(rows.ctypes.data_as(fp), nq, dim, metric, want_amax, qnorm.ctypes.data_as(fp), qinv.ctypes.data_as(fp),
                                              qamax.ctypes.data_as(fp))
                        w_norm, w_inv, w_amax, w_max = parent_norms(rows, metric, want_amax)
                        at = (dim, nq, start, metric)
                        assert np.array_equal(bits(qnorm), bits(w_norm)), (at, qnorm, w_norm)
                        assert np.array_equal(bits(qinv), bits(w_inv)), (at, qinv, w_inv)
                        assert np.array_equal(bits(qamax), bits(w_amax)), (at, qamax, w_amax)
                        assert bits(qn_max) == bits(w_max), at
                        for i in range(nq):
                            kind = (start + i) % len(pool)
                            regular = bool(lib.mp_query_regular(float(qnorm[i])))
                            # zero and ordinary rows are inside the error model; norms of 1e-20 and 1e19, an infinity and a NaN are not
                            # (with one dimension the denormal element is the whole row: a norm of 1e-42)
                            assert regular == (kind not in (2, 3, 4, 5) and not (kind == 1 and dim == 1)), (at, i, qnorm[i])
                            if not regular and kind != 1:
                                seen_irregular.add(kind)
    assert seen_irregular == {2, 3, 4, 5}


# ---- the query block ---------------------------------------------------------------------------------------------------------------
def parent_layout(nq_pad, ldq, n_runs, n_prefix, own_operand):
    """run_mfma's off_* chain (CNT_STRIDE = 32, sizeof(ott_run) = 16)"""
    q_bytes = nq_pad * ldq * 4
    off_qinv = q_bytes
    off_qnorm = off_qinv + nq_pad * 4
    off_tau = off_qnorm + nq_pad * 4
    off_cntA = (off_tau + nq_pad * 4 + 127) & ~127
    off_cntB = off_cntA + nq_pad * 32 * 4
    off_over = off_cntB + nq_pad * 32 * 4
    off_qrel = off_over + nq_pad * 4
    off_gate = off_qrel + nq_pad * 4
    off_runs = (off_gate + nq_pad * 4 + 15) & ~15
    off_prefix = off_runs + n_runs * 16
    off_qraw = ((off_prefix + n_prefix * 4 + 127) & ~127) if own_operand else 0
    tot = off_qraw + q_bytes if own_operand else off_prefix + n_prefix * 4
    return [q_bytes, off_qinv, off_qnorm, off_tau, off_cntA, off_cntB, off_over, off_qrel, off_gate, off_runs, off_prefix, off_qraw, tot]


def test_query_block_layout_is_the_parents(lib):
    o = (C.c_ulonglong * 13)()
    for nq_pad, ldq, n_runs, own in itertools.product((1, 16, 32, 64, 256, 1280), (32, 96, 1056, 3072), (1, 2, 5, 1000), (0, 1)):
        for n_prefix in (n_runs + 1, 64 * n_runs + 1):
            lib.mp_layout(nq_pad, ldq, n_runs, n_prefix, own, o)
            v = list(o)
            assert v == parent_layout(nq_pad, ldq, n_runs, n_prefix, own), (nq_pad, ldq, n_runs, n_prefix, own)
            q_bytes, qinv, qnorm, tau, cntA, cntB, over, qrel, gate, runs, prefix, qraw, total = v
            chain = [0, qinv, qnorm, tau, cntA, cntB, over, qrel, gate, runs, prefix] + ([qraw] if own else [])
            assert all(a < b for a, b in zip(chain, chain[1:])) and chain[-1] < total
            assert cntA % 128 == 0 and cntB % 128 == 0 and runs % 16 == 0 and qraw % 128 == 0
            assert cntA - tau >= nq_pad * 4 and runs - gate >= nq_pad * 4  # (the aligned fields start behind the column in front)
            assert total == (qraw + q_bytes if own else prefix + 4 * n_prefix)
            assert (qraw == 0) == (not own)
