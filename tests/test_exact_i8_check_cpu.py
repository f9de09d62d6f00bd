"""CPU: the int8 check of the pruned exact sweep's survivors (otters_amd/csrc/ott_i8_check.h, ott_exact_plan.h: prune_plan_i8_check;
DESIGN.md 3.1b, "survivors on the int8 plane").  The headers are compiled on their own with the host compiler, as in
test_exact_prune_head_bound.py, and driven over planes made the way i8_rows_kernel makes them (tests/adversarial_i8.py: i8_plane).
  1. the one quantiser: i8_query_quant against the numpy restatement of run_i8_single's (adversarial_i8.i8_query), the word form
     the kernel uses against the element form, NaN / inf / zero queries;
  2. |approximate - the oracle's exact-order score| <= eps on every regular row: uniform and Gaussian rows, the nearly constant
     rows of adversarial_i8.build_case, rows at int8 rounding midpoints; cosine and dot;
  3. the drop rule: no row whose score ordinal is at or above the gate is dropped, Take Max and Take Min, with the gate at every
     row's own ordinal and one either side; rows marked irregular, NaN and infinite approximate scores are kept; an open gate
     drops nothing; a bound shrunk through eps_scale_ppm does drop rows it must keep (the check can fail);
  4. the rule's table: plane not ready, option 0, a query outside the error model, a list wider than one entry per lane, no head;
  5. the keep rate on 100 000 uniform rows of dim 768 with the gate at the 10th best of the first 1/32 (printed; the README of
     profiles/exact_i8_check quotes it).
The GPU half is tests/test_gpu_exact_i8_check.py; the sanitizer walk is tests/host/exact_i8_check_walk.cpp."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import adversarial_i8 as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include "ott_exact_plan.h"
#include "ott_i8_check.h"
using namespace ott;
// o: pf, s_q, inv_sq, qnorm, qrel; returns regular
extern "C" int ck_quant(const float* q, unsigned dim, int cosine, float q_inv, signed char* q8, float* o) {
    const I8Query x = i8_query_quant(q, dim, cosine != 0, q_inv, (int8_t*)q8);
    o[0] = x.pf; o[1] = x.s_q; o[2] = x.inv_sq; o[3] = x.qnorm; o[4] = x.qrel;
    return x.regular ? 1 : 0;
}
// the operand as the kernel makes it: one word per four dims, zeros past dim
extern "C" void ck_words(const float* q, unsigned dim, float pf, float inv_sq, unsigned n_words, unsigned* w) {
    for (unsigned i = 0; i < n_words; i++) {
        float q4[4];
        for (unsigned j = 0; j < 4; j++) q4[j] = 4 * i + j < dim ? q[4 * i + j] : 0.0f;
        w[i] = i8_quant_word(q4, pf, inv_sq);
    }
}
extern "C" int ck_eps(const float* q, unsigned dim, unsigned metric, float q_inv, int ppm, float plane_rel, float vn_max, float* eps) {
    const I8Query x = i8_query_quant(q, dim, metric == OTT_METRIC_COSINE, q_inv, nullptr);
    const I8CheckEps e = i8_check_eps(dim, metric, ppm, plane_rel, x, vn_max);
    *eps = e.eps;
    return e.ok ? 1 : 0;
}
// rows of a plane (ld8 bytes each, the operand as words): the approximate scores
extern "C" void ck_approx(unsigned long long n, unsigned ld8, const signed char* plane, const float* s_v, const float* vinv, const unsigned* qw, int cosine, float s_q,
                          float* approx) {
    for (unsigned long long r = 0; r < n; r++) {
        int acc = 0;
        for (unsigned c = 0; c < ld8; c++) acc += (int)plane[r * ld8 + c] * (int)(signed char)((qw[c >> 2] >> (8 * (c & 3))) & 0xFFu);
        approx[r] = i8_approx_score(acc, i8_row_factor(cosine != 0, vinv[r], s_v[r], s_q));
    }
}
extern "C" int ck_drops(float approx, float eps, int take_max, unsigned gate, int outside) { return i8_check_drops(approx, eps, take_max != 0, gate, outside != 0) ? 1 : 0; }
extern "C" void ck_drops_rows(unsigned long long n, const float* approx, float eps, int take_max, unsigned gate, const unsigned char* flag, unsigned char* out) {
    for (unsigned long long r = 0; r < n; r++) out[r] = i8_check_drops(approx[r], eps, take_max != 0, gate, (flag[r] & 5u) != 0) ? 1 : 0;
}
extern "C" unsigned ck_ord(float f, int take_max) { return i8_check_ord(f, take_max != 0); }
extern "C" int ck_rule(unsigned c, int head, int E, int plane_ready, int option, int eps_ok) {
    PruneIn in{};
    in.E = E;
    return prune_plan_i8_check(in, PrunePlan{c, true, 64}, head != 0, I8CheckState{plane_ready != 0, option, eps_ok != 0}) ? 1 : 0;
}
"""

P = C.POINTER(C.c_float)
PU = C.POINTER(C.c_uint32)
PB = C.POINTER(C.c_ubyte)
PS = C.POINTER(C.c_byte)
COSINE, DOT = 0, 2
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("i8check")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    u, i, f, ull = C.c_uint, C.c_int, C.c_float, C.c_ulonglong
    for name, args, res in (("ck_quant", [P, u, i, f, PS, P], i), ("ck_words", [P, u, f, f, u, PU], None), ("ck_eps", [P, u, u, f, i, f, f, P], i),
                            ("ck_approx", [ull, u, PS, P, P, PU, i, f, P], None), ("ck_drops", [f, f, i, u, i], i),
                            ("ck_drops_rows", [ull, P, f, i, u, PB, PB], None), ("ck_ord", [f, i], u), ("ck_rule", [u, i, i, i, i, i], i)):
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, res
    return L


@pytest.fixture(scope="module")
def oracle():
    import oracle as O
    O.build()
    return O


def tkey(x):
    b = int(np.float32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def ord_of(x, take_max):
    k = tkey(x)
    return k if take_max else (~k & 0xFFFFFFFF)


def quant(lib, q, metric):
    q = np.ascontiguousarray(q, np.float32)
    q_inv = float(A.inv_norms(q[None, :])[0]) if np.isfinite(q).all() and np.any(q) else 0.0
    q8 = np.zeros(q.size, np.int8)
    o = np.zeros(5, np.float32)
    reg = lib.ck_quant(q.ctypes.data_as(P), q.size, int(metric == COSINE), q_inv, q8.ctypes.data_as(PS), o.ctypes.data_as(P))
    return dict(q8=q8, pf=o[0], s_q=o[1], inv_sq=o[2], qnorm=o[3], qrel=o[4], regular=bool(reg), q_inv=q_inv)


def plane_of(rows):
    """the plane, its scales, the flags (bit 2: a row that loses more than 2^-5) and the measured loss of the regular rows as the
    library keeps it (a float, rounded up)"""
    t, s_v, rel = A.i8_plane(rows)
    n, dim = rows.shape
    ld8 = (dim + 127) // 128 * 128
    plane = np.zeros((n, ld8), np.int8)
    plane[:, :dim] = t
    flag = np.where(rel > 2.0 ** -5, 4, 0).astype(np.uint8)
    reg = rel[flag == 0]
    plane_rel = float(np.nextafter(np.float32(reg.max() * (1 + 1e-6)), np.float32(np.inf))) if reg.size else 0.0
    return plane, s_v.astype(np.float32), flag, plane_rel


def check_inputs(lib, rows, q, metric, ppm=1000000):
    """approximate scores, flags and the certified eps of a corpus, all through the header"""
    rows = np.ascontiguousarray(rows, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    n, dim = rows.shape
    plane, s_v, flag, plane_rel = plane_of(rows)
    x = quant(lib, q, metric)
    nw = plane.shape[1] // 4
    qw = np.zeros(nw, np.uint32)
    lib.ck_words(q.ctypes.data_as(P), dim, x["pf"], x["inv_sq"], nw, qw.ctypes.data_as(PU))
    vinv = A.inv_norms(rows)
    approx = np.zeros(n, np.float32)
    lib.ck_approx(n, plane.shape[1], plane.ctypes.data_as(PS), s_v.ctypes.data_as(P), vinv.ctypes.data_as(P), qw.ctypes.data_as(PU), int(metric == COSINE), x["s_q"],
                  approx.ctypes.data_as(P))
    vn_max = float(np.float32(1.0) / vinv[np.isfinite(vinv) & (vinv > 0)].min()) * 1.000001
    eps = C.c_float(0.0)
    ok = lib.ck_eps(q.ctypes.data_as(P), dim, metric, x["q_inv"], ppm, plane_rel, vn_max, C.byref(eps))
    return approx, flag, float(eps.value), bool(ok), x, qw


def oracle_scores(O, rows, q, metric):
    h = O.vec_query(rows, q, metric, O.TAKE_MAX, rows.shape[0], 0, 0.0, ties=O.TIES_CANONICAL)
    assert h.size == rows.shape[0]
    out = np.empty(rows.shape[0], np.float32)
    out[h["index"].astype(np.int64)] = h["score"]
    return out


def midpoint_rows(rng, n, dim):
    """every element just below an int8 rounding midpoint of its row's own scale: the image loses nearly half a step everywhere,
    always downwards in magnitude"""
    k = rng.integers(1, 126, (n, dim)).astype(np.float64)
    k[:, 0] = 127.0  # the row's largest element fixes the scale: s_v = v_0 / 127
    sgn = np.where(rng.random((n, dim)) < 0.5, -1.0, 1.0)
    s = rng.uniform(0.002, 0.004, (n, 1))
    v = sgn * s * (k + 0.5 - 2.0 ** -12)
    v[:, 0] = s[:, 0] * 127.0
    return v.astype(np.float32)


def corpora(dim, seed):
    rng = np.random.default_rng(seed)
    yield "uniform", rng.uniform(-1, 1, (2048, dim)).astype(np.float32), rng.uniform(-1, 1, dim).astype(np.float32)
    yield "gaussian", rng.standard_normal((2048, dim)).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
    yield "midpoints", midpoint_rows(rng, 2048, dim), rng.uniform(0.1, 1, dim).astype(np.float32)
    # nearly constant int8-representable rows against a constant query: the measured losses are ~1e-7 and the exact-order lane sums
    # drift, every add rounding the same way (adversarial_i8.py) — the accumulation term of the bound is all there is
    s = np.float32(0.37 / 127)
    m = rng.integers(0, dim, 2048)
    c = rng.integers(40, 128, 2048)
    K = np.where(np.arange(dim)[None, :] < m[:, None], 127, c[:, None])
    K[:, -1] = 127
    yield "nearly constant", (K.astype(np.float32) * s).astype(np.float32), np.full(dim, np.float32(127) * s, np.float32)
    if dim == 768:  # the corpora that broke round 5's bound, as test_gpu_i8_bound.py builds them
        for metric in ("cosine", "dot"):
            case = A.build_case(dim, metric, seed=21 + dim, n=8000)
            yield "adversarial_i8 (" + metric + ")", np.ascontiguousarray(case["rows"], np.float32), np.ascontiguousarray(case["query"], np.float32)


def test_quantiser_is_the_single_query_sweeps(lib):
    rng = np.random.default_rng(3)
    for dim in (8, 96, 232, 768, 773):
        for metric, name in ((COSINE, "cosine"), (DOT, "dot")):
            q = (rng.uniform(-1, 1, dim) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
            x = quant(lib, q, metric)
            t, s_q, qrel = A.i8_query(q, name)
            assert x["regular"] and np.array_equal(x["q8"].astype(np.int32), t) and x["s_q"] == s_q
            assert abs(float(x["qrel"]) - qrel) <= 1e-6 * qrel and x["qnorm"] >= np.linalg.norm(q.astype(np.float64))
            # the kernel's word form: the same bytes, zeros past dim
            nw = (dim + 127) // 128 * 32
            qw = np.zeros(nw, np.uint32)
            lib.ck_words(q.ctypes.data_as(P), dim, x["pf"], x["inv_sq"], nw, qw.ctypes.data_as(PU))
            by = qw.view(np.int8)
            assert np.array_equal(by[:dim], x["q8"]) and not by[dim:].any()
    # queries outside the error model: not regular, never a bound; a NaN element quantises to 0
    for bad in (np.full(96, np.nan, np.float32), np.full(96, np.inf, np.float32), np.full(96, 1e30, np.float32), np.full(96, 1e-30, np.float32)):
        x = quant(lib, bad, DOT)
        eps = C.c_float(0.0)
        assert not x["regular"] and not lib.ck_eps(bad.ctypes.data_as(P), 96, DOT, 0.0, 1000000, 0.004, 1.0, C.byref(eps))
    q = np.ones(96, np.float32)
    q[5] = np.nan
    assert quant(lib, q, DOT)["q8"][5] == 0
    z = quant(lib, np.zeros(96, np.float32), COSINE)
    assert z["regular"] and z["s_q"] == 1.0 and not z["q8"].any() and z["qrel"] == 0.0
    # a loss above what the bound assumes of the operand's norm (one huge element among small ones): no bound
    q = np.full(768, 1e-3, np.float32)
    q[0] = 1.0
    eps = C.c_float(0.0)
    assert quant(lib, q, DOT)["qrel"] > 0.0158 and not lib.ck_eps(q.ctypes.data_as(P), 768, DOT, 0.0, 1000000, 0.004, 1.0, C.byref(eps))
    # metrics without the check
    q = np.ones(96, np.float32)
    assert not lib.ck_eps(q.ctypes.data_as(P), 96, 1, 0.1, 1000000, 0.004, 1.0, C.byref(eps))


@pytest.mark.parametrize("dim", [232, 768])
def test_bound_and_drop_rule_on_every_row(lib, oracle, dim):
    O = oracle
    for name, rows, q in corpora(dim, 11 + dim):
        for metric in (COSINE, DOT):
            approx, flag, eps, ok, x, _ = check_inputs(lib, rows, q, metric)
            assert ok and np.isfinite(eps) and eps > 0, (name, metric)
            exact = oracle_scores(O, rows, q[None, :], O.METRIC_COSINE if metric == COSINE else O.METRIC_DOT)
            assert np.array_equal(exact.view(np.uint32), A.exact_scores(rows, q, "cosine" if metric == COSINE else "dot")[0].view(np.uint32)), (name, metric)
            reg = flag == 0
            err = np.abs(approx.astype(np.float64) - exact.astype(np.float64))
            assert reg.any() and err[reg].max() <= eps, (name, metric, float(err[reg].max()), eps)
            print(f"{name:26s} dim {dim} metric {metric}: max |approx - exact| / eps = {err[reg].max() / eps:.3f}, eps = {eps:.3e}, qrel = {x['qrel']:.2e}")
            # the drop rule at gates on and around every row's own ordinal (a sample of rows), both takes
            n = rows.shape[0]
            out = np.zeros(n, np.uint8)
            for take_max in (1, 0):
                ords = np.array([ord_of(s, take_max) for s in exact], np.uint64)
                for r in np.random.default_rng(dim).choice(n, 24, replace=False):
                    for gate in {int(ords[r]) - 1, int(ords[r]), int(ords[r]) + 1} - {0, 1 << 32}:
                        lib.ck_drops_rows(n, approx.ctypes.data_as(P), eps, take_max, gate, flag.ctypes.data_as(PB), out.ctypes.data_as(PB))
                        must_stay = ords >= gate
                        assert not (out.astype(bool) & must_stay).any(), (name, metric, take_max, gate)
                        assert not out[flag != 0].any()
                # an open gate drops nothing
                lib.ck_drops_rows(n, approx.ctypes.data_as(P), eps, take_max, 0, flag.ctypes.data_as(PB), out.ctypes.data_as(PB))
                assert not out.any()


def test_a_shrunk_bound_drops_rows_it_must_keep(lib, oracle):
    """eps_scale_ppm = 1 leaves a bound far below the int8 plane's real loss: on midpoint rows the rule then drops rows at the gate."""
    O = oracle
    rng = np.random.default_rng(5)
    rows, q = midpoint_rows(rng, 2048, 768), rng.uniform(0.1, 1, 768).astype(np.float32)
    approx, flag, eps, ok, _, _ = check_inputs(lib, rows, q, COSINE, ppm=1)
    assert ok
    exact = oracle_scores(O, rows, q[None, :], O.METRIC_COSINE)
    gate = ord_of(np.sort(exact)[-100], True)
    out = np.zeros(rows.shape[0], np.uint8)
    lib.ck_drops_rows(rows.shape[0], approx.ctypes.data_as(P), eps, 1, gate, flag.ctypes.data_as(PB), out.ctypes.data_as(PB))
    ords = np.array([ord_of(s, True) for s in exact], np.uint64)
    assert (out.astype(bool) & (ords >= gate)).any()


def test_irregular_and_nan_rows_are_kept(lib):
    inf, nan = float("inf"), float("nan")
    gate = ord_of(0.5, True)
    assert lib.ck_drops(0.1, 0.01, 1, gate, 0) == 1       # well below the gate: goes
    assert lib.ck_drops(0.1, 0.01, 1, gate, 1) == 0       # ... unless the row is outside the plane's error model
    assert lib.ck_drops(nan, 0.01, 1, gate, 0) == 0 and lib.ck_drops(0.1, nan, 1, gate, 0) == 0
    assert lib.ck_drops(inf, 0.01, 1, gate, 0) == 0 and lib.ck_drops(-inf, 0.01, 1, gate, 0) == 0
    assert lib.ck_drops(0.1, inf, 1, gate, 0) == 0
    assert lib.ck_drops(0.1, 0.01, 1, 0, 0) == 0          # the gate is open
    # the edge is one float beyond the rounded sum: a score exactly approx + eps away is at the gate, not below it
    a, e = np.float32(0.25), np.float32(0.125)
    assert lib.ck_drops(a, e, 1, ord_of(a + e, True), 0) == 0 and lib.ck_drops(a, e, 1, ord_of(np.nextafter(a + e, np.float32(1)), True), 0) == 0
    assert lib.ck_drops(a, e, 1, ord_of(np.nextafter(np.nextafter(a + e, np.float32(1)), np.float32(1)), True), 0) == 1
    assert lib.ck_drops(a, e, 0, ord_of(a - e, False), 0) == 0 and lib.ck_drops(a, e, 0, ord_of(np.nextafter(a - e, np.float32(-1)), False), 0) == 0
    assert lib.ck_drops(a, e, 0, ord_of(np.nextafter(np.nextafter(a - e, np.float32(-1)), np.float32(-1)), False), 0) == 1
    for v in (0.0, -0.0, 1.5, -1.5, inf, -inf, 1e-45):
        for tm in (0, 1):
            assert lib.ck_ord(v, tm) == ord_of(v, tm)


def test_the_rules_table(lib):
    # c, head, E, plane_ready, option, eps_ok
    assert lib.ck_rule(1, 1, 1, 1, -1, 1) == 1 and lib.ck_rule(1, 1, 1, 1, 1, 1) == 1
    assert lib.ck_rule(1, 1, 1, 0, -1, 1) == 0   # the plane is not ready
    assert lib.ck_rule(1, 1, 1, 1, 0, 1) == 0    # the option says never
    assert lib.ck_rule(1, 1, 1, 1, -1, 0) == 0   # the query is outside the error model
    assert lib.ck_rule(1, 1, 2, 1, -1, 1) == 0 and lib.ck_rule(1, 1, 4, 1, -1, 1) == 0  # more than one list entry per lane
    assert lib.ck_rule(1, 0, 1, 1, -1, 1) == 0   # no head form
    assert lib.ck_rule(0, 1, 1, 1, -1, 1) == 0   # no pruned sweep at all


def test_keep_rate_on_uniform_rows(lib):
    """100 000 uniform rows of dim 768, the gate at the 10th best of the first 1/32: what the check lets through to the f32 finish
    (a figure, printed; exact scores by the numpy restatement of the reference's order)."""
    rng = np.random.default_rng(0)
    n, dim = 100_000, 768
    rows, q = rng.uniform(-1, 1, (n, dim)).astype(np.float32), rng.uniform(-1, 1, dim).astype(np.float32)
    approx, flag, eps, ok, x, _ = check_inputs(lib, rows, q, COSINE)
    assert ok
    exact = A.exact_scores(rows, q, "cosine")[0]
    gate_score = np.sort(exact[:n // 32])[-10]
    gate = ord_of(gate_score, True)
    out = np.zeros(n, np.uint8)
    lib.ck_drops_rows(n, approx.ctypes.data_as(P), eps, 1, gate, flag.ctypes.data_as(PB), out.ctypes.data_as(PB))
    kept = int((out == 0).sum())
    at_or_above = int((exact >= gate_score).sum())
    err = np.abs(approx.astype(np.float64) - exact).max()
    print(f"keep rate: {kept} of {n} rows ({100.0 * kept / n:.3f} %), {at_or_above} at or above the gate; eps = {eps:.3e} (cosine units), "
          f"max |approx - exact| = {err:.3e}, score sigma = {exact.std():.4f}, gate = {gate_score:.4f}")
    # (the upper figure is reasoned, not measured: the 10th best of 3 125 scores sits near z = 2.7 of the scores' distribution, eps is
    # 0.24 sigma at dim 768 (8.4e-3 against 1 / sqrt(768)), so the rows kept lie above z = 2.4 or so: under 1 %; 5 % leaves room)
    assert err <= eps and kept >= at_or_above and kept < n // 20
