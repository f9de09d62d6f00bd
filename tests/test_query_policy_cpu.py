"""CPU: which path a query takes and how a store's batch cascade backs off (otters_amd/csrc/ott_policy.h, DESIGN.md 3.2 "Path
choice").  The header is compiled on its own with the host compiler behind a small extern "C" driver, as test_exact_prune_sketch3_bound.py
does for ott_prune.h: the code under test is the code libotters_hip.so ships.
  1. the back-off rules (CascadeState) against tables written out by hand from the rules: more than 1/8 of a batch open widens the
     level first and backs off after that, the share of recent batches that needed a second pass is an average new = (3 old +
     1024 [any open]) / 4 in integers, a back-off doubles within its clamp and arms the skip counter with it;
  2. choose_path against a transcription of the cost model as query_core carried it before the header existed (`parent_choice`
     below: the same expressions in the same order on float64, broadcast over the grid's axes), on every point of the grid;
  3. the laziness of the plane state: only an AUTO query looks at it, and only ONE query asks whether the first plane is ready.
The GPU half: test_gpu_mfma.py, test_gpu_clustered.py (path_used, refined, i8_refined, retries, gate_failed on real stores)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include "ott_policy.h"
using namespace ott;
static PathIn path_in(unsigned long long rows, unsigned long long n_runs, unsigned dim, unsigned nq, unsigned long long k, int metric, int path,
                      int filter_cmp, int flat, int mfma_f32, int no_hi_pass, int no_batch_image, int hi_fmt, int exact_small) {
    return PathIn{rows, n_runs, dim, (dim + 7u) & ~7u, nq, k, (uint32_t)metric, (uint32_t)filter_cmp, (uint32_t)path, flat != 0,
                  mfma_f32 != 0, no_hi_pass != 0, no_batch_image != 0, hi_fmt, exact_small};
}
// one choice; planes = {have_hi, hi_f16, i8_off, first plane ready}; calls[0] / calls[1] count the two callbacks
extern "C" int pol_choose(unsigned long long rows, unsigned long long n_runs, unsigned dim, unsigned nq, unsigned long long k, int metric, int path,
                          int filter_cmp, int flat, int mfma_f32, int no_hi_pass, int no_batch_image, int hi_fmt, int exact_small,
                          const int* planes, int widened, int* calls) {
    const PathIn in = path_in(rows, n_runs, dim, nq, k, metric, path, filter_cmp, flat, mfma_f32, no_hi_pass, no_batch_image, hi_fmt, exact_small);
    return (int)choose_path(
        in,
        [&] {
            calls[0]++;
            return PathPlanes{planes[0] != 0, planes[1] != 0, planes[2] != 0, widened != 0};
        },
        [&] {
            calls[1]++;
            return planes[3] != 0;
        });
}
// the grid in C order: rows, dim, nq, k, hi_fmt, mfma_f32, no_hi_pass, planes, widened, exact_small
extern "C" void pol_grid(const long long* rows, int n_rows, const int* dim, int n_dim, const int* nq, int n_nq, const long long* k, int n_k,
                         const int* hi_fmt, int n_fmt, const int* planes, int n_pl, const int* exact_small, int n_es, int metric, int path,
                         int filter_cmp, int no_batch_image, unsigned char* out) {
    int calls[2] = {0, 0};
    for (int a = 0; a < n_rows; a++)
        for (int b = 0; b < n_dim; b++)
            for (int c = 0; c < n_nq; c++)
                for (int d = 0; d < n_k; d++)
                    for (int e = 0; e < n_fmt; e++)
                        for (int f32 = 0; f32 < 2; f32++)
                            for (int nhp = 0; nhp < 2; nhp++)
                                for (int p = 0; p < n_pl; p++)
                                    for (int w = 0; w < 2; w++)
                                        for (int x = 0; x < n_es; x++)
                                            *out++ = (unsigned char)pol_choose((unsigned long long)rows[a], 1, (unsigned)dim[b], (unsigned)nq[c],
                                                                               (unsigned long long)k[d], metric, path, filter_cmp, 0, f32, nhp,
                                                                               no_batch_image, hi_fmt[e], exact_small[x], planes + 4 * p, w, calls);
}
extern "C" const char* pol_refusal() { return kMfmaRefusal; }
extern "C" int pol_single_sweep(unsigned nq, unsigned long long k_q, int filter_cmp, int metric, unsigned dim, int last) {
    return i8_single_sweep(nq, k_q, (uint32_t)filter_cmp, (uint32_t)metric, dim, last != 0) ? 1 : 0;
}

extern "C" CascadeState* cs_new() { return new CascadeState(); }
extern "C" void cs_free(CascadeState* c) { delete c; }
static std::atomic<int>* cs_field(CascadeState* c, int i) {
    std::atomic<int>* f[11] = {&c->hi_skip, &c->hi_backoff, &c->i8_skip, &c->i8_backoff, &c->i8_t512, &c->i8_fail_ema,
                               &c->spec_skip, &c->spec_backoff, &c->wide_first, &c->hi_t512, &c->hi_fail_ema};
    return f[i];
}
extern "C" int cs_get(CascadeState* c, int i) { return cs_field(c, i)->load(); }
extern "C" void cs_set(CascadeState* c, int i, int v) { cs_field(c, i)->store(v); }
extern "C" int cs_consume(CascadeState* c, int i) { return CascadeState::consume(*cs_field(c, i)) ? 1 : 0; }
extern "C" int cs_i8_widened(CascadeState* c) { return c->i8_widened() ? 1 : 0; }
extern "C" int cs_hi_wide(CascadeState* c) { return c->hi_wide() ? 1 : 0; }
extern "C" void cs_after_i8(CascadeState* c, unsigned nq, unsigned long long open, unsigned gate_failed, int wide_now, unsigned long long k_q) {
    c->after_i8(nq, (size_t)open, gate_failed, wide_now != 0, k_q);
}
extern "C" void cs_after_hi(CascadeState* c, unsigned nq, unsigned long long open, unsigned gate_failed, int wide_now, unsigned hi_t) {
    c->after_hi(nq, (size_t)open, gate_failed, wide_now != 0, hi_t);
}
extern "C" void cs_after_spec(CascadeState* c, int gate_failed) { c->after_spec(gate_failed != 0); }
extern "C" void cs_arm_wide_first(CascadeState* c, unsigned long long open, unsigned nq) { c->arm_wide_first((size_t)open, nq); }
extern "C" int cs_take_wide_first(CascadeState* c, unsigned nq) { return c->take_wide_first(nq) ? 1 : 0; }
"""

EXACT, MFMA, REFUSED = 0, 1, 2                   # PathChoice
PATH_AUTO, PATH_EXACT, PATH_MFMA = 0, 1, 2       # ott_path
COSINE, EUCLIDEAN, DOT, MANHATTAN = 0, 1, 2, 3   # ott_metric
CMP_NONE, CMP_GT, CMP_EQ = 0, 2, 5               # ott_cmp
FIELDS = ["hi_skip", "hi_backoff", "i8_skip", "i8_backoff", "i8_t512", "i8_fail_ema", "spec_skip", "spec_backoff", "wide_first",
          "hi_t512", "hi_fail_ema"]
ULL, U, I = C.c_ulonglong, C.c_uint, C.c_int
PI, PLL = C.POINTER(C.c_int), C.POINTER(C.c_longlong)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("policy")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.pol_choose.argtypes = [ULL, ULL, U, U, ULL, I, I, I, I, I, I, I, I, I, PI, I, PI]
    L.pol_choose.restype = I
    L.pol_grid.argtypes = [PLL, I, PI, I, PI, I, PLL, I, PI, I, PI, I, PI, I, I, I, I, I, C.POINTER(C.c_ubyte)]
    L.pol_grid.restype = None
    L.pol_refusal.restype = C.c_char_p
    L.pol_single_sweep.argtypes = [U, ULL, I, I, U, I]
    L.cs_new.restype = C.c_void_p
    L.cs_free.argtypes = [C.c_void_p]
    for name, args in [("cs_get", [I]), ("cs_set", [I, I]), ("cs_consume", [I]), ("cs_i8_widened", []), ("cs_hi_wide", []),
                       ("cs_after_i8", [U, ULL, U, I, ULL]), ("cs_after_hi", [U, ULL, U, I, U]), ("cs_after_spec", [I]),
                       ("cs_arm_wide_first", [ULL, U]), ("cs_take_wide_first", [U])]:
        getattr(L, name).argtypes = [C.c_void_p] + args
    return L


class State:
    """one store's CascadeState, driven the way the cascade drives it"""

    def __init__(self, lib):
        self.L, self.p = lib, lib.cs_new()

    def __del__(self):
        self.L.cs_free(self.p)

    def get(self, *names):
        return tuple(self.L.cs_get(self.p, FIELDS.index(n)) for n in names)

    def all(self):
        return dict(zip(FIELDS, self.get(*FIELDS)))

    def consume(self, name):
        return bool(self.L.cs_consume(self.p, FIELDS.index(name)))

    def hi_batch(self, nq, open_, gate_failed=0):
        """a batch that reaches the hi level: sits out while hi_skip runs, else the pass re-scores 2k + 56 or, once wide, 512"""
        if self.consume("hi_skip"):
            return "skipped"
        wide = bool(self.L.cs_hi_wide(self.p))
        self.L.cs_after_hi(self.p, nq, open_, gate_failed, wide, 512 if wide else 0)
        return "ran"

    def i8_batch(self, nq, open_, k_q, gate_failed=0):
        if self.consume("i8_skip"):
            return "skipped"
        wide = self.consume("i8_t512")
        self.L.cs_after_i8(self.p, nq, open_, gate_failed, wide, k_q)
        return "ran"


HI = ("hi_skip", "hi_backoff", "hi_t512", "hi_fail_ema")
I8 = ("i8_skip", "i8_backoff", "i8_t512", "i8_fail_ema")


def test_hi_level_whole_batch_open_widens_then_backs_off(lib):
    """16 of 16 queries open in every batch the hi pass runs on, none through a gate"""
    s = State(lib)
    assert s.hi_batch(16, 16) == "ran" and s.get(*HI) == (0, 0, 1, 0)      # first answer: 512 candidates from the next batch on
    assert s.hi_batch(16, 16) == "ran" and s.get(*HI) == (4, 4, 1, 256)    # wide and still failing: sit out 4 batches
    untouched = {k: v for k, v in s.all().items() if k not in HI}
    assert all(v == 0 for v in untouched.values()), untouched              # the hi level's rules write the hi level's fields only
    # every re-probe fails again: the skip doubles up to 64; the average is (3 old + 1024) / 4 in integers
    for skip, (armed, ema) in zip([4, 8, 16, 32, 64], [(8, 448), (16, 592), (32, 700), (64, 781), (64, 841)]):
        for left in range(skip - 1, -1, -1):
            assert s.hi_batch(16, 16) == "skipped" and s.get("hi_skip")[0] == left
        assert s.hi_batch(16, 16) == "ran" and s.get(*HI) == (armed, armed, 1, ema), (skip, s.get(*HI))
    # a clean re-probe: the average drops to 3/4, and while it says that more than half of the recent batches needed the split pass
    # (> 512) the store keeps sitting out; the next clean one (472) forgets the back-off.  hi_t512 stays set
    for _ in range(64):
        assert s.hi_batch(16, 0) == "skipped"
    assert s.hi_batch(16, 0) == "ran" and s.get(*HI) == (64, 64, 1, 630)
    for _ in range(64):
        assert s.hi_batch(16, 0) == "skipped"
    assert s.hi_batch(16, 0) == "ran" and s.get(*HI) == (0, 0, 1, 472)
    assert s.hi_batch(16, 0) == "ran" and s.get(*HI) == (0, 0, 1, 354)


def test_hi_level_clean_batch_forgets_a_young_back_off(lib):
    s = State(lib)
    s.hi_batch(16, 16)
    s.hi_batch(16, 16)
    assert s.get(*HI) == (4, 4, 1, 256)
    for _ in range(4):
        assert s.hi_batch(16, 0) == "skipped"
    assert s.hi_batch(16, 0) == "ran" and s.get(*HI) == (0, 0, 1, 192)  # back-off 0, the wide setting stays
    # a batch whose open queries all failed through their speculative gate counts as clean (also when the gate count is the larger)
    s.L.cs_set(s.p, FIELDS.index("hi_backoff"), 8)
    assert s.hi_batch(16, 5, gate_failed=5) == "ran" and s.get(*HI) == (0, 0, 1, 144)
    assert s.hi_batch(16, 3, gate_failed=5) == "ran" and s.get(*HI) == (0, 0, 1, 108)
    # hi_tmin = 512 (debug option) on a store that is not wide: a failing batch backs off at once instead of widening
    t = State(lib)
    t.L.cs_after_hi(t.p, 16, 16, 0, 0, 512)
    assert t.get(*HI) == (4, 4, 0, 256)


def test_hi_level_few_open_backs_off_through_the_average(lib):
    """2 of 64 open in every batch (<= nq / 8): the average runs 256, 448, 592 and the third batch backs off"""
    s = State(lib)
    assert s.hi_batch(64, 2) == "ran" and s.get(*HI) == (0, 0, 0, 256)
    assert s.hi_batch(64, 2) == "ran" and s.get(*HI) == (0, 0, 0, 448)
    assert s.hi_batch(64, 2) == "ran" and s.get(*HI) == (4, 4, 0, 592)
    # exactly nq / 8 open is not "more than 1/8": it neither widens nor backs off by itself
    t = State(lib)
    assert t.hi_batch(64, 8) == "ran" and t.get(*HI) == (0, 0, 0, 256)
    assert t.hi_batch(64, 9) == "ran" and t.get(*HI) == (0, 0, 1, 0)


def test_i8_level_first_failure_widens_only_below_512_candidates(lib):
    for k_q, widens in [(1, True), (10, True), (105, True), (106, False), (128, False)]:  # 4k + 88 < 512 <=> k <= 105
        s = State(lib)
        assert s.i8_batch(16, 16, k_q) == "ran"
        assert s.get(*I8) == ((0, 0, 64, 0) if widens else (4, 4, 0, 256)), k_q
        assert bool(lib.cs_i8_widened(s.p)) == widens
    # widened: each call that runs the level counts one off the 64, and a failure now backs off
    s = State(lib)
    s.i8_batch(16, 16, 10)
    assert s.i8_batch(16, 0, 10) == "ran" and s.get(*I8) == (0, 0, 63, 0)
    assert s.i8_batch(16, 16, 10) == "ran" and s.get(*I8) == (4, 4, 62, 256)
    for left in (3, 2, 1, 0):
        assert s.i8_batch(16, 16, 10) == "skipped" and s.get(*I8) == (left, 4, 62, 256)
    assert s.i8_batch(16, 16, 10) == "ran" and s.get(*I8) == (8, 8, 61, 448)
    untouched = {k: v for k, v in s.all().items() if k not in I8}
    assert all(v == 0 for v in untouched.values()), untouched
    # the countdown runs out: not widened any more, the next failure widens again
    s = State(lib)
    s.L.cs_set(s.p, FIELDS.index("i8_t512"), 1)
    assert s.i8_batch(16, 0, 10) == "ran" and s.get(*I8) == (0, 0, 0, 0) and not lib.cs_i8_widened(s.p)
    assert s.i8_batch(16, 16, 10) == "ran" and s.get(*I8) == (0, 0, 64, 0)


def test_i8_level_average_threshold_by_batch_size(lib):
    """one query open per batch: up to 128 queries back off above 400 (the second batch, 448), up to 512 above 512 (the third,
    592), larger batches never through the average alone"""
    for nq, backs_off_at in [(16, 2), (128, 2), (129, 3), (512, 3), (513, None), (1024, None)]:
        s = State(lib)
        emas = []
        for batch in range(1, 41):
            assert s.i8_batch(nq, 1, 10) == "ran"
            emas.append(s.get("i8_fail_ema")[0])
            if batch == backs_off_at:
                assert s.get("i8_skip", "i8_backoff") == (4, 4), (nq, batch)
                break
            assert s.get("i8_skip", "i8_backoff") == (0, 0), (nq, batch)
        assert emas[:3] == [256, 448, 592][:len(emas)]
        if backs_off_at is None:
            assert emas[-1] == 1021  # the fixed point of (3 e + 1024) / 4 in integers
    # more than 1/8 of a large batch open still backs off (widened, or k too large to widen)
    s = State(lib)
    assert s.i8_batch(1024, 129, 128) == "ran" and s.get(*I8) == (4, 4, 0, 256)
    s = State(lib)
    assert s.i8_batch(1024, 128, 128) == "ran" and s.get(*I8) == (0, 0, 0, 256)
    # a clean batch forgets the back-off
    s = State(lib)
    s.L.cs_set(s.p, FIELDS.index("i8_backoff"), 32)
    assert s.i8_batch(64, 0, 10) == "ran" and s.get(*I8) == (0, 0, 0, 0)


def test_spec_gate_backs_off_8_to_256(lib):
    s = State(lib)
    for b in (8, 16, 32, 64, 128, 256, 256):
        lib.cs_after_spec(s.p, 1)
        assert s.get("spec_skip", "spec_backoff") == (b, b)
    assert s.consume("spec_skip") and s.get("spec_skip", "spec_backoff") == (255, 256)
    lib.cs_after_spec(s.p, 0)  # a clean batch: the next failure starts at 8 again (the running skip is left to run out)
    assert s.get("spec_skip", "spec_backoff") == (255, 0)
    lib.cs_after_spec(s.p, 1)
    assert s.get("spec_skip", "spec_backoff") == (8, 8)
    untouched = {k: v for k, v in s.all().items() if k not in ("spec_skip", "spec_backoff")}
    assert all(v == 0 for v in untouched.values()), untouched


def test_skip_counter_and_wide_first(lib):
    s = State(lib)
    assert not s.consume("hi_skip") and s.get("hi_skip") == (0,)
    lib.cs_set(s.p, FIELDS.index("hi_skip"), 2)
    assert s.consume("hi_skip") and s.consume("hi_skip") and not s.consume("hi_skip") and s.get("hi_skip") == (0,)
    lib.cs_set(s.p, FIELDS.index("hi_skip"), -1)  # (two contexts may both count the last one off)
    assert not s.consume("hi_skip") and s.get("hi_skip") == (-1,)
    # armed to 16 only when more than half the batch is open
    lib.cs_arm_wide_first(s.p, 8, 16)
    assert s.get("wide_first") == (0,)
    lib.cs_arm_wide_first(s.p, 9, 16)
    assert s.get("wide_first") == (16,)
    # consumed only for batches of more than 8 queries
    assert not lib.cs_take_wide_first(s.p, 8) and s.get("wide_first") == (16,)
    assert lib.cs_take_wide_first(s.p, 9) and s.get("wide_first") == (15,)
    for left in range(14, -1, -1):
        assert lib.cs_take_wide_first(s.p, 256) and s.get("wide_first") == (left,)
    assert not lib.cs_take_wide_first(s.p, 256) and s.get("wide_first") == (0,)


def test_single_sweep_predicate(lib):
    ok = dict(nq=1, k_q=24, cmp=CMP_GT, metric=COSINE, dim=3584, last=1)
    call = lambda **kw: lib.pol_single_sweep(*[{**ok, **kw}[n] for n in ("nq", "k_q", "cmp", "metric", "dim", "last")])  # noqa: E731
    assert call() == 1 and call(metric=DOT) == 1 and call(cmp=CMP_NONE) == 1 and call(k_q=1, dim=8) == 1
    for bad in (dict(nq=2), dict(k_q=25), dict(cmp=CMP_EQ), dict(metric=EUCLIDEAN), dict(dim=3585), dict(last=0)):
        assert call(**bad) == 0, bad


# ---- path choice ---------------------------------------------------------------------------------------------------------------
def hi_k_ok(k, half):
    return np.where(half, k + k // 3 + 28 <= 512, 2 * k + 56 <= 512)


def parent_choice(rows, dim, nq, k, metric, path, filter_cmp, hi_fmt, mfma_f32, no_hi_pass, no_batch_image, exact_small, have_hi, hi_f16,
                  i8_off, ready, widened, n_runs=1, flat=False):
    """query_core's path choice as it stood before ott_policy.h, expression by expression.  Integers are int64 arrays (or ints),
    times float64, every argument broadcasts; both sides of a C `?:` are computed and np.where picks."""
    rows, dim, nq, k = (np.asarray(v, np.int64) for v in (rows, dim, nq, k))
    hi_fmt, exact_small = np.asarray(hi_fmt, np.int64), np.asarray(exact_small, np.int64)
    mfma_f32, no_hi_pass, no_batch_image, have_hi, hi_f16, i8_off, ready, widened = (
        np.asarray(v, bool) for v in (mfma_f32, no_hi_pass, no_batch_image, have_hi, hi_f16, i8_off, ready, widened))
    dimq = (dim + 7) // 8 * 8
    k_q = np.minimum(k, rows)
    mfma_ok = (k_q + 28 <= 512) & (dim >= 8)
    if flat or metric == MANHATTAN:
        return np.full(np.broadcast(mfma_ok).shape, EXACT, np.uint8)
    if path == PATH_MFMA:
        return np.where(mfma_ok, MFMA, REFUSED).astype(np.uint8)
    if path == PATH_EXACT:
        return np.full(np.broadcast(mfma_ok).shape, EXACT, np.uint8)
    bytes_ = rows.astype(np.float64) * (4.0 * dim + 4.0)
    full_passes, last_m = nq // 4, nq % 4
    pass_fixed = np.array([0.0, 0.05, 0.06, 0.085, 0.115])

    def t_pass(m):
        return pass_fixed[m] + bytes_ / 6.5e9 * (1.0 + 0.027 * (m - 1))

    t_exact = full_passes * t_pass(np.int64(4)) + np.where(last_m != 0, t_pass(last_m), 0.0)
    bn = np.where(nq <= 16, 16, np.where(nq <= 32, 32, np.where(nq <= 64, 64, np.where(nq <= 128, 128, 256))))
    nq_pad = ((nq + bn - 1) // bn * bn).astype(np.float64)
    f32pipe = mfma_f32
    plane_half = np.where(have_hi, hi_f16, hi_fmt != 0)
    hi_ok = ~f32pipe & hi_k_ok(k_q, plane_half) & ~no_hi_pass
    i8_wanted = ((hi_fmt == -1) | (hi_fmt == 2)) & ~mfma_f32 & ~no_hi_pass & ~no_batch_image
    i8_ok = hi_ok & i8_wanted & ~i8_off & (k_q <= 128)
    t_stream = (np.where(i8_ok, 0.25, np.where(hi_ok, 0.5, 1.0)) * bytes_ * ((nq + 255) // 256).astype(np.float64)
                / np.where(i8_ok, 6.0e9, np.where(hi_ok, np.where(nq <= 32, 6.5e9, 6.2e9), 5.9e9)))
    t_pipe = (2.0 * dim * rows.astype(np.float64) * nq_pad
              / np.where(i8_ok, 1500e9, np.where(hi_ok, 800e9, np.where((bn >= 32) & ~f32pipe, 330e9, 125e9))))
    t_cand = np.where(i8_ok, 0.0003 * 384.0,
                      np.where(hi_ok & (k_q > 36), 0.0003 * ((2 * k_q + 56 + 63) // 64 * 64 - 128).astype(np.float64), 0.0))
    t_mfma = 0.16 + 0.0045 * nq + t_cand + np.where(t_stream > t_pipe, t_stream, t_pipe)
    single = i8_ok & (nq == 1) & (k_q <= 24) & (filter_cmp != CMP_EQ) & (metric != EUCLIDEAN) & (dim <= 3584) & ~widened
    t_mfma = np.where(single, 0.11 + 0.25 * bytes_ / 6.5e9, t_mfma)
    batch_worthy = (nq > np.where(hi_ok, 1, 4)) | ((nq == 1) & hi_ok & ready)
    use_mfma = mfma_ok & batch_worthy & (rows >= 2048) & (t_mfma < t_exact)
    k_e = np.minimum(k, rows * nq)
    small = use_mfma & (nq <= 16) & (k_e <= 128) & (dimq <= 2048) & (exact_small != 0) & (exact_small != 1) & (rows // 64 + n_runs <= 1024)
    t_rows8 = 0.035 + ((nq + 7) // 8).astype(np.float64) * (0.040 + 0.7e-6 * rows.astype(np.float64))
    use_mfma = use_mfma & ~(small & (t_rows8 < 0.9 * (0.12 + 0.0035 * nq)))
    return np.where(use_mfma, MFMA, EXACT).astype(np.uint8)


ROWS = [1, 2047, 2048, 10_000, 70_000, 300_000, 1_000_000, 10_000_000]
DIMS = [4, 8, 64, 768, 3584, 4096]
NQS = [1, 2, 4, 5, 8, 16, 17, 64, 256, 1024]
KS = [1, 10, 24, 25, 36, 37, 100, 128, 129, 228, 229, 363, 364, 484, 485]
HI_FMTS = [-1, 0, 1, 2]
# (have_hi, hi_f16, i8_off, first plane ready): nothing built yet; a half plane resident; a plane that fell back to bf16; the same
# on a store whose int8 plane is switched off
PLANES = [(0, 0, 0, 0), (1, 1, 0, 1), (1, 0, 0, 1), (1, 0, 1, 1)]
EXACT_SMALL = [0, 1, 2]


def grid_axes():
    shape = (len(ROWS), len(DIMS), len(NQS), len(KS), len(HI_FMTS), 2, 2, len(PLANES), 2, len(EXACT_SMALL))

    def ax(i, v, dtype=np.int64):
        return np.asarray(v, dtype).reshape([-1 if j == i else 1 for j in range(len(shape))])

    pl = np.asarray(PLANES, np.int64)
    return shape, dict(rows=ax(0, ROWS), dim=ax(1, DIMS), nq=ax(2, NQS), k=ax(3, KS), hi_fmt=ax(4, HI_FMTS), mfma_f32=ax(5, [0, 1]),
                       no_hi_pass=ax(6, [0, 1]), have_hi=ax(7, pl[:, 0]), hi_f16=ax(7, pl[:, 1]), i8_off=ax(7, pl[:, 2]),
                       ready=ax(7, pl[:, 3]), widened=ax(8, [0, 1]), exact_small=ax(9, EXACT_SMALL))


def header_grid(lib, metric, path, filter_cmp=CMP_GT, no_batch_image=0):
    shape, _ = grid_axes()
    out = np.empty(shape, np.uint8)
    arr = lambda v, t: np.ascontiguousarray(v, t)  # noqa: E731
    rows, ks = arr(ROWS, np.int64), arr(KS, np.int64)
    dims, nqs, fmts, pls, es = (arr(v, np.int32) for v in (DIMS, NQS, HI_FMTS, PLANES, EXACT_SMALL))
    lib.pol_grid(rows.ctypes.data_as(PLL), len(ROWS), dims.ctypes.data_as(PI), len(DIMS), nqs.ctypes.data_as(PI), len(NQS),
                 ks.ctypes.data_as(PLL), len(KS), fmts.ctypes.data_as(PI), len(HI_FMTS), pls.ctypes.data_as(PI), len(PLANES),
                 es.ctypes.data_as(PI), len(EXACT_SMALL), metric, path, filter_cmp, no_batch_image, out.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return out


@pytest.mark.parametrize("path", [PATH_AUTO, PATH_EXACT, PATH_MFMA], ids=["auto", "exact", "mfma"])
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN, DOT, MANHATTAN], ids=["cosine", "euclidean", "dot", "manhattan"])
def test_choose_path_equals_the_parent_on_the_grid(lib, metric, path):
    shape, axes = grid_axes()
    want = np.broadcast_to(parent_choice(metric=metric, path=path, filter_cmp=CMP_GT, no_batch_image=False, **axes), shape)
    got = header_grid(lib, metric, path)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])
    if path == PATH_AUTO and metric != MANHATTAN:  # the grid is no formality: both answers, and each option axis moves some point
        assert 0.05 < (want == MFMA).mean() < 0.95
        for axis in range(len(shape)):
            if axis == 8 and metric == EUCLIDEAN:
                continue  # (a widened int8 level matters to the single-query sweep alone, which scores cosine / dot)
            assert (np.diff(want.astype(np.int8), axis=axis) != 0).any(), axis
    if path == PATH_MFMA and metric != MANHATTAN:
        assert (want == REFUSED).any() and (want == MFMA).any() and not (want == EXACT).any()
    if metric == MANHATTAN:
        assert (want == EXACT).all()


@pytest.mark.parametrize("filter_cmp,no_batch_image", [(CMP_EQ, 0), (CMP_NONE, 1)], ids=["eq-filter", "no-batch-image"])
def test_choose_path_equals_the_parent_beside_the_grid(lib, filter_cmp, no_batch_image):
    """the two inputs the grid holds fixed: an equality filter (no single-query int8 sweep) and no_batch_image (no int8 level)"""
    shape, axes = grid_axes()
    want = np.broadcast_to(parent_choice(metric=COSINE, path=PATH_AUTO, filter_cmp=filter_cmp, no_batch_image=bool(no_batch_image), **axes), shape)
    got = header_grid(lib, COSINE, PATH_AUTO, filter_cmp, no_batch_image)
    assert np.array_equal(got, want)
    base = header_grid(lib, COSINE, PATH_AUTO)
    assert (got != base).any()


def choose(lib, rows, dim, nq, k, metric=COSINE, path=PATH_AUTO, filter_cmp=CMP_GT, flat=0, mfma_f32=0, no_hi_pass=0, no_batch_image=0,
           hi_fmt=-1, exact_small=-1, planes=(0, 0, 0, 0), widened=0):
    calls = (C.c_int * 2)(0, 0)
    r = lib.pol_choose(rows, 1, dim, nq, k, metric, path, filter_cmp, flat, mfma_f32, no_hi_pass, no_batch_image, hi_fmt, exact_small,
                       (C.c_int * 4)(*planes), widened, calls)
    return r, tuple(calls)


def test_choose_path_anchors(lib):
    """70 000 x 64, top-10 cosine, default options (what test_gpu_mfma.py asserts of a real store): 64 queries take the batch path
    (exact: 16 passes of 0.115 ms + 18.2 MB at 6.5 TB/s ~ 1.89 ms; batch < 0.6 ms), 4 queries one exact pass (0.118 ms against
    >= 0.178)"""
    for nq, want in [(64, MFMA), (4, EXACT)]:
        assert choose(lib, 70_000, 64, nq, 10)[0] == want
        assert int(parent_choice(70_000, 64, nq, 10, COSINE, PATH_AUTO, CMP_GT, -1, 0, 0, 0, -1, 0, 0, 0, 0, 0)) == want


def test_choose_path_refusal_and_laziness(lib):
    assert lib.pol_refusal() == b"ott_query: the MFMA path needs dim >= 8 and k <= 484"
    assert choose(lib, 70_000, 4, 64, 10, path=PATH_MFMA) == (REFUSED, (0, 0))
    assert choose(lib, 70_000, 64, 64, 485, path=PATH_MFMA) == (REFUSED, (0, 0))
    assert choose(lib, 300, 64, 64, 485, path=PATH_MFMA) == (MFMA, (0, 0))  # k is cut to the rows scored first
    # a Manhattan, flat or explicit-path query touches no plane state
    assert choose(lib, 70_000, 64, 64, 484, path=PATH_MFMA) == (MFMA, (0, 0))
    assert choose(lib, 70_000, 64, 64, 10, path=PATH_EXACT) == (EXACT, (0, 0))
    assert choose(lib, 70_000, 64, 64, 10, metric=MANHATTAN) == (EXACT, (0, 0))
    assert choose(lib, 70_000, 64, 64, 10, metric=MANHATTAN, path=PATH_MFMA) == (EXACT, (0, 0))
    assert choose(lib, 70_000, 64, 64, 10, flat=1) == (EXACT, (0, 0))
    # AUTO takes ONE snapshot; only one query that the hi pass could serve asks whether the first plane is ready
    assert choose(lib, 70_000, 64, 64, 10) == (MFMA, (1, 0))
    assert choose(lib, 70_000, 64, 2, 10)[1] == (1, 0)
    assert choose(lib, 10_000_000, 768, 1, 10) == (EXACT, (1, 1))
    assert choose(lib, 10_000_000, 768, 1, 10, planes=(1, 0, 0, 1)) == (MFMA, (1, 1))
    assert choose(lib, 10_000_000, 768, 1, 10, mfma_f32=1, planes=(1, 0, 0, 1)) == (EXACT, (1, 0))
    assert choose(lib, 10_000_000, 768, 1, 10, no_hi_pass=1, planes=(1, 0, 0, 1)) == (EXACT, (1, 0))
