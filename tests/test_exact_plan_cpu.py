"""CPU: what the exact path's host side decides before it launches anything (otters_amd/csrc/ott_exact_plan.h): lists or sort
path and the list width, which kernel variant sweeps, queries per pass, passes, grid and the number of block lists, whether a
call is lean, the pruned sweep's eligibility, form, checkpoint and seed, the layout of the result block and the bytes scanned.
The header is compiled on its own with the host compiler behind a small extern "C" driver, with the library's
-ffp-contract=off, as test_sort_plan_cpu.py does for ott_sort_plan.h: the code under test is the code libotters_hip.so ships.
Expected values: transcriptions of the expressions run_exact (ott_api.hip), sweep_shape and
choose_path carried before the header existed, quoted in the docstrings, and tables written out by hand.
The GPU half: test_gpu_vecstore.py::test_exact_path_branches_report_their_documented_passes."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include "ott_exact_plan.h"
#include "ott_sort_plan.h"
#include "ott_prune.h"
using namespace ott;
extern "C" void xp_consts(unsigned long long* o) {
    o[0] = OTT_QEMB_MAX; o[1] = OTT_SKETCH_MAX_WORDS; o[2] = OTT_SKETCH1_MAX_WORDS; o[3] = OTT_SKETCH4_MAX_WORDS;
    o[4] = OTT_X_SEED_DIV; o[5] = sizeof(ott_hit);
}
extern "C" int xp_E(unsigned long long k) { return list_E(k); }
extern "C" unsigned xp_KS(int E) { return list_stride(E); }
extern "C" int xp_route(unsigned long long k, unsigned nq, unsigned long long rows, int from, int fetch) { return (int)lists_or_sort(k, nq, rows, from, fetch != 0); }
extern "C" int xp_fits(unsigned dimq, unsigned long long tiles) { return small_variant_fits(dimq, tiles) ? 1 : 0; }
extern "C" unsigned xp_variant(int exact_small, unsigned nq, int perq, int E, unsigned dimq, unsigned tiles) { return exact_variant(exact_small, nq, perq != 0, E, dimq, tiles); }
extern "C" int xp_lean(unsigned nq, unsigned dimq, unsigned long long n_runs) { return exact_lean(nq, dimq, (size_t)n_runs) ? 1 : 0; }
// o: E, KS, variant, tile, passes, grid, lean, then the block lists: plain, pruned with (gridA, gridB)
extern "C" void xp_plan(unsigned long long k, unsigned nq, int perq, unsigned dimq, unsigned tiles, unsigned long long n_runs, int exact_small, int stream_grid, int gridA, int gridB,
                        unsigned long long* o) {
    const ExactPlan x = exact_plan(k, nq, perq != 0, dimq, tiles, (size_t)n_runs, exact_small, stream_grid);
    o[0] = x.E; o[1] = x.KS; o[2] = x.variant; o[3] = x.tile; o[4] = x.passes; o[5] = x.grid; o[6] = x.lean;
    o[7] = exact_n_lists(x, nq, perq != 0, false, gridA, gridB); o[8] = exact_n_lists(x, nq, perq != 0, true, gridA, gridB);
}
extern "C" void xp_prune(unsigned dim, unsigned ld, unsigned metric, int perq, int lean, int flat, unsigned variant, int exact_prune, int exact_sketch, int present, int covers,
                         unsigned bits, unsigned words, unsigned stage0, unsigned long long rows, int E, unsigned long long* o) {
    const PruneIn in{dim, ld, metric, perq != 0, lean != 0, flat != 0, variant, exact_prune, exact_sketch, SketchState{present != 0, covers != 0, bits, words, stage0}, rows, E};
    const PrunePlan p = prune_plan(in);
    o[0] = p.c; o[1] = p.sketch; o[2] = p.seed;
}
extern "C" unsigned xp_stage0(unsigned nst, unsigned bits) { return prune_sketchb_stage0(nst, bits); }  // (ott_prune.h: what the store sets sk_stage0 from)
extern "C" void xp_layout(unsigned groups, unsigned KS, unsigned long long* o) {
    const ExactResult r = exact_result_layout(groups, KS);
    o[0] = r.cnt_pad; o[1] = r.bytes; o[2] = r.host_bytes;
}
extern "C" unsigned long long xp_bytes(unsigned passes, unsigned long long rows, unsigned dim, unsigned metric) { return exact_bytes_scanned(passes, rows, dim, metric); }
extern "C" unsigned long long xp_sort_bytes(unsigned passes, unsigned long long rows, unsigned dim, unsigned metric) { return sort_bytes_scanned(passes, rows, dim, metric); }
extern "C" int xp_sweep_rows8(unsigned nq, unsigned dimq, unsigned tiles, int exact_small) { return sweep_shape(nq, dimq, tiles, exact_small).rows8 ? 1 : 0; }
"""

COSINE, EUCLIDEAN, DOT, MANHATTAN = 0, 1, 2, 3
LISTS, SORT, REFUSED = 0, 1, 2  # ExactRoute
MAX_WORDS = {1: 10, 3: 54, 4: 108}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("exact_plan")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    ullp, ull, u, i = C.POINTER(C.c_ulonglong), C.c_ulonglong, C.c_uint, C.c_int
    for name, args, res in (("xp_consts", [ullp], None), ("xp_E", [ull], i), ("xp_KS", [i], u), ("xp_route", [ull, u, ull, i, i], i), ("xp_fits", [u, ull], i),
                            ("xp_variant", [i, u, i, i, u, u], u), ("xp_lean", [u, u, ull], i),
                            ("xp_plan", [ull, u, i, u, u, ull, i, i, i, i, ullp], None), ("xp_prune", [u, u, u, i, i, i, u, i, i, i, i, u, u, u, ull, i, ullp], None),
                            ("xp_stage0", [u, u], u), ("xp_layout", [u, u, ullp], None), ("xp_bytes", [u, ull, u, u], ull), ("xp_sort_bytes", [u, ull, u, u], ull),
                            ("xp_sweep_rows8", [u, u, u, i], i)):
        f = getattr(L, name)
        f.argtypes, f.restype = args, res
    return L


def test_moved_constants_keep_their_values(lib):
    o = (C.c_ulonglong * 6)()
    lib.xp_consts(o)
    # OTT_QEMB_MAX, OTT_SKETCH_MAX_WORDS, OTT_SKETCH1_MAX_WORDS, OTT_SKETCH4_MAX_WORDS (ott_internal.h), OTT_X_SEED_DIV (ott_api.hip), sizeof(ott_hit)
    assert list(o) == [896, 54, 10, 108, 32, 16]


# ---- lists or sort, E ---------------------------------------------------------------------------------------------------------------
def parent_E(k):
    """int E = k_eff <= 64 ? 1 : k_eff <= 128 ? 2 : k_eff <= 256 ? 4 : 8;   (and list_E, the same expression)"""
    return 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8


def parent_route(k_eff, nq, rows_scored, large_k_from, fetch):
    """if (k_eff > 512) { if (!fetch) return fail(...); return run_large_k(...); }
    const uint64_t pairs = pl.rows_scored * nq;
    const uint64_t from = s->opt.large_k_from > 0 ? (uint64_t)s->opt.large_k_from : ((nq == 1 || pairs <= (1ull << 19)) ? 512u : 128u);
    if (k_eff > from && fetch && pairs <= (1ull << 28)) return run_large_k(...);"""
    if k_eff > 512:
        return SORT if fetch else REFUSED
    pairs = rows_scored * nq
    frm = large_k_from if large_k_from > 0 else (512 if (nq == 1 or pairs <= (1 << 19)) else 128)
    return SORT if (k_eff > frm and fetch and pairs <= (1 << 28)) else LISTS


KS_ = (1, 16, 17, 64, 65, 128, 129, 256, 257, 512, 513)


def test_route_and_list_width_on_the_grid(lib):
    for k in KS_:
        if k <= 512:
            assert lib.xp_E(k) == parent_E(k)
            assert lib.xp_KS(parent_E(k)) == 64 * parent_E(k)
    for k, nq, frm, fetch in itertools.product(KS_, (1, 2, 4, 5), (0, 1, 128, 512), (0, 1)):
        for pairs in (1 << 19, 1 << 28):
            for rows in (pairs // nq - 1, pairs // nq, pairs // nq + 1, (pairs - 1) // nq, (pairs + nq - 1) // nq):
                assert lib.xp_route(k, nq, rows, frm, fetch) == parent_route(k, nq, rows, frm, bool(fetch)), (k, nq, rows, frm, fetch)


def test_route_hand_table(lib):
    # (k, nq, rows, large_k_from, fetch) -> route
    for args, want in (((513, 1, 100, 0, 1), SORT), ((513, 1, 100, 0, 0), REFUSED), ((512, 1, 10 ** 7, 0, 1), LISTS),  # one query: the lists up to 512
                       ((129, 3, 180000, 0, 1), SORT), ((128, 3, 180000, 0, 1), LISTS),   # several queries, pairs > 2^19: sort path from 129 up
                       ((200, 3, 180000, 512, 1), LISTS), ((200, 3, 5000, 0, 1), LISTS),  # ... unless the option says 512, or the store is small
                       ((200, 4, 1 << 17, 0, 1), LISTS), ((200, 4, (1 << 17) + 1, 0, 1), SORT),  # pairs = 2^19 is still small
                       ((200, 4, 1 << 26, 0, 1), SORT), ((200, 4, (1 << 26) + 1, 0, 1), LISTS),  # beyond 2^28 pairs the dump does not fit: lists
                       ((200, 1, 5000, 128, 1), SORT), ((200, 1, 5000, 128, 0), LISTS), ((17, 1, 5000, 1, 1), SORT), ((1, 1, 5000, 1, 1), LISTS)):
        assert lib.xp_route(*args) == want, args
    assert [lib.xp_E(k) for k in KS_[:-1]] == [1, 1, 1, 1, 2, 2, 4, 4, 8, 8]


# ---- variant, queries per pass, passes, grid, block lists ---------------------------------------------------------------------------
def parent_pow2ceil(v):
    """uint32_t p = 1; while (p < v) p <<= 1; return p;"""
    p = 1
    while p < v:
        p <<= 1
    return p


def parent_shape(exact_small, nq, perq, E, dimq, n_tiles, stream_grid):
    """const int forced = s->opt.exact_small;
    const bool fits1 = nq == 1 && !perq && E <= 2 && s->dimq <= 2048 && n_tiles <= 1024;
    const bool fits8 = E <= 2 && s->dimq <= 2048 && n_tiles <= 1024 && nq <= 16;
    if (forced == 1) small = fits1 ? 1u : 0u; else if (forced == 2 || forced < 0) small = fits8 ? 2u : 0u;
    if (E >= 4) tile = 1; else tile = pow2ceil(nq) < (small == 2 ? 8u : 4u) ? pow2ceil(nq) : (small == 2 ? 8u : 4u);
    const uint32_t passes = (nq + tile - 1) / tile;
    const int grid = small ? (int)n_tiles : exact_grid(s, n_tiles);      (stream_grid: what exact_grid gives, an input of the plan)"""
    small = 0
    fits1 = nq == 1 and not perq and E <= 2 and dimq <= 2048 and n_tiles <= 1024
    fits8 = E <= 2 and dimq <= 2048 and n_tiles <= 1024 and nq <= 16
    if exact_small == 1:
        small = 1 if fits1 else 0
    elif exact_small == 2 or exact_small < 0:
        small = 2 if fits8 else 0
    most = 8 if small == 2 else 4
    tile = 1 if E >= 4 else (parent_pow2ceil(nq) if parent_pow2ceil(nq) < most else most)
    passes = (nq + tile - 1) // tile
    grid = n_tiles if small else stream_grid
    return small, tile, passes, grid


def header_plan(lib, k, nq, perq, dimq, tiles, n_runs, exact_small, stream_grid, gridA=0, gridB=0):
    o = (C.c_ulonglong * 9)()
    lib.xp_plan(k, nq, int(perq), dimq, tiles, n_runs, exact_small, stream_grid, gridA, gridB, o)
    return [int(v) for v in o]


def test_variant_passes_and_lists_on_the_grid(lib):
    k_of = {1: 10, 2: 100, 4: 200, 8: 300}
    for es, nq, perq, E, dimq, tiles in itertools.product((-1, 0, 1, 2), tuple(range(1, 10)) + (16, 17), (False, True), (1, 2, 4, 8), (2048, 2052), (1024, 1025)):
        small, tile, passes, grid = parent_shape(es, nq, perq, E, dimq, tiles, (tiles + 3) // 4)  # (256 or 257 workgroups: the persistent grid of 1024 or 1025 tiles)
        got = header_plan(lib, k_of[E], nq, perq, dimq, tiles, 1, es, (tiles + 3) // 4, 7, 11)
        # const size_t n_lists_total = prune_c ? (size_t)(gridA + gridB) : perq ? (size_t)nq * grid : (size_t)passes * grid;
        assert got == [E, 64 * E, small, tile, passes, grid, int(nq == 1 and dimq <= 896), nq * grid if perq else passes * grid, 18], (es, nq, perq, E, dimq, tiles)
        assert lib.xp_variant(es, nq, int(perq), E, dimq, tiles) == small
        assert lib.xp_fits(dimq, tiles) == int(dimq <= 2048 and tiles <= 1024)


def test_variant_and_passes_hand_table(lib):
    # 5000 rows = 79 tiles (a persistent grid of 20 workgroups: four tiles each), dimq 24, k 10: nq 1 / 5 / 17 -> rows8 with 1 / 8 queries per pass, and 17 queries do not fit rows8
    for es, want in ((-1, ((2, 1, 1, 79), (2, 8, 1, 79), (0, 4, 5, 20))), (0, ((0, 1, 1, 20), (0, 4, 2, 20), (0, 4, 5, 20))), (2, ((2, 1, 1, 79), (2, 8, 1, 79), (0, 4, 5, 20))),
                     (1, ((1, 1, 1, 79), (0, 4, 2, 20), (0, 4, 5, 20)))):
        for nq, w in zip((1, 5, 17), want):
            assert tuple(header_plan(lib, 10, nq, False, 24, 79, 1, es, 20)[2:6]) == w, (es, nq)
    assert header_plan(lib, 10, 1, True, 24, 79, 1, 1, 20)[2] == 0    # the one-wave variant is merged only
    assert header_plan(lib, 200, 3, False, 24, 79, 1, -1, 20)[:6] == [4, 256, 0, 1, 3, 20]  # the long lists: streaming, a query per pass
    assert header_plan(lib, 300, 1, False, 24, 79, 1, -1, 20)[:6] == [8, 512, 0, 1, 1, 20]
    assert header_plan(lib, 100, 3, False, 24, 79, 1, -1, 20)[:6] == [2, 128, 2, 4, 1, 79]


def test_lean(lib):
    """const bool lean = nq == 1 && s->dimq <= OTT_QEMB_MAX && pl.runs.size() <= 2;   (run_exact and small_slice of the sort path)"""
    for nq, dimq, n_runs in itertools.product((1, 2), (8, 896, 904), (0, 1, 2, 3)):
        assert lib.xp_lean(nq, dimq, n_runs) == int(nq == 1 and dimq <= 896 and n_runs <= 2)


# ---- the sort path's and the policy's predicate -------------------------------------------------------------------------------------
def test_sweep_shape_and_choose_path_share_the_core_predicate(lib):
    """sweep_shape: w.rows8 = dimq <= 2048 && tiles <= 1024 && exact_small != 0 && exact_small != 1;
    choose_path: ... in.dimq <= 2048 && in.exact_small != 0 && in.exact_small != 1 && in.rows_scored / 64 + in.n_runs <= 1024
    (their own grids: test_sort_plan_cpu.py and test_query_policy_cpu.py, which pass unedited)"""
    for nq, dimq, tiles, es in itertools.product((1, 5, 17), (8, 2048, 2056), (0, 1024, 1025, 2 ** 32 - 1), (-1, 0, 1, 2)):
        assert lib.xp_sweep_rows8(nq, dimq, tiles, es) == int(dimq <= 2048 and tiles <= 1024 and es != 0 and es != 1)
    for rows, n_runs in ((65472, 1), (65536, 0), (65536, 1), (2 ** 40, 3)):
        assert lib.xp_fits(2048, rows // 64 + n_runs) == int(rows // 64 + n_runs <= 1024)


# ---- the pruned sweep ---------------------------------------------------------------------------------------------------------------
def parent_prune(dim, ld, metric, perq, lean, flat, small, exact_prune, exact_sketch, present, covers, bits, words, stage0, rows, E):
    """if (lean && !perq && small == 0 && !s->cur_flat && s->opt.exact_prune != 0 && (d->metric == OTT_METRIC_COSINE || d->metric == OTT_METRIC_DOT)) {
        const uint32_t nst = (s->ld + 31) / 32;
        uint32_t c = nst * 7 / 8;
        while (c > 0 && c * 32 > s->dim - s->dim % 8) c--;
        if (s->opt.exact_sketch != 0 && s->d_sketch != nullptr && s->sk_n >= s->n &&
            s->sk_words <= (s->sk_bits == 4 ? OTT_SKETCH4_MAX_WORDS : s->sk_bits == 3 ? OTT_SKETCH_MAX_WORDS : OTT_SKETCH1_MAX_WORDS)) {
            const uint32_t cs = s->sk_stage0;
            if (cs >= 1 && cs < nst && cs * 32 <= s->dim - s->dim % 8) { c = cs; prune_sk = true; }
        }
        const bool worth = s->opt.exact_prune == 1 || (nst >= 8 && pl.rows_scored >= (1ull << 20));
        if (worth && c >= 1 && c < nst) {
            uint64_t seed = pl.rows_scored / 10;
            if (prune_sk && s->sk_bits >= 3 && E == 1 && seed > 131072) seed = pl.rows_scored / OTT_X_SEED_DIV > 131072 ? pl.rows_scored / OTT_X_SEED_DIV : 131072;
            seed = (seed + 63) & ~63ull;
            if (seed < 64) seed = 64;
            ... prune_c = c ...
    -> (c, sketch form, seed rows); (0, False, 0) = no pruned sweep"""
    if not (lean and not perq and small == 0 and not flat and exact_prune != 0 and metric in (COSINE, DOT)):
        return (0, False, 0)
    nst = (ld + 31) // 32
    c = nst * 7 // 8
    while c > 0 and c * 32 > dim - dim % 8:
        c -= 1
    sk = False
    if exact_sketch != 0 and present and covers and words <= (108 if bits == 4 else 54 if bits == 3 else 10):
        cs = stage0
        if cs >= 1 and cs < nst and cs * 32 <= dim - dim % 8:
            c, sk = cs, True
    worth = exact_prune == 1 or (nst >= 8 and rows >= (1 << 20))
    if not (worth and 1 <= c < nst):
        return (0, False, 0)
    seed = rows // 10
    if sk and bits >= 3 and E == 1 and seed > 131072:
        seed = rows // 32 if rows // 32 > 131072 else 131072
    seed = (seed + 63) & ~63
    if seed < 64:
        seed = 64
    return (c, sk, seed)


def header_prune(lib, *a):
    o = (C.c_ulonglong * 3)()
    lib.xp_prune(*[int(v) for v in a], o)
    return (int(o[0]), bool(o[1]), int(o[2]))


DIMS = (8, 31, 32, 33, 63, 64, 65, 224, 225, 256, 768, 896)
SEED_ROWS = (64, 639, 640, 30080, 1310720 - 64, 1310720, 1310720 + 64, 4194304 - 32, 4194304 + 32, 10000000)


def sketch_states(lib, dim):
    """(present, covers, bits, words, stage0): no sketch; each width as the store builds it (ott_store.hip: sk_stage0 = prune_sketchb_stage0(nst, bits),
    sk_words = (nst - sk_stage0) * bits), with the rows covered and not; and the same with sk_words at the width's limit and one above"""
    nst = (((dim + 3) & ~3) + 31) // 32
    out = [(0, 0, 0, 0, 0)]
    for bits in (1, 3, 4):
        st0 = lib.xp_stage0(nst, bits)
        words = (nst - st0) * bits
        out += [(1, 1, bits, words, st0), (1, 0, bits, words, st0), (1, 1, bits, MAX_WORDS[bits], st0), (1, 1, bits, MAX_WORDS[bits] + 1, st0)]
    return out


def test_pruned_sweep_on_the_grid(lib):
    n = 0
    for dim in DIMS:
        ld = (dim + 3) & ~3  # ott_store_create: s->ld = (dim + 3u) & ~3u
        nst = (ld + 31) // 32
        for sk, ep, es, rows, E in itertools.product(sketch_states(lib, dim), (0, 1, -1), (0, -1), (2 ** 20 - 1, 2 ** 20) + SEED_ROWS, (1, 2)):
            args = (dim, ld, COSINE, 0, 1, 0, 0, ep, es) + sk + (rows, E)
            got, want = header_prune(lib, *args), parent_prune(*args)
            assert got == want, (args, got, want)
            n += 1
            c, sketch, seed = got
            if c:
                assert 1 <= c < nst and 32 * c <= dim - dim % 8 and seed % 64 == 0 and seed >= 64, args
                assert not sketch or (sk[4] == c and sk[0] and sk[1] and sk[3] <= MAX_WORDS[sk[2]] and es != 0), args
            else:
                assert (sketch, seed) == (False, 0)
    assert n == len(DIMS) * 13 * 3 * 2 * 12 * 2


def test_pruned_sweep_eligibility(lib):
    """every condition in front of the sweep, one at a time, on a store that prunes (768 dims, the three-bit sketch, 2^20 rows)"""
    nst = 24
    st0 = lib.xp_stage0(nst, 3)
    assert st0 == 9  # 24 - (5 * 24 + 7) / 8
    base = dict(dim=768, ld=768, metric=COSINE, perq=0, lean=1, flat=0, small=0, ep=-1, es=-1, present=1, covers=1, bits=3, words=(nst - st0) * 3, stage0=st0, rows=2 ** 20, E=1)
    order = ("dim", "ld", "metric", "perq", "lean", "flat", "small", "ep", "es", "present", "covers", "bits", "words", "stage0", "rows", "E")

    def run(**kw):
        a = tuple({**base, **kw}[k] for k in order)
        got = header_prune(lib, *a)
        assert got == parent_prune(*a), (kw, got)
        return got

    assert run() == (9, True, 104896)  # 1048576 / 10 = 104857 -> the next multiple of 64
    assert run(metric=DOT) == (9, True, 104896)
    for off in (dict(metric=EUCLIDEAN), dict(metric=MANHATTAN), dict(perq=1), dict(lean=0), dict(flat=1), dict(small=1), dict(small=2), dict(ep=0), dict(rows=2 ** 20 - 1)):
        assert run(**off) == (0, False, 0), off
    assert run(rows=2 ** 20 - 1, ep=1) == (9, True, 104896)  # forced by the option
    # without a usable sketch: the 7/8 form, checkpoint at stage 21
    for plain in (dict(es=0), dict(present=0), dict(covers=0), dict(words=55), dict(stage0=0), dict(stage0=24)):
        assert run(**plain) == (21, False, 104896), plain
    assert run(bits=1, stage0=18, words=6) == (18, True, 104896)
    assert run(bits=4, stage0=1, words=92) == (1, True, 104896)
    assert run(dim=224, ld=224, ep=1, present=0) == (6, False, 104896)   # 7 stages: 7 * 7 / 8 = 6
    assert run(dim=224, ld=224, present=0) == (0, False, 0)              # automatic needs 8 stages
    assert run(dim=225, ld=228, present=0) == (7, False, 104896)         # ... = dim >= 225; 224 = 7 x 32 dims in whole chunks of eight
    assert run(dim=31, ld=32, ep=1, present=0) == (0, False, 0)          # one stage: nothing to skip
    assert run(dim=33, ld=36, ep=1, present=0) == (1, False, 104896)
    assert run(dim=63, ld=64, ep=1, present=0) == (1, False, 104896)     # 2 * 7 / 8 = 1


def test_seed_rows_hand_table(lib):
    """a tenth, in whole tiles, at least one; the three- and four-bit forms at E = 1 above 1 310 720 rows: a thirty-second, never below 131 072"""
    tenth = (64, 64, 64, 3008, 131072, 131072, 131136, 419456, 419456, 1000000)
    wide = (64, 64, 64, 3008, 131072, 131072, 131072, 131072, 131136, 312512)
    st0 = {1: 18, 3: 9, 4: 1}
    for rows, t, w in zip(SEED_ROWS, tenth, wide):
        for bits, E in itertools.product((0, 1, 3, 4), (1, 2)):
            sk = (1, 1, bits, (24 - st0[bits]) * bits, st0[bits]) if bits else (0, 0, 0, 0, 0)
            c, sketch, seed = header_prune(lib, 768, 768, DOT, 0, 1, 0, 0, 1, -1, *sk, rows, E)
            assert c == (st0[bits] if bits else 21) and sketch == bool(bits)
            assert seed == (w if bits >= 3 and E == 1 else t), (rows, bits, E, seed)


# ---- result block, bytes scanned ----------------------------------------------------------------------------------------------------
def test_result_block_layout(lib):
    """const size_t cnt_pad = (((size_t)groups * sizeof(uint64_t)) + 63) & ~(size_t)63;
    const size_t res_bytes = cnt_pad + (size_t)groups * KS * sizeof(ott_hit);   h_hits.ensure(res_bytes + 8); the tail counter at hh + res_bytes"""
    o = (C.c_ulonglong * 3)()
    for groups, KS in itertools.product((1, 5, 8, 9, 16, 17, 1000), (64, 128, 256, 512)):
        lib.xp_layout(groups, KS, o)
        cnt_pad = (groups * 8 + 63) & ~63
        assert list(o) == [cnt_pad, cnt_pad + groups * KS * 16, cnt_pad + groups * KS * 16 + 8]
    lib.xp_layout(1, 64, o)
    assert list(o) == [64, 1088, 1096]
    lib.xp_layout(9, 128, o)
    assert list(o) == [128, 128 + 18432, 128 + 18432 + 8]


def test_bytes_scanned(lib):
    """st.bytes_scanned += (uint64_t)passes * pl.rows_scored * ((uint64_t)s->dim * 4 + (d->metric == OTT_METRIC_COSINE ? 4 : 0));"""
    for passes, rows, dim, metric in itertools.product((0, 1, 5), (0, 5000, 10 ** 7, 2 ** 33), (1, 24, 768, 4096), (COSINE, EUCLIDEAN, DOT, MANHATTAN)):
        want = passes * rows * (dim * 4 + (4 if metric == COSINE else 0))
        assert lib.xp_bytes(passes, rows, dim, metric) == want
        assert lib.xp_sort_bytes(passes, rows, dim, metric) == want
    assert lib.xp_bytes(5, 5000, 24, COSINE) == 2500000
