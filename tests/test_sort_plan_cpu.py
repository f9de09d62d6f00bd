"""CPU: what the sort path's host side decides before it launches anything (otters_amd/csrc/ott_sort_plan.h): the bits of the row
and query fields, the radix sort's pass plan of every result order, which kernel sweeps, rank sort or radix sort, the layout of
the rank sort's control block, the two-phase prefix, the slice height, the groups' extents and the copy pieces.  The header is
compiled on its own with the host compiler behind a small extern "C" driver, with the library's -ffp-contract=off, as
test_mfma_plan_cpu.py does for ott_mfma_plan.h: the code under test is the code libotters_hip.so ships.
Expected values: transcriptions of the expressions large_k_slice, run_large_k and sort_group_pairs carried before the header
existed, with the same operation order (math.sqrt and math.ceil on doubles for the prefix), and tables written out by hand.  The
pass plans are also RUN, as stable least-significant-digit passes in numpy, and held to Python's sorted() by each order's key.
The GPU half: test_gpu_vecstore.py::test_sort_path_branches_report_their_documented_sweeps."""
import ctypes as C
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")

DRIVER = r"""
#include "ott_sort_plan.h"
using namespace ott;
extern "C" unsigned sp_index_bits(unsigned long long largest, unsigned from) { return index_bits(largest, from); }
extern "C" unsigned sp_query_bits(unsigned nq) { return query_bits(nq); }
extern "C" unsigned sp_row_bits(unsigned long long largest) { return row_bits(largest); }
// o: n_pass, abl, then (src, shift, mask, desc) per pass
extern "C" int sp_plan(int order, unsigned rbits, unsigned qbits, unsigned tie_sh, unsigned abl, unsigned* o) {
    RsPlan p;
    const bool ok = sort_order_plan((SortOrder)order, rbits, qbits, tie_sh, abl, p);
    o[0] = p.n_pass; o[1] = p.abl;
    for (unsigned i = 0; i < p.n_pass; i++) { o[2 + 4 * i] = p.pass[i].src; o[3 + 4 * i] = p.pass[i].shift; o[4 + 4 * i] = p.pass[i].mask; o[5 + 4 * i] = p.pass[i].desc; }
    return ok ? 1 : 0;
}
extern "C" int sp_add_digits_full(void) {  // a seventeenth digit is refused, not dropped
    RsPlan p = RsPlan();
    const bool a = rs_add_digits(p, 0, 0, 64, true), b = rs_add_digits(p, 1, 0, 32, false), c = rs_add_digits(p, 0, 0, 32, true), d = rs_add_digits(p, 1, 0, 1, false);
    return (a ? 1 : 0) | (b ? 2 : 0) | (c ? 4 : 0) | (d ? 8 : 0) | (int)(p.n_pass << 4);
}
extern "C" void sp_consts(unsigned long long* o) {
    o[0] = RS_MAXP; o[1] = RS_TILE; o[2] = SMALL_PAIRS; o[3] = SMALL_PERQ_MAX; o[4] = COPY_PIECE; o[5] = sizeof(RsPass); o[6] = sizeof(RsPlan); o[7] = sizeof(RsCtl);
    o[8] = rs_tiles(0); o[9] = rs_tiles(4096); o[10] = rs_tiles(4097); o[11] = rs_tmp_bytes(4097); o[12] = RS_THREADS; o[13] = RS_ITEMS;
}
extern "C" void sp_sweep(unsigned nq, unsigned dimq, unsigned tiles, int exact_small, unsigned* o) {
    const SweepShape w = sweep_shape(nq, dimq, tiles, exact_small);
    o[0] = w.rows8; o[1] = w.tile; o[2] = w.passes;
}
extern "C" unsigned long long sp_bytes(unsigned passes, unsigned long long rows, unsigned dim, unsigned metric) { return sort_bytes_scanned(passes, rows, dim, metric); }
extern "C" int sp_small_ok(unsigned long long pairs, unsigned nq, int perq, unsigned rbits, unsigned qbits, int small_sort, int gated) {
    return small_path_ok(pairs, nq, perq != 0, rbits, qbits, small_sort, gated != 0) ? 1 : 0;
}
extern "C" void sp_ctl(unsigned long long cap, unsigned nq, unsigned long long* o) {
    const SmallCtl c = small_ctl_layout(cap, nq);
    o[0] = c.cursor; o[1] = c.ticket; o[2] = c.rank; o[3] = c.hist; o[4] = c.total;
}
extern "C" unsigned long long sp_prefix_rows(unsigned long long rows, unsigned nq, int perq, unsigned long long k, int enabled, int flat) {
    return prefix_rows(rows, nq, perq != 0, k, enabled != 0, flat != 0);
}
extern "C" unsigned long long sp_slice_rows(unsigned nq, unsigned long long slice_pairs) { return slice_rows(nq, slice_pairs); }
extern "C" unsigned long long sp_extents(const unsigned* start, unsigned nq, unsigned long long n, unsigned long long k, unsigned long long* first, unsigned long long* count) {
    const std::vector<uint32_t> st(start, start + nq);
    std::vector<uint64_t> f, c;
    const uint64_t total = group_extents(st, n, k, f, c);
    if (f.size() != nq || c.size() != nq) return ~0ull;
    for (unsigned q = 0; q < nq; q++) { first[q] = f[q]; count[q] = c[q]; }
    return total;
}
extern "C" unsigned sp_pieces(const unsigned long long* count, unsigned groups, unsigned long long piece, unsigned long long* o, unsigned room) {
    const std::vector<uint64_t> c(count, count + groups);
    const std::vector<CopyPiece> p = copy_pieces(c, piece);
    for (unsigned i = 0; i < p.size() && i < room; i++) { o[4 * i] = p[i].g; o[4 * i + 1] = p[i].at; o[4 * i + 2] = p[i].n; o[4 * i + 3] = p[i].src; }
    return (unsigned)p.size();
}
"""

SCORE, SCORE_BY_QUERY, MERGED, BY_QUERY = range(4)  # SortOrder
ORDERS = (SCORE, SCORE_BY_QUERY, MERGED, BY_QUERY)
COSINE, EUCLIDEAN, DOT = 0, 1, 2
NONE = 0xFFFFFFFF
PIECE = 128 * 1024

NQS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 255, 256, 257, 1024, 1025, 2 ** 20)
ROW_MAX = (0, 1, 2, 7, 8, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 5)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sort_plan")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    up, ullp, ull, u, i = C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong), C.c_ulonglong, C.c_uint, C.c_int
    for name, args, res in (("sp_index_bits", [ull, u], u), ("sp_query_bits", [u], u), ("sp_row_bits", [ull], u), ("sp_plan", [i, u, u, u, u, up], i),
                            ("sp_add_digits_full", [], i), ("sp_consts", [ullp], None), ("sp_sweep", [u, u, u, i, up], None), ("sp_bytes", [u, ull, u, u], ull),
                            ("sp_small_ok", [ull, u, i, u, u, i, i], i), ("sp_ctl", [ull, u, ullp], None), ("sp_prefix_rows", [ull, u, i, ull, i, i], ull),
                            ("sp_slice_rows", [u, ull], ull), ("sp_extents", [up, u, ull, ull, ullp, ullp], ull), ("sp_pieces", [ullp, u, ull, ullp, u], u)):
        f = getattr(L, name)
        f.argtypes, f.restype = args, res
    return L


# ---- transcriptions of the parent's expressions -------------------------------------------------------------------------------------
def parent_qbits(nq):
    """while (nq > 1 && qbits < 32 && ((uint64_t)(nq - 1) >> qbits) != 0) qbits++;"""
    qbits = 0
    while nq > 1 and qbits < 32 and ((nq - 1) >> qbits) != 0:
        qbits += 1
    return qbits


def parent_rbits(largest):
    """while (rbits < 32 && ((s->n - 1 + s->cur_tie_off) >> rbits) != 0) rbits++;  (sort_group_pairs: span - 1)"""
    rbits = 1
    while rbits < 32 and (largest >> rbits) != 0:
        rbits += 1
    return rbits


def add_digits(plan, src, lo, hi, desc):
    """rs_add_digits as it was, its silent stop at 16 passes included"""
    b = lo
    while b < hi and len(plan) < 16:
        w = hi - b if hi - b < 8 else 8
        plan.append((src, b, (1 << w) - 1, 1 if desc else 0))
        b += 8


def parent_plan(order, rbits, qbits, tie_sh):
    """the sort_entries lambda of large_k_slice: score_only = order is one of the first two, perq = the grouped ones"""
    plan = []
    sh = tie_sh if tie_sh < rbits else 0

    def key_digits(frm):
        add_digits(plan, 0, frm, rbits, True)
        add_digits(plan, 0, 32, 64, True)

    if order in (SCORE, SCORE_BY_QUERY):
        add_digits(plan, 0, 32, 64, True)
        if order == SCORE_BY_QUERY:
            add_digits(plan, 1, 0, qbits, False)
    elif order == MERGED:
        if sh == 0:
            add_digits(plan, 1, 0, qbits, False)
            key_digits(0)
        else:
            add_digits(plan, 0, 0, sh, True)
            add_digits(plan, 1, 0, qbits, False)
            key_digits(sh)
    else:
        key_digits(0)
        add_digits(plan, 1, 0, qbits, False)
    return plan


def parent_group_plan(rbits, qbits):
    """sort_group_pairs' own three lines"""
    plan = []
    add_digits(plan, 0, 0, rbits, True)
    add_digits(plan, 0, 32, 64, True)
    add_digits(plan, 1, 0, qbits, False)
    return plan


def header_plan(lib, order, rbits, qbits, tie_sh, abl=0):
    o = (C.c_uint * 66)()
    ok = lib.sp_plan(order, rbits, qbits, tie_sh, abl, o)
    assert o[1] == abl
    return ok, [tuple(o[2 + 4 * i:6 + 4 * i]) for i in range(o[0])]


# ---- constants and layout of the moved declarations ----------------------------------------------------------------------------------
def test_moved_declarations_keep_their_values_and_layout(lib):
    o = (C.c_ulonglong * 14)()
    lib.sp_consts(o)
    ctl = (16 * 256 + 16 + 17 + 16 + 1) * 4
    assert list(o) == [16, 4096, 16384, 1024, PIECE, 16, 16 * 16 + 8, ctl, 0, 1, 2, ((ctl + 255) & ~255) + 2 * 256 * 8, 512, 8]
    # 16 digits fit; the next is refused, with nothing added: (64 bits = 8) + (32 = 4) + (32 = 4) = 16, then one more
    assert lib.sp_add_digits_full() == (1 | 2 | 4 | 0 | 16 << 4)


# ---- index_bits ---------------------------------------------------------------------------------------------------------------------
def test_index_bits_is_the_parents_loops(lib):
    by_hand_q = {1: 0, 2: 1, 3: 2, 4: 2, 5: 3, 8: 3, 9: 4, 16: 4, 17: 5, 255: 8, 256: 8, 257: 9, 1024: 10, 1025: 11, 2 ** 20: 20}
    for nq in NQS:
        assert lib.sp_query_bits(nq) == parent_qbits(nq) == by_hand_q[nq], nq
        assert lib.sp_index_bits(nq - 1, 0) == by_hand_q[nq], nq
    by_hand_r = {0: 1, 1: 1, 2: 2, 7: 3, 8: 4, 255: 8, 256: 9, 65535: 16, 65536: 17, 2 ** 24 - 1: 24, 2 ** 31: 32, 2 ** 32 - 1: 32, 2 ** 32 + 5: 32}
    for v in ROW_MAX:
        assert lib.sp_row_bits(v) == parent_rbits(v) == by_hand_r[v], v
        assert lib.sp_index_bits(v, 1) == by_hand_r[v], v
    assert lib.sp_row_bits(2 ** 64 - 1) == 32  # (an empty store: n - 1 wraps)


# ---- sort_order_plan ----------------------------------------------------------------------------------------------------------------
def covered(plan, src, lo, hi):
    """the bits of `src` in [lo, hi) the plan's digits cover, each as often as it is covered"""
    bits = []
    for s, shift, mask, _ in plan:
        if s == src and lo <= shift < hi:
            bits += list(range(shift, shift + mask.bit_length()))
    return sorted(bits)


def test_sort_order_plan_on_the_grid(lib):
    for nq, largest, tie_sh, order in itertools.product(NQS, ROW_MAX, (0, 3), ORDERS):
        rbits, qbits = parent_rbits(largest), parent_qbits(nq)
        ok, plan = header_plan(lib, order, rbits, qbits, tie_sh)
        assert ok == 1 and plan == parent_plan(order, rbits, qbits, tie_sh), (nq, largest, tie_sh, order)
        # never cut short: at most 16 digits, and every bit the order names is covered exactly once
        assert len(plan) <= 16
        assert covered(plan, 0, 32, 64) == list(range(32, 64))
        assert covered(plan, 0, 0, 32) == (list(range(rbits)) if order in (MERGED, BY_QUERY) else [])
        assert covered(plan, 1, 0, 32) == (list(range(qbits)) if order != SCORE else [])
        assert all(0 < m <= 255 for _, _, m, _ in plan)
    # the widest plan there is: 13 digits
    ok, plan = header_plan(lib, MERGED, 32, 32, 3)
    assert ok == 1 and len(plan) == 13
    assert header_plan(lib, MERGED, 24, 3, 0, abl=5)[0] == 1  # (the ablation word rides along)


def test_sort_order_plan_hand_tables(lib):
    score = [(0, 32, 255, 1), (0, 40, 255, 1), (0, 48, 255, 1), (0, 56, 255, 1)]
    # one query, 10M rows, merged canonical: 24 row bits, no query digit
    assert lib.sp_row_bits(10 ** 7 - 1) == 24 and lib.sp_query_bits(1) == 0
    assert header_plan(lib, MERGED, 24, 0, 0) == (1, [(0, 0, 255, 1), (0, 8, 255, 1), (0, 16, 255, 1)] + score)
    # 16 queries, 1000 rows, the reference's visit order: row & 7, then the query, then row >> 3 (7 bits), then the score
    assert lib.sp_row_bits(999) == 10 and lib.sp_query_bits(16) == 4
    assert header_plan(lib, MERGED, 10, 4, 3) == (1, [(0, 0, 7, 1), (1, 0, 15, 0), (0, 3, 127, 1)] + score)
    # ... on a store of 8 rows the shift falls back to 0: canonical
    assert header_plan(lib, MERGED, 3, 4, 3) == (1, [(1, 0, 15, 0), (0, 0, 7, 1)] + score)
    # 5 queries per query, 3000 rows: key, then the query
    assert lib.sp_row_bits(2999) == 12 and lib.sp_query_bits(5) == 3
    per_query = [(0, 0, 255, 1), (0, 8, 15, 1)] + score + [(1, 0, 7, 0)]
    assert header_plan(lib, BY_QUERY, 12, 3, 0) == (1, per_query)
    assert header_plan(lib, BY_QUERY, 12, 3, 3) == (1, per_query)  # (per query the row order IS the visit order)
    # first phase
    assert header_plan(lib, SCORE, 12, 3, 3) == (1, score)
    assert header_plan(lib, SCORE_BY_QUERY, 12, 3, 0) == (1, score + [(1, 0, 7, 0)])
    # grouped pairs: the per-query plan of the same bits (rbits from id_span - 1)
    for nq, span in itertools.product(NQS, (1, 2, 9, 257, 10 ** 6, 2 ** 32)):
        rbits, qbits = parent_rbits(span - 1), parent_qbits(nq)
        assert header_plan(lib, BY_QUERY, rbits, qbits, 0) == (1, parent_group_plan(rbits, qbits))


def run_plan(plan, keys, qs):
    """the plan as stable least-significant-digit passes"""
    for src, shift, mask, desc in plan:
        d = ((qs.astype(np.uint64) if src else keys) >> np.uint64(shift)) & np.uint64(mask)
        if desc:
            d = np.uint64(mask) - d
        o = np.argsort(d, kind="stable")
        keys, qs = keys[o], qs[o]
    return keys, qs


def test_plans_sort_into_their_documented_order(lib):
    rng = np.random.default_rng(20)
    ords = np.array([0x00000001, 0x3F800000, 0x3F800001, 0xBF800000, 0xFFFFFFFF], np.uint64)  # few scores, every byte in play
    for nq in (1, 5, 16):
        n = 2000
        score = ords[rng.integers(0, len(ords), n)]
        row = rng.integers(0, 37, n).astype(np.uint64)  # few rows: long runs of ties (and repeated pairs)
        qs = rng.integers(0, nq, n).astype(np.uint32)
        keys = (score << np.uint64(32)) | (~row & np.uint64(0xFFFFFFFF))
        rbits, qbits = lib.sp_row_bits(36), lib.sp_query_bits(nq)
        assert rbits == 6
        items = list(zip(score.tolist(), row.tolist(), qs.tolist()))
        documented = {
            (SCORE, 0): lambda e: -e[0],                                  # best score first, nothing else (stable)
            (SCORE_BY_QUERY, 0): lambda e: (e[2], -e[0]),                 # grouped by query, best score first
            (MERGED, 0): lambda e: (-e[0], e[1], e[2]),                   # canonical: score, lower row, lower query
            (MERGED, 3): lambda e: (-e[0], e[1] >> 3, e[2], e[1] & 7),    # the reference: score, 8-row block, query, row in the block
            (BY_QUERY, 0): lambda e: (e[2], -e[0], e[1]),                 # grouped by query: score, lower row
            (BY_QUERY, 3): lambda e: (e[2], -e[0], e[1]),
        }
        for (order, tie_sh), key in documented.items():
            ok, plan = header_plan(lib, order, rbits, qbits, tie_sh)
            assert ok == 1
            k2, q2 = run_plan(plan, keys, qs)
            got = list(zip((k2 >> np.uint64(32)).tolist(), ((~k2) & np.uint64(0xFFFFFFFF)).tolist(), q2.tolist()))
            assert got == sorted(items, key=key), (nq, order, tie_sh)


# ---- sweep_shape, sort_bytes_scanned ------------------------------------------------------------------------------------------------
def parent_sweep(nq, dimq, tiles, exact_small):
    tile = 1 if nq == 1 else 4
    passes = (nq + tile - 1) // tile
    rows8 = dimq <= 2048 and tiles <= 1024 and exact_small != 0 and exact_small != 1
    t8 = 1
    while t8 < nq and t8 < 8:
        t8 <<= 1
    return [1, t8, (nq + t8 - 1) // t8] if rows8 else [0, tile, passes]


def test_sweep_shape_and_bytes_are_the_parents(lib):
    o = (C.c_uint * 3)()
    for nq, dimq, tiles, small in itertools.product(NQS, (8, 24, 2048, 2049, 4096), (0, 1, 157, 1024, 1025, 10 ** 6), (-1, 0, 1, 2)):
        lib.sp_sweep(nq, dimq, tiles, small, o)
        assert list(o) == parent_sweep(nq, dimq, tiles, small), (nq, dimq, tiles, small)
    lib.sp_sweep(5, 8, 47, -1, o)
    assert list(o) == [1, 8, 1]
    lib.sp_sweep(5, 8, 47, 0, o)
    assert list(o) == [0, 4, 2]
    lib.sp_sweep(1, 768, 2000, -1, o)
    assert list(o) == [0, 1, 1]
    for passes, rows, dim, metric in itertools.product((1, 2, 258), (0, 1, 90000, 2 ** 29), (1, 7, 768, 4096), (COSINE, EUCLIDEAN, DOT, 3)):
        assert lib.sp_bytes(passes, rows, dim, metric) == passes * rows * (dim * 4 + (4 if metric == COSINE else 0))


# ---- small_path_ok, small_ctl_layout ------------------------------------------------------------------------------------------------
def test_small_path_predicate(lib):
    def parent(pairs, nq, perq, rbits, qbits, small_sort, gated):
        return int(pairs <= 16384 and (nq <= 1024 if perq else rbits + qbits <= 32) and small_sort != 0 and not gated)

    for pairs, nq, perq, rbits, qbits, small_sort, gated in itertools.product((0, 1, 16383, 16384, 16385, 2 ** 30), (1, 5, 1024, 1025), (0, 1),
                                                                               (1, 14, 22, 23, 32), (0, 3, 10, 11), (0, 1, -1), (0, 1)):
        assert lib.sp_small_ok(pairs, nq, perq, rbits, qbits, small_sort, gated) == parent(pairs, nq, perq, rbits, qbits, small_sort, gated)
    ok = lib.sp_small_ok
    assert (ok(16384, 1, 0, 14, 0, 1, 0), ok(16385, 1, 0, 14, 0, 1, 0)) == (1, 0)        # both sides of 16384 pairs
    assert (ok(1024, 1024, 1, 32, 10, 1, 0), ok(1025, 1025, 1, 32, 11, 1, 0)) == (1, 0)  # per query: both sides of 1024 queries
    assert (ok(9000, 1025, 0, 14, 11, 1, 0), ok(9000, 3, 1, 32, 32, 1, 0)) == (1, 1)     # ... which bind nothing else
    assert (ok(100, 5, 0, 29, 3, 1, 0), ok(100, 5, 0, 30, 3, 1, 0)) == (1, 0)            # merged: row bits + query bits = 32, 33
    assert ok(100, 1, 0, 14, 0, 0, 0) == 0                                               # small_sort = 0
    assert ok(100, 1, 0, 14, 0, 1, 1) == 0                                               # a gated slice


def test_small_ctl_layout(lib):
    o = (C.c_ulonglong * 5)()
    by_hand = {(1, 1): [0, 64, 320, 324, 328], (16384, 1): [0, 64, 320, 65856, 65860], (700, 23): [0, 64, 320, 3120, 3212]}
    for (cap, nq), want in by_hand.items():
        lib.sp_ctl(cap, nq, o)
        assert list(o) == want, (cap, nq)
        assert (o[3] - o[1]) // 4 == 64 + cap  # the words small_copy_kernel zeroes: 64 tickets and a rank per pair


# ---- prefix_rows, slice_rows --------------------------------------------------------------------------------------------------------
def parent_prefix(rows, nq, perq, k_eff, enabled, flat):
    m_rows = 0
    if enabled and not flat and rows > 0:
        pairs = float(rows) * (1.0 if perq else float(nq))
        f = math.sqrt(float(k_eff) / pairs)
        if f <= 0.25:
            m_rows = (int(math.ceil(f * float(rows))) + 63) & ~63
            if m_rows < 4096:
                m_rows = 4096
            if m_rows * 4 > rows:
                m_rows = 0
    return m_rows


def test_prefix_rows_is_the_parents(lib):
    seen = set()
    for rows, nq, perq, enabled, flat in itertools.product((0, 1, 4095, 16384, 16385, 65536, 90000, 10 ** 7, 2 ** 29), (1, 3, 16), (0, 1), (0, 1), (0, 1)):
        for k in (513, 600, 3000, rows // 16, rows):
            got = lib.sp_prefix_rows(rows, nq, perq, k, enabled, flat)
            assert got == parent_prefix(rows, nq, perq, k, enabled, flat), (rows, nq, perq, k, enabled, flat)
            seen.add(got)
    assert 0 in seen and 4096 in seen and len(seen) > 10  # (the grid reaches the floor and the region above it)
    # by hand: sqrt(600 / 270000) = 0.04714..., x 90000 = 4242.6 -> 4243 -> 4288 (67 x 64); four times that is below 90000
    assert lib.sp_prefix_rows(90000, 3, 0, 600, 1, 0) == 4288
    # by hand: sqrt(0.06) = 0.2449 <= 0.25, 2450 -> 2496 -> the floor 4096, which is more than a quarter of 10000 rows
    assert lib.sp_prefix_rows(10000, 1, 0, 600, 1, 0) == 0
    assert lib.sp_prefix_rows(90000, 3, 0, 600, 0, 0) == 0 and lib.sp_prefix_rows(90000, 3, 0, 600, 1, 1) == 0


def test_slice_rows(lib):
    def parent(nq, slice_pairs):
        r = (slice_pairs // nq) & ~63
        return 64 if r < 64 else r

    assert lib.sp_slice_rows(1, 2 ** 14) == 16384
    assert lib.sp_slice_rows(9, 2 ** 14) == 1792
    assert lib.sp_slice_rows(2 ** 14 + 1, 2 ** 14) == 64
    for nq, pairs in ((3, 2 ** 29), (1030, 2 ** 29), (1, 2 ** 29), (255, 2 ** 14), (256, 2 ** 14), (257, 2 ** 14)):
        assert lib.sp_slice_rows(nq, pairs) == parent(nq, pairs)
    assert lib.sp_slice_rows(3, 2 ** 29) == 178956928 and lib.sp_slice_rows(1030, 2 ** 29) == 521216


# ---- group_extents, copy_pieces -----------------------------------------------------------------------------------------------------
def extents(lib, start, n, k):
    nq = len(start)
    first, count = (C.c_ulonglong * nq)(), (C.c_ulonglong * nq)()
    total = lib.sp_extents((C.c_uint * nq)(*start), nq, n, k, first, count)
    return list(first), list(count), total


def parent_slice_extents(start, n, k):
    """group_hist (sizes, walking back from n) and the running sum behind it in large_k_slice"""
    nq = len(start)
    h, nxt = [0] * nq, n
    for q in reversed(range(nq)):
        if start[q] == NONE:
            continue
        h[q] = nxt - start[q]
        nxt = start[q]
    first, count, off = [0] * nq, [0] * nq, 0
    for q in range(nq):
        first[q] = off
        count[q] = h[q] if h[q] < k else k
        off += h[q]
    return first, count, sum(count)


def parent_pairs_extents(start, n, k):
    """sort_group_pairs: first = the start word (a group without entries: 0, never read)"""
    nq = len(start)
    first, count, nxt, total = [0] * nq, [0] * nq, n, 0
    for q in reversed(range(nq)):
        if start[q] == NONE:
            continue
        first[q] = start[q]
        count[q] = min(nxt - start[q], k)
        nxt = start[q]
        total += count[q]
    return first, count, total


def test_group_extents(lib):
    cases = [
        [NONE, 0, NONE, 40, NONE],  # absent at the front, in the middle and at the end: groups of 40 and 60
        [0, 40, 41, 99],
        [NONE, NONE, 0],
        [0, NONE, NONE],
        [0],                        # one group
    ]
    for start, k in itertools.product(cases, (1, 39, 40, 41, 59, 60, 61, 100, 2 ** 40)):
        first, count, total = extents(lib, start, 100, k)
        assert (first, count, total) == parent_slice_extents(start, 100, k), (start, k)
        pf, pc, pt = parent_pairs_extents(start, 100, k)
        assert (count, total) == (pc, pt)
        assert all(first[q] == pf[q] for q in range(len(start)) if count[q]), (start, k)
    # by hand
    assert extents(lib, [NONE, 0, NONE, 40, NONE], 100, 40) == ([0, 0, 40, 40, 100], [0, 40, 0, 40, 0], 80)
    assert extents(lib, [NONE, 0, NONE, 40, NONE], 100, 41) == ([0, 0, 40, 40, 100], [0, 40, 0, 41, 0], 81)
    assert extents(lib, [NONE, 0, NONE, 40, NONE], 100, 39) == ([0, 0, 40, 40, 100], [0, 39, 0, 39, 0], 78)
    assert extents(lib, [0], 77, 600) == ([0], [77], 77) and extents(lib, [0], 77, 10) == ([0], [10], 10)
    assert extents(lib, [NONE, NONE], 0, 5) == ([0, 0], [0, 0], 0)


def pieces(lib, count, piece=PIECE):
    o = (C.c_ulonglong * (4 * 64))()
    n = lib.sp_pieces((C.c_ulonglong * len(count))(*count), len(count), piece, o, 64)
    assert n <= 64
    return [tuple(o[4 * i:4 * i + 4]) for i in range(n)]


def test_copy_pieces(lib):
    P = PIECE
    assert pieces(lib, [0, 1, P, P + 1, 3 * P]) == [(1, 0, 1, 0), (2, 0, P, 1), (3, 0, P, 1 + P), (3, P, 1, 1 + 2 * P),
                                                    (4, 0, P, 2 + 2 * P), (4, P, P, 2 + 3 * P), (4, 2 * P, P, 2 + 4 * P)]
    assert pieces(lib, [P - 1, 2]) == [(0, 0, P - 1, 0), (1, 0, 2, P - 1)]
    assert pieces(lib, []) == [] and pieces(lib, [0, 0]) == []
    for count in ([0, 1, P, P + 1, 3 * P], [P - 1, 2], [5, 0, 7, 16, 1], [300000]):
        for piece in (P, 4, 7):
            if sum(count) > 60 * piece:
                continue
            got, src = pieces(lib, count, piece), 0
            for g, at, n, s in got:
                assert 0 < n <= piece and at + n <= count[g]  # never across two groups
                assert s == src and s == sum(count[:g]) + at  # src runs on
                src += n
            assert src == sum(count)
