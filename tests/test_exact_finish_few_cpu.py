"""The narrow finish of the pruned exact sweep (otters_amd/csrc/ott_finish_few.h; ott_exact.hip: pq_finish_few) on the CPU.

The header's index functions are compiled into a small shared object and drive a numpy float32 restatement of both finishes —
a wave of 64 lanes, eight load instructions per round, an 8-KB stage buffer, one IEEE operation at a time:

  * wide  (pq_finish): every 128-B stage of the n rows as one tile of 64, stage after stage;
  * narrow (pq_finish_few): rounds of 8 / G stages of G row groups, the lane walking its row's slabs in stage order.

Both must give the oracle's score (oracle.dot / oracle.cosine, either reduce order) bit for bit, on dims below one piece, below
one stage, with a remainder (dim % 8), with a ragged last stage (dim % 32) and with fewer stages than a round holds.
The sanitizer walk over the same header, with its own main, is tests/host/finish_few_walk.cpp: it is built and run here too.
The GPU half is tests/test_gpu_exact_finish_few.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")
KC = 32

DRIVER = r"""
#include "ott_finish_few.h"
using namespace ott;
extern "C" unsigned ffd_groups(unsigned n) { return ff_groups(n); }
extern "C" unsigned ffd_stages(unsigned n) { return ff_stages(n); }
extern "C" unsigned ffd_rounds(unsigned n, unsigned pstage, unsigned nstages) { return ff_rounds(n, pstage, nstages); }
extern "C" unsigned ffd_load_slab(unsigned m, unsigned n) { return ff_load_slab(m, n); }
extern "C" unsigned ffd_load_row(unsigned m, unsigned n, unsigned lrow) { return ff_load_row(m, n, lrow); }
extern "C" unsigned ffd_stage(unsigned n, unsigned pstage, unsigned r, unsigned j) { return ff_stage(n, pstage, r, j); }
extern "C" unsigned ffd_stage_clamp(unsigned s, unsigned nstages) { return ff_stage_clamp(s, nstages); }
extern "C" unsigned ffd_load_off(unsigned sc, unsigned lslot, unsigned ld) { return ff_slot_off(lslot, ld) + ff_col_off(sc, lslot, ld); }
extern "C" int ffd_col_ok(unsigned s, unsigned lslot, unsigned ld) { return ff_col_ok(s, lslot, ld) ? 1 : 0; }
extern "C" unsigned ffd_store_off(unsigned m, unsigned lrow, unsigned lslot) { return ff_store_off(m, lrow, lslot); }
extern "C" unsigned ffd_read_off(unsigned i, unsigned n, unsigned j, unsigned slot) { return ff_read_off(i, n, j, slot); }
extern "C" unsigned ffd_max_rows() { return FF_MAX_ROWS; }
"""


@pytest.fixture(scope="module")
def ff(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("finish_few")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    for name in ("groups", "stages", "rounds", "load_slab", "load_row", "stage", "stage_clamp", "load_off", "col_ok", "store_off", "read_off", "max_rows"):
        getattr(L, "ffd_" + name).restype = C.c_uint
    L.ffd_col_ok.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def oracle():
    import oracle as O
    O.build()
    return O


def consume(acc, tail, piece32, s, q, dim):
    """pq_consume: one stage (32 floats of the lane's row, zero past ld) into the eight chains and the remainder sum"""
    for j in range(KC // 8):
        col = s * KC + 8 * j
        if col >= dim:
            continue
        x = piece32[8 * j:8 * j + 8]
        if col + 8 <= dim:
            for l in range(8):
                acc[l] = np.float32(acc[l] + np.float32(q[col + l] * x[l]))
        else:
            for l in range(dim - col):
                tail = np.float32(tail + np.float32(q[col + l] * x[l]))
    return tail


def load16(row, off, ld):
    """a 16-B load at float offset `off` of a row of ld floats (the row's bytes only)"""
    assert 0 <= off < ld
    v = np.zeros(4, np.float32)
    m = min(4, ld - off)
    v[:m] = row[off:off + m]
    return v


def finish_wide(rows, q, dim, ld, pstage):
    """pq_finish: lane = row of a dense tile, one stage per round trip"""
    n = rows.shape[0]
    nst = (ld + KC - 1) // KC
    acc = np.zeros((n, 8), np.float32)
    tail = np.zeros(n, np.float32)
    for s in range(pstage, nst):
        for i in range(n):
            piece = np.zeros(KC, np.float32)
            for sl in range(8):
                if s * KC + sl * 4 < ld:
                    piece[4 * sl:4 * sl + 4] = load16(rows[i], s * KC + sl * 4, ld)
            tail[i] = consume(acc[i], tail[i], piece, s, q, dim)
    return acc, tail


def finish_narrow(ff, rows, q, dim, ld, pstage):
    """pq_finish_few through the header: loads, stores into the stage buffer, and each lane's walk of its slabs"""
    n = rows.shape[0]
    assert 1 <= n <= ff.ffd_max_rows()
    nst = (ld + KC - 1) // KC
    S = ff.ffd_stages(n)
    acc = np.zeros((n, 8), np.float32)
    tail = np.zeros(n, np.float32)
    for r in range(ff.ffd_rounds(n, pstage, nst)):
        st = np.full(64 * KC, np.nan, np.float32)  # (what nobody stored would poison a sum)
        for m in range(8):
            for lane in range(64):
                lrow, lslot = lane >> 3, lane & 7
                i = ff.ffd_load_row(m, n, lrow)
                s = ff.ffd_stage(n, pstage, r, ff.ffd_load_slab(m, n))
                sc = ff.ffd_stage_clamp(s, nst)
                v = load16(rows[i if i < n else 0], ff.ffd_load_off(sc, lslot, ld), ld)
                ok = i < n and ff.ffd_col_ok(s, lslot, ld)
                at = ff.ffd_store_off(m, lrow, lslot)
                st[at:at + 4] = v if ok else 0.0
        for i in range(n):
            for j in range(S):
                s = ff.ffd_stage(n, pstage, r, j)
                if s >= nst:
                    break
                piece = np.concatenate([st[ff.ffd_read_off(i, n, j, sl):ff.ffd_read_off(i, n, j, sl) + 4] for sl in range(8)])
                tail[i] = consume(acc[i], tail[i], piece, s, q, dim)
    return acc, tail


def reduce8(a, mode):
    if mode == 1:
        return np.float32(np.float32(np.float32(np.float32(a[0] + a[1]) + a[2]) + a[3]) + np.float32(np.float32(np.float32(a[4] + a[5]) + a[6]) + a[7]))
    return np.float32(np.float32(np.float32(a[0] + a[4]) + np.float32(a[2] + a[6])) + np.float32(np.float32(a[1] + a[5]) + np.float32(a[3] + a[7])))


# below one piece, below a short row's clamp (dim < 29), one stage, a remainder, a ragged last stage, three stages (fewer than a
# round), exactly one and two rounds of eight and of four, the headline's 24 stages, and the widest row of the walk
DIMS = (1, 3, 8, 12, 28, 29, 32, 33, 37, 96, 100, 128, 131, 232, 237, 256, 257, 512, 768, 771, 896)


@pytest.mark.parametrize("n", (1, 2, 7, 8, 9, 10, 15, 16))
def test_narrow_order_is_the_wide_order_is_the_oracles_score(ff, oracle, n):
    O = oracle
    rng = np.random.default_rng(1000 + n)
    with np.errstate(all="ignore"):
        for dim in DIMS:
            ld = (dim + 3) & ~3  # the store's row pitch: whole 16-B pieces, zeros past dim
            rows = np.zeros((n, ld), np.float32)
            rows[:, :dim] = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
            q = rng.uniform(-1, 1, dim).astype(np.float32)
            nst = (ld + KC - 1) // KC
            accw, tailw = finish_wide(rows, q, dim, ld, 0)
            accn, tailn = finish_narrow(ff, rows, q, dim, ld, 0)
            assert np.array_equal(accw.view(np.uint32), accn.view(np.uint32)), (n, dim)
            assert np.array_equal(tailw.view(np.uint32), tailn.view(np.uint32)), (n, dim)
            inv_q = O.inv_norms(q[None, :])[0]
            inv_v = O.inv_norms(rows[:, :dim])
            for mode in (O.REDUCE_AVX, O.REDUCE_SEQ4):
                for i in range(n):
                    dot = np.float32(reduce8(accn[i], mode) + tailn[i])
                    assert dot.view(np.uint32) == np.float32(O.dot(q, rows[i, :dim], mode)).view(np.uint32), (n, dim, i, mode)
                    cos = np.float32(np.float32(dot * inv_q) * inv_v[i])
                    assert cos.view(np.uint32) == np.float32(O.cosine(q, rows[i, :dim], inv_q, inv_v[i], mode)).view(np.uint32), (n, dim, i, mode)
            if nst > 1:  # a checkpoint behind stage 0 (the forms without a head): the same partial chains from stage 1 on
                a1, t1 = finish_narrow(ff, rows, q, dim, ld, 1)
                aw1, tw1 = finish_wide(rows, q, dim, ld, 1)
                assert np.array_equal(a1.view(np.uint32), aw1.view(np.uint32)) and np.array_equal(t1.view(np.uint32), tw1.view(np.uint32)), (n, dim)


def test_rounds_and_slabs(ff):
    for n in range(1, 17):
        G, S = ff.ffd_groups(n), ff.ffd_stages(n)
        assert (G, S) == ((1, 8) if n <= 8 else (2, 4))
        assert ff.ffd_rounds(n, 0, 24) == 24 // S and ff.ffd_rounds(n, 0, 3) == 1 and ff.ffd_rounds(n, 1, 1) == 0
        # a round fills the stage buffer exactly: 64 rows x 8 slots, every slot once
        seen = set()
        for m in range(8):
            for lane in range(64):
                seen.add(ff.ffd_store_off(m, lane >> 3, lane & 7))
        assert seen == set(range(0, 64 * KC, 4))


def test_sanitizer_walk(tmp_path):
    """tests/host/finish_few_walk.cpp: its own main, built with ASan and UBSan linked into the program, run on the CPU"""
    cxx = shutil.which("clang++") or shutil.which("c++") or shutil.which("g++")
    exe = tmp_path / "finish_few_walk"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", HDR, os.path.join(ROOT, "tests", "host", "finish_few_walk.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "finish_few_walk ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
