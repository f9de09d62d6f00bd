"""GPU: sparse layouts past 2^32 bytes and sparse keys with row ids above 2^24.  The large-offset suite
(tests/test_gpu_large_offsets.py) was written before sparse rows existed: no sliced-ELL layout had been built past 2^32 bytes and no
sparse key had held a row id above 2^24.  Bar: the project's usual one — index, f32 score bits, order, counts and `query` equal to the
model's (tests/sparse_ref.py), no tolerance, through the helpers of tests/test_gpu_sparse.py (imported, not copied).  One store is
alive at a time; each is skipped with its byte count where the device has too little free memory.

  L  the smallest layout whose index array crosses 2^32 bytes while the LDS form is still eligible (tests/sparse_cases.py:
     large_case): vocab 32768, 520 slices = 33 280 rows of dim 1, one row of 32 767 entries per slice at lane 7 t mod 64, the others
     0 to 3 entries; full-mantissa values and weights.  520 x 64 x 32 767 = 1 090 485 760 padded entries = 2^30.02: the index array
     ends at byte 4 361 943 040, the value array lies between there and byte 8 723 886 080 of the allocation; about 17.1 M entries,
     a host CSR of about 140 MB.  Entry 2^29 — byte 2^31 of the index array — is position 256 of slice 256, entry 2^30 — byte 2^32 —
     position 512 of slice 512; slices 512 to 519 lie wholly or partly past the line, and their long rows sit at the lanes of the
     long rows of slices 0 to 7 with other values: tests/test_sparse_rounding_cpu.py proves that a kernel whose entry byte offset
     wraps mod 2^32 gives every one of them other bits.  Checked: both forms, 1 and 5 queries, both takes, k = n; read_sparse of the
     windows around slices 255/256 and 511/512 and of the last rows; sparse_df under both of its forms against np.bincount, with a
     long row past the line deleted and restored; sparse_info() and bytes_scanned against the layout arithmetic.
     NOT reached: 2^31 and 2^32 ENTRIES (entry offsets, not byte offsets, past 32 bits) would need 16 to 32 GiB of layout and as
     much host staging work; the entry offsets are 64-bit by reading (ott_sparse.hip: `at`, `(uint64_t)e * 64`; ott_sparse_plan.h).
     Building L copies 8.7 GB to the device through the 32 MiB staging.  Measured once on an MI355X: set_sparse (with the 33 280
     dense rows) 0.82 s, the rows on the host before it 0.64 s, the model's scores for five queries after it 1.99 s — more than one
     test of this suite usually costs, so L is one module-scoped object shared by all of its tests.  The whole file took 15.2 s
     alone (about 10 s of that is the process's first use of the device, in the test that asks for L first) and R's store 0.08 s;
     every other test of the file is under 0.2 s.

  R  row ids above 2^24: dim 1, 2^24 + 300 rows (reserve + append_random), vocab 512.  Sparse entries exist only in
     large_offsets.windows(n, (2^24,)) — 130 rows at both ends and on either side of row 2^24, ring_case's lengths and values —
     every other row is empty.  The model runs over the compact rows and its indices are mapped through K, as 3.1p does; a row
     without entries is no candidate, so the FIRST run needs no row mask: whole empty slices are skipped by the ballot and ids on both
     sides of 2^24 compete.  The second run deletes rows on both sides of 2^24.  Both forms, 1 and 5 queries (the key table of a
     four-query pass is 512 MiB), both takes, k = 50 and k = 600 (the pair form of the top-k).  Five queries x (2^24 + 300) rows are
     above the 2^26 pairs the pair form serves (ott_sparse_plan.h: SPARSE_MAX_SORT_PAIRS), so k = 600 runs with one and with three
     queries and the refusal of five is asserted.  Document frequencies with and without the deleted rows, both forms."""
import time

import numpy as np
import pytest

import hybrid_ref as H
import large_offsets as LO
import sparse_cases as SC
import sparse_ref as SR
from otters_amd import OttersError, Path, VecStore
from test_gpu_sparse import Sparse, check, run, same

pytestmark = pytest.mark.gpu

SEED = 0x5BA75E
L_PADDED = SC.LARGE_SLICES * SC.LARGE_SLICE_ENTRIES
L_BYTES = L_PADDED * 8 + (SC.LARGE_SLICES + 1) * 8 + SC.LARGE_SLICES * 256
R_ROWS = (1 << 24) + 300
R_BYTES = 4 << 30  # dense rows and sparse lengths (0.2 GiB), the key table of a four-query pass (0.5 GiB), the top-k's pair form over 3 x 2^24 pairs


def need_free(name, need):
    import torch
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        pytest.skip(f"store {name} needs {need} bytes of device memory (the layout, the tables and a quarter more), {free} are free")


class Large:
    """L: the store, its CSR and the model's scores for five queries, made once and never changed"""

    def __init__(self):
        need_free("L", int(1.25 * L_BYTES))
        t0 = time.perf_counter()
        rows, vocab, self.q5 = SC.large_case()
        t1 = time.perf_counter()
        self.sp = Sparse(rows, vocab)
        t2 = time.perf_counter()
        # the model: the 520 long rows and the others apart (two calls of sparse_ref.scores over disjoint rows: the same serial sums,
        # without 32 767 scans of all the lengths)
        long = np.array([64 * t + SC.large_long_lane(t) for t in range(SC.LARGE_SLICES)])
        none = (SC.u32(), SC.f32())
        is_long = np.zeros(len(rows), bool)
        is_long[long] = True
        S, cand = SR.scores(*SR.csr([none if is_long[r] else row for r, row in enumerate(rows)]), self.q5, vocab)
        S[:, long], cand[:, long] = SR.scores(*SR.csr([rows[r] for r in long]), self.q5, vocab)
        self.q1 = self.q5[:1]
        self.sp._scores[id(self.q5)] = (self.q5, (S, cand))
        self.sp._scores[id(self.q1)] = (self.q1, (S[:1], cand[:1]))
        self.long = long
        print(f"store L: {len(rows)} rows, {int(self.sp.ptr[-1])} entries: the rows on the host took {t1 - t0:.2f} s, the dense rows and set_sparse "
              f"(8.7 GB through the staging) {t2 - t1:.2f} s, the model's scores {time.perf_counter() - t2:.2f} s")

    def close(self):
        self.sp.store.close()


class RowIds:
    """R: the store, the compact rows of K and their CSR over the whole store"""

    def __init__(self):
        need_free("R", int(1.25 * R_BYTES))
        t0 = time.perf_counter()
        self.n, self.vocab = R_ROWS, 512
        self.K, _ = LO.windows(self.n, (1 << 24,))
        rng = np.random.default_rng(SEED)
        pool = np.arange(self.vocab, dtype=np.uint32)
        self.rows_c = [SC.ring_row(rng, SC.RING_LENS[i % len(SC.RING_LENS)], pool) for i in range(self.K.size)]
        self.ptr_c, self.idx, self.val = SR.csr(self.rows_c)
        lens = np.zeros(self.n, np.uint64)
        lens[self.K] = np.diff(self.ptr_c.astype(np.int64)).astype(np.uint64)
        ptr = np.zeros(self.n + 1, np.uint64)
        np.cumsum(lens, out=ptr[1:])
        self.store = VecStore(1)
        self.store.reserve(self.n)
        self.store.append_random(self.n, SEED)
        self.store.set_sparse(ptr, self.idx, self.val, self.vocab)
        self.q5 = [SC.ring_query(rng, pool, 400) for _ in range(5)]
        self.scores = {nq: SR.scores(self.ptr_c, self.idx, self.val, self.q5[:nq], self.vocab) for nq in (1, 3, 5)}
        print(f"store R: {self.n} rows, {self.K.size} of them with entries, made in {time.perf_counter() - t0:.2f} s")

    def expected(self, nq, take, k, keep_c=None):
        S, cand = self.scores[nq]
        return [LO.to_store_index(self.K, h) for h in SR.expected(S, cand, take, k, keep=keep_c)]

    def close(self):
        self.store.close()


class Stores:
    def __init__(self):
        self.name, self.obj = None, None

    def get(self, name):
        if self.name != name:
            self.drop()
            self.obj, self.name = (Large if name == "L" else RowIds)(), name
        return self.obj

    def drop(self):
        if self.obj is not None:
            self.obj.close()
        self.obj, self.name = None, None


@pytest.fixture(scope="module")
def stores():
    s = Stores()
    yield s
    s.drop()


# ---- L: the layout past 2^32 bytes -----------------------------------------------------------------------------------------------------------------

def test_l_the_layout_is_where_the_arithmetic_says(stores):
    b = stores.get("L")
    lens = np.diff(b.sp.ptr.astype(np.int64))
    assert b.sp.n == SC.LARGE_ROWS and (lens[b.long] == SC.LARGE_LONG).all() and np.delete(lens, b.long).max() == 3
    assert L_PADDED * 4 > 1 << 32 > 512 * SC.LARGE_SLICE_ENTRIES * 4 and L_PADDED * 8 > 1 << 33
    assert b.sp.store.sparse_info() == {"vocab": SC.LARGE_VOCAB, "nnz": int(lens.sum()), "padded_entries": L_PADDED, "bytes": L_BYTES}


@pytest.mark.parametrize("nq", [1, 5])
def test_l_both_forms_against_the_model(stores, nq):
    b = stores.get("L")
    qs = b.q1 if nq == 1 else b.q5
    S, cand = b.sp.scores(qs)
    assert cand[:, b.long].all()
    for take in (1, 0):
        got, st = check(b.sp, qs, take, b.sp.n, ("L", nq, take))  # sparse_table 0, 1 and the automatic choice
        assert all(np.isin(b.long[512:], g["index"]).all() for g in got)  # the long rows past the line are among the hits
        passes = 1 if nq == 1 else 2  # automatic: the LDS form for one query, the table form (four to a pass) for five
        assert st["passes"] == passes and st["vectors_compared"] == b.sp.n * nq, st
        assert st["bytes_scanned"] == passes * (L_PADDED * 8 + SC.LARGE_SLICES * 264), st
    b.sp.store.set_option("sparse_table", 0)
    _, st = run(b.sp.store, qs, 1, 10)
    assert st["passes"] == nq and st["bytes_scanned"] == nq * (L_PADDED * 8 + SC.LARGE_SLICES * 264) and st["path_used"] == int(Path.Exact), st
    b.sp.store.set_option("sparse_table", -1)


def test_l_read_sparse_on_both_sides_of_byte_2_31_and_2_32(stores):
    b = stores.get("L")
    sp = b.sp
    for first, n in ((255 * 64, 128), (511 * 64, 128), (sp.n - 130, 130), (512 * 64 - 1, 2)):
        ptr, idx, val = sp.store.read_sparse(first, n)
        lo, hi = int(sp.ptr[first]), int(sp.ptr[first + n])
        assert hi - lo >= SC.LARGE_LONG and np.array_equal(ptr, sp.ptr[first:first + n + 1] - sp.ptr[first]), (first, n)
        assert np.array_equal(idx, sp.idx[lo:hi]) and np.array_equal(val.view(np.uint32), sp.val[lo:hi].view(np.uint32)), (first, n)


def test_l_document_frequencies_under_both_forms(stores):
    b = stores.get("L")
    sp = b.sp
    everything = np.bincount(sp.idx.astype(np.int64), minlength=sp.vocab).astype(np.uint32)
    dead = int(b.long[515])  # a long row past the line
    live = np.ones(sp.n, bool)
    live[dead] = False
    without, n_live = H.df(sp.ptr, sp.idx, sp.vocab, live)
    assert n_live == sp.n - 1 and int(everything.sum()) - int(without.sum()) == SC.LARGE_LONG
    builds = sp.store.sparse_df_builds()
    for form in (0, 1):  # global atomic adds, a histogram in LDS; the option is read by the build
        sp.store.set_option("sparse_df_lds", form)
        assert sp.store.delete_rows([dead]) == 1
        counts, n_docs = sp.store.sparse_df()
        assert n_docs == n_live and counts.dtype == np.uint32 and np.array_equal(counts, without), (form, np.flatnonzero(counts != without)[:8])
        assert sp.store.restore_rows([dead]) == 1
        counts, n_docs = sp.store.sparse_df()
        assert n_docs == sp.n and np.array_equal(counts, everything), (form, np.flatnonzero(counts != everything)[:8])
        builds += 2
        assert sp.store.sparse_df_builds() == builds
    sp.store.set_option("sparse_df_lds", -1)


# ---- R: row ids above 2^24 --------------------------------------------------------------------------------------------------------------------------

def r_runs(b, keep_c, where):
    for form in (0, 1):
        b.store.set_option("sparse_table", form)
        for nq, k in ((1, 50), (5, 50), (1, 600), (3, 600)):
            for take in (1, 0):
                exp = b.expected(nq, take, k, keep_c)
                ids = np.concatenate([h["index"] for h in exp]).astype(np.int64)
                assert (ids >= 1 << 24).any() and (ids < 1 << 24).any()
                got, st = run(b.store, b.q5[:nq], take, k)
                same(got, exp, (where, form, nq, k, take))
                assert st["passes"] == (nq if form == 0 else -(-nq // 4)) and st["vectors_compared"] == b.n * nq, st
        with pytest.raises(OttersError, match="k above 512 is served only up to 2\\^26"):
            run(b.store, b.q5, 1, 600)
    b.store.set_option("sparse_table", -1)


def r_df(b, keep_c, n_docs_exp, where):
    exp, _ = H.df(b.ptr_c, b.idx, b.vocab, keep_c)
    for form in (0, 1):
        b.store.set_option("sparse_df_lds", form)
        assert b.store.delete_rows([1000]) == 1  # (a row without entries and back again: the counts are stale, the next read builds them under `form`)
        assert b.store.restore_rows([1000]) == 1
        counts, n_docs = b.store.sparse_df()
        assert n_docs == n_docs_exp and np.array_equal(counts, exp), (where, form, np.flatnonzero(counts != exp)[:8])
    b.store.set_option("sparse_df_lds", -1)


def test_r_no_mask_ids_on_both_sides_of_2_24_compete(stores):
    b = stores.get("R")
    assert b.K.size == 4 * LO.HALF and (b.K == (1 << 24) - 1).any() and (b.K == 1 << 24).any() and b.K[-1] == b.n - 1
    r_runs(b, None, "R, no mask")
    r_df(b, None, b.n, "R")


def test_r_deleted_rows_on_both_sides_of_2_24(stores):
    b = stores.get("R")
    rng = np.random.default_rng(2)
    dead = np.unique(np.concatenate([np.arange((1 << 24) - 40, (1 << 24) + 40), rng.choice(b.K, 100, replace=False)]))
    assert b.store.delete_rows(dead) == dead.size
    keep_c = ~np.isin(b.K, dead)
    r_runs(b, keep_c, "R, deleted rows")
    r_df(b, keep_c, b.n - dead.size, "R, deleted rows")
    b.store.restore_rows(dead)
