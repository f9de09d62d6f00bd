"""GPU: the sparse sweep's ROUNDING and ORDER held to the model (sparse_lds_kernel, sparse_table_kernel, sparse_walk in
ott_sparse.hip).  The contract: S is summed in the row's index order, one rounded f32 operation at a time, nothing
fused, nothing flushed to zero, and the LDS form and the table form give the same bits.  tests/test_gpu_sparse.py and
tests/test_gpu_hybrid.py feed the kernels multiples of 1/4 and 1/2: every product and partial sum is exact there, so a kernel that
adds in another order, rotates its register ring wrongly, fuses the product, keeps two accumulators or flushes subnormals passes them
bit for bit.  Here the values and weights have full mantissas (tests/sparse_cases.py: ring_case, ring_large_case, subnormal_case);
tests/test_sparse_rounding_cpu.py proves on the model alone that each of those mutations changes S's bits on a large share of the
pairs.  Bar: index, f32 score bits, order, counts and `query` equal to the model's (tests/sparse_ref.py), no tolerance, through the
helpers of tests/test_gpu_sparse.py and tests/test_gpu_hybrid.py (imported, not copied): `check` runs both forms where the vocab
allows, the automatic choice, and the caller names the take."""
import numpy as np
import pytest

import sparse_cases as SC
import test_gpu_hybrid as TH
from test_gpu_hybrid import World, expect
from test_gpu_sparse import Sparse, check, run

pytestmark = pytest.mark.gpu

CASES = {name: (rows, vocab, queries) for name, rows, vocab, queries in SC.cpu_cases()}
TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def ring():
    rows, vocab, queries = CASES["ring"]
    return Sparse(rows, vocab), queries


# ---- every case the CPU tests hold the plan header to, on the device: k = the row count, so every candidate's bits are compared -------------

@pytest.mark.parametrize("name", list(CASES))
def test_every_cpu_case_on_the_device(name):
    rows, vocab, queries = CASES[name]
    sp = Sparse(rows, vocab)
    for take in (1, 0):
        got, _ = check(sp, queries, take, sp.n, (name, "take", take))
        S, cand = sp.scores(queries)
        assert [g.size for g in got] == [int((c & ~np.isnan(s)).sum()) for s, c in zip(S, cand)], name  # every candidate came back
    sp.store.close()


# ---- the ring case: every table slot, every survivor pattern -------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5])
def test_ring_case_by_batch_size(ring, nq):
    """one to four queries fill one to four slots of the table form's pass; five make a second pass"""
    sp, queries = ring
    for take in (1, 0):
        check(sp, queries[:nq], take, sp.n, ("ring", "nq", nq, take))


@pytest.mark.parametrize("rot", [1, 2, 3, 4])
def test_ring_case_rotated_so_that_each_query_visits_each_slot(ring, rot):
    sp, queries = ring
    check(sp, queries[rot:] + queries[:rot], 1, sp.n, ("ring", "rotated by", rot))


def test_ring_case_the_sum_of_a_lane_does_not_depend_on_its_neighbours(ring):
    """a row mask that leaves one row of a slice — of the cycling slice 1, of the slice of 16-entry rows and of the 17-entry one — and
    one that leaves every second row: the lanes beside a survivor load nothing"""
    sp, queries = ring
    lone = np.ones(sp.n, bool)
    for t, lane in ((1, 17), (2, 63), (3, 0)):
        lone[64 * t:64 * t + 64] = False
        lone[64 * t + lane] = True
    for keep, name in ((lone, "one row of a slice"), (np.arange(sp.n) % 2 == 1, "every second row")):
        for take in (1, 0):
            got, st = check(sp, queries, take, sp.n, ("ring", name, take), keep=keep, mask=keep)
            assert all(g.size and keep[g["index"].astype(np.int64)].all() for g in got)


def test_ring_case_a_chunk_mask_that_cuts_through_slices():
    """chunks of 100 rows, the second and the fourth dropped: slices 1, 3 and 4 are cut at rows 100, 200 and 300"""
    rows, vocab, queries = CASES["ring"]
    sp = Sparse(rows, vocab, chunk=100)
    cm = np.array([True, False, True, False])
    keep = np.repeat(cm, 100)[: sp.n]
    for take in (1, 0):
        got, st = check(sp, queries, take, sp.n, ("ring", "chunk mask", take), keep=keep, chunk_mask=cm)
        assert st["vectors_compared"] == int(keep.sum()) * len(queries)
    sp.store.close()


# ---- subnormal products and sums ---------------------------------------------------------------------------------------------------------------

def test_subnormal_sums_are_kept_by_both_forms():
    rows, vocab, queries = CASES["subnormal"]
    sp = Sparse(rows, vocab)
    check(sp, queries, 1, sp.n, "subnormal")
    S, cand = sp.scores(queries)
    for form in sp.forms():
        sp.store.set_option("sparse_table", form)
        got, _ = run(sp.store, queries, 0, sp.n)
        scores = np.concatenate([g["score"] for g in got])
        assert scores.size == int(cand.sum())
        assert int(((scores != 0) & (np.abs(scores) < TINY)).sum()) >= 100, form  # nothing was flushed to zero
        assert not (scores.view(np.uint32) == 0x80000000).any(), form             # S is never -0.0
    sp.store.set_option("sparse_table", -1)
    sp.store.close()


# ---- hybrid: DBSF and min-max normalise sparse legs whose scores have full mantissas ---------------------------------------------------------------

@pytest.mark.parametrize("vocab", [100, 40000])  # the LDS form and the table form of the sparse sweep
def test_hybrid_with_full_mantissa_sparse_legs(oracle, vocab):
    rng = np.random.default_rng(vocab)
    if vocab == 100:
        pool = np.arange(vocab, dtype=np.uint32)
        rows = SC.ring_rows(rng, pool, tuple(L for L in SC.RING_LENS if L <= 64))
        supports = (1, 30, 80)
    else:
        rows, _, _ = SC.ring_large_case(rng, vocab)
        pool = SC.used_indices(rows)
        supports = (1, 40, 280)
    w = World(8, len(rows), vocab, seed=3, sparse=rows)
    dense = w.dense_sets([d for d, _ in TH.LEGS])
    sparse = [[SC.ring_query(rng, pool, supports[(b + j) % 3]) for j in range(s)] for b, (_, s) in enumerate(TH.LEGS)]
    for idf in (False, True):
        for metric in TH.TAKE:
            for fusion in TH.FUSIONS:
                got = TH.plan_of(w.store, dense, sparse, metric, fusion, 9, 30, idf=idf).collect_arrays()
                TH.same(got, expect(oracle, w, dense, sparse, metric, fusion, 9, 30, idf=idf), (vocab, idf, metric, fusion))
    w.close()
