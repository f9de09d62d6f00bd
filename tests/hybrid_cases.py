"""The sharp cases of hybrid search (tests/test_hybrid_cpu.py proves them sharp in numpy, tests/test_gpu_hybrid.py runs them on the
device): tiny stores on which a WRONG implementation returns another first hit than the model (tests/hybrid_ref.py).  Every store has
dim 8; a dense leg e_c = (0, .., 1, .., 0) scores a row by its column c under the dot product, and a sparse query ([i], [1.0]) scores
a row by the value it stores under index i.

Each case is a dict: rows [n, 8] f32, sparse = the rows' sparse vectors as (indices, values) pairs, vocab, dense = [legs, 8] f32 or
None, sparse_q = the sparse queries of the one request, metric, take (of the dense legs), fusion, rrf_k, weights, fetch, k, idf."""
import numpy as np

import fuse_ref as R
from otters_amd import Metric

DIM = 8


def _rows(cols):
    rows = np.zeros((len(cols), DIM), np.float32)
    cols = np.asarray(cols, np.float32)
    rows[:, :cols.shape[1]] = cols
    return rows


def _unit(*which):
    legs = np.zeros((len(which), DIM), np.float32)
    for i, c in enumerate(which):
        legs[i, c] = 1.0
    return legs


def sparse_take(fusion=R.MINMAX):
    """(a) A squared-L2 dense leg (take Min) beside a sparse leg (take Max).  Distances from (1, 0, ..): rows 0, 1, 2 lie at 0, 1, 4, so
    the dense leg gives 1, 3/4, 0 under MINMAX.  The sparse leg scores them 1, 10, 5: normalised under ITS take (Max) it gives 0, 1,
    4/9 and row 1 wins with 7/4.  Normalised under the dense leg's Min take the list — best first under Max — has its 'worst minus
    best' negative, every entry gets 0.5 and row 0 wins with 3/2.  (DBSF: the same list measured from mean + 3 sigma downwards turns
    the sparse ranking upside down, and row 0 wins as well.)"""
    return dict(rows=_rows([(1,), (2,), (3,)]), sparse=[([0], [1.0]), ([0], [10.0]), ([0], [5.0])], vocab=4, dense=_unit(0), sparse_q=[([0], [1.0])],
                metric=Metric.Euclidean, take=0, fusion=fusion, rrf_k=0.0, weights=None, fetch=3, k=1, idf=False, wrong=dict(takes=[0, 0]), first=1, wrong_first=0)


def leg_order():
    """(b) Row 0 is first in two dense legs and in the sparse leg, with weights 1e8, 1, -1e8 and rrf_k = 0 (a first position
    contributes the weight itself).  In leg order — dense, dense, sparse — F = ((0 + 1e8) + 1) - 1e8 = 0: the 1 is lost below 1e8's ulp
    of 8.  Row 2 is second in the first dense leg and in the sparse leg: 5e7 - 5e7 = 0 in either order.  Row 1 is second in the other
    dense leg, F = 1/2, and wins.  With the sparse leg summed first, row 0's F = (-1e8 + 1e8) + 1 = 1 and row 0 wins."""
    return dict(rows=_rows([(2, 2), (0, 1), (1, 0)]), sparse=[([0], [5.0]), ([1], [1.0]), ([0], [3.0])], vocab=4, dense=_unit(0, 1), sparse_q=[([0], [1.0])],
                metric=Metric.DotProduct, take=1, fusion=R.RRF, rrf_k=0.0, weights=[1e8, 1.0, -1e8], fetch=2, k=1, idf=False, wrong=dict(leg_order=(2, 0, 1)),
                first=1, wrong_first=0)


def idf_rank():
    """(c) Index 0 is stored by five of six rows, index 1 by one.  The query weighs them 1 and 0.8: as it stands row 0 (value 1 under
    index 0) scores 1 and leads row 5 (value 1 under index 1) at 0.8.  With IDF the weights become 1 x log(1 + 1.5 / 5.5) = 0.241 and
    0.8 x log(1 + 5.5 / 1.5) = 1.233, and row 5 leads."""
    sparse = [([0], [1.0])] + [([0], [0.5])] * 4 + [([1], [1.0])]
    return dict(rows=_rows([(1,)] * 6), sparse=sparse, vocab=3, dense=None, sparse_q=[([0, 1], [1.0, 0.8])], metric=Metric.DotProduct, take=1, fusion=R.RRF,
                rrf_k=60.0, weights=None, fetch=6, k=1, idf=True, wrong=dict(idf=False), first=5, wrong_first=0)


CASES = {"sparse_take_minmax": sparse_take, "sparse_take_dbsf": lambda: sparse_take(R.DBSF), "leg_order": leg_order, "idf_rank": idf_rank}
