"""The sharp cases of rank fusion (tests/test_fuse_cpu.py proves them sharp in numpy, tests/test_gpu_fuse.py runs them on the device):
small stores whose leg lists make a WRONG implementation return a different top-k than the model (tests/fuse_ref.py).  Every store has
dim 8 and is queried with the dot product under take Max; a leg (1, 0, ...) ranks by column 0, a leg (0, 1, 0, ...) by column 1, so
a list's scores are the column's values exactly.

Each case is a dict: rows [n, 8] f32, legs [L, 8] f32 (one request), fusion, rrf_k, weights, fetch, k."""
import numpy as np

import fuse_ref as R

DIM = 8


def _rows(cols):
    rows = np.zeros((len(cols), DIM), np.float32)
    rows[:, :2] = np.asarray(cols, np.float32)
    return rows


def _legs(*which):
    legs = np.zeros((len(which), DIM), np.float32)
    for i, c in enumerate(which):
        legs[i, c] = 1.0
    return legs


def leg_order():
    """Row 0 is first in three legs with weights 1e8, 1, -1e8 (rrf_k = 0: a first position contributes the weight itself).  In leg
    order F = ((0 + 1e8) + 1) - 1e8 = 0: the 1 is lost below 1e8's ulp of 8, and row 1 (F = 1/2) wins.  Summed as legs 0, 2, 1,
    F = 1 and row 0 wins."""
    return dict(rows=_rows([(2, 2), (0, 1), (1, 0)]), legs=_legs(0, 1, 0), fusion=R.RRF, rrf_k=0.0, weights=[1e8, 1.0, -1e8], fetch=2, k=1,
                wrong=dict(leg_order=(0, 2, 1)))


def rrf_rank():
    """Lists [0, 1] and [2, 1] with rrf_k = 0.5: with r + 1, row 0 gets 1 / 1.5 and row 1 gets 2 / 2.5, so row 1 wins; with r in
    its place row 0 gets 1 / 0.5 and row 1 gets 2 / 1.5, so row 0 wins."""
    return dict(rows=_rows([(2, 0), (1, 1), (0, 2)]), legs=_legs(0, 1), fusion=R.RRF, rrf_k=0.5, weights=None, fetch=2, k=1, wrong=dict(rank_from=0))


def equal_f():
    """The same store: rows 0 and 2 are first in one leg each, so their F are the same bits and row 0 must come before row 2."""
    c = rrf_rank()
    c.update(k=3, wrong=None)
    return c


def seq_sum(terms):
    """a WRONG mean: the f64 terms added one after the other"""
    a = np.float64(0.0)
    for x in np.asarray(terms, np.float64):
        a = a + x
    return a


def f32_sum(terms):
    """a WRONG mean: the terms added in f32"""
    a = np.float32(0.0)
    with np.errstate(all="ignore"):
        for x in np.asarray(terms, np.float64).astype(np.float32):
            a = np.float32(a + x)
    return np.float64(a)


DBSF_SEED = 0  # chosen so that both wrong means move the probes' F (test_fuse_cpu.py checks that it still does)


def dbsf_mean(seed=DBSF_SEED):
    """Leg 0's list has 512 entries: 461 scores near 2^40 and 49 small ones, whose f64 sum depends on the order of the additions,
    and two PROBES whose score is the f32 next to the list's own mean - 3 sigma, so that score - worst cancels down to the bits the
    order decides.  Leg 1 scores every row 0 (sigma = 0: every entry gets 0.5) and lists the 512 lowest rows it may, which are the
    FILLERS: rows too bad for leg 0, whose F is half of leg 1's weight — set to the probes' F under the model.  Leg 0's weight is -1,
    so the probes and the fillers lead the ranking.  Probe 0 is row 0
    (kept out of leg 1 by column 1), probe 1 the last row.  The model's top-2 is [probe 0, first filler]: a tie goes to the lower
    row.  A mean that moves the probes' F up gives [probe 0, probe 1], one that moves it down two fillers."""
    rng = np.random.default_rng(seed)
    big = (np.float32(2.0 ** 40) * (1 + rng.random(461).astype(np.float32))).astype(np.float32)
    small = (rng.random(49).astype(np.float32) * np.float32(1024.0)).astype(np.float32)
    probe = np.float32(0.0)
    for _ in range(20):  # the probes are part of the list they lie at the edge of: a fixed point, reached in a few rounds
        scores = np.sort(np.concatenate([big, small, [probe, probe]]).astype(np.float32))[::-1]
        worst, _ = R.leg_stats(R.DBSF, True, scores)
        nxt = np.float32(worst)
        if nxt == probe:
            break
        probe = nxt
    assert scores[-1] == probe and scores[-2] == probe, "the probes are the list's last two entries"
    target = R.contributions(R.DBSF, True, 0.0, -1.0, scores)[-1]  # the probes' F under the model (leg 0 weighs -1: its worst rows come first)
    cols = [(probe, -1.0)] + [(-1e30, 0.0)] * 512 + [(x, 0.0) for x in np.concatenate([big, small])] + [(probe, 0.0)]
    return dict(rows=_rows(cols), legs=_legs(0, 1), fusion=R.DBSF, rrf_k=0.0, weights=[-1.0, float(np.float32(2.0) * target)], fetch=512, k=2,
                wrong=[dict(mean_of=seq_sum), dict(mean_of=f32_sum)], scores=scores, target=target)
