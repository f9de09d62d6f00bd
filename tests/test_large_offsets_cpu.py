"""CPU: what tests/test_gpu_large_offsets.py rests on, proved without a GPU.

1. The helper: windows(), the packed mask made without an n-element array, window_rows(), to_store_index().
2. The subset identity: for every kind's host model, "the model on all rows under the row mask K" equals "the model on R[K] with
   no mask, mapped through K" — indices, order, counts, side outputs and score bits — on a store of 3000 rows that the models can
   score whole.
3. The planted rows' separation (the precondition of the unmasked GPU cases, in the manner of tests/test_i8_bound_cases.py): against
   unplanted rows at the cube's corners, the worst an element in [-1, 1) can do, every planted row still wins; and the figure of the
   Hoeffding bound quoted in the GPU file.
4. The mutation check: a "kernel" whose `row * ld` wraps at 32 bits reads row r mod 2^k; its answers, made by the same models from the
   rows such a kernel would read, differ from the expected ones for every kind at every boundary of W — and a row id put through a
   float differs on N.  A comparison that passes against wrapped addresses would prove nothing."""
import numpy as np
import pytest

import grouped_ref as GR
import large_offsets as LO
import masks_ref as MKR
import maxsim_ref as MS
import mmr_ref as MR
import recommend_ref as RR
import recommend_strategy_ref as RS
import test_gpu_discover as TD
import test_gpu_groups as G
import test_gpu_idlist as IL
import test_gpu_maxsim_groups as MG
import test_gpu_recommend_strategy as TS
from otters_amd import Metric

TAKE = IL.TAKE
ALL_METRICS = IL.ALL_METRICS
SEED = 0x1A46E


# ---- 1. the helper ---------------------------------------------------------------------------------------------------------------

def test_windows_are_two_tiles_and_a_part_on_each_side_unaligned():
    n, bnd = (1 << 21) + 300, (1 << 18, 1 << 19, 1 << 20, 1 << 21)
    K, words = LO.windows(n, bnd)
    assert K.dtype == np.int64 and np.all(np.diff(K) > 0) and K[0] == 0 and K[-1] == n - 1
    assert LO.runs_of(K) == [(0, 130)] + [(b - 130, 260) for b in bnd] + [(n - 130, 130)]
    for b in bnd:
        assert {b - 130, b - 1, b, b + 129} <= set(K.tolist()) and b - 131 not in K and b + 130 not in K
    assert 130 > 2 * 64 and (1 << 18) % 64 == 0 and ((1 << 18) - 130) % 64 != 0  # two full tiles and a part, unaligned
    assert words.dtype == np.uint64 and words.size == (n + 63) // 64
    assert np.array_equal(np.flatnonzero(LO.mask_bool(words, n)), K)
    assert int(sum(bin(int(w)).count("1") for w in words[words != 0])) == K.size


def test_windows_clip_and_merge():
    K, words = LO.windows(300, (100, 150), half=60)
    assert LO.runs_of(K) == [(0, 210), (240, 60)]  # [0, 60) + [40, 160) + [90, 210) merge; [240, 300)
    K, _ = LO.windows(1000, (500,), half=10)
    assert LO.runs_of(K) == [(0, 10), (490, 20), (990, 10)]
    assert LO.compact_of(K, [0, 490, 999]).tolist() == [0, 10, 39]
    with pytest.raises(AssertionError):
        LO.compact_of(K, [11])
    assert LO.to_store_index(K, np.array([0, 10, 39])).tolist() == [0, 490, 999]


def test_window_rows_are_the_corpus_rows(oracle):
    n, dim = 5000, 24
    K, _ = LO.windows(n, (1000, 3000), half=33)
    assert np.array_equal(LO.window_rows(oracle, K, dim, SEED).view(np.uint32), oracle.rand_rows(0, n, dim, SEED)[K].view(np.uint32))


# ---- 2. the subset identity ------------------------------------------------------------------------------------------------------

class Small:
    def __init__(self, oracle, n=3000, dim=24, bnd=(1000, 2000), quantised=False):
        self.oracle, self.n, self.dim = oracle, n, dim
        rng = np.random.default_rng(dim)
        self.rows = oracle.rand_rows(0, n, dim, SEED)
        if quantised:  # many equal scores: the tie order (the lower row) must survive the mapping
            self.rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
            self.rows[np.all(self.rows == 0, axis=1), 0] = 1.0
        self.inv = oracle.inv_norms(self.rows)
        self.K, words = LO.windows(n, bnd)
        self.keep = LO.mask_bool(words, n)
        self.R, self.invK = np.ascontiguousarray(self.rows[self.K]), self.inv[self.K]
        self.q = rng.uniform(-1, 1, (5, dim)).astype(np.float32) if not quantised else rng.integers(-2, 3, (5, dim)).astype(np.float32)
        self.rng = rng

    def S(self, hits):
        return LO.to_store_index(self.K, hits)


@pytest.fixture(scope="module", params=[False, True], ids=["uniform", "quantised"])
def small(oracle, request):
    return Small(oracle, quantised=request.param)


def same_hits(a, b, where):
    assert a.size == b.size, where
    for f in ("index", "query"):
        assert np.array_equal(a[f].astype(np.int64), b[f].astype(np.int64)), (where, f)
    assert np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)), where


@pytest.mark.parametrize("metric", ALL_METRICS, ids=lambda m: m.name)
def test_identity_id_lists_grouped_maxsim_and_masks(small, metric):
    s, take = small, TAKE[metric]
    full_all = IL.ranking(s.oracle, s.rows, s.q, metric, take)
    full_K = IL.ranking(s.oracle, s.R, s.q, metric, take)
    # the ranking itself, then id lists
    same_hits(IL.expected(full_all, s.keep, s.n * 5, 5, False)[0], s.S(full_K), (metric, "ranking"))
    ids_c = np.concatenate([s.rng.choice(s.K.size, 200), [0, 0, s.K.size - 1]])
    for k in (1, 10, 300):
        for perq in (False, True):
            a, ca = IL.expected(full_all, IL.id_mask(s.n, s.K[ids_c]), k, 5, perq)
            b, cb = IL.expected(full_K, IL.id_mask(s.K.size, ids_c), k, 5, perq)
            same_hits(a, s.S(b), (metric, "ids", k, perq))
            assert ca == cb
    assert np.array_equal(IL.dense_scores(full_all, 5, s.K[ids_c]).view(np.uint32), IL.dense_scores(full_K, 5, ids_c).view(np.uint32))
    # grouped search: gid = row // 4 straddles every window edge
    gid = np.arange(s.n) // 4
    labels, gid_c = np.unique(s.K // 4, return_inverse=True)
    gid_c = gid_c.reshape(-1)
    ones = np.ones(s.K.size, bool)
    for nq in (1, 5):
        fa, fk = full_all[full_all["query"] < nq], full_K[full_K["query"] < nq]
        a, ca = G.expected(fa, gid, s.keep, 10, nq)
        b, cb = G.expected(fk, gid_c, ones, 10, nq)
        same_hits(a, s.S(b), (metric, "one_per_group", nq))
        assert ca == cb
        a, ca, ga = GR.expected(fa, gid, s.keep, 10, nq, 3)
        b, cb, gb = GR.expected(fk, gid_c, ones, 10, nq, 3)
        same_hits(a, s.S(b), (metric, "per_group(3)", nq))
        assert ca == cb and np.array_equal(ga, labels[gb])
        # MaxSim: the sweep and a list
        a = MS.expected(fa, gid, s.keep, 10, nq, take, n_groups=int(gid.max()) + 1)
        b = MS.expected(fk, gid_c, ones, 10, nq, take, n_groups=labels.size)
        assert np.array_equal(a["index"], labels[b["index"].astype(np.int64)]) and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)), (metric, nq)
        listed_c = s.rng.choice(labels.size, 40)
        a = MG.reference(fa, gid, int(gid.max()) + 1, s.keep, labels[listed_c], 10, nq, take)
        b = MG.reference(fk, gid_c, labels.size, ones, listed_c, 10, nq, take)
        assert a.size and np.array_equal(a["index"], labels[b["index"].astype(np.int64)]) and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32))
    # a row mask per query, K the common mask; one mask shorter than the store
    masks_c = [s.rng.random(s.K.size) < 0.5 for _ in range(5)]
    masks = []
    for i, mc in enumerate(masks_c):
        m = np.zeros(s.n if i != 4 else s.n - 60, bool)
        rows = s.K[mc]
        m[rows[rows < m.size]] = True
        masks.append(m)
    masks_c[4] = masks_c[4] | (s.K >= s.n - 60)
    a = MKR.expected(s.oracle, s.rows, s.q, masks, metric, take, 20, common=s.keep)
    b = MKR.expected(s.oracle, s.R, s.q, masks_c, metric, take, 20)
    for x, y in zip(a, b):
        same_hits(x, s.S(y), (metric, "masks"))


@pytest.mark.parametrize("metric", ALL_METRICS, ids=lambda m: m.name)
def test_identity_recommend_discover_and_mmr(small, metric):
    s, take = small, TAKE[metric]
    ex_c = s.rng.choice(s.K.size, 8, replace=False).tolist()
    ex = s.K[ex_c].tolist()
    P_all = RR.pair_scores(s.oracle, s.rows, s.inv, ex, metric)
    P_K = RR.pair_scores(s.oracle, s.R, s.invK, ex_c, metric)
    for k in (10, s.n):
        for flags in (0, RR.FILL):
            a, sa = RR.recommend(s.oracle, s.rows, s.inv, ex[:5], ex[5:], metric, take, k, flags=flags, keep=s.keep, P=P_all)
            b, sb = RR.recommend(s.oracle, s.R, s.invK, ex_c[:5], ex_c[5:], metric, take, k, flags=flags, P=P_K)
            same_hits(a, s.S(b), (metric, "best_score", k, flags))
            assert sa.tolist() == sb.tolist()
        a, sa = RS.sum_scores(s.oracle, s.rows, s.inv, ex[:5], ex[5:], metric, take, k, keep=s.keep, P=P_all)
        b, sb = RS.sum_scores(s.oracle, s.R, s.invK, ex_c[:5], ex_c[5:], metric, take, k, P=P_K)
        same_hits(a, s.S(b), (metric, "sum_scores", k))
        a, _ = TS.average_model(s.oracle, s.rows, s.inv, ex[:5], ex[5:], metric, take, min(k, 500), keep=s.keep)
        b, _ = TS.average_model(s.oracle, s.R, s.invK, ex_c[:5], ex_c[5:], metric, take, min(k, 500))
        same_hits(a, s.S(b), (metric, "average_vector", k))
    # discover: 3 pairs; a target row, a vector, none; min_wins
    m_all, m_K = TD.Model(s.oracle, s.rows, s.inv), TD.Model(s.oracle, s.R, s.invK)
    ctx_c = [(ex_c[0], ex_c[1]), (ex_c[2], ex_c[3]), (ex_c[4], ex_c[5])]
    ctx = [(int(s.K[p]), int(s.K[g])) for p, g in ctx_c]
    for tgt_c, tgt in (({"target_row": ex_c[6]}, {"target_row": ex[6]}), ({"target": s.q[0]},) * 2, ({}, {})):
        for min_wins in (0, 2):
            a, wa = m_all(ctx, metric, take, 50, min_wins=min_wins, keep=s.keep, **tgt)
            b, wb = m_K(ctx_c, metric, take, 50, min_wins=min_wins, **tgt_c)
            same_hits(a, s.S(b), (metric, "discover", sorted(tgt), min_wins))
            assert wa.tolist() == wb.tolist() and a.size
    # MMR
    for lam in (0.0, 0.5):
        a, ca, va = MR.mmr(s.oracle, s.rows, s.q[0], metric, take, 10, 64, lam, row_mask=s.keep, inv=s.inv)
        b, cb, vb = MR.mmr(s.oracle, s.R, s.q[0], metric, take, 10, 64, lam, inv=s.invK)
        MR.same(a, va, s.S(b), vb)
        assert ca == cb


# ---- 3. the planted rows win by construction ----------------------------------------------------------------------------------------

NAMES = {Metric.Cosine: "cosine", Metric.Euclidean: "l2", Metric.DotProduct: "dot", Metric.Manhattan: "l1"}


@pytest.mark.parametrize("dim", [4, 2048])
@pytest.mark.parametrize("metric", [Metric.Euclidean, Metric.DotProduct, Metric.Manhattan], ids=lambda m: m.name)
def test_planted_rows_beat_the_cube_s_corners(oracle, dim, metric):
    """unplanted elements lie in [-1, 1): no unplanted row scores better than the best corner of the closed cube — the sign vector
    itself — and every planted row beats that, with distinct scores"""
    q, rows = LO.planted(dim, 12, NAMES[metric], SEED)
    s = LO.sign_vector(dim, SEED)
    rng = np.random.default_rng(dim)
    corners = np.concatenate([s[None, :], -s[None, :], np.where(rng.random((50, dim)) < 0.5, -1.0, 1.0).astype(np.float32), s[None, :] * np.float32(0.999)])
    full = IL.ranking(oracle, np.concatenate([corners, rows]), q[None, :], metric, TAKE[metric])
    assert sorted(full["index"][:12].tolist()) == list(range(corners.shape[0], corners.shape[0] + 12))
    assert np.unique(full["score"][:12]).size == 12
    best_corner = full["score"][12]
    assert full["index"][12] == 0  # the sign vector: the best a row of the cube can do
    if metric == Metric.DotProduct:
        assert best_corner == np.float32(3 * dim) and full["score"][11] >= np.float32(6 * dim)
    else:
        per_element = 2.0 if metric == Metric.Manhattan else 4.0
        assert best_corner == np.float32(per_element * dim) and full["score"][11] <= np.float32(0.25 * dim if metric == Metric.Euclidean else 0.5 * dim)


def test_planted_cosine_rows_and_the_hoeffding_figure(oracle):
    dim, n = 2048, (1 << 21) + 300
    q, rows = LO.planted(dim, 12, "cosine", SEED)
    cos = np.array([oracle.cosine(q, r, oracle.inv_norms(q)[0], oracle.inv_norms(r)[0]) for r in rows])
    assert cos.min() >= 0.9 and np.unique(cos).size == 12 and cos.max() > 0.9999
    bound = LO.hoeffding_cosine_bound(n, dim, 0.5, 0.2)
    assert 1.2e-16 < bound < 1.3e-16, bound  # the figure in tests/test_gpu_large_offsets.py
    # the bound's two steps on a sample: a uniform row's squared norm is above 0.2 dim, its cosine far below 0.5
    sample = oracle.rand_rows(12345, 2000, dim, SEED)
    assert (np.square(sample.astype(np.float64)).sum(axis=1) > 0.2 * dim).all()
    c = (sample.astype(np.float64) @ q.astype(np.float64)) / (np.linalg.norm(sample.astype(np.float64), axis=1) * np.sqrt(dim))
    assert np.abs(c).max() < 0.15


# ---- 4. the mutation check -------------------------------------------------------------------------------------------------------------

def answers(oracle, K, R, inv, q, metric, ids_c, ex_c):
    """what the GPU file compares, per kind, from the model over the compact rows R (compact indices)"""
    take = TAKE[metric]
    m = K.size
    full = IL.ranking(oracle, R, q, metric, take)
    ones = np.ones(m, bool)
    labels, gid_c = np.unique(K // 4, return_inverse=True)
    gid_c = gid_c.reshape(-1)
    model = TD.Model(oracle, R, inv)
    ctx = [(ex_c[0], ex_c[1]), (ex_c[2], ex_c[3]), (ex_c[4], ex_c[5])]
    masks = [np.arange(m) % 5 != b for b in range(q.shape[0])]
    out = {
        "id list": IL.expected(full, IL.id_mask(m, ids_c), 100, q.shape[0], False)[0],
        "score_rows": IL.dense_scores(full, q.shape[0], ids_c),
        "mmr": MR.mmr(oracle, R, q[0], metric, take, 10, 64, 0.5, inv=inv),
        "best_score": RR.recommend(oracle, R, inv, ex_c[:5], ex_c[5:], metric, take, m),
        "sum_scores": RS.sum_scores(oracle, R, inv, ex_c[:5], ex_c[5:], metric, take, m),
        "average_vector": TS.average_model(oracle, R, inv, ex_c[:5], ex_c[5:], metric, take, m),
        "discover": model(ctx, metric, take, m, target=q[1]),
        "context search": model(ctx, metric, take, m),
        "one_per_group": G.expected(full, gid_c, ones, m, q.shape[0])[0],
        "per_group(3)": GR.expected(full, gid_c, ones, m, q.shape[0], 3)[0],
        "maxsim": MS.expected(full, gid_c, ones, labels.size, q.shape[0], take, n_groups=labels.size),
        "masks": np.concatenate(MKR.expected(oracle, R, q, masks, metric, take, m)),
        "base query": full,
    }
    return out


def differs(a, b):
    if isinstance(a, tuple):
        return any(differs(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return True
    if a.dtype.names:
        return not (np.array_equal(a["index"], b["index"]) and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)))
    if a.dtype == np.float32:
        return not np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return not np.array_equal(a, b)


@pytest.mark.parametrize("k2", [18, 19, 20, 21])
def test_wrapped_addresses_fail_every_masked_case_on_w(oracle, k2):
    """W: a byte offset held in 32 bits wraps at row 2^19 (2^18 when the int is signed), a float offset at 2^21 (2^20).  The rows at
    and above 2^k2 are read from row mod 2^k2: every kind's answer changes"""
    dim, n, bnd = 2048, (1 << 21) + 300, (1 << 18, 1 << 19, 1 << 20, 1 << 21)
    K, _ = LO.windows(n, bnd)
    R = LO.window_rows(oracle, K, dim, SEED)
    bad = R.copy()
    above = K >= (1 << k2)
    src = LO.wrapped_source(K[above], 1 << k2)
    assert above.any() and (src < (1 << k2)).all()
    bad[above] = np.concatenate([oracle.rand_rows(int(r), 1, dim, SEED) for r in src])
    rng = np.random.default_rng(k2)
    q = rng.uniform(-1, 1, (2, dim)).astype(np.float32)
    sides = LO.compact_of(K, [0, n - 1] + [r for b in bnd for r in (b - 1, b)])
    ids_c = np.concatenate([rng.choice(K.size, 300, replace=False), sides])
    ex_c = list(dict.fromkeys(sides[2:].tolist()))[:8]
    metric = ALL_METRICS[k2 % 4]
    good = answers(oracle, K, R, oracle.inv_norms(R), q, metric, ids_c, ex_c)
    wrong = answers(oracle, K, bad, oracle.inv_norms(bad), q, metric, ids_c, ex_c)
    for kind in good:
        assert differs(good[kind], wrong[kind]), (k2, metric, kind)


@pytest.mark.parametrize("name, dim, n, bnd", [("W", 2048, (1 << 21) + 300, (1 << 18, 1 << 19, 1 << 20, 1 << 21)), ("N", 4, (1 << 27) + 300, (1 << 24, 1 << 26))])
def test_wrapped_addresses_fail_the_planted_cases(oracle, name, dim, n, bnd):
    """section 3: a planted row at or above a boundary is read from row mod 2^k, which holds another row's values, so a planted row
    drops out of the top 12 or shows another score; a row id put through a float (N) reports an even row for an odd one above 2^24"""
    at = np.array(sorted(([0, n - 1] + [r for x in bnd for r in (x - 1, x)] + [r for x in bnd for r in (x - 130, x + 129)] + [129, n - 130])[:12]))
    for metric in (Metric.Euclidean, Metric.DotProduct, Metric.Manhattan):
        q, rows = LO.planted(dim, 12, NAMES[metric], SEED)
        full = IL.ranking(oracle, rows, q[None, :], metric, TAKE[metric])
        for x in bnd:
            seen = rows.copy()
            for i, r in enumerate(at):
                if r >= x:  # the address wraps: what lies at r mod x — another planted row's values, or an unplanted row's
                    w = int(r % x)
                    seen[i] = rows[list(at).index(w)] if w in at else oracle.rand_rows(w, 1, dim, SEED)[0]
            wrong = IL.ranking(oracle, seen, q[None, :], metric, TAKE[metric])
            assert differs(full, wrong), (name, metric, x)
    if name == "N":
        through_float = np.float32(at).astype(np.int64)
        assert (through_float != at).any() and (through_float[at < (1 << 24)] == at[at < (1 << 24)]).all()
