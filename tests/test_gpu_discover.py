"""GPU: discovery and context search (ott_query_discover, VecStore.discover, MetaStore.discover).  Bar: every case
is bit-equal to the host model tests/discover_ref.py — indices, order, score bits, wins, counts.  No tolerances.

The model's pair scores come from the oracle over ALL rows with the STORE's inverse norms (store.inv_norms()); they are made once
per (corpus, example row, metric) and shared by the targets, takes, k's and filters of a test.  Stores have at most 2000 rows."""
import ctypes as C

import numpy as np
import pytest

import discover_ref as D
import grouped_ref as G
import ieee_edges as E
import maxsim_ref as MS
import mmr_ref as MR
import recommend_ref as RR
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, TakeType, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)
N_ROWS = 2000
NO_ROW = 2 ** 64 - 1


@pytest.fixture(scope="module", autouse=True)
def collect_the_models_garbage():
    """The host model makes many short-lived Python objects (one oracle call per pair score).  They are collected here, when the
    module is done, so that the interpreter's next full collection does not fall into a test of another module that holds its own
    work to the host clock."""
    yield
    import gc
    gc.collect()


def make(dim, n=N_ROWS, seed=0, reduce_mode=0, rows=None):
    rng = np.random.default_rng(1000 * dim + seed)
    if rows is None:
        rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    store = VecStore(dim)
    store.set_reduce_order(reduce_mode)  # before the rows: the stored inverse norms are summed in it
    store.add_vectors(rows)
    return store, rows, store.inv_norms()


def run(store, ctx, metric, take, k, target=None, target_row=None, min_wins=0, flt=None, mask=None, path=None):
    p = store.discover(ctx, target=target, target_row=target_row, metric=metric)
    if k is not None:
        p = p.take_max(k) if take == 1 else p.take_min(k)
    else:
        p.take_type = TakeType.Max if take == 1 else TakeType.Min  # the default take: every row
    if flt is not None:
        p = p.filter(*flt)
    if mask is not None:
        p = p.with_row_mask(mask)
    if path is not None:
        p = p.with_path(path)
    return p.min_wins(min_wins).collect_arrays()


class Model:
    """the host model over one corpus: every example row's pair scores are made once and never changed"""

    def __init__(self, oracle, rows, inv, reduce_mode=0):
        self.oracle, self.rows, self.inv, self.reduce_mode = oracle, np.ascontiguousarray(rows, np.float32), inv, reduce_mode
        self.have = {}

    def row(self, e, metric):
        key = (int(e), int(metric))
        if key not in self.have:
            self.have[key] = MR.pair_row(self.oracle, self.rows, self.inv, int(e), metric, self.reduce_mode)
            self.have[key].setflags(write=False)
        return self.have[key]

    def P(self, ctx, metric):
        return np.stack([self.row(e, metric) for pair in ctx for e in pair])

    def T(self, metric, target=None, target_row=None):
        if target is not None:
            return D.target_scores(self.oracle, self.rows, self.inv, target, metric, self.reduce_mode)
        return None if target_row is None else self.row(target_row, metric)

    def __call__(self, ctx, metric, take, k, target=None, target_row=None, **kw):
        ex = {int(e) for pair in ctx for e in pair} | ({int(target_row)} if target_row is not None else set())
        return D.discover(self.P(ctx, metric), take, self.rows.shape[0] if k is None else k, T=self.T(metric, target, target_row), examples=sorted(ex), **kw)


def context(rng, n, n_pairs, pool=None):
    """n_pairs pairs of distinct rows; from a small pool the rows repeat across pairs, on both sides"""
    out = []
    while len(out) < n_pairs:
        a, b = (rng.choice(pool, 2, replace=False) if pool is not None else rng.choice(n, 2, replace=False)).tolist()
        out.append((a, b))
    return out


def targets(rng, dim, n):
    """the three forms of the target: a vector, a stored row, none"""
    return ({"target": rng.uniform(-1, 1, dim).astype(np.float32)}, {"target_row": int(rng.integers(0, n))}, {})


# ---- dims, metrics, takes, reduce orders, targets -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [3, 8, 13, 64, 200, 768])  # below 8, no remainder, a remainder, two stages, a short last stage, wide
def test_every_metric_take_reduce_order_and_target(oracle, dim):
    rng = np.random.default_rng(dim)
    ctx = context(rng, N_ROWS, 3)  # with a target 7 slots: the target rides in the second pass
    tgts = targets(rng, dim, N_ROWS)
    for reduce_mode in (oracle.REDUCE_AVX, oracle.REDUCE_SEQ4):
        store, rows, inv = make(dim, reduce_mode=reduce_mode)
        model = Model(oracle, rows, inv, reduce_mode)
        for metric in ALL_METRICS:
            for tgt in tgts:
                for take in (0, 1):
                    D.same(run(store, ctx, metric, take, 25, **tgt), model(ctx, metric, take, 25, **tgt), (dim, reduce_mode, metric, take, sorted(tgt)))
                assert store.last_stats["passes"] == 2 and store.last_stats["path_used"] == int(Path.Exact)
                assert store.last_stats["vectors_compared"] == N_ROWS * (7 if tgt else 6)
        store.close()


# ---- row counts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2000])  # no pair possible, the pair alone, around one tile, many tiles
def test_row_counts(oracle, n):
    store, rows, inv = make(13, n=n, seed=2)
    if n == 1:
        with pytest.raises(OttersError, match="row 0 is both the positive and the negative of a pair"):
            run(store, [(0, 0)], Metric.Cosine, 1, 5)
        with pytest.raises(OttersError, match="row id 1 is not below the store's length 1"):
            run(store, [(0, 1)], Metric.Cosine, 1, 5)
        store.close()
        return
    model = Model(oracle, rows, inv)
    ctx = [(0, n - 1)] if n == 2 else [(0, n - 1), (n // 2, 0)]
    q = np.random.default_rng(n).uniform(-1, 1, 13).astype(np.float32)
    for metric in (Metric.Cosine, Metric.Euclidean):
        for k in (1, 10, None):  # None: the default take, every row
            for tgt in ({"target": q}, {"target_row": n - 1}, {}):
                got = run(store, ctx, metric, TAKE[metric], k, **tgt)
                D.same(got, model(ctx, metric, TAKE[metric], k, **tgt), (n, metric, k, sorted(tgt)))
                if k is None:
                    assert got[0].size == n - len({e for p in ctx for e in p})  # random rows: every row but the examples comes out
    store.close()


# ---- pair counts and the level cut -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus(oracle):
    store, rows, inv = make(13, seed=3)
    yield store, rows, inv, Model(oracle, rows, inv)
    store.close()


TARGET13 = np.random.default_rng(77).uniform(-1, 1, 13).astype(np.float32)


@pytest.mark.parametrize("n_pairs,target,passes", [(1, False, 1), (1, True, 1), (2, True, 2), (3, True, 2), (32, True, 17), (32, False, 16)])
def test_pair_counts(corpus, n_pairs, target, passes):
    store, rows, inv, model = corpus
    rng = np.random.default_rng(n_pairs * 10 + target)
    ctx = context(rng, N_ROWS, n_pairs, pool=rng.choice(N_ROWS, 20, replace=False) if n_pairs == 32 else None)
    tgt = {"target": TARGET13} if target else {}
    for metric in (Metric.Cosine, Metric.Manhattan):
        for k in (10, 600):  # the lists and the sort path of the top-k
            D.same(run(store, ctx, metric, TAKE[metric], k, **tgt), model(ctx, metric, TAKE[metric], k, **tgt), (n_pairs, target, metric, k))
            assert store.last_stats["passes"] == passes and store.last_stats["vectors_compared"] == N_ROWS * (2 * n_pairs + target)


def test_the_most_rows_a_call_gathers(corpus):
    """32 pairs and a target ROW: 65 gathered rows, the last entry of the gather kernel's row array and the 65th lane of the clear
    kernel (both shared with recommend, whose most is 64).  The target row's state is cleared like the examples': it is no hit."""
    store, rows, inv, model = corpus
    rng = np.random.default_rng(65)
    pool = rng.choice(N_ROWS, 20, replace=False)
    ctx = context(rng, N_ROWS, 32, pool=pool)
    target_row = int(rng.choice(np.setdiff1d(np.arange(N_ROWS), pool)))  # a 65th row, not among the pairs'
    for metric in (Metric.Cosine, Metric.Manhattan):
        for k in (10, 600):  # the lists and the sort path of the top-k
            got = run(store, ctx, metric, TAKE[metric], k, target_row=target_row)
            D.same(got, model(ctx, metric, TAKE[metric], k, target_row=target_row), (metric, k))
            assert target_row not in got[0]["index"].tolist()
            assert store.last_stats["passes"] == 17 and store.last_stats["vectors_compared"] == N_ROWS * 65


def test_one_row_in_several_pairs_on_both_sides(corpus):
    store, rows, inv, model = corpus
    ctx = [(5, 9), (9, 5), (5, 70), (70, 9), (5, 9)]  # row 5 a positive three times and a negative once; a pair listed twice counts twice
    for tgt in ({"target": TARGET13}, {"target_row": 5}, {"target_row": 1234}, {}):
        exp = model(ctx, Metric.Cosine, 1, 40, **tgt)
        assert exp[1].max() <= 4  # (5, 9) and (9, 5) cannot both be won
        D.same(run(store, ctx, Metric.Cosine, 1, 40, **tgt), exp, sorted(tgt))


def level_cases():
    """the contexts of the level cut's cases"""
    rng = np.random.default_rng(2024)
    return {n_pairs: context(rng, N_ROWS, n_pairs) for n_pairs in (6, 8, 32)}


def test_level_cut(corpus):
    store, rows, inv, model = corpus
    ctxs = level_cases()
    metric, take, tgt = Metric.Cosine, 1, {"target": TARGET13}

    def both(ctx, k, **kw):
        exp = model(ctx, metric, take, k, **tgt, **kw)
        D.same(run(store, ctx, metric, take, k, **tgt, **kw), exp, (len(ctx), k, kw))
        return exp

    # 6 pairs, k = 25: the top level is short of k, the hits span two levels
    exp = both(ctxs[6], 25)
    assert len(set(exp[1].tolist())) == 2 and exp[0].size == 25
    # 8 pairs, k = 100: three levels
    exp = both(ctxs[8], 100)
    assert len(set(exp[1].tolist())) == 3 and exp[0].size == 100
    # 32 pairs, k = 25: sparse top levels, three or more, and rows above the cut level
    exp = both(ctxs[32], 25)
    assert len(set(exp[1].tolist())) >= 3 and (exp[1] > exp[1].min()).sum() > 0
    # k 512 and 513: the register lists and the radix path of the top-k, a cut level deep inside
    for k in (512, 513):
        exp = both(ctxs[8], k)
        assert exp[0].size == k and len(set(exp[1].tolist())) >= 3
    # k equal to a level's exact cumulative count: the level fills k, nothing of the next level comes out
    wins_all = model(ctxs[8], metric, take, N_ROWS, **tgt)[1]
    levels = sorted(set(wins_all.tolist()), reverse=True)
    for depth in (1, 2, 3):
        k = int((wins_all >= levels[depth - 1]).sum())
        exp = both(ctxs[8], k)
        assert exp[1].min() == levels[depth - 1] and exp[0].size == k
        exp = both(ctxs[8], k + 1)
        assert exp[1].min() == levels[depth]
    # min_wins = n_pairs: only the rows inside the fenced region, fewer than k
    exp = both(ctxs[6], 100, min_wins=6)
    assert 0 < exp[0].size < 100 and (exp[1] == 6).all()
    exp = both(ctxs[8], 100, min_wins=7)
    assert 0 < exp[0].size < 100 and exp[1].min() == 7
    # min_wins above every row's wins: nothing
    assert wins_all.max() < 32 and model(ctxs[32], metric, take, N_ROWS, **tgt)[1].max() < 32
    exp = both(ctxs[32], 25, min_wins=32)
    assert exp[0].size == 0
    # the same with a stored row as the target and under take Min
    D.same(run(store, ctxs[8], metric, 0, 100, target_row=321), model(ctxs[8], metric, 0, 100, target_row=321), "row target, take Min")
    # context search with min_wins
    D.same(run(store, ctxs[8], metric, take, 100, min_wins=5), model(ctxs[8], metric, take, 100, min_wins=5), "context search, min_wins")


# ---- ties ----------------------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_lower_row(oracle):
    rng = np.random.default_rng(7)
    base = rng.uniform(-1, 1, (100, 8)).astype(np.float32)
    rows = np.repeat(base, 4, axis=0)  # every row four times: rows 4i .. 4i + 3 are equal
    store, rows, inv = make(8, rows=rows)
    store.set_tie_order("reference")  # the order stays the canonical one
    model = Model(oracle, rows, inv)
    q = rng.uniform(-1, 1, 8).astype(np.float32)
    # (0, 1): two distinct rows with one vector — never won, +-0 to the loss; the other pairs split the corpus
    ctx = [(0, 1), (40, 80), (120, 160)]
    for metric in ALL_METRICS:
        take = TAKE[metric]
        P = model.P(ctx, metric)
        wins, loss, _, terms = D.fold(P, take)
        assert wins.max() == 2 and (terms[0] == 0).all(), "the pair of identical rows is never won"
        for tgt in ({"target": q}, {"target_row": 200}, {}):
            for k in (400, 9):
                exp = model(ctx, metric, take, k, **tgt)
                D.same(run(store, ctx, metric, take, k, **tgt), exp, (metric, sorted(tgt), k))
            exp = model(ctx, metric, take, 400, **tgt)
            idx, sc = exp[0]["index"].astype(np.int64), exp[0]["score"].view(np.uint32)
            tied = (sc[1:] == sc[:-1]) & (exp[1][1:] == exp[1][:-1])
            assert tied.any() and (np.diff(idx)[tied] > 0).all(), "equal scores and wins, the lower row first"
        # context search: many rows have loss +0 (they win both splitting pairs) and come out by row
        exp = model(ctx, metric, take, 400)
        zero = exp[0]["score"].view(np.uint32) == 0
        assert zero.sum() > 8 and zero[: zero.sum()].all() and (np.diff(exp[0]["index"][zero].astype(np.int64)) > 0).all()
    store.close()


# ---- masks, filters and store state ----------------------------------------------------------------------------------------------------

CMPS = (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq)


def test_row_mask_filter_deleted_rows_and_base_offset(oracle):
    store, rows, inv = make(24, seed=8)
    rng = np.random.default_rng(8)
    model = Model(oracle, rows, inv)
    ctx = context(rng, N_ROWS, 3)
    metric, take = Metric.Cosine, 1
    q = rng.uniform(-1, 1, 24).astype(np.float32)
    forms = ({"target": q}, {"target_row": 1500}, {})
    # a row mask: half of the rows, an example among the masked ones (an example need not survive the mask), shorter than the store
    mask = rng.uniform(size=N_ROWS - 100) < 0.5
    mask[min(ctx[0][0], mask.size - 1)] = False
    keep = np.ones(N_ROWS, bool)
    keep[: mask.size] = mask
    for tgt in forms:
        D.same(run(store, ctx, metric, take, N_ROWS, mask=mask, **tgt), model(ctx, metric, take, N_ROWS, keep=keep, **tgt), ("row mask", sorted(tgt)))
        D.same(run(store, ctx, metric, take, 10, mask=mask, **tgt), model(ctx, metric, take, 10, keep=keep, **tgt), ("row mask, k = 10", sorted(tgt)))
    # the score filter acts on the hit's score — the target score, or the loss — with every comparator
    for tgt in forms:
        full = model(ctx, metric, take, N_ROWS, **tgt)[0]["score"]
        thr = float(np.sort(full)[full.size // 2]) if tgt else float(np.sort(full[full < 0])[(full < 0).sum() // 2])
        for cmp in CMPS:
            exp = model(ctx, metric, take, N_ROWS, cmp=int(cmp), thr=thr, **tgt)
            assert 0 < exp[0].size < full.size
            D.same(run(store, ctx, metric, take, N_ROWS, flt=(thr, cmp), **tgt), exp, ("filter", cmp, sorted(tgt)))
            D.same(run(store, ctx, metric, take, 7, flt=(thr, cmp), **tgt), model(ctx, metric, take, 7, cmp=int(cmp), thr=thr, **tgt), ("filter, k = 7", cmp, sorted(tgt)))
    # the base offset shifts the hits, not the example ids or the target row
    store.set_base_offset(1 << 33)
    for tgt in forms:
        D.same(run(store, ctx, metric, take, 40, **tgt), model(ctx, metric, take, 40, base=1 << 33, **tgt), ("base offset", sorted(tgt)))
        D.same(run(store, ctx, metric, take, 600, **tgt), model(ctx, metric, take, 600, base=1 << 33, **tgt), ("base offset, k = 600", sorted(tgt)))
    store.set_base_offset(0)
    # deleted rows: never hits; a deleted row works as an example and as the target row (stored data is read)
    first = model(ctx, metric, take, 30, target=q)[0]["index"].astype(np.int64)
    dead = np.concatenate([first[::2], [ctx[1][0], ctx[2][1], 1500]])
    store.delete_rows(dead)
    live = np.ones(N_ROWS, bool)
    live[dead] = False
    for tgt in forms:
        exp = model(ctx, metric, take, N_ROWS, keep=live, **tgt)
        assert not np.isin(exp[0]["index"], dead).any()
        D.same(run(store, ctx, metric, take, N_ROWS, **tgt), exp, ("deleted rows", sorted(tgt)))
        D.same(run(store, ctx, metric, take, 30, mask=mask, **tgt), model(ctx, metric, take, 30, keep=keep & live, **tgt), ("deleted rows and a row mask", sorted(tgt)))
    store.close()


def test_device_mask_and_chunk_pruning_through_the_meta_store(oracle):
    rng = np.random.default_rng(9)
    n, dim = 2000, 24
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ms = (MetaStore.from_columns([Column("a", DataType.Int64).from_(list(range(n)))]).with_vectors(rows).with_chunk_size(256).build())
    inv = ms._store.inv_norms()
    model = Model(oracle, rows, inv)
    flt = col("a").gte(300) & col("a").lt(1500)  # prunes whole chunks (a chunk mask) and needs a row mask inside two
    ctx = [(10, 700), (1900, 800), (700, 10)]  # examples inside and outside the filter, inside and outside the pruned chunks
    keep = (np.arange(n) >= 300) & (np.arange(n) < 1500)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    for tgt in ({"target": q}, {"target_row": 50}, {}):
        for k in (20, n):
            exp = model(ctx, Metric.Cosine, 1, k, keep=keep, **tgt)
            got = ms.discover(ctx, metric=Metric.Cosine, **tgt).meta_filter(flt).take(k).collect_arrays()
            D.same(got, exp, ("meta", k, sorted(tgt)))
            assert ms._store.last_stats["pruned_chunks"] > 0
    res, wins = ms.discover(ctx, target=q).meta_filter(flt).take(20).min_wins(1).collect()
    exp = model(ctx, Metric.Cosine, 1, 20, keep=keep, target=q, min_wins=1)
    assert res.indices == exp[0]["index"].tolist() and wins == exp[1].tolist()
    assert res.column("a").values().tolist() == res.indices
    # a filter that prunes every chunk: no hits, no call
    got = ms.discover(ctx, target=q).meta_filter(col("a").gt(10 ** 6)).take(5).collect_arrays()
    assert got[0].size == 0 and got[1].size == 0
    # without a filter it is the vector store's answer
    D.same(ms.discover(ctx, target=q).take(20).collect_arrays(), model(ctx, Metric.Cosine, 1, 20, target=q), "meta, no filter")


# ---- IEEE edges ----------------------------------------------------------------------------------------------------------------------

def test_ieee_edge_rows(oracle):
    rng = np.random.default_rng(10)
    # overflowing dots (+-inf, inf - inf = NaN) and squared differences (+inf): examples among the huge rows and the ordinary ones
    rows, q, _ = E.overflow(rng)
    store, rows, inv = make(rows.shape[1], rows=rows)
    model = Model(oracle, rows, inv)
    n = rows.shape[0]
    ctx = [(0, 5), (20, n - 2), (n - 1, 0), (5, 20)]
    seen_nan = seen_inf_minus_inf = False
    for metric in ALL_METRICS:
        P = model.P(ctx, metric)
        seen_nan |= bool(np.isnan(P).any())
        both_inf = np.isinf(P[0::2]) & (P[0::2] == P[1::2]) & ~np.isnan(P).any(axis=0)
        seen_inf_minus_inf |= bool(both_inf.any())
        for take in (0, 1):
            for tgt in ({"target": np.asarray(q, np.float32).reshape(-1)[: rows.shape[1]]}, {"target_row": 7}, {}):
                D.same(run(store, ctx, metric, take, n, **tgt), model(ctx, metric, take, n, **tgt), ("overflow", metric, take, sorted(tgt)))
    assert seen_nan, "the corpus must produce NaN pair scores"
    assert seen_inf_minus_inf, "the corpus must produce inf - inf loss terms on rows that stay candidates"
    store.close()
    # cosines of +0.0 and -0.0 (a stored inverse norm of 0, subnormal elements): +0.0 ranks above -0.0 under Max, so a pair of
    # signed zeros is won or lost by the ordinals while its loss term is +-0
    rows, q, info = E.signed_zero_cosines(rng)
    store, rows, inv = make(rows.shape[1], rows=rows)
    model = Model(oracle, rows, inv)
    n = rows.shape[0]
    ctx = [(info["huge_rows"][0], info["subnormal_rows"][0]), (info["subnormal_rows"][1], 3), (3, info["huge_rows"][0]), (4, info["subnormal_rows"][0])]
    P = model.P(ctx, Metric.Cosine)
    zeros = P[P == 0].view(np.uint32)
    assert (zeros == 0).any() and (zeros == 0x80000000).any(), "the corpus must produce both signed zeros"
    signed_pair = (P[0::2] == 0) & (P[1::2] == 0) & (np.signbit(P[0::2]) != np.signbit(P[1::2]))
    assert signed_pair.any(), "the corpus must produce a pair of -0 and +0"
    for take in (0, 1):
        for tgt in ({"target_row": 5}, {}):
            for cmp, thr in ((Cmp.Gte, 0.0), (Cmp.Lt, -0.0), (Cmp.Eq, 0.0), (None, None)):
                kw = {} if cmp is None else {"cmp": int(cmp), "thr": thr}
                exp = model(ctx, Metric.Cosine, take, n, **tgt, **kw)
                D.same(run(store, ctx, Metric.Cosine, take, n, flt=None if cmp is None else (thr, cmp), **tgt), exp, ("zeros", take, cmp, sorted(tgt)))
    store.close()


# ---- the library's own exact path --------------------------------------------------------------------------------------------------------

def test_a_wins_level_is_the_plain_query_over_that_levels_rows(corpus):
    store, rows, inv, model = corpus
    ctx = context(np.random.default_rng(31), N_ROWS, 4)
    for metric in ALL_METRICS:
        take = TAKE[metric]
        hits, wins = run(store, ctx, metric, take, None, target=TARGET13)
        exp = model(ctx, metric, take, None, target=TARGET13)
        D.same((hits, wins), exp, metric)
        for level in sorted(set(exp[1].tolist())):
            mask = np.zeros(N_ROWS, bool)
            mask[exp[0]["index"][exp[1] == level].astype(np.int64)] = True  # the level's rows, from the model
            plan = store.query(TARGET13, metric).with_row_mask(mask).with_path(Path.Exact)
            plan.take_type = TakeType.Max if take == 1 else TakeType.Min  # the default take, every row, in the discover call's direction
            plain, _ = plan.collect_arrays()
            mine = hits[wins == level]
            assert mine["index"].tolist() == plain["index"].tolist() and np.array_equal(mine["score"].view(np.uint32), plain["score"].view(np.uint32)), (metric, level)


# ---- the state table's protocol ------------------------------------------------------------------------------------------------------

def test_scratch_is_shared_with_the_other_sweeps_and_survives_refusals(oracle):
    rng = np.random.default_rng(15)
    n, dim = 1000, 13
    store, rows, inv = make(dim, n=n, seed=15)
    model = Model(oracle, rows, inv)
    gid = rng.integers(0, 37, n)
    gid[:37] = np.arange(37)
    store.set_groups(gid)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    keep = np.ones(n, bool)
    ctx_a, ctx_b = context(rng, n, 5), context(rng, n, 2)
    L = N.lib()

    def refused_call():
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.k = None, 0, int(Metric.Cosine), 1, 8
        p, g = np.array([1, n], np.uint64), np.array([2, 3], np.uint64)
        out = np.zeros(8, N.HIT_DTYPE)
        assert L.ott_query_discover(store._handle(), C.byref(d), NO_ROW, N.ptr(p), N.ptr(g), 2, 0, 0, N.ptr(out), 8, None, None, None) == -1
        assert b"is not below the store's length" in L.ott_last_error() and not out["index"].any()

    for metric in (Metric.Cosine, Metric.Euclidean):
        take = TAKE[metric]
        for k in (10, 600):  # the lists and the sort path
            D.same(run(store, ctx_a, metric, take, k, target=q[0]), model(ctx_a, metric, take, k, target=q[0]), ("discover", metric, k))
            RR.same(store.recommend([3, 4], [5], metric).take(k).collect_arrays(), RR.recommend(oracle, rows, inv, [3, 4], [5], metric, take, k), ("recommend", metric, k))
            D.same(run(store, ctx_b, metric, take, k), model(ctx_b, metric, take, k), ("context", metric, k))
            refused_call()
            full = G.ranking(oracle, rows, q[:1], metric, take)
            ref, _, _ = G.expected(full, gid, keep, 10, 1, 1)
            G.bits_equal(store.query(q[:1], metric).one_per_group().take(10).collect_arrays()[0], ref, ("one_per_group", metric))
            D.same(run(store, ctx_b, metric, take, k, target_row=17), model(ctx_b, metric, take, k, target_row=17), ("row target", metric, k))
            ref = MS.expected(MS.ranking(oracle, rows, q, metric, take), gid, keep, 10, 5, take)
            G.bits_equal(store.query(q, metric).max_sim().take(10).collect_arrays()[0], ref, ("max_sim", metric))
            D.same(run(store, ctx_a, metric, take, k), model(ctx_a, metric, take, k), ("context again", metric, k))
            with pytest.raises(OttersError, match="min_wins is above the number of pairs"):
                run(store, ctx_b, metric, take, k, min_wins=3)
            RR.same(store.recommend([3], [5, 6], metric).take(k).collect_arrays(), RR.recommend(oracle, rows, inv, [3], [5, 6], metric, take, k), ("recommend again", metric, k))
    # appends that reallocate: the tables grow and are zeroed again
    more = np.random.default_rng(12).uniform(-1, 1, (1000, dim)).astype(np.float32)
    store.clear_groups()
    store.add_vectors(more)
    model2 = Model(oracle, np.concatenate([rows, more]), store.inv_norms())
    ctx_c = [(1, 1900), (1950, 2)]
    for k in (10, 2000):
        D.same(run(store, ctx_c, Metric.Cosine, 1, k, target=q[1]), model2(ctx_c, Metric.Cosine, 1, k, target=q[1]), ("after appends", k))
        D.same(run(store, ctx_c, Metric.Cosine, 1, k), model2(ctx_c, Metric.Cosine, 1, k), ("context after appends", k))
    store.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_through_the_c_abi_and_python(oracle):
    store, rows, inv = make(13, n=500, seed=11)
    model = Model(oracle, rows, inv)
    metric, take = Metric.Euclidean, 0
    L = N.lib()
    out = np.zeros(8, N.HIT_DTYPE)
    wins = np.full(8, 7, np.uint32)
    n_out = C.c_uint64(99)
    q = np.ones(26, np.float32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k = None, 0, int(metric), take, 8

    def call(pos, neg, n_pairs=None, target_row=NO_ROW, min_wins=0, flags=0, cap=8, outp=out):
        p, g = (None if pos is None else np.asarray(pos, np.uint64)), (None if neg is None else np.asarray(neg, np.uint64))
        n_pairs = (p.size if p is not None else g.size) if n_pairs is None else n_pairs
        return L.ott_query_discover(store._handle(), C.byref(d), target_row, N.ptr(p) if p is not None else None, N.ptr(g) if g is not None else None, n_pairs, min_wins,
                                    flags, N.ptr(outp) if outp is not None else None, cap, C.byref(n_out), N.ptr(wins), None)

    err = L.ott_last_error
    assert call([1], [2], n_pairs=0) == -1 and b"between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed" in err()
    assert call(list(range(33)), list(range(33, 66))) == -1 and b"between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed" in err()
    assert call(None, [2]) == -1 and b"a pair list is NULL" in err()
    assert call([1], None) == -1 and b"a pair list is NULL" in err()
    assert call([1, 500], [2, 3]) == -1 and b"row id 500 is not below the store's length 500" in err()
    assert call([1, 2], [2, 500]) == -1 and b"row id 500 is not below the store's length 500" in err()
    assert call([1], [2], target_row=500) == -1 and b"row id 500 is not below the store's length 500" in err()
    assert call([1, 4], [2, 4]) == -1 and b"row 4 is both the positive and the negative of a pair" in err()
    d.queries, d.nq = q.ctypes.data, 1
    assert call([1], [2], target_row=3) == -1 and b"a target vector and a target row are both given" in err()
    d.nq = 2
    assert call([1], [2]) == -1 and b"at most one target vector (d->nq <= 1)" in err()
    d.queries, d.nq = None, 0
    assert call([1], [2], min_wins=2) == -1 and b"min_wins is above the number of pairs" in err()
    assert call([1], [2], flags=1) == -1 and b"flags must be 0" in err()
    assert call([1], [2], cap=7) == -1 and b"output capacity is smaller than min(k, rows)" in err()
    assert call([1], [2], outp=None) == -1 and b"out is NULL" in err()
    d.mode = 1
    assert call([1], [2]) == -4 and b"PER_QUERY is not served" in err()
    d.mode, d.path = 0, 2
    assert call([1], [2]) == -4 and b"the MFMA path does not serve discovery queries" in err()
    d.path = 0
    d.use_device_row_mask = 1
    assert call([1], [2]) == -1 and b"ott_store_eval_row_mask was not called" in err()
    d.use_device_row_mask = 0
    assert n_out.value == 99 and not out["index"].any() and (wins == 7).all()
    # ... and the same call with good arguments answers, with every form of the target
    for tgt_kw, tgt in (({}, {}), ({"target_row": 9}, {"target_row": 9}), ({}, {"target": q[:13]})):
        d.queries, d.nq = (q.ctypes.data, 1) if "target" in tgt else (None, 0)
        assert call([1, 1, 3], [2, 3, 1], **tgt_kw) == 0 and n_out.value == 8
        exp = model([(1, 2), (1, 3), (3, 1)], metric, take, 8, **tgt)
        assert out["index"].tolist() == exp[0]["index"].tolist() and wins.tolist() == exp[1].tolist()
        assert np.array_equal(out["score"].view(np.uint32), exp[0]["score"].view(np.uint32))
    d.queries, d.nq = None, 0
    # wins_of_hit and n_out may be NULL
    p, g = np.array([1], np.uint64), np.array([2], np.uint64)
    out2 = np.zeros(8, N.HIT_DTYPE)
    assert L.ott_query_discover(store._handle(), C.byref(d), 5, N.ptr(p), N.ptr(g), 1, 0, 0, N.ptr(out2), 8, None, None, None) == 0
    assert out2["index"].tolist() == model([(1, 2)], metric, take, 8, target_row=5)[0]["index"].tolist()
    # Python: the same refusals, the same messages
    for plan, text in ((store.discover([(1, 500)]), "row id 500 is not below the store's length 500"),
                       (store.discover([(4, 4)]), "row 4 is both the positive and the negative of a pair"),
                       (store.discover([(1, 2)], target_row=500), "row id 500 is not below the store's length 500"),
                       (store.discover([(1, 2)], target=q[:13], target_row=3), "a target vector and a target row are both given"),
                       (store.discover([(1, 2)]).min_wins(2), "min_wins is above the number of pairs"),
                       (store.discover([]), "between 1 and OTT_DISCOVER_MAX_PAIRS (32) context pairs are needed"),
                       (store.discover([(1, 2)]).with_path(Path.Mfma), "the MFMA path does not serve discovery queries")):
        with pytest.raises(OttersError) as e:
            plan.take(5).collect()
        assert text in str(e.value)
    res = store.discover([(1, 2)], target_row=5, metric=metric).take(3).collect()
    exp = model([(1, 2)], metric, take, 3, target_row=5)
    assert [r.index for r in res] == exp[0]["index"].tolist() and [r.wins for r in res] == exp[1].tolist()
    store.close()


def test_multi_gpu_store_is_refused():
    multi = VecStore(8, devices=[0, 0])
    multi.add_vectors(np.random.default_rng(14).uniform(-1, 1, (64, 8)).astype(np.float32))
    with pytest.raises(OttersError, match="a multi-GPU store is not served"):
        multi.discover([(1, 2)]).take(3).collect()
    L = N.lib()
    d = N.QueryDesc()
    d.metric, d.take, d.k = int(Metric.Cosine), 1, 3
    out = np.zeros(3, N.HIT_DTYPE)
    p, g = np.array([1], np.uint64), np.array([2], np.uint64)
    assert L.ott_query_discover(multi._handle(), C.byref(d), NO_ROW, N.ptr(p), N.ptr(g), 1, 0, 0, N.ptr(out), 3, None, None, None) == -4
    assert b"a multi-GPU store is not served" in L.ott_last_error()
    multi.close()
