"""GPU: recommend by example rows (ott_query_recommend, VecStore.recommend, MetaStore.recommend).  Bar: every case
is bit-equal to the host model tests/recommend_ref.py — indices, order, score bits, sides, counts.  No tolerances.

The model's pair scores come from the oracle over ALL rows with the STORE's inverse norms (store.inv_norms()); they are made once
per (corpus, examples, metric) and shared by the takes, k's, flags and filters of a test.  Stores have at most 2000 rows."""
import ctypes as C

import numpy as np
import pytest

import grouped_ref as G
import ieee_edges as E
import maxsim_ref as MS
import recommend_ref as R
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)
N_ROWS = 2000


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


def run(store, pos, neg, metric, take, k, fill=True, flt=None, mask=None, path=None):
    p = store.recommend(pos, neg, metric)
    if k is not None:
        p = p.take_max(k) if take == 1 else p.take_min(k)
    if flt is not None:
        p = p.filter(*flt)
    if mask is not None:
        p = p.with_row_mask(mask)
    if path is not None:
        p = p.with_path(path)
    return p.fill_negative_side(fill).collect_arrays()


def examples(rng, n, n_pos, n_neg):
    ids = rng.choice(n, n_pos + n_neg, replace=False)
    return ids[:n_pos].tolist(), ids[n_pos:].tolist()


# ---- dims, metrics, takes, reduce orders ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [3, 8, 13, 64, 200, 768])  # below 8, no remainder, a remainder, two stages, a short last stage, wide
def test_every_metric_take_and_reduce_order(oracle, dim):
    rng = np.random.default_rng(dim)
    pos, neg = examples(rng, N_ROWS, 3, 2)  # the positive / negative boundary falls inside the first pass
    for reduce_mode in (oracle.REDUCE_AVX, oracle.REDUCE_SEQ4):
        store, rows, inv = make(dim, reduce_mode=reduce_mode)
        for metric in ALL_METRICS:
            P = R.pair_scores(oracle, rows, inv, pos + neg, metric, reduce_mode)
            for take in (0, 1):
                exp = R.recommend(oracle, rows, inv, pos, neg, metric, take, 25, P=P)
                R.same(run(store, pos, neg, metric, take, 25), exp, (dim, reduce_mode, metric, take))
            assert store.last_stats["passes"] == 2 and store.last_stats["path_used"] == int(Path.Exact)
            assert store.last_stats["vectors_compared"] == N_ROWS * 5
        store.close()


# ---- row counts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])  # one row (the example itself: no candidate), around one tile, many tiles
def test_row_counts(oracle, n):
    store, rows, inv = make(13, n=n, seed=2)
    pos, neg = ([0], []) if n == 1 else ([0, n // 2], [n - 1])
    for metric in (Metric.Cosine, Metric.Euclidean):
        for k in (1, 10, None):  # None: the default take, every row
            exp = R.recommend(oracle, rows, inv, pos, neg, metric, TAKE[metric], n if k is None else k)
            got = run(store, pos, neg, metric, TAKE[metric], k)
            R.same(got, exp, (n, metric, k))
            if k is None:
                assert got[0].size == n - len(pos) - len(neg)  # random rows: every row but the examples has a score and comes out
    store.close()


# ---- example counts ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus(oracle):
    store, rows, inv = make(13, seed=3)
    cache = {}

    def pairs(pos, neg, metric):
        key = (tuple(pos), tuple(neg), int(metric))
        if key not in cache:
            cache[key] = R.pair_scores(oracle, rows, inv, list(dict.fromkeys(pos)) + list(dict.fromkeys(neg)), metric)
            cache[key].setflags(write=False)
        return cache[key]

    def model(pos, neg, metric, take, k, **kw):
        return R.recommend(oracle, rows, inv, pos, neg, metric, take, k, P=pairs(pos, neg, metric), **kw)

    yield store, rows, inv, model
    store.close()


@pytest.mark.parametrize("n_pos,n_neg,passes", [(1, 0, 1), (2, 0, 1), (3, 2, 2), (4, 4, 2), (5, 4, 3), (40, 24, 16)])  # the NQ = 1 kernel ... the limit
def test_example_counts(corpus, n_pos, n_neg, passes):
    store, rows, inv, model = corpus
    pos, neg = examples(np.random.default_rng(n_pos * 100 + n_neg), N_ROWS, n_pos, n_neg)
    for metric in (Metric.Cosine, Metric.Manhattan):
        for k in (10, 600):  # the lists and the sort path of the top-k
            R.same(run(store, pos, neg, metric, TAKE[metric], k), model(pos, neg, metric, TAKE[metric], k), (n_pos, n_neg, metric, k))
            assert store.last_stats["passes"] == passes
    # duplicates inside a list count once, in any position
    dup_pos, dup_neg = pos + pos[::-1] + pos[:1], neg * 3
    R.same(run(store, dup_pos, dup_neg, Metric.Cosine, 1, 10), model(pos, neg, Metric.Cosine, 1, 10), "duplicates")
    assert store.last_stats["passes"] == passes


def test_one_positive_is_the_plain_query_with_the_row_masked(corpus):
    store, rows, inv, _ = corpus
    for metric in (Metric.DotProduct, Metric.Euclidean, Metric.Manhattan):  # (cosine: the host's query norm is another quantity than the stored one)
        mask = np.ones(N_ROWS, bool)
        mask[77] = False
        p = store.query(rows[77], metric).with_row_mask(mask)
        plain, _ = (p.take_max(15) if TAKE[metric] == 1 else p.take_min(15)).collect_arrays()
        hits, sides = run(store, [77], [], metric, TAKE[metric], 15)
        assert hits.tobytes() == plain.tobytes() and sides.tolist() == [1] * 15


# ---- sides ---------------------------------------------------------------------------------------------------------------------------

def test_second_round_runs_when_the_positive_side_is_short(corpus):
    store, rows, inv, model = corpus
    pos, neg = examples(np.random.default_rng(5), N_ROWS, 2, 3)
    for metric in (Metric.Cosine, Metric.Euclidean):
        take = TAKE[metric]
        for k in (N_ROWS, 1500):  # every candidate; a cut inside the negative side
            exp = model(pos, neg, metric, take, k)
            n1 = int(exp[1].sum())
            assert 0 < n1 < min(k, N_ROWS) and (exp[1] == 0).any(), "the model's negative side must be non-empty and the positive side short of k"
            R.same(run(store, pos, neg, metric, take, k), exp, (metric, k))
        # a k the positive side fills: no second round, the same prefix
        exp = model(pos, neg, metric, take, 50)
        assert exp[1].tolist() == [1] * 50
        R.same(run(store, pos, neg, metric, take, 50), exp, (metric, 50))
        # without the flag the negative side never comes out
        exp = model(pos, neg, metric, take, N_ROWS, flags=0)
        assert exp[1].all() and 0 < exp[0].size < N_ROWS - 5
        R.same(run(store, pos, neg, metric, take, N_ROWS, fill=False), exp, (metric, "no fill"))
    # a second round of few rows: the lists path of the second top-k
    exp = model(pos, neg, Metric.Cosine, 1, N_ROWS)
    n1 = int(exp[1].sum())
    exp = model(pos, neg, Metric.Cosine, 1, n1 + 7)
    assert exp[1].tolist() == [1] * n1 + [0] * 7
    R.same(run(store, pos, neg, Metric.Cosine, 1, n1 + 7), exp, "seven of the negative side")


def test_every_row_on_the_negative_side(oracle):
    rng = np.random.default_rng(6)
    n, dim = 300, 13
    rows = (rng.uniform(-1, 1, (n, dim)) * 0.01).astype(np.float32)
    rows[0] += np.float32(50.0)  # the positive example lies far away from everything; row 1, the negative, in the cloud
    store, rows, inv = make(dim, rows=rows)
    exp = R.recommend(oracle, rows, inv, [0], [1], Metric.Euclidean, 0, 20)
    assert exp[1].tolist() == [0] * 20, "the model must put every row on the negative side"
    R.same(run(store, [0], [1], Metric.Euclidean, 0, 20), exp, "all negative")
    exp = R.recommend(oracle, rows, inv, [0], [1], Metric.Euclidean, 0, 20, flags=0)
    assert exp[0].size == 0
    R.same(run(store, [0], [1], Metric.Euclidean, 0, 20, fill=False), exp, "all negative, no fill")
    store.close()


def test_equal_best_scores_go_to_the_negative_side_and_ties_to_the_lower_row(oracle):
    rng = np.random.default_rng(7)
    base = rng.uniform(-1, 1, (100, 8)).astype(np.float32)
    base[0] = np.float32(2.0)  # longer than any other row: under every metric a copy of row 0 has row 0 as its best positive
    rows = np.repeat(base, 4, axis=0)  # every row four times: rows 4i .. 4i + 3 are equal
    store, rows, inv = make(8, rows=rows)
    store.set_tie_order("reference")  # the order stays the canonical one
    # rows 0 and 1 are the same vector, one a positive and one a negative: rows 2 and 3 duplicate both, and every row whose best
    # positive is row 0 has bp == bn.  Row 40 is a second positive
    pos, neg = [0, 40], [1]
    for metric in ALL_METRICS:
        take = TAKE[metric]
        P = R.pair_scores(oracle, rows, inv, pos + neg, metric)
        bp, bn, cand, positive = R.sides(P[:2], P[2:], take, pos + neg)
        assert cand[2] and bp[2] == bn[2] and not positive[2], "a row that duplicates a positive and a negative must tie"
        exp = R.recommend(oracle, rows, inv, pos, neg, metric, take, 400, P=P)
        n1 = int(exp[1].sum())
        assert 0 < n1 < exp[0].size
        idx = exp[0]["index"].astype(np.int64)
        sc = exp[0]["score"].view(np.uint32)
        tied = (sc[1:] == sc[:-1]) & (exp[1][1:] == exp[1][:-1])
        assert tied[:n1 - 1].any() and tied[n1:].any() and (np.diff(idx)[tied] > 0).all(), "equal scores on both sides, the lower row first"
        R.same(run(store, pos, neg, metric, take, 400), exp, metric)
        R.same(run(store, pos, neg, metric, take, 9), R.recommend(oracle, rows, inv, pos, neg, metric, take, 9, P=P), (metric, 9))
    store.close()


# ---- masks and store state -----------------------------------------------------------------------------------------------------------

CMPS = (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq)


def test_row_mask_filter_deleted_rows_and_base_offset(oracle):
    store, rows, inv = make(24, seed=8)
    rng = np.random.default_rng(8)
    pos, neg = examples(rng, N_ROWS, 3, 3)
    metric, take = Metric.Cosine, 1
    P = R.pair_scores(oracle, rows, inv, pos + neg, metric)
    model = lambda k, **kw: R.recommend(oracle, rows, inv, pos, neg, metric, take, k, P=P, **kw)  # noqa: E731
    # a row mask: half of the rows, an example among the masked ones (an example need not survive the mask), shorter than the store
    mask = rng.uniform(size=N_ROWS - 100) < 0.5
    mask[min(pos[0], mask.size - 1)] = False
    keep = np.ones(N_ROWS, bool)
    keep[: mask.size] = mask
    R.same(run(store, pos, neg, metric, take, N_ROWS, mask=mask), model(N_ROWS, keep=keep), "row mask")
    R.same(run(store, pos, neg, metric, take, 10, mask=mask), model(10, keep=keep), "row mask, k = 10")
    # the score filter acts on BP, with every comparator, on both sides
    bp = R.decode(R.best(P[:3], take), take)
    thr = float(np.sort(bp)[N_ROWS // 2])
    for cmp in CMPS:
        exp = model(N_ROWS, cmp=int(cmp), thr=thr)
        assert 0 < exp[0].size < N_ROWS - 6
        R.same(run(store, pos, neg, metric, take, N_ROWS, flt=(thr, cmp)), exp, ("filter", cmp))
    # the base offset shifts the hits, not the example ids
    store.set_base_offset(1 << 33)
    R.same(run(store, pos, neg, metric, take, 40), model(40, base=1 << 33), "base offset")
    store.set_base_offset(0)
    # deleted rows: never candidates; a deleted row may be an example (stored data is read)
    first = model(30)[0]["index"].astype(np.int64)
    dead = np.concatenate([first[::2], [pos[1], neg[0]]])
    store.delete_rows(dead)
    live = np.ones(N_ROWS, bool)
    live[dead] = False
    exp = model(N_ROWS, keep=live)
    assert not np.isin(exp[0]["index"], dead).any()
    R.same(run(store, pos, neg, metric, take, N_ROWS), exp, "deleted rows")
    R.same(run(store, pos, neg, metric, take, 30, mask=mask), model(30, keep=keep & live), "deleted rows and a row mask")
    store.close()


def test_device_mask_and_chunk_pruning_through_the_meta_store(oracle):
    rng = np.random.default_rng(9)
    n, dim = 2000, 24
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ms = (MetaStore.from_columns([Column("a", DataType.Int64).from_(list(range(n)))]).with_vectors(rows).with_chunk_size(256).build())
    inv = ms._store.inv_norms()
    flt = col("a").gte(300) & col("a").lt(1500)  # prunes whole chunks (a chunk mask) and needs a row mask inside two
    pos, neg = [10, 700], [1900, 800]  # examples inside and outside the filter, inside and outside the pruned chunks
    keep = (np.arange(n) >= 300) & (np.arange(n) < 1500)
    for k in (20, n):
        exp = R.recommend(oracle, rows, inv, pos, neg, Metric.Cosine, 1, k, keep=keep)
        got = ms.recommend(pos, neg, Metric.Cosine).meta_filter(flt).take(k).collect_arrays()
        R.same(got, exp, ("meta", k))
        assert ms._store.last_stats["pruned_chunks"] > 0
    res, sides = ms.recommend(pos, neg, Metric.Cosine).meta_filter(flt).take(20).collect()
    exp = R.recommend(oracle, rows, inv, pos, neg, Metric.Cosine, 1, 20, keep=keep)
    assert res.indices == exp[0]["index"].tolist() and sides == exp[1].tolist()
    assert res.column("a").values().tolist() == res.indices
    # a filter that prunes every chunk: no hits, no call
    got = ms.recommend(pos, neg, Metric.Cosine).meta_filter(col("a").gt(10 ** 6)).take(5).collect_arrays()
    assert got[0].size == 0 and got[1].size == 0
    # without a filter it is the vector store's answer
    R.same(ms.recommend(pos, neg, Metric.Cosine).take(20).collect_arrays(), R.recommend(oracle, rows, inv, pos, neg, Metric.Cosine, 1, 20), "meta, no filter")


# ---- IEEE edges ----------------------------------------------------------------------------------------------------------------------

def test_ieee_edge_rows(oracle):
    rng = np.random.default_rng(10)
    # overflowing dots (+-inf, inf - inf = NaN) and squared differences (+inf): examples among the huge rows and the ordinary ones
    rows, _, _ = E.overflow(rng)
    store, rows, inv = make(rows.shape[1], rows=rows)
    n = rows.shape[0]
    pos, neg = [0, 20, n - 1], [5, n - 2]
    seen_nan = False
    for metric in ALL_METRICS:
        P = R.pair_scores(oracle, rows, inv, pos + neg, metric)
        seen_nan |= bool(np.isnan(P).any())
        for take in (0, 1):
            for fill in (True, False):
                exp = R.recommend(oracle, rows, inv, pos, neg, metric, take, n, flags=int(fill), P=P)
                R.same(run(store, pos, neg, metric, take, n, fill=fill), exp, ("overflow", metric, take, fill))
    assert seen_nan, "the corpus must produce NaN pair scores"
    store.close()
    # cosines of +0.0 and -0.0 (a stored inverse norm of 0, subnormal elements): +0.0 ranks above -0.0 under Max
    rows, _, info = E.signed_zero_cosines(rng)
    store, rows, inv = make(rows.shape[1], rows=rows)
    n = rows.shape[0]
    pos, neg = [info["huge_rows"][0], info["subnormal_rows"][0], 3], [info["subnormal_rows"][1], 4]
    P = R.pair_scores(oracle, rows, inv, pos + neg, Metric.Cosine)
    zeros = P[P == 0].view(np.uint32)
    assert (zeros == 0).any() and (zeros == 0x80000000).any(), "the corpus must produce both signed zeros"
    for take in (0, 1):
        for cmp, thr in ((Cmp.Gte, 0.0), (Cmp.Lt, -0.0), (Cmp.Eq, 0.0), (None, None)):
            kw = {} if cmp is None else {"cmp": int(cmp), "thr": thr}
            exp = R.recommend(oracle, rows, inv, pos, neg, Metric.Cosine, take, n, P=P, **kw)
            R.same(run(store, pos, neg, Metric.Cosine, take, n, flt=None if cmp is None else (thr, cmp)), exp, ("zeros", take, cmp))
    store.close()


# ---- the state table's protocol ------------------------------------------------------------------------------------------------------

def test_queries_back_to_back_a_refusal_between_and_after_a_reallocation(oracle):
    store, rows, inv = make(13, n=500, seed=11)
    metric, take = Metric.Euclidean, 0
    a = ([1, 2, 3, 4, 5], [6, 7])      # two passes, fill possible: the second round or the memset clears the states
    b = ([400], [])                    # one pass: the first keys kernel clears them
    c = ([10, 11], [12, 13, 14, 15])
    model = lambda ex, k, r=rows, i=inv, **kw: R.recommend(oracle, r, i, ex[0], ex[1], metric, take, k, **kw)  # noqa: E731
    for k in (10, 500):  # 10: no second round (the memset); 500: the second round
        R.same(run(store, *a, metric, take, k), model(a, k), ("a", k))
        R.same(run(store, *b, metric, take, k), model(b, k), ("b after a", k))
        R.same(run(store, *c, metric, take, k, fill=False), model(c, k, flags=0), ("c without fill after b", k))
        R.same(run(store, *a, metric, take, k), model(a, k), ("a again", k))
    # refused queries between two good ones: nothing is written, the next answer is right
    L = N.lib()
    out = np.zeros(8, N.HIT_DTYPE)
    sides = np.full(8, 7, np.uint32)
    n_out = C.c_uint64(99)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k = None, 0, int(metric), take, 8

    def call(pos, neg, flags=1, cap=8, outp=out):
        p, g = np.asarray(pos, np.uint64), np.asarray(neg, np.uint64)
        return L.ott_query_recommend(store._handle(), C.byref(d), N.ptr(p), p.size, N.ptr(g) if g.size else None, g.size, flags, N.ptr(outp) if outp is not None else None, cap,
                                     C.byref(n_out), N.ptr(sides), None)

    assert call([1, 500], []) == -1 and b"example id 500 is not below the store's length 500" in L.ott_last_error()
    assert call([1], [2, 1]) == -1 and b"row 1 is listed as both a positive and a negative example" in L.ott_last_error()
    assert call(list(range(65)), []) == -1 and b"more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples" in L.ott_last_error()
    assert call([1], [], cap=7) == -1 and b"output capacity is smaller than min(k, rows)" in L.ott_last_error()
    assert call([1], [], outp=None) == -1 and b"out is NULL" in L.ott_last_error()
    assert call([1], [], flags=3) == -1 and b"unknown flag bits" in L.ott_last_error()
    d.use_device_row_mask = 1
    assert call([1], []) == -1 and b"ott_store_eval_row_mask was not called" in L.ott_last_error()
    d.use_device_row_mask = 0
    assert n_out.value == 99 and not out["index"].any() and (sides == 7).all()
    assert call([1, 1, 2], [3]) == 0 and n_out.value == 8  # ... and the same call with good arguments answers
    exp = model(([1, 2], [3]), 8)
    assert out["index"].tolist() == exp[0]["index"].tolist() and sides.tolist() == exp[1].tolist()
    with pytest.raises(OttersError, match="is not below the store's length 500"):
        run(store, [500], [], metric, take, 5)
    R.same(run(store, *a, metric, take, 500), model(a, 500), "a after the refusals")
    # appends that reallocate: the tables grow and are zeroed again
    more = np.random.default_rng(12).uniform(-1, 1, (1500, 13)).astype(np.float32)
    store.add_vectors(more)
    rows2, inv2 = np.concatenate([rows, more]), store.inv_norms()
    a2 = ([1, 2, 1900], [6, 1950])
    for k in (10, 2000):
        R.same(run(store, *a2, metric, take, k), model(a2, k, rows2, inv2), ("after appends", k))
    store.close()


def test_pair_scores_are_score_rows_with_the_examples_rows_as_queries(oracle):
    store, rows, inv = make(200, n=300, seed=13)
    ex = [5, 250, 17]
    for metric in (Metric.DotProduct, Metric.Euclidean, Metric.Manhattan):
        got = store.score_rows(store.rows()[ex], metric, np.arange(300))
        assert np.array_equal(got.view(np.uint32), R.pair_scores(oracle, rows, inv, ex, metric).view(np.uint32)), metric
    store.close()


def test_multi_gpu_store_is_refused():
    multi = VecStore(8, devices=[0, 0])
    multi.add_vectors(np.random.default_rng(14).uniform(-1, 1, (64, 8)).astype(np.float32))
    with pytest.raises(OttersError, match="a multi-GPU store is not served"):
        multi.recommend([1], [2]).take(3).collect()
    L = N.lib()
    d = N.QueryDesc()
    d.metric, d.take, d.k = int(Metric.Cosine), 1, 3
    out = np.zeros(3, N.HIT_DTYPE)
    p = np.array([1], np.uint64)
    assert L.ott_query_recommend(multi._handle(), C.byref(d), N.ptr(p), 1, None, 0, 1, N.ptr(out), 3, None, None, None) == -4
    assert b"a multi-GPU store is not served" in L.ott_last_error()
    multi.close()


# ---- the shared sweep: grouped and late-interaction search still equal their models ----------------------------------------------------

def test_grouped_and_maxsim_queries_on_a_grouped_store(oracle):
    rng = np.random.default_rng(15)
    n, dim = 1000, 13
    store, rows, inv = make(dim, n=n, seed=15)
    gid = rng.integers(0, 37, n)
    gid[:37] = np.arange(37)
    store.set_groups(gid)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    keep = np.ones(n, bool)
    for metric in (Metric.Cosine, Metric.Euclidean):
        take = TAKE[metric]
        full = G.ranking(oracle, rows, q[:1], metric, take)
        ref, _, _ = G.expected(full, gid, keep, 10, 1, 1)
        G.bits_equal(store.query(q[:1], metric).one_per_group().take(10).collect_arrays()[0], ref, ("one_per_group", metric))
        ref = MS.expected(MS.ranking(oracle, rows, q, metric, take), gid, keep, 10, 5, take)
        G.bits_equal(store.query(q, metric).max_sim().take(10).collect_arrays()[0], ref, ("max_sim", metric))
        # ... and recommend on the same store reads no group id
        R.same(run(store, [3, 4], [5], metric, take, 10), R.recommend(oracle, rows, inv, [3, 4], [5], metric, take, 10), ("recommend on a grouped store", metric))
    store.close()
