"""GPU: the recommend strategies average_vector and sum_scores (ott_query_recommend_strategy, VecStore.recommend and
MetaStore.recommend with strategy=...).  Bar: every case is bit-equal to the host model
tests/recommend_strategy_ref.py — indices, order, score bits, query == 0, sides all 1, counts.  No tolerances.

sum_scores: the model's pair scores come from the oracle over ALL rows with the STORE's inverse norms; they are made once per
(corpus, examples, metric) and shared by the takes, k's and filters of a test.  average_vector: the model's vector goes through the
oracle's ranking under the combined mask, and through the same store's own query() with that mask.  Stores have at most 3001 rows:
47 tiles, so that several workgroups of four waves run and the last tile is short."""
import ctypes as C
import threading

import numpy as np
import pytest

import mmr_ref as MR
import recommend_ref as R
import recommend_strategy_ref as RS
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, RecommendStrategy, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)
BEST, AVG, SUM = RecommendStrategy.BestScore, RecommendStrategy.AverageVector, RecommendStrategy.SumScores
CMPS = (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq)
N_ROWS = 3001


@pytest.fixture(scope="module", autouse=True)
def collect_the_models_garbage():
    """As tests/test_gpu_recommend.py: the model's many short-lived objects are collected when the module is done."""
    yield
    import gc
    gc.collect()


def make(dim, n=N_ROWS, seed=0, rows=None, options=()):
    rng = np.random.default_rng(1000 * dim + seed)
    if rows is None:
        rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    store = VecStore(dim)
    for name, value in options:
        store.set_option(name, value)
    store.add_vectors(rows)
    return store, rows, store.inv_norms()


def run(store, pos, neg, metric, take, k, strategy, flt=None, mask=None, path=None):
    p = store.recommend(pos, neg, metric, strategy)
    if k is not None:
        p = p.take_max(k) if take == 1 else p.take_min(k)
    if flt is not None:
        p = p.filter(*flt)
    if mask is not None:
        p = p.with_row_mask(mask)
    if path is not None:
        p = p.with_path(path)
    return p.collect_arrays()


def examples(rng, n, n_pos, n_neg):
    ids = rng.choice(n, n_pos + n_neg, replace=False)
    return ids[:n_pos].tolist(), ids[n_pos:].tolist()


def plain_model(oracle, rows, inv, q, metric, take, k, keep, cmp=0, thr=0.0):
    """(hits, sides): the oracle's canonical ranking of one query under a mask"""
    h = MR.candidates(oracle, rows, q, metric, take, min(int(k), rows.shape[0]), int(cmp), thr, row_mask=keep, inv=inv)
    return h, np.ones(h.size, np.uint32)


def average_model(oracle, rows, inv, pos, neg, metric, take, k, keep=None, cmp=0, thr=0.0):
    return plain_model(oracle, rows, inv, RS.average_vector(rows, pos, neg), metric, take, k, RS.keep_without(rows.shape[0], pos, neg, keep), cmp, thr)


def plain_query(store, q, metric, take, k, keep, flt=None, path=None):
    p = store.query(q, metric).with_row_mask(keep)
    p = p.take_max(k) if take == 1 else p.take_min(k)
    if flt is not None:
        p = p.filter(*flt)
    if path is not None:
        p = p.with_path(path)
    return p.collect_arrays()[0]


# ---- sum_scores: rows, dims, metrics, takes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, N_ROWS])  # one row (the example itself: no candidate), around one tile, 47 tiles
def test_sum_scores_row_counts_dims_metrics_and_takes(oracle, n):
    # dims: below the staging guard (dim < 29: 5, 24), at it (29), a remainder of dim % 8 (5, 29, 100), a partial 32-float stage (40, 100)
    for dim in (5, 24, 29, 40, 100):
        store, rows, inv = make(dim, n=n, seed=n)
        pos, neg = ([0], []) if n == 1 else ([0, n // 2, n // 3], [n - 1, 1, n // 5])  # the sign changes inside pass 0
        for metric in ALL_METRICS:
            P = R.pair_scores(oracle, rows, inv, pos + neg, metric)
            for take in (0, 1):
                for k in ((10, None) if take == TAKE[metric] else (10,)):
                    exp = RS.sum_scores(oracle, rows, inv, pos, neg, metric, take, n if k is None else k, P=P)
                    got = run(store, pos, neg, metric, take, k, SUM)
                    R.same(got, exp, (n, dim, metric, take, k))
                    if k is None:
                        assert got[0].size == n - len(pos) - len(neg)  # random rows: every row but the examples comes out
            assert store.last_stats["passes"] == (1 if n == 1 else 2) and store.last_stats["path_used"] == int(Path.Exact)
            assert store.last_stats["vectors_compared"] == n * len(pos + neg)
        store.close()


def test_sum_scores_rows_of_1030_floats(oracle):
    store, rows, inv = make(1030, n=300, seed=1)  # 33 stages, the last of 6 floats
    pos, neg = examples(np.random.default_rng(1030), 300, 3, 2)
    for metric in ALL_METRICS:
        exp = RS.sum_scores(oracle, rows, inv, pos, neg, metric, TAKE[metric], 300)
        R.same(run(store, pos, neg, metric, TAKE[metric], 300, SUM), exp, metric)
    store.close()


# ---- sum_scores: example counts, masks, filters, k ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus(oracle):
    store, rows, inv = make(24, seed=3)
    cache = {}

    def pairs(pos, neg, metric):
        key = (tuple(pos), tuple(neg), int(metric))
        if key not in cache:
            p, g = RS.slots(pos, neg)
            cache[key] = R.pair_scores(oracle, rows, inv, p + g, metric)
            cache[key].setflags(write=False)
        return cache[key]

    def model(pos, neg, metric, take, k, **kw):
        return RS.sum_scores(oracle, rows, inv, pos, neg, metric, take, k, P=pairs(pos, neg, metric), **kw)

    yield store, rows, inv, model, pairs
    store.close()


# the single-query kernel; one pass of positives; the sign changes inside pass 0; a last pass with one slot; three passes; the limit
@pytest.mark.parametrize("n_pos,n_neg,passes", [(1, 0, 1), (4, 0, 1), (3, 3, 2), (4, 1, 2), (5, 4, 3), (32, 32, 16)])
def test_sum_scores_example_counts(corpus, n_pos, n_neg, passes):
    store, rows, inv, model, _ = corpus
    pos, neg = examples(np.random.default_rng(n_pos * 100 + n_neg), N_ROWS, n_pos, n_neg)
    for metric in (Metric.Cosine, Metric.Manhattan):
        for k in (10, 600):  # the lists and the sort path of the top-k
            R.same(run(store, pos, neg, metric, TAKE[metric], k, SUM), model(pos, neg, metric, TAKE[metric], k), (n_pos, n_neg, metric, k))
            assert store.last_stats["passes"] == passes and store.last_stats["vectors_compared"] == N_ROWS * (n_pos + n_neg)
            assert store.last_stats["bytes_scanned"] == passes * N_ROWS * (24 * 4 + (4 if metric == Metric.Cosine else 0))
    # duplicates inside a list count once, in any position
    R.same(run(store, pos + pos[::-1] + pos[:1], neg * 3, Metric.Cosine, 1, 10, SUM), model(pos, neg, Metric.Cosine, 1, 10), "duplicates")
    assert store.last_stats["passes"] == passes


def test_sum_scores_one_positive_is_the_plain_query_with_the_row_masked(corpus):
    store, rows, inv, _, _ = corpus
    for metric in (Metric.DotProduct, Metric.Euclidean, Metric.Manhattan):  # (cosine: the host's query norm is another quantity than the stored one)
        keep = RS.keep_without(N_ROWS, [77], [])
        for strategy in (SUM, AVG):
            hits, sides = run(store, [77], [], metric, TAKE[metric], 15, strategy)
            assert hits.tobytes() == plain_query(store, rows[77], metric, TAKE[metric], 15, keep).tobytes() and sides.tolist() == [1] * 15, (metric, strategy)


def test_sum_scores_row_mask_filter_k_deleted_rows_and_base_offset(oracle):
    store, rows, inv = make(24, seed=8)
    rng = np.random.default_rng(8)
    pos, neg = examples(rng, N_ROWS, 3, 3)
    metric, take = Metric.Cosine, 1
    P = R.pair_scores(oracle, rows, inv, pos + neg, metric)
    model = lambda k, **kw: RS.sum_scores(oracle, rows, inv, pos, neg, metric, take, k, P=P, **kw)  # noqa: E731
    # a row mask: half of the rows, an example among the masked ones, shorter than the store
    mask = rng.uniform(size=N_ROWS - 100) < 0.5
    mask[min(pos[0], mask.size - 1)] = False
    keep = np.ones(N_ROWS, bool)
    keep[: mask.size] = mask
    for k in (1, 10, 600, None):
        R.same(run(store, pos, neg, metric, take, k, SUM), model(N_ROWS if k is None else k), ("k", k))
        R.same(run(store, pos, neg, metric, take, k, SUM, mask=mask), model(N_ROWS if k is None else k, keep=keep), ("row mask", k))
    # the score filter acts on S, with every comparator
    thr = float(model(N_ROWS)[0]["score"][N_ROWS // 2])  # a candidate's S: Eq keeps it
    for cmp in CMPS:
        exp = model(N_ROWS, cmp=int(cmp), thr=thr)
        assert 0 < exp[0].size < N_ROWS - 6
        R.same(run(store, pos, neg, metric, take, N_ROWS, SUM, flt=(thr, cmp)), exp, ("filter", cmp))
    # the base offset shifts the hits, not the example ids
    store.set_base_offset(1 << 33)
    R.same(run(store, pos, neg, metric, take, 40, SUM), model(40, base=1 << 33), "base offset")
    store.set_base_offset(0)
    # deleted rows: never candidates; a deleted row may be an example (stored data is read)
    first = model(30)[0]["index"].astype(np.int64)
    dead = np.concatenate([first[::2], [pos[1], neg[0]]])
    store.delete_rows(dead)
    live = np.ones(N_ROWS, bool)
    live[dead] = False
    exp = model(N_ROWS, keep=live)
    assert not np.isin(exp[0]["index"], dead).any()
    R.same(run(store, pos, neg, metric, take, N_ROWS, SUM), exp, "deleted rows")
    R.same(run(store, pos, neg, metric, take, 30, SUM, mask=mask), model(30, keep=keep & live), "deleted rows and a row mask")
    # ... and average_vector under the same masks
    R.same(run(store, pos, neg, metric, take, 30, AVG, mask=mask), average_model(oracle, rows, inv, pos, neg, metric, take, 30, keep=keep & live), "average, deleted rows and a row mask")
    store.close()


def test_device_mask_and_chunk_pruning_through_the_meta_store(oracle):
    rng = np.random.default_rng(9)
    n, dim = 2000, 24
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ms = (MetaStore.from_columns([Column("a", DataType.Int64).from_(list(range(n)))]).with_vectors(rows).with_chunk_size(256).build())
    inv = ms._store.inv_norms()
    flt = col("a").gte(300) & col("a").lt(1500)  # prunes whole chunks (a chunk mask: runs drop out) and needs a row mask inside two
    pos, neg = [10, 700], [1900, 800]  # examples inside and outside the filter, inside and outside the pruned chunks
    keep = (np.arange(n) >= 300) & (np.arange(n) < 1500)
    for k in (20, n):
        exp = RS.sum_scores(oracle, rows, inv, pos, neg, Metric.Cosine, 1, k, keep=keep)
        R.same(ms.recommend(pos, neg, Metric.Cosine, SUM).meta_filter(flt).take(k).collect_arrays(), exp, ("meta sum", k))
        assert ms._store.last_stats["pruned_chunks"] > 0
        exp = average_model(oracle, rows, inv, pos, neg, Metric.Cosine, 1, k, keep=keep)
        R.same(ms.recommend(pos, neg, Metric.Cosine, AVG).meta_filter(flt).take(k).collect_arrays(), exp, ("meta average", k))
        assert ms._store.last_stats["pruned_chunks"] > 0
    res, sides = ms.recommend(pos, neg, Metric.Cosine, strategy=SUM).meta_filter(flt).take(20).collect()
    exp = RS.sum_scores(oracle, rows, inv, pos, neg, Metric.Cosine, 1, 20, keep=keep)
    assert res.indices == exp[0]["index"].tolist() and sides == [1] * 20
    for strategy in (SUM, AVG):  # a filter that prunes every chunk: no hits
        got = ms.recommend(pos, neg, Metric.Cosine, strategy).meta_filter(col("a").gt(10 ** 6)).take(5).collect_arrays()
        assert got[0].size == 0 and got[1].size == 0


# ---- sum_scores: ties, cancellations, IEEE edges --------------------------------------------------------------------------------------------

def test_sum_scores_quantised_corpus_ties_and_exact_cancellations(oracle):
    rng = np.random.default_rng(10)
    n, dim = 1000, 13
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    rows[5] = rows[4]  # a positive and a negative with the same vector: their scores cancel exactly for every row
    store, rows, inv = make(dim, rows=rows)
    for pos, neg in (([4, 17], [5, 23]), ([4], [5]), ([100, 200, 300, 400, 500], [])):
        for metric in ALL_METRICS:
            P = R.pair_scores(oracle, rows, inv, pos + neg, metric)
            S = RS.sum_chain(P, len(pos))
            if len(pos) == 1 and neg:
                assert (S == 0).all(), "a positive and a negative with the same vector cancel exactly, for every row"
            elif neg and metric == Metric.DotProduct:  # (integer scores: every step of the chain is exact)
                assert (S == 0).sum() > 2, "the corpus must produce exact cancellations"
            if metric != Metric.Cosine:
                assert np.unique(S).size < n // 2, "the corpus must produce tied sums"
            for take in (0, 1):
                for k in (10, n):
                    R.same(run(store, pos, neg, metric, take, k, SUM), RS.sum_scores(oracle, rows, inv, pos, neg, metric, take, k, P=P), (pos, neg, metric, take, k))
    store.close()


def test_sum_scores_infinite_and_nan_sums(oracle):
    rng = np.random.default_rng(11)
    n, dim, k = 400, 8, 10
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    rows[:20, 0] = np.float32(3e38) * np.sign(rows[:20, 0])        # one huge entry: a finite score against an ordinary row, +-inf against a huge one
    rows[20:40] = np.float32(3e38) * np.sign(rows[20:40])          # every entry huge: +-inf and inf - inf = NaN inside the dot
    store, rows, inv = make(dim, rows=rows)
    seen_nan = seen_inf = False
    for metric in ALL_METRICS:
        # huge examples on both sides; under L2 a huge example makes every score +inf, so the examples are ordinary rows there and
        # the huge rows of the corpus bring the infinities
        pos, neg = ([100, 150, 200], [250, 300]) if metric == Metric.Euclidean else ([100, 3, 200], [7, 300])
        P = R.pair_scores(oracle, rows, inv, pos + neg, metric)
        S = RS.sum_chain(P, len(pos))
        seen_inf |= bool(np.isinf(P).any())
        seen_nan |= bool(np.isnan(S).any())
        finite = np.isfinite(S) & RS.keep_without(n, pos, neg)
        assert finite.sum() >= k, "the model must keep at least k finite candidates"
        for take in (0, 1):
            exp = RS.sum_scores(oracle, rows, inv, pos, neg, metric, take, n, P=P)
            assert exp[0].size >= finite.sum() >= k
            R.same(run(store, pos, neg, metric, take, n, SUM), exp, ("overflow", metric, take))
            R.same(run(store, pos, neg, metric, take, k, SUM), RS.sum_scores(oracle, rows, inv, pos, neg, metric, take, k, P=P), ("overflow", metric, take, k))
    assert seen_nan and seen_inf, "the corpus must produce infinite pair scores and NaN sums"
    store.close()


# ---- average_vector -------------------------------------------------------------------------------------------------------------------------

PRUNED = (("exact_small", 0), ("exact_prune", 1), ("exact_sketch", 1), ("exact_sketch_bits", 4), ("exact_sketch_head", -1))


@pytest.mark.parametrize("form", ["plain", "pruned"])  # pruned: the four-bit sketch and the head, so that the pruned sweep serves the query
def test_average_vector_is_the_plain_query_of_the_model_vector(oracle, form):
    dim = 100
    store, rows, inv = make(dim, seed=12, options=PRUNED if form == "pruned" else ())
    rng = np.random.default_rng(12)
    mask = rng.uniform(size=N_ROWS) < 0.7
    for n_pos in (1, 2, 3, 5, 7):
        for n_neg in (0, 3):
            pos, neg = examples(rng, N_ROWS, n_pos, n_neg)
            q = RS.average_vector(rows, pos, neg)
            if n_pos in (3, 5, 7) and n_neg == 0:  # a reciprocal multiply would give another vector
                sp = rows[pos[0]].copy()
                for e in pos[1:]:
                    sp = (sp + rows[e]).astype(np.float32)
                assert (sp / np.float32(n_pos) != sp * np.float32(1.0 / n_pos)).any(), "the seed must tell a division from a reciprocal multiply"
            for metric in ALL_METRICS:
                take = TAKE[metric]
                for path in (Path.Auto, Path.Exact, Path.Mfma):
                    if path == Path.Mfma and (metric == Metric.Manhattan or n_pos in (2, 5)):
                        continue  # (the MFMA path does not score Manhattan; it runs for three of the five example counts)
                    for keep in ((mask,) if n_neg else (None,)):
                        exp = average_model(oracle, rows, inv, pos, neg, metric, take, 10, keep=keep)
                        assert np.unique(exp[0]["score"]).size == exp[0].size, "no ties at the cut: both tie orders give this list"
                        own = plain_query(store, q, metric, take, 10, RS.keep_without(N_ROWS, pos, neg, keep), path=path)
                        own_stats = dict(store.last_stats)
                        for tie_order in ("canonical", "reference"):
                            store.set_tie_order(tie_order)
                            got = run(store, pos, neg, metric, take, 10, AVG, mask=keep, path=path)
                            R.same(got, exp, (form, n_pos, n_neg, metric, path, keep is not None, tie_order))
                            assert got[0].tobytes() == own.tobytes()
                            if tie_order == "canonical":  # the same path served it, with the same work
                                for name in ("path_used", "passes", "vectors_compared", "evaluated_chunks") + (("rescored", "bytes_scanned") if path == Path.Exact else ()):
                                    assert store.last_stats[name] == own_stats[name], (name, form, metric, path)
                        store.set_tie_order("canonical")
    store.close()


def test_average_vector_k_filter_and_small_stores(oracle):
    store, rows, inv = make(24, seed=13)
    pos, neg = examples(np.random.default_rng(13), N_ROWS, 3, 2)
    q = RS.average_vector(rows, pos, neg)
    keep = RS.keep_without(N_ROWS, pos, neg)
    for metric in (Metric.Cosine, Metric.Euclidean):
        take = TAKE[metric]
        for k in (1, 10, 600, None):
            got = run(store, pos, neg, metric, take, k, AVG)
            R.same(got, average_model(oracle, rows, inv, pos, neg, metric, take, N_ROWS if k is None else k), (metric, k))
            assert got[0].tobytes() == plain_query(store, q, metric, take, N_ROWS if k is None else k, keep).tobytes()
        thr = float(average_model(oracle, rows, inv, pos, neg, metric, take, N_ROWS)[0]["score"][N_ROWS // 2])
        for cmp in CMPS:  # the filter acts on the query's score
            exp = average_model(oracle, rows, inv, pos, neg, metric, take, N_ROWS, cmp=int(cmp), thr=thr)
            assert 0 < exp[0].size < N_ROWS - 5
            R.same(run(store, pos, neg, metric, take, N_ROWS, AVG, flt=(thr, cmp)), exp, ("filter", metric, cmp))
    store.close()
    for n in (1, 63, 64, 65):
        store, rows, inv = make(5, n=n, seed=n)
        pos, neg = ([0], []) if n == 1 else ([0, n // 2], [n - 1])
        for metric in ALL_METRICS:
            got = run(store, pos, neg, metric, TAKE[metric], None, AVG)
            if n == 1:
                assert got[0].size == 0 and got[1].size == 0
            else:
                R.same(got, average_model(oracle, rows, inv, pos, neg, metric, TAKE[metric], n), (n, metric))
        store.close()


# ---- the shared tables: every query kind equals its serial answer, one after the other and from four threads ---------------------------------

def test_state_hygiene_between_the_query_kinds_serial_and_from_four_threads(oracle):
    n, dim = 2000, 24
    rng = np.random.default_rng(14)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    inv = store.inv_norms()
    ids = rng.choice(n, 9, replace=False)
    pos, neg = ids[:5].tolist(), ids[5:].tolist()
    ctx = [(pos[0], neg[0]), (pos[1], neg[1]), (pos[2], neg[2])]
    metric = Metric.Cosine
    jobs = [
        store.recommend(pos, neg, metric).take(n).collect_arrays,                                  # best_score, two rounds
        store.recommend(pos, neg, metric, SUM).take(n).collect_arrays,                             # the sort path
        store.discover(ctx, metric=metric).take(20).collect_arrays,                                # context search
        store.recommend(pos, neg, metric, AVG).take(20).collect_arrays,
        store.recommend(pos, neg, metric).take(20).fill_negative_side(False).collect_arrays,       # best_score without FILL
        store.recommend(pos[:1], [], metric, SUM).take(20).collect_arrays,                         # the single-query kernel
        store.discover(ctx, target_row=int(ids[8]), metric=metric).take(20).collect_arrays,        # with a target
        store.recommend(pos, neg[:1], metric, SUM).take(10).collect_arrays,                        # a last pass of two slots, the lists path
    ]

    def flat(res):
        return tuple(np.asarray(a).tobytes() for a in res)

    serial = [flat(j()) for j in jobs]
    # the serial answers of the new kinds are the model's, and best_score's its own
    R.same(jobs[0](), R.recommend(oracle, rows, inv, pos, neg, metric, 1, n), "best_score")
    R.same(jobs[1](), RS.sum_scores(oracle, rows, inv, pos, neg, metric, 1, n), "sum_scores")
    R.same(jobs[3](), average_model(oracle, rows, inv, pos, neg, metric, 1, 20), "average_vector")
    R.same(jobs[4](), R.recommend(oracle, rows, inv, pos, neg, metric, 1, 20, flags=0), "best_score, no fill")
    R.same(jobs[5](), RS.sum_scores(oracle, rows, inv, pos[:1], [], metric, 1, 20), "sum_scores, one example")
    R.same(jobs[7](), RS.sum_scores(oracle, rows, inv, pos, neg[:1], metric, 1, 10), "sum_scores, 5 + 1")
    # one after the other on one context, every kind behind every other kind
    for a in range(len(jobs)):
        for b in range(len(jobs)):
            assert flat(jobs[a]()) == serial[a] and flat(jobs[b]()) == serial[b], (a, b)
    # ... and from four threads, every thread its own interleaving
    threads_n, rounds = 4, 2
    gate = threading.Barrier(threads_n)
    bad, errors = [], []

    def work(t):
        try:
            gate.wait()
            for r in range(rounds):
                for i in range(len(jobs)):
                    j = (i * (2 * t + 1) + t + r) % len(jobs)
                    if flat(jobs[j]()) != serial[j]:
                        bad.append((t, r, j))
        except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(threads_n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert not bad, bad
    store.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------

def test_refusals_at_the_c_abi_leave_nothing_behind(oracle):
    store, rows, inv = make(13, n=500, seed=15)
    metric, take = Metric.Euclidean, 0
    L = N.lib()
    out = np.zeros(8, N.HIT_DTYPE)
    sides = np.full(8, 7, np.uint32)
    n_out = C.c_uint64(99)
    err = L.ott_last_error
    who = b"ott_query_recommend_strategy: "

    def desc(**kw):
        d = N.QueryDesc()
        d.queries, d.nq, d.metric, d.take, d.k = None, 0, int(metric), take, 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(strategy, pos, neg, d=None, flags=0, cap=8, outp=out, handle=None):
        d = desc() if d is None else d
        p, g = np.asarray(pos, np.uint64), np.asarray(neg, np.uint64)
        return L.ott_query_recommend_strategy(store._handle() if handle is None else handle, C.byref(d), strategy, N.ptr(p), p.size, N.ptr(g) if g.size else None, g.size,
                                              flags, N.ptr(outp) if outp is not None else None, cap, C.byref(n_out), N.ptr(sides), None)

    def still_works(strategy):
        assert n_out.value == 99 and not out["index"].any() and (sides == 7).all()  # the refusal wrote nothing
        assert call(strategy, [1, 1, 2], [3]) == 0 and n_out.value == 8
        model = RS.sum_scores if strategy == 2 else average_model
        exp = model(oracle, rows, inv, [1, 2], [3], metric, take, 8)
        assert out["index"].tolist() == exp[0]["index"].tolist() and out["score"].view(np.uint32).tolist() == exp[0]["score"].view(np.uint32).tolist()
        assert sides.tolist() == [1] * 8
        out[:] = 0
        sides[:] = 7
        n_out.value = 99

    q = np.zeros(13, np.float32)
    multi = VecStore(13, devices=[0, 0])
    multi.add_vectors(rows[:64])
    for st in (1, 2):
        assert call(3, [1], []) == -1 and who + b"unknown strategy" in err()
        still_works(st)
        assert call(st, [1], [], flags=1) == -1 and who + b"flags must be 0 (OTT_RECOMMEND_FILL belongs to best_score)" in err()
        still_works(st)
        assert call(st, [1], [], d=desc(nq=1, queries=q.ctypes.data)) == -1 and who + b"the examples are the queries; d->queries must be NULL and d->nq 0" in err()
        still_works(st)
        assert call(st, [1], [], d=desc(mode=1)) == -4 and who + b"the examples make ONE query; PER_QUERY is not served" in err()
        still_works(st)
        if st == 2:
            assert call(st, [1], [], d=desc(path=2)) == -4 and who + b"the MFMA path does not serve sum_scores; use path AUTO or EXACT" in err()
            still_works(st)
        assert call(st, [1], [2], handle=multi._handle()) == -4 and who + b"a multi-GPU store is not served" in err()
        still_works(st)
        assert call(st, [1], [], cap=7) == -1 and who + b"output capacity is smaller than min(k, rows)" in err()
        still_works(st)
        assert call(st, [1], [], outp=None) == -1 and who + b"out is NULL" in err()
        assert call(st, [1, 500], []) == -1 and who + b"example id 500 is not below the store's length 500" in err()
        assert call(st, [1], [2, 1]) == -1 and who + b"row 1 is listed as both a positive and a negative example" in err()
        assert call(st, list(range(65)), []) == -1 and who + b"more than OTT_RECOMMEND_MAX_EXAMPLES (64) distinct examples" in err()
        assert call(st, [1], [], d=desc(use_device_row_mask=1)) == -1 and who + b"use_device_row_mask set but ott_store_eval_row_mask was not called" in err()
        still_works(st)
        with pytest.raises(OttersError, match="ott_query_recommend_strategy: a multi-GPU store is not served"):
            multi.recommend([1], [2], strategy=RecommendStrategy(st)).take(3).collect()
    multi.close()
    # strategy 0 through the new entry point is ott_query_recommend: hits and sides, with FILL
    pos, neg = np.array([1, 2, 3, 4, 5], np.uint64), np.array([6, 7], np.uint64)
    d = desc(k=500)
    o0, o1 = np.zeros(500, N.HIT_DTYPE), np.zeros(500, N.HIT_DTYPE)
    s0, s1 = np.full(500, 7, np.uint32), np.full(500, 7, np.uint32)
    n0, n1 = C.c_uint64(0), C.c_uint64(0)
    for flags in (1, 0):
        assert L.ott_query_recommend(store._handle(), C.byref(d), N.ptr(pos), 5, N.ptr(neg), 2, flags, N.ptr(o0), 500, C.byref(n0), N.ptr(s0), None) == 0
        assert L.ott_query_recommend_strategy(store._handle(), C.byref(d), 0, N.ptr(pos), 5, N.ptr(neg), 2, flags, N.ptr(o1), 500, C.byref(n1), N.ptr(s1), None) == 0
        assert n0.value == n1.value > 0 and o0[: n0.value].tobytes() == o1[: n1.value].tobytes() and s0[: n0.value].tolist() == s1[: n1.value].tolist()
        if flags:
            assert (s0[: n0.value] == 0).any() and (s0[: n0.value] == 1).any()
    assert L.ott_query_recommend_strategy(store._handle(), C.byref(d), 0, N.ptr(pos), 5, N.ptr(neg), 2, 2, N.ptr(o1), 500, C.byref(n1), N.ptr(s1), None) == -1
    assert b"ott_query_recommend: unknown flag bits" in err()
    store.close()
