"""GPU: the extension query kinds at rows of 1024 to 4096 floats — id lists and score_rows, MMR, recommend and
discover, grouped search, MaxSim (the sweep, the listed gather, the batched gather).  Every kind has a thorough test file of its
own, which stops at narrow rows; this one runs each at the widths people store, where the by-id kernels' LDS opt-ins, their declared
maxima and the sweeps' many stages per row are.  Bar: the project's usual one — indices, order, counts and f32 score bits equal to
the host model each kind's own test file uses (imported from there, none is copied), no tolerance anywhere.  Where a route is asked
for, it is asserted from the stats: a case cannot pass by quietly running another kernel.

Corpora: per dim one set of rows, made once per module — 1000 rows (15 full tiles and a short one of 40), 300 at dims 3072 and 4096,
uniform in [-1, 1), a few rows duplicated so that ties occur — and ONE canonical ranking of all (row, query) pairs per (dim, metric,
take), over a pool of 33 queries.  The ranking of the first nq queries, or of a slice of the pool, is that ranking with the other
queries' pairs taken out: a pair's score does not depend on the other queries, and the order's last key is the query.

Why these dims: 1024 the top of the MaxSim gather's 16-token tier; 1536 the MMR pair kernel's LDS at exactly 48 KiB and the id
gather's first opt-in at eight queries; 1544 MMR's first width above 48 KiB; 2041 a padded width of 2048 with a remainder of one
float; 2048 every LDS figure at its declared maximum; 2049 one past the by-id kernels' limit; 3072 and 4096 the sweeps at 96 and 128
stages; 512 the MaxSim gather's 32-token tier.  Where crossing every value would make a case slow the values rotate: every value
and every pair of values occurs, not every tuple."""
import numpy as np
import pytest

import discover_ref as D
import grouped_ref as GR
import maxsim_ref as MS
import mmr_ref as MR
import recommend_ref as RR
import test_gpu_discover as TD
import test_gpu_groups as G
import test_gpu_groups_top as GT
import test_gpu_idlist as IL
import test_gpu_maxsim as MX
import test_gpu_maxsim_batch as MB
import test_gpu_maxsim_groups as MG
import test_gpu_mmr as TM
import test_gpu_recommend as TR
from otters_amd import Metric, OttersError, Path, VecStore

pytestmark = pytest.mark.gpu

TAKE = IL.TAKE
ALL_METRICS = IL.ALL_METRICS
POOL = 33  # queries / tokens per corpus


@pytest.fixture(scope="module", autouse=True)
def collect_the_models_garbage():
    """as tests/test_gpu_mmr.py: the models' short-lived objects are collected when the module is done"""
    yield
    import gc
    gc.collect()


class Corpus:
    """one dim's rows, query pool and canonical rankings: made once, never changed"""

    def __init__(self, oracle, dim):
        self.oracle, self.dim = oracle, dim
        self.n = n = 300 if dim >= 3072 else 1000
        rng = np.random.default_rng(14000 + dim)
        rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        rows[17] = rows[5]          # duplicates: equal scores under every query, inside a tile ...
        rows[130] = rows[5]         # ... across tiles ...
        rows[n - 1] = rows[64]      # ... and on the last row of the short tile
        rows[n // 2 + 1] = rows[n // 2]
        rows.setflags(write=False)
        self.rows = rows
        self.q_pool = rng.uniform(-1, 1, (POOL, dim)).astype(np.float32)
        self.q_pool.setflags(write=False)
        self.have = {}

    def store(self, reduce_mode=0):
        s = VecStore(self.dim)
        s.set_reduce_order(reduce_mode)  # before the rows: the stored inverse norms are summed in it
        s.add_vectors(self.rows)
        return s

    def full(self, metric, take, nq, reduce_mode=0, first=0):
        """the canonical ranking of queries [first, first + nq) of the pool, numbered from 0"""
        key = (int(metric), int(take), int(reduce_mode))
        if key not in self.have:
            self.have[key] = {None: IL.ranking(self.oracle, self.rows, self.q_pool, metric, int(take), reduce_mode)}
        cache = self.have[key]
        if (first, nq) not in cache:
            f = cache[None]
            f = f[(f["query"] >= first) & (f["query"] < first + nq)].copy()
            f["query"] -= first
            f.setflags(write=False)
            cache[(first, nq)] = f
        return cache[(first, nq)]


class ByTake:
    """grouped_ref.Rankings' interface — get(metric, nq, take) — over a corpus's shared rankings"""

    def __init__(self, corpus):
        self.c = corpus

    def get(self, metric, nq, take):
        return self.c.full(metric, take, nq)


@pytest.fixture(scope="module")
def corpora(oracle):
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = Corpus(oracle, dim)
        return made[dim]

    yield get
    made.clear()


# ---- 1. id lists and score_rows --------------------------------------------------------------------------------------------------

def id_lists(rng, n):
    return {"one id": np.array([n - 1]), "500 ids": rng.choice(n, 500, replace=False),
            "700 with duplicates": np.concatenate([rng.choice(n, 695), [5, 17, 5, n - 1, 64]])}


@pytest.mark.parametrize("dim", [1024, 1536, 2041, 2048])
def test_id_lists_every_metric_query_count_list_k_and_route(corpora, dim):
    """1, 5, 8 and 16 queries: the one-query kernel, the eight-query tile part filled and full (from 1536 on: more than 48 KiB of
    LDS, the opt-in; 2048: G8_SMEM_MAX) and two passes of it; 2041: 255 chains and a tail of one float, in both reduce orders.  With
    id_gather = 1 the gather must have run: it compares at most the distinct listed rows per query, the mask route the whole store"""
    c = corpora(dim)
    n = c.n
    lists = id_lists(np.random.default_rng(dim), n)
    for reduce_mode in ((0, 1) if dim == 2041 else (0,)):
        store = c.store(reduce_mode)
        for metric in ALL_METRICS:
            for nq in (1, 5, 8, 16):
                full = c.full(metric, TAKE[metric], nq, reduce_mode)
                for lname, ids in lists.items():
                    keep, distinct = IL.id_mask(n, ids), np.unique(ids).size
                    for k in (1, 10, 100):
                        for perq in ((False, True) if nq > 1 else (False,)):
                            plan = IL.build(store, c.q_pool[:nq], metric, k, Path.Auto, perq, ids=ids)
                            ref, ref_counts = IL.expected(full, keep, k, nq, perq)
                            for gather in (1, 0):
                                where = (dim, reduce_mode, metric, nq, lname, k, perq, gather)
                                store.set_option("id_gather", gather)
                                got, counts = plan.collect_arrays()
                                IL.bits_equal(got, ref, where)
                                assert list(counts) == ref_counts, where
                                compared = store.last_stats["vectors_compared"]
                                if gather:
                                    assert 0 < compared <= distinct * nq and store.last_stats["path_used"] == int(Path.Exact), (where, store.last_stats)
                                    assert store.last_stats["passes"] == (2 if nq == 16 else 1), (where, store.last_stats)
                                else:
                                    assert compared == n * nq, (where, store.last_stats)
        store.close()


@pytest.mark.parametrize("dim", [1024, 1536, 2041, 2048])
def test_score_rows_are_the_dense_scores(corpora, dim):
    """lists that cross a tile of 64 slots (65 ids; 130 unsorted with duplicates: two full tiles and a part), every query count"""
    c = corpora(dim)
    n = c.n
    rng = np.random.default_rng(100 + dim)
    lists = {"65 ids": rng.choice(n, 65, replace=False), "130 with duplicates": np.concatenate([[n - 1, 0, 0, 17, 5], rng.choice(n, 125)]), "one id": np.array([64])}
    for reduce_mode in ((0, 1) if dim == 2041 else (0,)):
        store = c.store(reduce_mode)
        for metric in ALL_METRICS:
            for nq in (1, 5, 8, 16):
                full = c.full(metric, TAKE[metric], nq, reduce_mode)
                for lname, ids in lists.items():
                    got = store.score_rows(c.q_pool[:nq], metric, ids)
                    IL.scores_equal(got, IL.dense_scores(full, nq, ids), (dim, reduce_mode, metric, nq, lname))
        store.close()


def test_past_2048_floats_id_lists_take_the_mask_route_and_score_rows_refuses(corpora):
    """a padded width of 2056: with id_gather = 1 a list still answers, by the mask route (every row of the store is compared);
    score_rows refuses and leaves the store usable"""
    c = corpora(2049)
    n = c.n
    store = c.store()
    store.set_option("id_gather", 1)
    lists = id_lists(np.random.default_rng(2049), n)
    for metric in ALL_METRICS:
        for nq in (1, 5):
            full = c.full(metric, TAKE[metric], nq)
            for lname, ids in lists.items():
                for k in (1, 10, 100):
                    got, _ = IL.build(store, c.q_pool[:nq], metric, k, Path.Exact, False, ids=ids).collect_arrays()
                    IL.bits_equal(got, IL.expected(full, IL.id_mask(n, ids), k, nq, False)[0], (metric, nq, lname, k))
                    assert store.last_stats["vectors_compared"] == n * nq, (metric, nq, lname, k, store.last_stats)
        with pytest.raises(OttersError) as e:
            store.score_rows(c.q_pool[:3], metric, lists["500 ids"])
        assert e.value.status == -4 and "rows of more than 2048 floats are not served" in str(e.value)
        plain, _ = store.query(c.q_pool[:3], metric).take(10).collect_arrays()
        IL.bits_equal(plain, c.full(metric, TAKE[metric], 3)[:10], ("plain after the refusal", metric))
    store.close()


# ---- 2. MMR ----------------------------------------------------------------------------------------------------------------------

MMR_SHAPES = ((8, 3), (8, 8), (64, 10), (64, 64), (65, 7), (65, 65), (200, 20), (200, 200))  # (fetch_k, k): k below and equal
MMR_SHAPES_BATCH = ((8, 8), (64, 10), (65, 65), (200, 20))
MMR_FETCH_MAX = 200


class MmrModel:
    """mmr_ref over one (corpus, store, metric): a query's candidates are the first fetch_k pairs of its shared ranking among the
    kept rows; the pair rows P[s] are made once over the first 200 candidates and shared by every fetch_k (a prefix), k and lambda"""

    def __init__(self, c, inv, metric, reduce_mode=0):
        self.c, self.inv, self.metric, self.reduce_mode, self.have = c, inv, metric, reduce_mode, {}

    def of(self, qi, keep, tag):
        if (qi, tag) not in self.have:
            f = self.c.full(self.metric, TAKE[self.metric], 1, self.reduce_mode, first=qi)
            if keep is not None:
                f = f[keep[f["index"].astype(np.int64)]]
            cand = f[:MMR_FETCH_MAX].copy()
            cand["query"] = qi
            idx = cand["index"].astype(np.int64)
            self.have[(qi, tag)] = (cand, np.ascontiguousarray(self.c.rows[idx]), self.inv[idx], {})
        return self.have[(qi, tag)]

    def __call__(self, nq, keep, tag, k, fetch_k, lam):
        take = TAKE[self.metric]
        hits, counts, vals = [], [], []
        for qi in range(nq):
            cand, crow, cinv, prow = self.of(qi, keep, tag)

            def pair_of(s):
                if s not in prow:
                    prow[s] = MR.pair_row(self.c.oracle, crow, cinv, s, self.metric, self.reduce_mode)
                return prow[s][:fetch_k]

            picks, v = MR.greedy(cand["score"][:fetch_k], pair_of, k, lam, take)
            hits.append(cand[picks])
            counts.append(int(picks.size))
            vals.append(v)
        return np.concatenate(hits), counts, np.concatenate(vals)


@pytest.mark.parametrize("dim", [1024, 1536, 1544, 2041, 2048])
def test_mmr_every_metric_shape_lambda_batch_and_id_list(corpora, dim):
    """the pair kernel keeps eight selected rows in LDS: 48 KiB exactly at 1536 (no opt-in), the first opt-in at 1544, 64 KiB at 2048;
    fetch_k 8 is one tile of selected rows, 64 and 65 one and two candidate tiles, 200 with an id list a first stage on the mask route"""
    c = corpora(dim)
    n = c.n
    ids = np.random.default_rng(200 + dim).choice(n, 500, replace=False)
    listed = IL.id_mask(n, ids)
    for reduce_mode in ((0, 1) if dim == 2041 else (0,)):
        store = c.store(reduce_mode)
        inv = store.inv_norms()
        for metric in (ALL_METRICS if reduce_mode == 0 else (Metric.Cosine, Metric.Manhattan)):
            model = MmrModel(c, inv, metric, reduce_mode)
            take = TAKE[metric]
            for nq, shapes in ((1, MMR_SHAPES), (3, MMR_SHAPES_BATCH)):
                for with_ids in (False, True):
                    for fetch_k, k in shapes:
                        for lam in (0.0, 0.5, 1.0):
                            q = c.q_pool[0] if nq == 1 else c.q_pool[:nq]
                            got = TM.run(store, q, metric, take, k, fetch_k, lam, perq=nq > 1, ids=ids if with_ids else None)
                            exp = model(nq, listed if with_ids else None, with_ids, k, fetch_k, lam)
                            assert exp[1] == [k] * nq
                            TM.check(got, exp, (dim, reduce_mode, metric, nq, with_ids, fetch_k, k, lam))
        store.close()


# ---- 3. recommend and discover ---------------------------------------------------------------------------------------------------

SWEEP_DIMS = [1024, 2041, 2049, 3072, 4096]  # 32, 64 (a remainder of one float), 65 (a stage of nine floats), 96 and 128 stages per row


def short_mask(rng, n, drop):
    """a row mask shorter than the store (the rows past it are kept) that keeps about half of its rows and drops `drop`"""
    mask = rng.uniform(size=n - 60) < 0.5
    mask[min(int(drop), mask.size - 1)] = False
    keep = np.ones(n, bool)
    keep[: mask.size] = mask
    return mask, keep


@pytest.mark.parametrize("dim", SWEEP_DIMS)
def test_recommend_every_metric_take_example_count_fill_and_k(corpora, dim):
    c = corpora(dim)
    n = c.n
    rng = np.random.default_rng(300 + dim)
    store = c.store()
    inv = store.inv_norms()
    pos5, neg3 = TR.examples(rng, n, 5, 3)
    mask, keep = short_mask(rng, n, pos5[0])
    for metric in ALL_METRICS:
        P8 = RR.pair_scores(c.oracle, c.rows, inv, pos5 + neg3, metric)

        def model(n_pos, n_neg, take, k, **kw):
            return RR.recommend(c.oracle, c.rows, inv, pos5[:n_pos], neg3[:n_neg], metric, take, k, P=P8[list(range(n_pos)) + list(range(5, 5 + n_neg))], **kw)

        for take in (0, 1):
            for n_pos, n_neg in ((1, 0), (1, 3), (5, 0), (5, 3)):  # 1, 4, 5 and 8 slots: one pass, one full, two, two full
                for fill in (True, False):
                    for k in (10, 600):
                        where = (dim, metric, take, n_pos, n_neg, fill, k)
                        got = TR.run(store, pos5[:n_pos], neg3[:n_neg], metric, take, k, fill=fill)
                        RR.same(got, model(n_pos, n_neg, take, k, flags=int(fill)), where)
                        st = store.last_stats
                        assert st["passes"] == -(-(n_pos + n_neg) // 4) and st["path_used"] == int(Path.Exact), (where, st)
                        assert st["vectors_compared"] == n * (n_pos + n_neg), (where, st)
            # a row mask shorter than the store, an example among the masked rows
            for k in (10, 600):
                RR.same(TR.run(store, pos5, neg3, metric, take, k, mask=mask), model(5, 3, take, k, keep=keep), (dim, metric, take, k, "row mask"))
        # deleted rows: never candidates; a deleted row may be an example (stored data is read)
        take = TAKE[metric]
        first = model(5, 3, take, 20)[0]["index"].astype(np.int64)
        dead = np.concatenate([first[::2], [pos5[1], neg3[0]]])
        assert store.delete_rows(dead) == dead.size
        live = np.ones(n, bool)
        live[dead] = False
        for k in (10, 600):
            exp = model(5, 3, take, k, keep=live)
            assert not np.isin(exp[0]["index"], dead).any()
            RR.same(TR.run(store, pos5, neg3, metric, take, k), exp, (dim, metric, k, "deleted"))
            RR.same(TR.run(store, pos5, neg3, metric, take, k, mask=mask), model(5, 3, take, k, keep=keep & live), (dim, metric, k, "deleted and a row mask"))
        assert store.restore_rows(dead) == dead.size
    store.close()


@pytest.mark.parametrize("dim", SWEEP_DIMS)
def test_discover_every_metric_take_pair_count_target_and_k(corpora, dim):
    c = corpora(dim)
    n = c.n
    rng = np.random.default_rng(400 + dim)
    store = c.store()
    model = TD.Model(c.oracle, c.rows, store.inv_norms())
    ctx3 = TD.context(rng, n, 3)
    tgts = TD.targets(rng, dim, n)  # a vector, a stored row, none (context search)
    mask, keep = short_mask(rng, n, ctx3[0][0])
    for metric in ALL_METRICS:
        for take in (0, 1):
            for n_pairs in (1, 3):
                ctx = ctx3[:n_pairs]
                for tgt in tgts:
                    for k in (25, 600):
                        where = (dim, metric, take, n_pairs, sorted(tgt), k)
                        D.same(TD.run(store, ctx, metric, take, k, **tgt), model(ctx, metric, take, k, **tgt), where)
                        st = store.last_stats
                        slots = 2 * n_pairs + (1 if tgt else 0)
                        assert st["passes"] == -(-slots // 4) and st["path_used"] == int(Path.Exact), (where, st)
                        assert st["vectors_compared"] == n * slots, (where, st)
            for tgt in tgts:
                D.same(TD.run(store, ctx3, metric, take, 25, mask=mask, **tgt), model(ctx3, metric, take, 25, keep=keep, **tgt), (dim, metric, take, sorted(tgt), "row mask"))
        take = TAKE[metric]
        exp = model(ctx3, metric, take, 600, min_wins=2, **tgts[0])
        assert exp[0].size and exp[1].min() >= 2
        D.same(TD.run(store, ctx3, metric, take, 600, min_wins=2, **tgts[0]), exp, (dim, metric, "min_wins"))
        # deleted rows: never hits; a deleted row works as an example and as the target row
        first = model(ctx3, metric, take, 20, **tgts[0])[0]["index"].astype(np.int64)
        dead = np.unique(np.concatenate([first[::2], [ctx3[1][0], ctx3[2][1], tgts[1]["target_row"]]]))
        assert store.delete_rows(dead) == dead.size
        live = np.ones(n, bool)
        live[dead] = False
        for tgt in tgts:
            exp = model(ctx3, metric, take, 600, keep=live, **tgt)
            assert not np.isin(exp[0]["index"], dead).any()
            D.same(TD.run(store, ctx3, metric, take, 600, **tgt), exp, (dim, metric, sorted(tgt), "deleted"))
            D.same(TD.run(store, ctx3, metric, take, 25, mask=mask, **tgt), model(ctx3, metric, take, 25, keep=keep & live, **tgt), (dim, metric, sorted(tgt), "deleted and a row mask"))
        assert store.restore_rows(dead) == dead.size
    store.close()


# ---- 4. grouped search -----------------------------------------------------------------------------------------------------------

def one_per_group(store, c, gid, metric, nq, k, where, keep=None, mask=None):
    plan = G.build(store, c.q_pool[:nq], metric, k, perq=nq > 1, mask=mask)
    keep = np.ones(c.n, bool) if keep is None else keep
    ref, ref_counts = G.expected(c.full(metric, G.take_of(metric, k), nq), gid, keep, plan.resolve().k, nq)
    got, counts = plan.collect_arrays()
    G.bits_equal(got, ref, where)
    assert list(counts) == ref_counts, where
    return got, counts


@pytest.mark.parametrize("dim", [1024, 2049, 4096])
def test_grouped_search_every_metric_m_batch_layout_and_k(corpora, dim):
    """1, 4 and 5 queries per query: the one-query sweep, a full pass of four, a pass and a part; a contiguous and a shuffled layout"""
    c = corpora(dim)
    n = c.n
    rng = np.random.default_rng(500 + dim)
    lay = G.layouts(rng, n)
    store = c.store()
    ranks = ByTake(c)
    mask, keep = short_mask(rng, n, 0)
    for lname in ("contiguous by row", "37 random groups"):
        store.set_groups(lay[lname])
        gid = GR.dense(lay[lname])
        for metric in ALL_METRICS:
            for nq in (1, 4, 5):
                for k in (1, 10, None):
                    got, counts = one_per_group(store, c, gid, metric, nq, k, (dim, lname, metric, nq, k, "one_per_group"))
                    for m in (1, 3, 16):
                        top, top_counts, _ = GT.check(store, ranks, c.q_pool, gid, metric, nq, m, k, (dim, lname, metric, nq, k, m))
                        if m == 1:
                            assert top.tobytes() == got.tobytes() and list(top_counts) == list(counts), (dim, lname, metric, nq, k)
            # a row mask shorter than the store, then deleted rows (the best row of the best group among them), then both
            best = c.full(metric, TAKE[metric], 1)["index"][:3].astype(np.int64)
            dead = np.unique(np.concatenate([best, rng.choice(n, 40, replace=False)]))
            live = np.ones(n, bool)
            live[dead] = False
            for step_keep, step_mask, deleted in ((keep, mask, False), (live, None, True), (keep & live, mask, True)):
                if deleted:
                    assert store.delete_rows(dead) == dead.size
                for nq in (1, 5):
                    for k in (10, None):
                        where = (dim, lname, metric, nq, k, step_mask is not None, deleted)
                        one_per_group(store, c, gid, metric, nq, k, where, keep=step_keep, mask=step_mask)
                        GT.check(store, ranks, c.q_pool, gid, metric, nq, 3, k, where, keep=step_keep, mask=step_mask)
                if deleted:
                    assert store.restore_rows(dead) == dead.size
    store.close()


# ---- 5. MaxSim -------------------------------------------------------------------------------------------------------------------

def mixed_groups(rng, n):
    """n = 1000: 350 groups of one row (ids 0 .. 349), 175 pairs (350 .. 524) and one group of 300 rows — nine full steps of the gather's
    workgroup and a part — with the LAST id, 525, so that lists_of's "one group" is that group; the rows are shuffled over the store"""
    base = np.concatenate([np.arange(350), 350 + np.arange(350) // 2, np.full(n - 700, 525)])
    return base[rng.permutation(n)]


@pytest.mark.parametrize("dim", [1024, 2041, 2048, 4096])
def test_maxsim_sweep_on_many_tiles(corpora, dim):
    """1, 4, 5 and 33 tokens: the one-token sweep, a full pass of four, a pass and a part, nine passes, each over every tile"""
    c = corpora(dim)
    n = c.n
    rng = np.random.default_rng(600 + dim)
    lay = {"contiguous by row": np.arange(n) // 8, "shuffled": mixed_groups(rng, n) if n == 1000 else rng.integers(0, 37, n)}
    store = c.store()
    mask, keep = short_mask(rng, n, 0)
    ks = (1, 10, None)
    turn = 0
    for lname, labels in lay.items():
        store.set_groups(labels)
        gid = MX.dense(labels)
        ng = int(gid.max()) + 1
        for metric in ALL_METRICS:
            for nq in (1, 4, 5, 33):
                for k in ks:
                    take = G.take_of(metric, k)
                    ref = MS.expected(c.full(metric, take, nq), gid, np.ones(n, bool), k if k is not None else ng, nq, take, n_groups=ng)
                    got, counts = MX.build(store, c.q_pool[:nq], metric, k).collect_arrays()
                    MX.bits_equal(got, ref, (dim, lname, metric, nq, k))
                    assert counts == [ref.size]
                    assert store.last_stats["vectors_compared"] == n * nq
                turn += 1
                k = ks[turn % 3]
                take = G.take_of(metric, k)
                ref = MS.expected(c.full(metric, take, nq), gid, keep, k if k is not None else ng, nq, take, n_groups=ng)
                MX.bits_equal(MX.build(store, c.q_pool[:nq], metric, k, mask=mask).collect_arrays()[0], ref, (dim, lname, metric, nq, k, "row mask"))
    store.close()


TIER_TOP = {512: 32, 1024: 16, 2041: 8, 2048: 8}  # tokens per pass of the listed gather at the top of each tier


@pytest.mark.parametrize("dim", [512, 1024, 2041, 2048])
def test_listed_maxsim_at_the_top_of_each_token_tier(corpora, dim):
    """as many tokens as one pass holds at this width (74 368, 82 240 and 98 464 bytes of LDS: the token block, its padding of four floats
    per dim and the waves' maxima at their largest) and one more, so that the reduce kernel runs too; a group of 300 rows, single rows
    and pairs; both routes, told apart by the rows compared and the passes"""
    c = corpora(dim)
    n = c.n
    rng = np.random.default_rng(700 + dim)
    gid = mixed_groups(rng, n)
    ng = int(gid.max()) + 1
    store = c.store()
    store.set_groups(gid)
    lists = MG.lists_of(rng, ng)
    keep = np.ones(n, bool)
    ks = (1, 10, 65, None)
    turn = 0
    for metric in ALL_METRICS:
        for nq in (TIER_TOP[dim], TIER_TOP[dim] + 1):
            for lname, listed in lists.items():
                turn += 1
                k = ks[turn % len(ks)]
                take = G.take_of(metric, k)
                ref = MG.reference(c.full(metric, take, nq), gid, ng, keep, listed, k, nq, take)
                for route in MG.ROUTES:
                    where = (dim, metric, nq, lname, k, route)
                    got, st = MG.run(store, c.q_pool[:nq], metric, k, listed, route)
                    MG.bits_equal(got, ref, where)
                    if listed.size:
                        MG.took(st, route, gid, listed, nq, n)
                        if route == MG.GATHER:
                            assert st["passes"] == (1 if nq == TIER_TOP[dim] else 2), (where, st)
    assert st["group_index_builds"] == 1
    store.close()


@pytest.mark.parametrize("dim", [512, 1024, 2048])
def test_batched_listed_maxsim_at_the_top_of_each_token_tier(corpora, dim):
    """three queries of unequal token counts, the longest at the top of the tier, each with its own list: the batched gather answers
    in ONE pass (the loop over the single call reports the sum of the queries' passes, three at least)"""
    c = corpora(dim)
    n = c.n
    rng = np.random.default_rng(800 + dim)
    gid = mixed_groups(rng, n)
    ng = int(gid.max()) + 1
    store = c.store()
    store.set_groups(gid)
    top = TIER_TOP[dim]
    tokens, first = (max(top // 4, 1), top, top // 2 + 1), (0, 1, 2)  # slices of the pool that overlap: 1 + 32 tokens are all it has
    sets = [c.q_pool[a:a + t] for a, t in zip(first, tokens)]
    lists = [rng.permutation(ng), np.array([ng - 1, 3, 400, 3]), rng.choice(ng, ng // 2, replace=False)]
    keep = np.ones(n, bool)
    for metric, ks in zip(ALL_METRICS, ((1, None), (10, 65), (None, 10), (65, 1))):
        for k in ks:
            take = G.take_of(metric, k)
            fulls = [c.full(metric, take, tokens[b], first=first[b]) for b in range(3)]
            refs = MB.batch_reference(fulls, sets, gid, ng, keep, lists, k, take)
            for route in MB.ROUTES:
                got, counts, st = MB.run_batch(store, sets, metric, k, lists, route)
                MB.batch_equal(got, counts, refs, (dim, metric, k, route))
                if route == MB.GATHER:
                    assert st["passes"] == 1 and st["path_used"] == 1, st
                    assert st["vectors_compared"] == sum(MB.listed_rows(gid, l) * t.shape[0] for l, t in zip(lists, sets)), st
                else:
                    assert st["passes"] >= 3, st
    store.close()
