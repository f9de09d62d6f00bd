"""GPU: the extension query kinds on stores past 2^32 bytes, 2^24 rows and 4 GiB of per-row state — id lists and
score_rows, MMR, recommend (three strategies), discover and context search, grouped search (one_per_group, per_group(m)), MaxSim (the
sweep, the listed gather, the batched gather), the per-query masks sweep, deleted rows and compact().  Every kind has a thorough test
file of its own, which stops at about 100k rows and a few MB; none of their kernels had computed an address past 2^31 bytes or seen a
row id above 2^24.  Bar: the project's usual one — indices, order, counts, `query`, f32 score bits and the side outputs equal to the
host model each kind's own test file uses (imported from there, none is copied), no tolerance anywhere, the route asserted from the
stats.

How a host model answers for 16 GiB: tests/large_offsets.py.  Every kind applies its row mask first, so the model over the compact
rows R[K], mapped through K, is the answer for the whole store under the row mask K (proved in tests/test_large_offsets_cpu.py); K is
130 rows at both ends of the store and on either side of every boundary row.  Masked runs skip whole tiles, so section 3 runs every
sweep once over the whole store unmasked, with twelve planted rows at K's window edges that win by construction.

The stores, the smallest that cross each line:
  W  dim 2048, 2^21 + 300 rows (16 GiB): row 2^18 starts at byte 2^31, 2^19 at byte 2^32, 2^20 at float 2^31, 2^21 at float 2^32;
     2048 floats is the by-id kernels' declared maximum, so one store serves gathers and sweeps
  N  dim 4, 2^27 + 300 rows (2 GiB): row ids pass 2^24 (a row id put through a float breaks there) and 2^26; the (query, row) and
     (query, group) key tables of a four-query pass are 4 GiB; tile counts reach 2^21; live_scan_kernel scans 2^21 words
  S  dim 4, 2^29 + 300 rows (8 GiB): recommend's and discover's 8-byte state per row and the key table cross 4 GiB each, the inverse
     norms are 2 GiB, a row mask 64 MiB
  P  dim 512, 2^21 + 300 rows (4 GiB): row 2^20 starts at byte 2^31, 2^21 at byte 2^32.  The pruned exact sweep serves single queries
     of at most 896 floats (ott_exact_plan.h: exact_lean, the query rides in the kernel arguments), so on W the plain sweep answers
     average_vector and the base query — asserted there — and P is where "it pruned" can be, and is, asserted.
One store is alive at a time: asking for the next closes the one before; the tests at the end of the file name the cases in the
stores' order."""
import time

import numpy as np
import pytest

import discover_ref as D
import grouped_ref as GR
import large_offsets as LO
import masks_ref as MKR
import maxsim_ref as MS
import mmr_ref as MR
import recommend_ref as RR
import recommend_strategy_ref as RS
import test_gpu_discover as TD
import test_gpu_groups as G
import test_gpu_groups_top as GT
import test_gpu_idlist as IL
import test_gpu_masks as TMK
import test_gpu_maxsim as MX
import test_gpu_maxsim_batch as MB
import test_gpu_maxsim_groups as MG
import test_gpu_mmr as TM
import test_gpu_recommend as TR
import test_gpu_recommend_strategy as TS
from otters_amd import Metric, OttersError, Path, RecommendStrategy, VecStore
from otters_amd import _native as N
from otters_amd.vec import lower_row_masks

pytestmark = pytest.mark.gpu

TAKE = IL.TAKE
ALL_METRICS = IL.ALL_METRICS
NO_COSINE = (Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)
POOL = 16  # queries / tokens per store
SEED = 0x1A46E
HALF = LO.HALF

SHAPES = {  # name: (dim, rows, boundary rows, bytes of the largest tables a case makes beside the rows)
    "W": (2048, (1 << 21) + 300, (1 << 18, 1 << 19, 1 << 20, 1 << 21), 2 << 30),
    "N": (4, (1 << 27) + 300, (1 << 24, 1 << 26), 10 << 30),
    "S": (4, (1 << 29) + 300, (1 << 29,), 12 << 30),
    "P": (512, (1 << 21) + 300, (1 << 20, 1 << 21), 2 << 30),
}


@pytest.fixture(scope="module", autouse=True)
def collect_the_models_garbage():
    """as tests/test_gpu_mmr.py: the models' short-lived objects are collected when the module is done"""
    yield
    import gc
    gc.collect()


def make_store(name):
    """the store `name` filled on the device, or a skip that states the bytes when the device cannot hold it"""
    import torch
    dim, n, _, tables = SHAPES[name]
    need = int(1.25 * (n * (dim * 4 + 5) + tables))
    t0 = time.perf_counter()
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        pytest.skip(f"store {name} needs {need} bytes of device memory (rows, tables and a quarter more), {free} are free")
    t1 = time.perf_counter()
    store = VecStore(dim)
    store.reserve(n)
    store.append_random(n, SEED)
    store.inv_norms(n - 1, 1)  # (waits for the fill)
    print(f"store {name}: {n} x {dim}; asking for the free device memory took {t1 - t0:.2f} s, making the store {time.perf_counter() - t1:.2f} s")
    return store


class Big:
    """one store, its window rows and the canonical rankings over them: made once, never changed"""

    def __init__(self, oracle, name):
        self.oracle, self.name = oracle, name
        self.dim, self.n, self.boundaries, _ = SHAPES[name]
        self.store = make_store(name)
        t1 = time.perf_counter()
        self.K, self.words = LO.windows(self.n, self.boundaries)
        self.m = self.K.size
        self.mask = LO.mask_bool(self.words, self.n)  # the plans take bool[n]
        self.R = LO.window_rows(oracle, self.K, self.dim, SEED)
        self.R.setflags(write=False)
        self.inv = np.concatenate([self.store.inv_norms(a, c) for a, c in LO.runs_of(self.K)])
        self.q_pool = np.random.default_rng(SEED + self.dim).uniform(-1, 1, (POOL, self.dim)).astype(np.float32)
        self.have = {}
        print(f"store {name}: {self.m} window rows, their norms and the mask in {time.perf_counter() - t1:.2f} s")

    def full(self, metric, take, nq, first=0):
        """the canonical ranking of R[K] under queries [first, first + nq) of the pool (compact indices), numbered from 0"""
        key = (int(metric), int(take))
        if key not in self.have:
            self.have[key] = {None: IL.ranking(self.oracle, self.R, self.q_pool, metric, int(take))}
        cache = self.have[key]
        if (first, nq) not in cache:
            f = cache[None]
            f = f[(f["query"] >= first) & (f["query"] < first + nq)].copy()
            f["query"] -= first
            f.setflags(write=False)
            cache[(first, nq)] = f
        return cache[(first, nq)]

    def S(self, hits):
        return LO.to_store_index(self.K, hits)

    def both_sides(self):
        """compact indices of the rows on either side of every boundary, and of the store's first and last row"""
        rows = [0, self.n - 1] + [r for b in self.boundaries for r in (b - 1, b)]
        return LO.compact_of(self.K, rows)

    def close(self):
        self.store.close()
        self.have.clear()


class Stores:
    def __init__(self, oracle):
        self.oracle, self.name, self.big = oracle, None, None

    def get(self, name):
        if self.name != name:
            self.drop()
            self.big, self.name = Big(self.oracle, name), name
        return self.big

    def drop(self):
        if self.big is not None:
            self.big.close()
        self.big, self.name = None, None


@pytest.fixture(scope="module")
def stores(oracle):
    s = Stores(oracle)
    yield s
    s.drop()


def sweep_stats(st, n, slots, where):
    assert st["path_used"] == int(Path.Exact) and st["passes"] == (1 if slots == 1 else -(-slots // 4)), (where, st)
    assert st["vectors_compared"] == n * slots, (where, st)


# ---- 1. id lists and score_rows (W, N) -------------------------------------------------------------------------------------------

def listed(b, rng):
    """compact ids: 300 random rows of K, every row beside a boundary, duplicates"""
    c = np.concatenate([rng.choice(b.m, 300, replace=False), b.both_sides(), b.both_sides()[::2], rng.choice(b.m, 20)])
    return c[rng.permutation(c.size)]


def case_id_lists_both_routes_and_score_rows(stores, name):
    """1, 5 and 16 queries: the one-query gather, a part filled pass of eight and two passes; id_gather 1 must have gathered (it
    compares at most the distinct listed rows per query), 0 takes the mask route and sweeps the store"""
    b = stores.get(name)
    rng = np.random.default_rng(1)
    ids_c = listed(b, rng)
    ids = b.K[ids_c]
    assert ids.max() == b.n - 1 and (ids >= b.boundaries[-1]).any() and (ids < b.boundaries[0]).any()
    keep, distinct = IL.id_mask(b.m, ids_c), np.unique(ids_c).size
    for metric in ALL_METRICS:
        for nq in (1, 5, 16):
            full = b.full(metric, TAKE[metric], nq)
            IL.scores_equal(b.store.score_rows(b.q_pool[:nq], metric, ids), IL.dense_scores(full, nq, ids_c), (name, metric, nq, "score_rows"))
            for k in (10, 100):
                # (path EXACT: on AUTO the mask route of a batch goes through the cascade and its planes, which are not this file's)
                plan = IL.build(b.store, b.q_pool[:nq], metric, k, Path.Exact if nq > 1 else Path.Auto, False, ids=ids)
                ref, ref_counts = IL.expected(full, keep, k, nq, False)
                for gather in (1, 0):
                    where = (name, metric, nq, k, gather)
                    b.store.set_option("id_gather", gather)
                    got, counts = plan.collect_arrays()
                    IL.bits_equal(got, b.S(ref), where)
                    assert list(counts) == ref_counts, where
                    st = b.store.last_stats
                    if gather:
                        assert 0 < st["vectors_compared"] <= distinct * nq and st["path_used"] == int(Path.Exact), (where, st)
                        assert st["passes"] == (2 if nq == 16 else 1), (where, st)
                    else:
                        assert st["vectors_compared"] == b.n * nq, (where, st)
    b.store.set_option("id_gather", -1)


# ---- 2. MMR (W) ------------------------------------------------------------------------------------------------------------------

def case_mmr_reads_its_candidates_by_id_beyond_every_boundary(stores, name):
    """the mask is K, fetch_k 64, k 10: the first stage's 64 candidates lie in every window, and the pair kernel reads them by id"""
    b = stores.get(name)
    for metric in ALL_METRICS:
        take = TAKE[metric]
        for qi, lam in ((0, 0.5), (1, 0.0)):
            q = b.q_pool[qi]
            hits, counts, vals = MR.mmr(b.oracle, b.R, q, metric, take, 10, 64, lam, inv=b.inv)
            cand = MR.candidates(b.oracle, b.R, q, metric, take, 64, inv=b.inv)
            assert (b.K[cand["index"].astype(np.int64)] >= b.boundaries[-1]).any() and (b.K[cand["index"].astype(np.int64)] < b.boundaries[0]).any()
            got = TM.run(b.store, q, metric, take, 10, 64, lam, mask=b.mask)
            TM.check(got, (b.S(hits), counts, vals), (name, metric, qi, lam))


# ---- 3. recommend, all three strategies (W, S, P) ----------------------------------------------------------------------------------

def examples_of(b, rng, n_pos, n_neg):
    """compact ids of distinct examples: rows beside the boundaries first (both sides), then random rows of K"""
    c = list(dict.fromkeys(b.both_sides()[2:].tolist() + rng.choice(b.m, n_pos + n_neg, replace=False).tolist()))[: n_pos + n_neg]
    return c[:n_pos], c[n_pos:]


def case_recommend_three_strategies_fill_on(stores, name):
    """5 positives and 3 negatives (two passes of four slots) on both sides of the boundaries, one positive alone (the one-slot
    sweep).  best_score fills the negative side; sum_scores keeps a running sum in the 8-byte state; average_vector is ott_query
    itself with the model vector and one more mask"""
    b = stores.get(name)
    rng = np.random.default_rng(3)
    for metric in ALL_METRICS:
        take = TAKE[metric]
        for n_pos, n_neg in ((5, 3), (1, 0)):
            pos_c, neg_c = examples_of(b, rng, n_pos, n_neg)
            pos, neg = b.K[pos_c].tolist(), b.K[neg_c].tolist()
            P = RR.pair_scores(b.oracle, b.R, b.inv, pos_c + neg_c, metric)
            for k in (10, b.m):
                where = (name, metric, n_pos, n_neg, k)
                hits, side = RR.recommend(b.oracle, b.R, b.inv, pos_c, neg_c, metric, take, k, flags=RR.FILL, P=P)
                if n_neg and k == b.m:
                    assert (side == 0).any(), where  # the second round ran
                RR.same(TR.run(b.store, pos, neg, metric, take, k, fill=True, mask=b.mask), (b.S(hits), side), where + ("best_score",))
                sweep_stats(b.store.last_stats, b.n, n_pos + n_neg, where)
                hits, side = RS.sum_scores(b.oracle, b.R, b.inv, pos_c, neg_c, metric, take, k, P=P)
                RR.same(TS.run(b.store, pos, neg, metric, take, k, RecommendStrategy.SumScores, mask=b.mask), (b.S(hits), side), where + ("sum_scores",))
                sweep_stats(b.store.last_stats, b.n, n_pos + n_neg, where)
            hits, side = TS.average_model(b.oracle, b.R, b.inv, pos_c, neg_c, metric, take, 10)
            # (path AUTO answers a single query on a store this large through the cascade; EXACT is the sweep whose route is asserted)
            RR.same(TS.run(b.store, pos, neg, metric, take, 10, RecommendStrategy.AverageVector, mask=b.mask), (b.S(hits), side), (name, metric, n_pos, n_neg, "average_vector"))
            RR.same(TS.run(b.store, pos, neg, metric, take, 10, RecommendStrategy.AverageVector, mask=b.mask, path=Path.Exact), (b.S(hits), side), (name, metric, n_pos, n_neg, "average_vector, exact"))
            st = b.store.last_stats
            assert st["path_used"] == int(Path.Exact) and st["vectors_compared"] == b.n, st
            if name == "P" and metric in (Metric.Cosine, Metric.DotProduct):
                assert 0 < st["rescored"] < b.n, st  # the pruned sweep: only rows that passed the gate had their tails read
            else:  # Euclidean and Manhattan have no pruned sweep; W's 2048 floats are above exact_lean's 896; S's rows are one stage
                assert st["rescored"] == 0, st


# ---- 4. discover and context search (W, S) -----------------------------------------------------------------------------------------

def case_discover_and_context_search(stores, name):
    """3 pairs and a target: 7 slots, two passes; the target a stored row above the last boundary, a vector, or none"""
    b = stores.get(name)
    rng = np.random.default_rng(4)
    model = TD.Model(b.oracle, b.R, b.inv)
    ex_c, _ = examples_of(b, rng, 6, 0)
    ctx_c = [(ex_c[0], ex_c[1]), (ex_c[2], ex_c[3]), (ex_c[4], ex_c[5])]
    ctx = [(int(b.K[p]), int(b.K[g])) for p, g in ctx_c]
    above = int(LO.compact_of(b.K, [b.boundaries[-1] + 77])[0])
    assert above not in ex_c
    targets = (({"target_row": above}, {"target_row": int(b.K[above])}), ({"target": b.q_pool[3]},) * 2, ({}, {}))
    for metric in ALL_METRICS:
        take = TAKE[metric]
        for tgt_c, tgt in targets:
            for min_wins in (0, 2):
                for k in (25, b.m):
                    where = (name, metric, sorted(tgt), min_wins, k)
                    hits, wins = model(ctx_c, metric, take, k, min_wins=min_wins, **tgt_c)
                    assert hits.size and wins.min() >= min_wins, where
                    D.same(TD.run(b.store, ctx, metric, take, k, min_wins=min_wins, mask=b.mask, **tgt), (b.S(hits), wins), where)
                    sweep_stats(b.store.last_stats, b.n, 6 + (1 if tgt else 0), where)


# ---- 5. grouped search, m = 1 and m = 3 (W, N) -------------------------------------------------------------------------------------

def set_groups(b, div):
    """gid = row // div, dense already; (labels of the groups K touches, their compact dense ids per row of K)"""
    gid = (np.arange(b.n, dtype=np.int64) // div).astype(np.uint32)
    ng = int(gid[-1]) + 1
    b.store._set_dense_groups(gid, ng)
    labels, gid_c = np.unique(b.K // div, return_inverse=True)
    return ng, labels, gid_c.reshape(-1)


def grouped_case(b, metric, nq, k, m, labels, gid_c, where):
    keep = np.ones(b.m, bool)
    if m == 1:
        plan = G.build(b.store, b.q_pool[:nq], metric, k, perq=nq > 1, mask=b.mask)
        ref, ref_counts = G.expected(b.full(metric, G.take_of(metric, k), nq), gid_c, keep, plan.resolve().k, nq)
        got, counts = plan.collect_arrays()
        G.bits_equal(got, b.S(ref), where)
        assert list(counts) == ref_counts, where
    plan = GT.build(b.store, b.q_pool[:nq], metric, m, k, perq=nq > 1, mask=b.mask)
    ref, ref_counts, ref_groups = GR.expected(b.full(metric, GT.take_of(metric, k), nq), gid_c, keep, plan.resolve().k, nq, m)
    got, counts, groups = plan.collect_arrays()
    GR.bits_equal(got, b.S(ref), where)
    assert list(counts) == ref_counts, where
    assert groups.dtype == np.uint32 and np.array_equal(groups.astype(np.int64), labels[ref_groups.astype(np.int64)]), where
    sweep_stats(b.store.last_stats, b.n, nq, where)


def case_grouped_search_groups_of_four_straddle_every_boundary(stores, name):
    b = stores.get(name)
    try:
        ng, labels, gid_c = set_groups(b, 4)
        for metric in ALL_METRICS:
            for nq in (1, 5):
                for m in (1, 3):
                    if name == "N" and m == 3 and nq == 5:
                        continue  # 5 x 3 x 2^25 x 8 bytes: above the 2 GiB of ott_query_groups_top's table, refused (below)
                    for k in (10, None) if nq == 1 and metric == Metric.DotProduct and (name == "W" or m == 1) else (10,):
                        grouped_case(b, metric, nq, k, m, labels, gid_c, (name, metric, nq, m, k))
        if name == "N":
            grouped_case(b, Metric.Euclidean, 2, 10, 3, labels, gid_c, (name, "two queries x three levels: 1.5 GiB"))
            with pytest.raises(OttersError, match="above 2 GiB"):
                GT.build(b.store, b.q_pool[:5], Metric.DotProduct, 3, 10, perq=True, mask=b.mask).collect_arrays()
            grouped_case(b, Metric.DotProduct, 1, 10, 1, labels, gid_c, (name, "after the refusal"))
    finally:
        b.store.clear_groups()


def case_grouped_search_a_group_per_row_is_a_4_gib_table(stores, name):
    """N with gid = row: 2^27 groups, the (query, group) table of a four-query pass is 4 GiB"""
    b = stores.get(name)
    try:
        ng, labels, gid_c = set_groups(b, 1)
        assert ng == b.n
        for metric, nq in ((Metric.Cosine, 5), (Metric.Euclidean, 1), (Metric.DotProduct, 5), (Metric.Manhattan, 4)):
            grouped_case(b, metric, nq, 10, 1, labels, gid_c, ("N", "gid = row", metric, nq))
        with pytest.raises(OttersError, match="above 2 GiB"):
            GT.build(b.store, b.q_pool[:1], Metric.DotProduct, 3, 10, mask=b.mask).collect_arrays()
    finally:
        b.store.clear_groups()


# ---- 6. MaxSim: the sweep, the listed gather, the batched gather (W, N) ------------------------------------------------------------

def maxsim_ref(b, metric, nq, k, gid_c, ng_c, labels, listed_c=None, first=0):
    take = G.take_of(metric, k)
    full = b.full(metric, take, nq, first)
    keep = np.ones(b.m, bool)
    if listed_c is None:
        ref = MS.expected(full, gid_c, keep, k if k is not None else ng_c, nq, take, n_groups=ng_c)
    else:
        ref = MG.reference(full, gid_c, ng_c, keep, listed_c, k, nq, take)
    ref = ref.copy()
    ref["index"] = labels[ref["index"].astype(np.int64)]
    return ref


def case_maxsim_sweep_listed_gather_and_batch(stores, name):
    b = stores.get(name)
    rng = np.random.default_rng(6)
    try:
        ng, labels, gid_c = set_groups(b, 4)
        ng_c = labels.size
        builds = None
        for metric in ALL_METRICS:
            for nq in (1, 5):
                for k in (10, None) if metric == Metric.Cosine else (10,):
                    where = (name, metric, nq, k)
                    got, counts = MX.build(b.store, b.q_pool[:nq], metric, k, mask=b.mask).collect_arrays()
                    MX.bits_equal(got, maxsim_ref(b, metric, nq, k, gid_c, ng_c, labels), where + ("sweep",))
                    sweep_stats(b.store.last_stats, b.n, nq, where)
                # the listed gather: groups on both sides of every boundary, duplicates, both routes
                listed_c = np.concatenate([np.unique(gid_c[b.both_sides()]), rng.choice(ng_c, 60), rng.choice(ng_c, 5)])
                listed = labels[listed_c]
                ref = maxsim_ref(b, metric, nq, 10, gid_c, ng_c, labels, listed_c)
                assert ref.size == 10
                rows_listed = 4 * np.unique(listed).size  # (every group of the store has four rows)
                for route in MG.ROUTES:
                    got, st = MG.run(b.store, b.q_pool[:nq], metric, 10, listed, route, mask=b.mask)
                    MG.bits_equal(got, ref, (name, metric, nq, "listed", route))
                    assert st["vectors_compared"] == (rows_listed if route == MG.GATHER else b.n) * nq, (route, st)
                    builds = st["group_index_builds"]
            # the batch: three queries of 2, 5 and 1 tokens with lists of their own
            tokens, first = (2, 5, 1), (0, 2, 7)
            sets = [b.q_pool[a:a + t] for a, t in zip(first, tokens)]
            lists_c = [np.concatenate([np.unique(gid_c[b.both_sides()]), rng.choice(ng_c, 30)]), rng.choice(ng_c, 50), np.unique(gid_c[b.both_sides()])[::-1]]
            refs = [maxsim_ref(b, metric, tokens[i], 10, gid_c, ng_c, labels, lists_c[i], first[i]) for i in range(3)]
            for route in MB.ROUTES:
                got, counts, st = MB.run_batch(b.store, sets, metric, 10, [labels[l] for l in lists_c], route, mask=b.mask)
                MB.batch_equal(got, counts, refs, (name, metric, "batch", route))
                if route == MB.GATHER:
                    assert st["passes"] == 1 and st["vectors_compared"] == sum(4 * np.unique(l).size * t for l, t in zip(lists_c, tokens)), st
                else:
                    assert st["passes"] >= 3, st
        assert builds == 1
    finally:
        b.store.clear_groups()
        b.store.set_option("group_gather", -1)


def case_maxsim_above_the_index_limit_takes_the_mask_route(stores, name):
    """N with gid = row: 2^27 groups are above MG_INDEX_MAX_GROUPS = 2^26.  The group-to-rows index must not be built, a listed
    query with group_gather = 1 must still answer, by the mask route, with the model's bits; three tokens (four would make the
    (token, group) table 2 GiB + 4800 bytes, which ott_query_maxsim refuses)"""
    b = stores.get(name)
    rng = np.random.default_rng(7)
    try:
        ng, labels, gid_c = set_groups(b, 1)
        before = int(N.lib().ott_store_group_index_builds(b.store._handle()))
        listed_c = np.concatenate([b.both_sides(), rng.choice(b.m, 100)])
        for metric, nq in ((Metric.DotProduct, 3), (Metric.Manhattan, 1)):
            ref = maxsim_ref(b, metric, nq, 10, gid_c, b.m, labels, listed_c)
            for route in MG.ROUTES:
                got, st = MG.run(b.store, b.q_pool[:nq], metric, 10, labels[listed_c], route, mask=b.mask)
                MG.bits_equal(got, ref, ("N", "gid = row", metric, nq, route))
                assert st["vectors_compared"] == b.n * nq and st["group_index_builds"] == before, st
            got, _ = MX.build(b.store, b.q_pool[:nq], metric, 10, mask=b.mask).collect_arrays()
            MX.bits_equal(got, maxsim_ref(b, metric, nq, 10, gid_c, b.m, labels), ("N", "gid = row", metric, nq, "sweep"))
        with pytest.raises(OttersError, match="above 2 GiB"):
            MX.build(b.store, b.q_pool[:4], Metric.DotProduct, 10, mask=b.mask).collect_arrays()
    finally:
        b.store.clear_groups()
        b.store.set_option("group_gather", -1)


# ---- 7. the per-query masks sweep (W, N) -------------------------------------------------------------------------------------------

def case_masks_sweep_five_queries_a_mask_each(stores, name):
    """query b keeps K intersected with a different half of every window; query 4's mask is shorter than the store (the rows past it
    are kept), so K itself is the common mask; query 0's mask sits in a device mask slot in one of the runs"""
    b = stores.get(name)
    rng = np.random.default_rng(8)
    pos = np.concatenate([np.arange(c) for _, c in LO.runs_of(b.K)])  # a row's place in its window
    size = np.concatenate([np.full(c, c) for _, c in LO.runs_of(b.K)])
    halves = [pos < size // 2, pos >= size // 2, pos % 2 == 0, (pos // 64) % 2 == 1, rng.random(b.m) < 0.5]
    short = b.n - 60
    masks_c, masks = [], []
    for i, h in enumerate(halves):
        m = np.zeros(b.n if i != 4 else short, bool)
        rows = b.K[h]
        m[rows[rows < m.size]] = True
        masks.append(m)
        masks_c.append(h | (b.K >= m.size))  # (rows at and past a mask's end are kept; the common mask K still applies)
    assert (masks_c[4] & ~halves[4]).any()
    for metric in ALL_METRICS:
        take = TAKE[metric]
        exp = [b.S(h) for h in MKR.expected(b.oracle, b.R, b.q_pool[:5], masks_c, metric, take, 20)]
        for route in (TMK.SWEEP, TMK.LOOP):
            got, st = TMK.run(b.store, b.q_pool[:5], masks, metric, take, 20, route, common=b.mask)
            TMK.same(got, exp, (name, metric, route))
            assert st["passes"] == 2 if route == TMK.SWEEP else st["passes"] >= 5, (route, st)
            if route == TMK.SWEEP:
                assert st["vectors_compared"] == b.n * 5, st
    # query 0's mask from a device slot, the others from the host
    N.check(TMK.slot_write(b.store, 5, masks[0]))
    moq, qm = lower_row_masks(masks[1:])
    raw = (np.concatenate([[N.MASK_SLOT_BASE + 5], moq]).astype(np.uint32), qm)
    for route in (TMK.SWEEP, TMK.LOOP):
        got, st = TMK.run(b.store, b.q_pool[:5], masks, metric, take, 20, route, common=b.mask, raw=raw)
        TMK.same(got, exp, (name, metric, route, "slot"))
    N.check(N.lib().ott_store_clear_row_mask_slots(b.store._handle()))
    b.store.set_option("masks_sweep", 2)


# ---- 8. the sweeps unmasked, with planted rows (W, N) ------------------------------------------------------------------------------

METRIC_NAME = {Metric.Cosine: "cosine", Metric.Euclidean: "l2", Metric.DotProduct: "dot", Metric.Manhattan: "l1"}
# The cosine case (W only): 2^21 + 300 uniform rows against a sign vector, P(any cosine >= 0.5) <= LO.hoeffding_cosine_bound(
# 2^21 + 300, 2048, 0.5, 0.2) = 1.22e-16 (tests/test_large_offsets_cpu.py checks the figure); the planted rows' cosines are >= 0.914.


def planted_positions(b):
    """twelve rows at K's window edges: the store's first and last row, both sides of every boundary, then the windows' outer edges"""
    rows = [0, b.n - 1] + [r for x in b.boundaries for r in (x - 1, x)] + [r for x in b.boundaries for r in (x - HALF, x + HALF - 1)] + [HALF - 1, b.n - HALF]
    return np.array(sorted(rows[:12]), np.int64)


class Planted:
    """the store with twelve planted rows (and the example rows a kind needs) written, restored on exit; Kp: the rows of every
    four-row group that holds a written row — the model's compact rows"""

    def __init__(self, b, metric, extra=()):
        self.b, self.metric = b, metric
        self.at = planted_positions(b)
        self.query, rows = LO.planted(b.dim, 12, METRIC_NAME[metric], SEED)
        self.written = {int(r): rows[i] for i, r in enumerate(self.at)}
        for r, v in extra:
            assert int(r) not in self.written
            self.written[int(r)] = np.asarray(v, np.float32)
        self.Kp = np.unique(np.concatenate([np.arange(4) + 4 * (r // 4) for r in self.written]))

    def __enter__(self):
        b = self.b
        for r, v in self.written.items():
            b.store.write_rows(r, v[None, :])
        self.R = LO.window_rows(b.oracle, self.Kp, b.dim, SEED)
        for r, v in self.written.items():
            self.R[LO.compact_of(self.Kp, [r])[0]] = v
        self.inv = np.concatenate([b.store.inv_norms(a, c) for a, c in LO.runs_of(self.Kp)])
        self.planted_c = LO.compact_of(self.Kp, self.at)
        return self

    def __exit__(self, *exc):
        b = self.b
        for r in self.written:
            b.store.write_rows(r, b.oracle.rand_rows(r, 1, b.dim, SEED))
        for r in self.written:
            assert np.array_equal(b.store.rows(r, 1).view(np.uint32), b.oracle.rand_rows(r, 1, b.dim, SEED).view(np.uint32))
        return False

    def S(self, hits):
        return LO.to_store_index(self.Kp, hits)


def case_unmasked_sweeps_return_the_planted_rows(stores, name):
    """no mask: every tile of the store is read.  The top 12 rows (or groups) are the planted ones by construction
    (large_offsets.planted), in the model's order, with the bits of the model over the written rows' four-row groups alone"""
    b = stores.get(name)
    try:
        gid = (np.arange(b.n, dtype=np.int64) // 4).astype(np.uint32)  # every planted row in a group of its own, with three unplanted rows
        b.store._set_dense_groups(gid, int(gid[-1]) + 1)
        del gid
        for metric in (ALL_METRICS if name == "W" else NO_COSINE):
            take = TAKE[metric]
            q = LO.planted(b.dim, 12, METRIC_NAME[metric], SEED)[0]
            # recommend (best_score, sum_scores) and discover: the example row 1 is the query itself, row 2 its negative
            with Planted(b, metric, extra=((1, q), (2, -q))) as p:
                ex = LO.compact_of(p.Kp, [1, 2]).tolist()
                want = set(p.at.tolist())
                hits, side = RR.recommend(b.oracle, p.R, p.inv, ex[:1], [], metric, take, 12)
                assert set(p.S(hits)["index"].tolist()) == want
                RR.same(TR.run(b.store, [1], [], metric, take, 12), (p.S(hits), side), (name, metric, "best_score"))
                sweep_stats(b.store.last_stats, b.n, 1, (name, metric))
                hits, side = RS.sum_scores(b.oracle, p.R, p.inv, ex[:1], [], metric, take, 12)
                RR.same(TS.run(b.store, [1], [], metric, take, 12, RecommendStrategy.SumScores), (p.S(hits), side), (name, metric, "sum_scores"))
                model = TD.Model(b.oracle, p.R, p.inv)
                hits, wins = model([(ex[0], ex[1])], metric, take, 12, target=q)
                assert set(p.S(hits)["index"].tolist()) == want and (wins == 1).all()
                D.same(TD.run(b.store, [(1, 2)], metric, take, 12, target=q), (p.S(hits), wins), (name, metric, "discover"))
                sweep_stats(b.store.last_stats, b.n, 3, (name, metric))
            with Planted(b, metric) as p:
                want = set(p.at.tolist())
                labels, gid_c = np.unique(p.Kp // 4, return_inverse=True)
                gid_c = gid_c.reshape(-1)
                keep = np.ones(p.Kp.size, bool)
                for nq in (1, 5):
                    Q = np.repeat(q[None, :], nq, axis=0)
                    full = IL.ranking(b.oracle, p.R, Q, metric, take)
                    ref, ref_counts = G.expected(full, gid_c, keep, 12, nq)
                    assert set(p.S(ref)["index"][:12].tolist()) == want
                    got, counts = G.build(b.store, Q, metric, 12, perq=nq > 1).collect_arrays()
                    G.bits_equal(got, p.S(ref), (name, metric, nq, "one_per_group"))
                    sweep_stats(b.store.last_stats, b.n, nq, (name, metric, nq))
                    if not (name == "N" and nq == 5):  # (N: the table of 5 x 3 x 2^25 slots is refused, section 5)
                        ref, ref_counts, ref_groups = GR.expected(full, gid_c, keep, 12, nq, 3)
                        got, counts, groups = GT.build(b.store, Q, metric, 3, 12, perq=nq > 1).collect_arrays()
                        GR.bits_equal(got, p.S(ref), (name, metric, nq, "per_group(3)"))
                        assert list(counts) == ref_counts == [36] * nq and np.array_equal(groups.astype(np.int64), labels[ref_groups.astype(np.int64)])
                    nt = 1 if nq == 1 else 3  # tokens: the same vector three times, the sums are the model's
                    ref = MS.expected(IL.ranking(b.oracle, p.R, Q[:nt], metric, take), gid_c, keep, 12, nt, take, n_groups=labels.size).copy()
                    ref["index"] = labels[ref["index"].astype(np.int64)]
                    assert set(ref["index"].tolist()) == set((p.at // 4).tolist())
                    plan = b.store.query(Q[:nt], metric).max_sim()
                    got, _ = (plan.take_max(12) if take else plan.take_min(12)).collect_arrays()
                    MX.bits_equal(got, ref, (name, metric, nt, "maxsim"))
                    sweep_stats(b.store.last_stats, b.n, nt, (name, metric, nt))
                # the masks sweep with no mask at all: five queries, two passes over every tile
                Q = np.repeat(q[None, :], 5, axis=0)
                exp = [p.S(h) for h in MKR.expected(b.oracle, p.R, Q, [None] * 5, metric, take, 12)]
                assert set(exp[4]["index"].tolist()) == want
                got, st = TMK.run(b.store, Q, [None] * 5, metric, take, 12, TMK.SWEEP)
                TMK.same(got, exp, (name, metric, "masks sweep"))
                assert st["passes"] == 2 and st["vectors_compared"] == b.n * 5, st
    finally:
        b.store.clear_groups()
        b.store.set_option("masks_sweep", 2)


# ---- 9. deleted rows and compact() (W, N, P) ---------------------------------------------------------------------------------------

def case_deleted_rows_and_compact_move_every_window_across_a_boundary(stores, name):
    """the store's last case: it shrinks, and is closed behind it.  Rows [100, first boundary + 50) and every second row of the window at the third (W), second
    (N, P) boundary are deleted; under the mask K the survivors answer; compact() returns numpy's cumulative count for every row; the
    survivors, now at lower indices (every window behind the first has crossed a boundary downwards), answer the base query, an id
    list and a recommend call with the same bits"""
    b = stores.get(name)
    oracle, store, q_pool, K, R, inv_K, n = b.oracle, b.store, b.q_pool, b.K, b.R, b.inv, b.n
    try:
        bnd = SHAPES[name][2]
        second = bnd[2] if name == "W" else bnd[1]
        dead = np.concatenate([np.arange(100, bnd[0] + 50), np.arange(second - HALF, second + HALF, 2)])
        assert store.delete_rows(dead) == dead.size
        live = np.ones(n, bool)
        live[dead] = False
        live_c = live[K]
        mask = np.zeros(n, bool)
        mask[K] = True
        metric = Metric.DotProduct
        full = IL.ranking(oracle, R, q_pool[:1], metric, TAKE[metric])
        got, _ = store.query(q_pool[:1], metric).with_row_mask(mask).take(10).collect_arrays()
        IL.bits_equal(got, LO.to_store_index(K, IL.expected(full, live_c, 10, 1, False)[0]), (name, "deleted, masked"))
        new_index = store.compact()
        want = np.cumsum(live, dtype=np.int64) - 1
        want[~live] = -1
        assert new_index.dtype == np.int64 and np.array_equal(new_index, want), name
        del want
        n2 = int(live.sum())
        assert store.len() == store.live_len() == n2
        K2, R2 = new_index[K[live_c]], np.ascontiguousarray(R[live_c])
        moved = K[live_c] >= bnd[0] + 50  # every window behind the first: down by at least the block deleted in front of it
        assert K2[-1] == n2 - 1 and moved.sum() > K2.size - HALF and (K[live_c][moved] - K2[moved] >= bnd[0] - 50).all()
        del new_index, live
        inv2 = np.concatenate([store.inv_norms(a, c) for a, c in LO.runs_of(K2)])
        assert np.array_equal(inv2.view(np.uint32), inv_K[live_c].view(np.uint32))
        mask2 = np.zeros(n2, bool)
        mask2[K2] = True
        rng = np.random.default_rng(9)
        for metric in ALL_METRICS:
            take = TAKE[metric]
            full = IL.ranking(oracle, R2, q_pool[:1], metric, take)
            keep = np.ones(K2.size, bool)
            ref = LO.to_store_index(K2, IL.expected(full, keep, 10, 1, False)[0])
            got, _ = store.query(q_pool[:1], metric).with_row_mask(mask2).take(10).collect_arrays()
            IL.bits_equal(got, ref, (name, metric, "compacted, base query"))
            got, _ = store.query(q_pool[:1], metric).with_row_mask(mask2).take(10).with_path(Path.Exact).collect_arrays()
            IL.bits_equal(got, ref, (name, metric, "compacted, base query, exact"))
            st = store.last_stats
            assert st["path_used"] == int(Path.Exact), st
            if name == "P" and metric in (Metric.Cosine, Metric.DotProduct):
                assert 0 < st["rescored"] < n2, st  # still the pruned sweep: the sketch lines and heads moved with the rows
            else:
                assert st["rescored"] == 0, st
            ids_c = rng.choice(K2.size, 200)
            for gather in (1, 0):
                store.set_option("id_gather", gather)
                got, _ = IL.build(store, q_pool[:1], metric, 10, Path.Auto, False, ids=K2[ids_c]).collect_arrays()
                IL.bits_equal(got, LO.to_store_index(K2, IL.expected(full, IL.id_mask(K2.size, ids_c), 10, 1, False)[0]), (name, metric, "compacted, id list", gather))
            c = rng.choice(K2.size, 8, replace=False).tolist()
            hits, side = RR.recommend(oracle, R2, inv2, c[:5], c[5:], metric, take, 10, flags=RR.FILL)
            RR.same(TR.run(store, K2[c[:5]].tolist(), K2[c[5:]].tolist(), metric, take, 10, fill=True, mask=mask2), (LO.to_store_index(K2, hits), side), (name, metric, "compacted, recommend"))
            sweep_stats(store.last_stats, n2, 8, (name, metric))
    finally:
        stores.drop()


# ---- the cases in the stores' order: one store is alive at a time --------------------------------------------------------------------

def test_w_id_lists_and_score_rows(stores):
    case_id_lists_both_routes_and_score_rows(stores, "W")


def test_w_mmr(stores):
    case_mmr_reads_its_candidates_by_id_beyond_every_boundary(stores, "W")


def test_w_recommend(stores):
    case_recommend_three_strategies_fill_on(stores, "W")


def test_w_discover(stores):
    case_discover_and_context_search(stores, "W")


def test_w_grouped_search(stores):
    case_grouped_search_groups_of_four_straddle_every_boundary(stores, "W")


def test_w_maxsim(stores):
    case_maxsim_sweep_listed_gather_and_batch(stores, "W")


def test_w_masks_sweep(stores):
    case_masks_sweep_five_queries_a_mask_each(stores, "W")


def test_w_unmasked_with_planted_rows(stores):
    case_unmasked_sweeps_return_the_planted_rows(stores, "W")


def test_w_deleted_rows_and_compact(stores):
    case_deleted_rows_and_compact_move_every_window_across_a_boundary(stores, "W")


def test_n_id_lists_and_score_rows(stores):
    case_id_lists_both_routes_and_score_rows(stores, "N")


def test_n_grouped_search(stores):
    case_grouped_search_groups_of_four_straddle_every_boundary(stores, "N")


def test_n_grouped_search_a_group_per_row(stores):
    case_grouped_search_a_group_per_row_is_a_4_gib_table(stores, "N")


def test_n_maxsim(stores):
    case_maxsim_sweep_listed_gather_and_batch(stores, "N")


def test_n_maxsim_above_the_index_limit(stores):
    case_maxsim_above_the_index_limit_takes_the_mask_route(stores, "N")


def test_n_masks_sweep(stores):
    case_masks_sweep_five_queries_a_mask_each(stores, "N")


def test_n_unmasked_with_planted_rows(stores):
    case_unmasked_sweeps_return_the_planted_rows(stores, "N")


def test_n_deleted_rows_and_compact(stores):
    case_deleted_rows_and_compact_move_every_window_across_a_boundary(stores, "N")


def test_s_recommend(stores):
    case_recommend_three_strategies_fill_on(stores, "S")


def test_s_discover(stores):
    case_discover_and_context_search(stores, "S")


def test_p_recommend(stores):
    case_recommend_three_strategies_fill_on(stores, "P")


def test_p_deleted_rows_and_compact(stores):
    case_deleted_rows_and_compact_move_every_window_across_a_boundary(stores, "P")
