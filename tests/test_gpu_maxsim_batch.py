"""GPU: MaxSim re-ranking in batches (ott_query_maxsim_groups_batch, VecStore.max_sim_batch).  Bar: for every query b
of a batch the hits — dense group id, score bits of the sum, order — are those of tests/maxsim_ref.py over the full canonical ranking
of query b's own tokens with `keep` ANDed with "the row's group is in query b's list" (test_gpu_maxsim_groups.py::reference), with
query = b, and they are the hits of the single call ott_query_maxsim_groups for that query.  Both routes (option group_gather = 1:
the batched gather kernel; 0: the loop over the single call's mask route) are held to the reference and therefore to each other.  Bit
for bit, no tolerances.  The shapes are the smallest that reach each mechanism."""
import ctypes as C

import numpy as np
import pytest

import ieee_edges as E
import maxsim_ref as R
import test_gpu_groups as G
from otters_amd import Cmp, Metric, OttersError, VecStore
from otters_amd import _native as N
from test_gpu_maxsim_groups import dense, lists_of, reference
from test_gpu_maxsim_groups import run as run_single

pytestmark = pytest.mark.gpu

ALL_METRICS = G.ALL_METRICS
GATHER, LOOP = 1, 0
ROUTES = (GATHER, LOOP)


def run_batch(store, token_sets, metric, k, lists_of_labels, route, mask=None, flt=None, chunk_mask=None, device_mask=False):
    """(hits, counts, stats) of a batch plan on one route"""
    store.set_option("group_gather", route)
    p = store.max_sim_batch(token_sets, metric).with_groups(lists_of_labels)
    if mask is not None:
        p = p.with_row_mask(mask)
    if flt is not None:
        p = p.filter(*flt)
    if k is not None:
        p = p.take(k)
    return store._run_maxsim_batch(p.resolve(), chunk_mask=chunk_mask, use_device_row_mask=device_mask)


def batch_equal(got, counts, refs, where):
    """the lists back to back in query order, query = b, n_per_query their lengths"""
    assert list(counts) == [r.size for r in refs], (where, list(counts), [r.size for r in refs])
    assert got.size == sum(counts), (where, got.size, counts)
    at = 0
    for b, ref in enumerate(refs):
        part = got[at:at + ref.size]
        at += ref.size
        assert np.array_equal(part["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, b, part["index"][:12], ref["index"][:12])
        assert np.array_equal(part["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, b, part["score"][:12], ref["score"][:12])
        assert (part["query"] == b).all(), (where, b, part["query"][:12])


def batch_reference(fulls, token_sets, gid, ng, keep, lists, k, take, cmp=0, thr=0.0):
    """per query the single query's reference; k = None is the plan's default take, the largest number of distinct listed groups"""
    if k is None:
        k = max(np.unique(np.asarray(l, np.int64)).size for l in lists)
    return [reference(fulls[b], gid, ng, keep, lists[b], k, token_sets[b].shape[0], take, cmp, thr) for b in range(len(lists))]


def listed_rows(gid, listed):
    return int(np.isin(gid, np.asarray(listed, np.int64)).sum())


TOKENS = (1, 3, 8, 9, 32)  # one batch mixes them: NT = 32, the narrower queries' blocks are zero padded


def token_sets_of(pool, counts=TOKENS):
    at = np.concatenate([[0], np.cumsum(counts)])
    return [pool[at[i]:at[i + 1]] for i in range(len(counts))]


# ---- 1. small store ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 40])
def test_small_store_every_metric_layout_token_count_list_k_and_route(oracle, dim):
    """300 rows; dims cover tail only (1, 3, 7), chains only (8, 40) and both (9).  Every batch holds five queries of 1, 3, 8, 9 and 32
    tokens with the five lists (empty, one group, every group, unsorted with duplicates, half; "every group" shares its groups with
    all others), assigned to the queries in a rotating order; k rotates through 1, 10, 64, 65 and no take over (layout, metric), so
    every metric meets every k and both takes (take(k) infers Min / Max from the metric, no take ranks by Max)"""
    rng = np.random.default_rng(12100 + dim)
    n = 300
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    sets = token_sets_of(rng.uniform(-1, 1, (sum(TOKENS), dim)).astype(np.float32))
    store = VecStore(dim)
    store.add_vectors(rows)
    keep = np.ones(n, bool)
    fulls = {}
    ks = (1, 10, 64, 65, None)
    turn = 0
    for lname, labels in G.layouts(rng, n).items():
        store.set_groups(labels)
        gid, uniq = dense(labels), np.unique(labels)
        ng = uniq.size
        named = list(lists_of(rng, ng).items())
        for metric in ALL_METRICS:
            k = ks[turn % len(ks)]
            order = [named[(i + turn) % 5] for i in range(5)]
            turn += 1
            lists = [l for _, l in order]
            take = G.take_of(metric, k)
            if (metric, take) not in fulls:
                fulls[(metric, take)] = [R.ranking(oracle, rows, t, metric, take) for t in sets]
            refs = batch_reference(fulls[(metric, take)], sets, gid, ng, keep, lists, k, take)
            where = (lname, metric, k, [name for name, _ in order])
            for route in ROUTES:
                got, counts, st = run_batch(store, sets, metric, k, [uniq[l] for l in lists], route)
                batch_equal(got, counts, refs, where + (route,))
                if route == GATHER:
                    assert st["passes"] == 1 and st["path_used"] == 1, st
                    assert st["vectors_compared"] == sum(listed_rows(gid, l) * t.shape[0] for l, t in zip(lists, sets)), st
            # ... and the single call, query by query (its own default take is the query's own distinct count: the batch's k is named)
            k_named = k if k is not None else max(np.unique(l).size for l in lists)
            store.set_option("group_gather", GATHER)
            for b in range(5):
                p = store.query(sets[b], metric).max_sim().with_groups(uniq[lists[b]])
                p = p.take(k_named) if k is not None else p.take_max(k_named)
                single = store._run(p.resolve())[0]
                assert single.size == refs[b].size and np.array_equal(single["index"], refs[b]["index"].astype(np.uint64)), (where, b)
                assert np.array_equal(single["score"].view(np.uint32), refs[b]["score"].view(np.uint32)), (where, b)
    store.close()


# ---- 2. a batch of one --------------------------------------------------------------------------------------------------------------

def test_a_batch_of_one_is_the_single_call_and_short_lists_return_what_they_have(oracle):
    rng = np.random.default_rng(12200)
    n, dim, ng = 300, 9, 38
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    gid = np.arange(n) // 8
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    listed = np.array([30, 2, 9, 9, 17, 2, 31, 4])
    for metric in (Metric.Cosine, Metric.Manhattan):
        for k in (3, 10, None):  # 6 distinct groups: k = 10 returns 6
            for route in ROUTES:
                single, _ = run_single(store, q, metric, k, listed, route)
                got, counts, _ = run_batch(store, [q], metric, k, [listed], route)
                assert counts == [single.size] and single.size == min(k or 6, 6)
                assert got.tobytes() == single.tobytes(), (metric, k, route)  # every field, query = b = 0 included
    # three queries, k = 10: 6, 1 and 0 distinct groups return 6, 1 and 0 hits
    full = [R.ranking(oracle, rows, t, Metric.Cosine, 1) for t in (q[:3], q[3:4], q[4:])]
    lists = [listed, np.array([37, 37]), np.zeros(0, np.int64)]
    refs = batch_reference(full, [q[:3], q[3:4], q[4:]], gid, ng, np.ones(n, bool), lists, 10, 1)
    for route in ROUTES:
        got, counts, _ = run_batch(store, [q[:3], q[3:4], q[4:]], Metric.Cosine, 10, lists, route)
        batch_equal(got, counts, refs, route)
        assert counts == [6, 1, 0]
    # all lists empty: a valid batch with no hits
    got, counts, _ = run_batch(store, [q[:3], q[3:]], Metric.Cosine, None, [[], []], GATHER)
    assert got.size == 0 and counts == [0, 0]
    store.close()


# ---- 3. more slots than the grid holds ------------------------------------------------------------------------------------------------

def test_workgroups_walk_several_slots_and_cross_query_boundaries(oracle):
    """3 000 rows of dim 8 in 600 groups of uneven size, some emptied by deletes; 40 queries of 1 .. 4 tokens.  Query 0 lists every
    group, the others 150 each: 6 450 slots against 256 CUs x 8 = 2 048 workgroups, so a workgroup walks several slots and ranges
    cross query boundaries.  No take: k = 600 = the largest distinct count, above 512, so the ONE top-k takes the sort path over 40
    tables at stride 600 (150 listed groups alone would stay on the register lists); take(10): the select / merge path"""
    rng = np.random.default_rng(12300)
    n, dim, ng, B = 3000, 8, 600, 40
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    gid = np.minimum((rng.random(n) ** 2 * ng).astype(np.int64), ng - 1)  # uneven: low ids hold many rows
    gid[:ng] = np.arange(ng)
    sizes = [1 + b % 4 for b in range(B)]
    sets = token_sets_of(rng.uniform(-1, 1, (sum(sizes), dim)).astype(np.float32), sizes)
    lists = [rng.permutation(ng)] + [rng.choice(ng, 150, replace=False) for _ in range(B - 1)]
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    dead = np.flatnonzero(np.isin(gid, [3, 77, 599, 300]))  # four groups lose every row
    assert store.delete_rows(dead) == dead.size
    alive = np.ones(n, bool)
    alive[dead] = False
    fulls = [R.ranking(oracle, rows, t, Metric.Cosine, 1) for t in sets]
    for k in (None, 10):
        refs = batch_reference(fulls, sets, gid, ng, alive, lists, k, 1)
        assert refs[0].size == (596 if k is None else 10)
        got, counts, st = run_batch(store, sets, Metric.Cosine, k, lists, GATHER)
        batch_equal(got, counts, refs, ("gather", k))
        assert st["passes"] == 1 and st["vectors_compared"] == sum(listed_rows(gid, l) * t.shape[0] for l, t in zip(lists, sets))
    got, counts, _ = run_batch(store, sets, Metric.Cosine, 10, lists, LOOP)
    batch_equal(got, counts, batch_reference(fulls, sets, gid, ng, alive, lists, 10, 1), "loop")
    store.close()


# ---- 4. masks ---------------------------------------------------------------------------------------------------------------------

def test_row_mask_device_mask_chunk_mask_deleted_rows_and_the_filter(oracle):
    n, dim, cs, ng = 300, 40, 64, 38
    rng = np.random.default_rng(12400)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    sets = token_sets_of(rng.uniform(-1, 1, (10, dim)).astype(np.float32), (5, 2, 3))
    gid = np.arange(n) // 8
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_chunk_size(cs)
    store.set_groups(gid)
    caller = rng.random(n) < 0.5
    caller[16:40] = False      # groups 2, 3, 4 lose every row
    caller[40:47] = False      # group 5 keeps one row
    caller[47] = True
    dead = np.unique(np.concatenate([np.arange(80, 88), rng.choice(n, 30)]))  # group 10 deleted entirely, others thinned
    alive = np.ones(n, bool)
    alive[dead] = False
    chunks = np.array([True, False, True, True, False])  # rows 64 .. 127 and 256 .. 299 are never scored
    in_chunk = np.repeat(chunks, cs)[:n]
    # groups 2 and 3 are masked out entirely: query 0 and query 2 list them; query 1 lists neither but shares 12 and 20 with query 0
    lists = [np.array([2, 3, 5, 10, 12, 20, 37, 33, 9, 8, 1, 15, 5]), np.array([12, 20, 36, 0]), np.array([3, 2, 10, 37, 4, 11, 30])]
    # the evaluated device mask: an int32 column, "value < 150" (the mask every query with use_device_row_mask reads)
    col = rng.integers(0, 300, n).astype(np.int32)
    cid = C.c_uint32(0)
    N.check(N.lib().ott_store_add_column(store._handle(), 0, N.ptr(col), None, n, C.byref(cid)))
    leaf = N.Leaf()
    leaf.column, leaf.op, leaf.clause, leaf.lit_i64 = cid.value, 2, 0, 150  # Lt
    N.check(N.lib().ott_store_eval_row_mask(store._handle(), (N.Leaf * 1)(leaf), 1, 1, None))
    device = col < 150

    for metric in (Metric.Cosine, Metric.Euclidean):
        take = G.TAKE[metric]
        fulls = [R.ranking(oracle, rows, t, metric, take) for t in sets]
        ref = lambda keep, k, cmp=0, thr=0.0: batch_reference(fulls, sets, gid, ng, keep, lists, k, take, cmp, thr)  # noqa: E731
        sums = np.sort(np.concatenate([r["score"] for r in ref(np.ones(n, bool), ng)]))
        thr = float(sums[sums.size // 2])
        for route in ROUTES:
            for k in (1, 10):
                got, counts, _ = run_batch(store, sets, metric, k, lists, route, mask=caller)
                batch_equal(got, counts, ref(caller, k), ("row mask", metric, k, route))
                if k == 10:
                    assert not np.isin(got["index"], [2, 3]).any() and 5 in got["index"]  # every row masked: dropped in both queries; one row left: kept
                got, counts, _ = run_batch(store, sets, metric, k, lists, route, device_mask=True)
                batch_equal(got, counts, ref(device, k), ("device mask", metric, k, route))
                got, counts, _ = run_batch(store, sets, metric, k, lists, route, chunk_mask=chunks)
                batch_equal(got, counts, ref(in_chunk, k), ("chunk mask", metric, k, route))
                for cmp in (Cmp.Gt, Cmp.Lte):  # the filter applies to the sum
                    got, counts, _ = run_batch(store, sets, metric, k, lists, route, flt=(thr, cmp))
                    batch_equal(got, counts, ref(np.ones(n, bool), k, int(cmp), thr), ("filter", metric, k, cmp, route))
                    assert R.holds(got["score"], int(cmp), thr).all()
            assert store.delete_rows(dead) == dead.size
            for k in (1, 10):
                got, counts, _ = run_batch(store, sets, metric, k, lists, route)
                batch_equal(got, counts, ref(alive, k), ("deleted", metric, k, route))
                assert 10 not in got["index"]
                got, counts, _ = run_batch(store, sets, metric, k, lists, route, mask=caller, chunk_mask=chunks, flt=(thr, Cmp.Gt))
                batch_equal(got, counts, ref(alive & caller & in_chunk, k, int(Cmp.Gt), thr), ("all", metric, k, route))
            assert store.restore_rows(dead) == dead.size
    store.close()


# ---- 5. IEEE edge rows -------------------------------------------------------------------------------------------------------------

def test_ieee_edge_rows_nan_inf_and_signed_zeros(oracle):
    """tests/ieee_edges.py families a (signed-zero cosines) and c (dots that overflow to +-inf, inf - inf = NaN pairs that are dropped),
    plus planted rows: a group whose bests are +inf and -inf (a NaN sum: dropped), a group of NaN rows only (no score at all), and -0.0
    sums that must stay -0.0"""
    rng = np.random.default_rng(12500)
    for family, metrics in ((E.signed_zero_cosines, (Metric.Cosine, Metric.DotProduct)), (E.overflow, (Metric.DotProduct, Metric.Euclidean, Metric.Manhattan))):
        rows, q, _ = family(rng)
        n, dim = rows.shape
        gid = np.arange(n) // 4
        ng = int(gid.max()) + 1
        sets = [q[:1], q[1:], q, q[::-1].copy()]
        lists = [np.arange(ng), rng.permutation(ng)[: ng // 2], np.array([ng - 1, 0, ng - 2, 0]), np.arange(ng)[::-1]]
        store = VecStore(dim)
        store.add_vectors(rows)
        store.set_groups(gid)
        for metric in metrics:
            for k in (3, None):
                take = G.take_of(metric, k)
                fulls = [R.ranking(oracle, rows, t, metric, take) for t in sets]
                refs = batch_reference(fulls, sets, gid, ng, np.ones(n, bool), lists, k, take)
                for route in ROUTES:
                    got, counts, _ = run_batch(store, sets, metric, k, lists, route)
                    batch_equal(got, counts, refs, (family.__name__, metric, k, route))
        store.close()
    # planted: test_gpu_maxsim_groups.py's construction
    n, dim = 200, 8
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    rows[40:44] = 0.0
    rows[40, 0] = np.inf       # token 0 (only its first element set): best +inf
    rows[41, 1] = -np.inf      # token 1 (only its second element set): row 40 gives NaN, row 41 -inf
    rows[20:24] = np.nan       # group 5: only NaN rows
    rows[60:64] = np.float32(-1e30)  # group 15: the norm overflows, cosine -0.0 against positive tokens
    gid = np.arange(n) // 4
    two = np.zeros((2, dim), np.float32)
    two[0, 0], two[1, 1] = 1.0, 1.0
    pos = (np.abs(rng.uniform(-1, 1, (2, dim))) + 1).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    pm = np.zeros(n, bool)     # of group 10 only rows 40 and 41 are kept, of group 30 none
    pm[40:42] = True
    pm[100:104] = True
    pm[20:24] = True
    cases = ((Metric.DotProduct, [two, two[:1]], [np.array([25, 10, 5, 30]), np.array([10, 5, 25])], pm),
             (Metric.Cosine, [pos, pos[:1]], [np.array([15, 30]), np.array([15])], np.ones(n, bool)))
    for metric, sets, lists, keep in cases:
        fulls = [R.ranking(oracle, rows, t, metric, 1) for t in sets]
        refs = batch_reference(fulls, sets, gid, 50, keep, lists, None, 1)
        for route in ROUTES:
            got, counts, _ = run_batch(store, sets, metric, None, lists, route, mask=keep)
            batch_equal(got, counts, refs, (metric, route))
            if metric == Metric.DotProduct:
                assert got[:counts[0]]["index"].tolist() == [25]  # group 10: +inf + -inf, a NaN sum; group 5: no score at all; group 30: no row survives
                assert got[counts[0]:]["index"].tolist() == [10, 25] and np.isposinf(got[counts[0]]["score"])  # one token: +inf is a sum like any other
            else:
                assert got[got["index"] == 15]["score"].view(np.uint32).tolist() == [0x80000000, 0x80000000]  # -0.0 + -0.0, and -0.0
    store.close()


# ---- 6. the loop route, forced by shape ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim, tokens, per_pass", [(40, (33, 3), 32), (520, (17, 2), 16), (2056, (3, 2), 0)])
def test_shapes_the_batched_gather_does_not_serve_take_the_loop(oracle, dim, tokens, per_pass):
    """64 rows, option group_gather = 1: 33 tokens at dim 40 and 17 at a padded dim of 520 are more than one pass holds, 2056 floats are
    past the kernel's LDS (no index, the mask route).  The batch still answers, query by query; `passes` is the sum of the queries'"""
    rng = np.random.default_rng(12600 + dim)
    n = 64
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    sets = token_sets_of(rng.uniform(-1, 1, (sum(tokens), dim)).astype(np.float32), tokens)
    gid = rng.integers(0, 9, n)
    gid[:9] = np.arange(9)
    lists = [np.array([7, 1, 3, 8, 1]), np.arange(9)]
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    for metric in (Metric.Cosine, Metric.Manhattan):
        for k in (4, None):
            take = G.take_of(metric, k)
            fulls = [R.ranking(oracle, rows, t, metric, take) for t in sets]
            refs = batch_reference(fulls, sets, gid, 9, np.ones(n, bool), lists, k, take)
            got, counts, st = run_batch(store, sets, metric, k, lists, GATHER)
            batch_equal(got, counts, refs, (dim, metric, k))
            singles = [run_single(store, t, metric, k if k is not None else 9, l, GATHER)[1] for t, l in zip(sets, lists)]
            assert st["passes"] == sum(s["passes"] for s in singles) and st["path_used"] == 1, (st, singles)
            assert st["vectors_compared"] == sum(s["vectors_compared"] for s in singles) and st["bytes_scanned"] == sum(s["bytes_scanned"] for s in singles)
            if per_pass:
                assert st["passes"] == sum(-(-t // per_pass) for t in tokens) == 3
    assert st["group_index_builds"] == (1 if per_pass else 0)
    store.close()


# ---- 7. refusals that need a store, 8. the index's life cycle -----------------------------------------------------------------------------

def raw_batch(store, q, tokens, lists, k, cap):
    """straight at the C ABI: (status, message, out, n_out, per)"""
    d = N.QueryDesc()
    qq = np.ascontiguousarray(q, np.float32)
    g = np.ascontiguousarray(np.concatenate(lists), np.uint32)
    tok, listed = np.array(tokens, np.uint32), np.array([len(l) for l in lists], np.uint64)
    d.queries, d.nq, d.metric, d.take, d.k = qq.ctypes.data, qq.shape[0], int(Metric.Cosine), 1, k
    out = np.zeros(max(cap, 1), N.HIT_DTYPE)
    out["index"] = 12345
    n_out, per = C.c_uint64(77), np.full(len(lists), 77, np.uint64)
    rc = N.lib().ott_query_maxsim_groups_batch(store._handle(), C.byref(d), N.ptr(tok), N.ptr(listed), len(lists), N.ptr(g), N.ptr(out), cap, C.byref(n_out), N.ptr(per), None)
    return rc, N.lib().ott_last_error(), out, n_out.value, per


def test_refusals_that_need_a_store_and_the_index_is_built_once(oracle):
    n, dim = 300, 8
    rng = np.random.default_rng(12700)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (6, dim)).astype(np.float32)
    gid = np.arange(n) // 8
    sets, lists = [q[:3], q[3:4], q[4:]], [np.array([3, 30, 11]), np.array([4, 9, 4]), np.array([36, 0])]
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(gid)
    builds = lambda: int(N.lib().ott_store_group_index_builds(store._handle()))  # noqa: E731
    assert builds() == 0
    # refused before any device work: nothing is built and nothing is written
    rc, msg, out, n_out, per = raw_batch(store, q, [3, 1, 2], [lists[0], lists[1], np.array([36, 38])], 5, 16)
    assert rc == -1 and b"ott_query_maxsim_groups_batch: query 2: group 38 is out of range (the store holds 38 groups)" in msg
    assert builds() == 0 and n_out == 77 and (per == 77).all() and (out["index"] == 12345).all()
    store.set_option("group_gather", GATHER)
    rc, msg, out, n_out, per = raw_batch(store, q, [3, 1, 2], lists, 5, 6)  # k_eff = 3 + 2 + 2
    assert rc == -1 and b"ott_query_maxsim_groups_batch: output capacity is smaller than the sum over the queries of min(k, distinct listed groups)" in msg
    assert n_out == 77 and (per == 77).all() and (out["index"] == 12345).all()
    rc, msg, out, n_out, per = raw_batch(store, q, [3, 1, 2], lists, 5, 7)
    assert rc == 0 and n_out == 7 and per.tolist() == [3, 2, 2] and out["query"].tolist() == [0, 0, 0, 1, 1, 2, 2]
    # the life cycle: the first batch after set_groups builds the index in its clean step, the next finds it there
    assert builds() == 1
    fulls = [R.ranking(oracle, rows, t, Metric.Cosine, 1) for t in sets]
    refs = batch_reference(fulls, sets, gid, 38, np.ones(n, bool), lists, None, 1)
    got, counts, st = run_batch(store, sets, Metric.Cosine, None, lists, GATHER)
    batch_equal(got, counts, refs, "found")
    assert st["group_index_builds"] == 1 == builds()
    store.set_groups(gid)
    assert builds() == 1
    store.max_sim_batch(sets, Metric.Cosine).with_groups(lists).collect()
    assert store.last_stats["group_index_builds"] == 2
    res = store.max_sim_batch(sets, Metric.Cosine).with_groups(lists).collect()
    assert store.last_stats["group_index_builds"] == 2
    assert [[(r.index, np.float32(r.score).view(np.uint32)) for r in l] for l in res] == [[(int(h["index"]), h["score"].view(np.uint32)) for h in r] for r in refs]
    store.clear_groups()
    rc, msg, *_ = raw_batch(store, q, [3, 1, 2], lists, 5, 16)
    assert rc == -1 and b"ott_query_maxsim_groups_batch: no group ids are set" in msg
    store.close()
    multi = VecStore(dim, devices=[0, 0])
    multi.add_vectors(rows)
    multi.set_groups(gid)
    with pytest.raises(OttersError, match="ott_query_maxsim_groups_batch: a multi-GPU store is not served") as e:
        run_batch(multi, sets, Metric.Cosine, 5, lists, GATHER)
    assert e.value.status == -4
    multi.close()
