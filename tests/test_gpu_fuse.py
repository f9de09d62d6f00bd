"""GPU: rank fusion (ott_query_fuse, VecStore.fuse, MetaStore.fuse) against the numpy model (tests/fuse_ref.py) fed
with the ORACLE's leg lists.  Bar: index, F's f32 bits, order, counts and `query`, no tolerances.

Stores hold 200 to 3000 rows of dims 8, 33 and 128 with integer elements in -2..2, so exact score ties are frequent (inside a leg:
the canonical order decides the positions RRF reads; between rows: equal F goes to the lower row).  Where the first stage runs under
a tie order of its own (tie_order 1, 2: the host route), the model is fed with the library's own ott_query lists, which are held
to the oracle's literal collector the way tests/test_gpu_ties.py holds them."""
import ctypes as C
import threading

import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as R
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
FUSIONS = (R.RRF, R.DBSF, R.MINMAX)
ROUTE = -1


@pytest.fixture(params=[0, 1], ids=["host_route", "device_route"], autouse=True)
def route(request):
    """every test runs on both routes (option fuse_device); the tests about the routes set the option themselves"""
    global ROUTE
    ROUTE = request.param
    return ROUTE


def quantised(rng, shape):
    a = rng.integers(-2, 3, shape).astype(np.float32)
    flat = a.reshape(-1, a.shape[-1])
    flat[np.all(flat == 0, axis=1)] = 1.0
    return a


def make(dim, n, seed=0, rows=None):
    rng = np.random.default_rng(7000 + 10 * dim + seed)
    if rows is None:
        rows = quantised(rng, (n, dim))
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_option("fuse_device", ROUTE)
    return store, rows, rng, store.inv_norms()


def plan_of(store, sets, metric, fusion, k, fetch=None, take=None, rrf_k=60.0, weights=None, flt=None, mask=None, path=None):
    p = store.fuse(sets, metric)
    p = p.take_max(k) if (TAKE[metric] if take is None else take) == 1 else p.take_min(k)
    p = p.rrf(rrf_k) if fusion == R.RRF else p.dbsf() if fusion == R.DBSF else p.min_max()
    if fetch is not None:
        p = p.fetch(fetch)
    if weights is not None:
        p = p.weights(weights)
    if flt is not None:
        p = p.filter(*flt)
    if mask is not None:
        p = p.with_row_mask(mask)
    if path is not None:
        p = p.with_path(path)
    return p


def expect(oracle, rows, inv, sets, metric, fusion, k, fetch, take=None, rrf_k=60.0, weights=None, flt=None, mask=None, base=0, lists=None):
    take = TAKE[metric] if take is None else take
    if lists is None:
        cmp, thr = (0, 0.0) if flt is None else (int(flt[1]), flt[0])
        lists = R.leg_lists(oracle, rows, np.concatenate(sets), metric, take, min(fetch, rows.shape[0]), cmp, thr, mask, inv=inv, base=base)
    flat = None if weights is None else [x for w in weights for x in w]
    return R.fuse(lists, [len(s) for s in sets], fusion, take, k, rrf_k, flat)


def same(got, exp, where):
    (gh, gc), (eh, ec) = got, exp
    assert list(gc) == list(ec), (where, list(gc), list(ec))
    assert np.array_equal(gh["index"], eh["index"]), (where, gh["index"][:12], eh["index"][:12])
    assert np.array_equal(gh["score"].view(np.uint32), eh["score"].view(np.uint32)), (where, gh["score"][:12], eh["score"][:12])
    assert np.array_equal(gh["query"], eh["query"]), where


def sets_of(rng, dim, legs):
    return [quantised(rng, (l, dim)) for l in legs]


# ---- fusions, metrics, takes, dims ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [8, 33, 128])
def test_every_fusion_metric_and_take(oracle, dim):
    store, rows, rng, inv = make(dim, 1000)
    sets = sets_of(rng, dim, (1, 3, 2))
    weights = [[1.0], [0.5, -1.5, 2.0], [0.0, 3.0]]
    for metric in TAKE:
        for take in (0, 1):
            for fusion in FUSIONS:
                for w in (None, weights):
                    got = plan_of(store, sets, metric, fusion, 9, 7, take, weights=w).collect_arrays()
                    same(got, expect(oracle, rows, inv, sets, metric, fusion, 9, 7, take, weights=w), (dim, metric, take, fusion, w is not None))
    store.close()


# ---- entry counts around the sort's edges -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide_store():
    store, rows, rng, inv = make(8, 3000, seed=1)
    yield store, rows, rng, inv
    store.close()


@pytest.mark.parametrize("legs,fetch", [(1, 1), (1, 63), (1, 64), (1, 65), (1, 511), (1, 512), (3, 171), (3, 341), (5, 205), (2, 512), (16, 7), (16, 512)])
def test_entry_counts_straddle_the_network(oracle, wide_store, legs, fetch):
    """legs x fetch = 1, 63, 64, 65, 511, 512, 513, 1023, 1025, 1024, 112 and 8192 entries; k below, at and above the union"""
    store, rows, rng, inv = wide_store
    store.set_option("fuse_device", ROUTE)
    sets = [quantised(np.random.default_rng(legs * 1000 + fetch), (legs, 8))]
    for fusion in FUSIONS:
        full = expect(oracle, rows, inv, sets, Metric.DotProduct, fusion, 10 ** 6, fetch)
        union = full[1][0]
        for k in sorted({1, union, union + 5, 10}):
            got = plan_of(store, sets, Metric.DotProduct, fusion, k, fetch).collect_arrays()
            same(got, (full[0][:k], [min(k, union)]), (legs, fetch, fusion, k))


def test_identical_and_disjoint_legs(oracle):
    """sixteen copies of one leg: every row is a run of 16; sixteen legs whose lists share no row: every run has length 1"""
    store, rows, rng, inv = make(128, 2000, seed=2)
    one = quantised(rng, (1, 128))
    sets = [np.repeat(one, 16, axis=0)]
    for fusion in FUSIONS:
        got = plan_of(store, sets, Metric.Cosine, fusion, 600, 512, weights=[[1.0, -0.5] * 8]).collect_arrays()
        exp = expect(oracle, rows, inv, sets, Metric.Cosine, fusion, 600, 512, weights=[[1.0, -0.5] * 8])
        assert exp[1] == [512]
        same(got, exp, ("identical", fusion))
    store.close()
    rows = np.zeros((1600, 128), np.float32)  # block g of 100 rows lives in dims 8g .. 8g + 7, and so does leg g
    for g in range(16):
        rows[100 * g:100 * (g + 1), 8 * g:8 * g + 8] = quantised(rng, (100, 8))
    store, rows, rng, inv = make(128, 0, rows=rows)
    legs = np.zeros((16, 128), np.float32)
    for g in range(16):
        legs[g, 8 * g:8 * g + 8] = quantised(rng, (1, 8))
    flt = (0.0, Cmp.Gt)  # a row outside a leg's block scores 0: the filter keeps it out
    for fusion in FUSIONS:
        got = plan_of(store, [legs], Metric.DotProduct, fusion, 2000, 100, flt=flt).collect_arrays()
        exp = expect(oracle, rows, inv, [legs], Metric.DotProduct, fusion, 2000, 100, flt=flt)
        lists = R.leg_lists(oracle, rows, legs, Metric.DotProduct, 1, 100, int(Cmp.Gt), 0.0, inv=inv)
        assert sum(l[0].size for l in lists) == exp[1][0] > 100  # disjoint: the union is the sum
        same(got, exp, ("disjoint", fusion))
    store.close()


def test_many_requests(oracle):
    """1024 requests of one leg each, and 3 requests of 1 / 16 / 2 legs"""
    store, rows, rng, inv = make(8, 200, seed=3)
    sets = sets_of(rng, 8, (1,) * 1024)
    for fusion in (R.RRF, R.DBSF):
        got = plan_of(store, sets, Metric.Euclidean, fusion, 3, 5).collect_arrays()
        same(got, expect(oracle, rows, inv, sets, Metric.Euclidean, fusion, 3, 5), ("1024", fusion))
    sets = sets_of(rng, 8, (1, 16, 2))
    for fusion in FUSIONS:
        got = plan_of(store, sets, Metric.Manhattan, fusion, 50, 20).collect_arrays()
        same(got, expect(oracle, rows, inv, sets, Metric.Manhattan, fusion, 50, 20), ("1/16/2", fusion))
    store.close()


# ---- lists shorter than fetch -------------------------------------------------------------------------------------------------------------

def test_short_and_empty_lists(oracle):
    store, rows, rng, inv = make(33, 200, seed=4)
    sets = sets_of(rng, 33, (3, 2))
    for fusion in FUSIONS:
        # a store smaller than fetch
        got = plan_of(store, sets, Metric.Cosine, fusion, 500, 512).collect_arrays()
        exp = expect(oracle, rows, inv, sets, Metric.Cosine, fusion, 500, 512)
        assert exp[1] == [200, 200]
        same(got, exp, ("store < fetch", fusion))
        # a row mask shorter than the store that keeps 11 of its rows
        mask = np.zeros(150, bool)
        mask[::14] = True
        got = plan_of(store, sets, Metric.Cosine, fusion, 500, 100, mask=mask).collect_arrays()
        exp = expect(oracle, rows, inv, sets, Metric.Cosine, fusion, 500, 100, mask=mask)
        assert exp[1] == [61, 61]  # 11 kept rows and the 50 behind the mask's end
        same(got, exp, ("row mask", fusion))
    # a filter that empties one leg (the zero vector scores 0 everywhere), and all legs
    sets = [np.concatenate([sets[0][:2], np.zeros((1, 33), np.float32)]), np.zeros((2, 33), np.float32)]
    for fusion in FUSIONS:
        flt = (0.0, Cmp.Gt)
        got = plan_of(store, sets, Metric.DotProduct, fusion, 40, 30, flt=flt).collect_arrays()
        exp = expect(oracle, rows, inv, sets, Metric.DotProduct, fusion, 40, 30, flt=flt)
        assert exp[1][0] > 0 and exp[1][1] == 0
        same(got, exp, ("filter", fusion))
    store.close()


# ---- weights, rrf_k, the 0.5 branch, infinite scores --------------------------------------------------------------------------------------

def test_weights_and_rrf_k(oracle):
    store, rows, rng, inv = make(8, 500, seed=5)
    sets = sets_of(rng, 8, (3, 2))
    for fusion in FUSIONS:
        absent = plan_of(store, sets, Metric.DotProduct, fusion, 40, 30).collect_arrays()
        ones = plan_of(store, sets, Metric.DotProduct, fusion, 40, 30, weights=[[1, 1, 1], [1, 1]]).collect_arrays()
        same(ones, absent, ("all 1 = absent", fusion))
        for w in ([[1.0, -1.0, 0.25], [-3.0, 1e-3]], [[0.0, 0.0, 0.0], [0.0, 1.0]]):
            got = plan_of(store, sets, Metric.DotProduct, fusion, 40, 30, weights=w).collect_arrays()
            same(got, expect(oracle, rows, inv, sets, Metric.DotProduct, fusion, 40, 30, weights=w), ("weights", fusion, w))
    for rrf_k in (0.0, 60.0, 0.5):
        got = plan_of(store, sets, Metric.Cosine, R.RRF, 40, 30, rrf_k=rrf_k).collect_arrays()
        same(got, expect(oracle, rows, inv, sets, Metric.Cosine, R.RRF, 40, 30, rrf_k=rrf_k), ("rrf_k", rrf_k))
    # a leg whose scores are all equal: the zero vector under the dot product, every entry gets 0.5
    sets = [np.concatenate([sets[0][:1], np.zeros((1, 8), np.float32)])]
    for fusion in (R.DBSF, R.MINMAX):
        got = plan_of(store, sets, Metric.DotProduct, fusion, 100, 50, weights=[[1.0, 4.0]]).collect_arrays()
        exp = expect(oracle, rows, inv, sets, Metric.DotProduct, fusion, 100, 50, weights=[[1.0, 4.0]])
        assert (exp[0]["score"] >= 2.0).sum() == 50  # rows 0 .. 49 hold the second leg's list: 4 x 0.5 each
        same(got, exp, ("all equal", fusion))
    store.close()


def test_infinite_scores(oracle):
    """Euclidean overflow: a row of 2e19s is at distance inf of every leg.  MINMAX: the span is inf, the row's own inf / inf is NaN
    and its NaN F drops it (the finite rows get 0); DBSF: the span is NaN, so the whole list gets 0.5; RRF does not read the score."""
    rng = np.random.default_rng(11)
    rows = quantised(rng, (300, 8))
    rows[5] = 2e19
    store, rows, _, inv = make(8, 0, rows=rows)
    sets = [quantised(rng, (2, 8)), quantised(rng, (1, 8))]
    for fusion in FUSIONS:
        got = plan_of(store, sets, Metric.Euclidean, fusion, 400, 512, take=1).collect_arrays()  # take Max: the far rows first, the infinite one leads
        exp = expect(oracle, rows, inv, sets, Metric.Euclidean, fusion, 400, 512, take=1)
        assert exp[1] == ([299, 299] if fusion == R.MINMAX else [300, 300]), exp[1]
        assert (5 in exp[0]["index"]) == (fusion != R.MINMAX)
        same(got, exp, ("inf", fusion))
    # a weight of 0 does not save the row: 0 x NaN is NaN
    got = plan_of(store, sets[:1], Metric.Euclidean, R.MINMAX, 400, 512, take=1, weights=[[1.0, 0.0]]).collect_arrays()
    same(got, expect(oracle, rows, inv, sets[:1], Metric.Euclidean, R.MINMAX, 400, 512, take=1, weights=[[1.0, 0.0]]), "inf, two legs")
    store.close()


# ---- the sharp cases of tests/fuse_cases.py on the device ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [FC.leg_order, FC.rrf_rank, FC.equal_f, FC.dbsf_mean])
def test_sharp_cases(oracle, case):
    c = case()
    store, rows, _, inv = make(FC.DIM, 0, rows=c["rows"])
    lists = R.leg_lists(oracle, rows, c["legs"], Metric.DotProduct, 1, c["fetch"], inv=inv)
    weights = None if c["weights"] is None else [c["weights"]]
    got = plan_of(store, [c["legs"]], Metric.DotProduct, c["fusion"], c["k"], c["fetch"], rrf_k=c["rrf_k"], weights=weights).collect_arrays()
    right = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"])
    same(got, (right, [right.size]), case.__name__)
    wrongs = c["wrong"] if isinstance(c["wrong"], list) else [c["wrong"]] if c["wrong"] else []
    for w in wrongs:
        wrong = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"], **w)
        assert got[0]["index"].tolist() != wrong["index"].tolist(), (case.__name__, w)
    store.close()


# ---- store state ----------------------------------------------------------------------------------------------------------------------------

def test_base_offset_and_deleted_rows(oracle):
    store, rows, rng, inv = make(33, 1200, seed=6)
    sets = sets_of(rng, 33, (2, 3))
    store.set_base_offset(5_000_000_000)
    dead = rng.choice(1200, 300, replace=False)
    store.delete_rows(dead)
    live = np.ones(1200, bool)
    live[dead] = False
    for fusion in FUSIONS:
        got = plan_of(store, sets, Metric.Cosine, fusion, 25, 40).collect_arrays()
        exp = expect(oracle, rows, inv, sets, Metric.Cosine, fusion, 25, 40, mask=live, base=5_000_000_000)
        assert exp[0]["index"].min() >= 5_000_000_000
        same(got, exp, ("base offset, deleted", fusion))
    store.close()


def test_chunk_mask_and_device_row_mask_through_the_meta_plan(oracle):
    rng = np.random.default_rng(13)
    n, dim = 2048, 8
    rows = quantised(rng, (n, dim))
    ms = MetaStore.from_columns([Column("a", DataType.Int64).from_(list(range(n)))]).with_vectors(rows).with_chunk_size(64).build()
    flt = col("a").gte(300) & col("a").lt(1500)  # prunes whole chunks (a chunk mask) and needs a row mask inside two
    keep = (np.arange(n) >= 300) & (np.arange(n) < 1500)
    sets = sets_of(rng, dim, (3, 1))
    inv = ms._store.inv_norms()
    ms._store.set_option("fuse_device", ROUTE)
    for fusion in FUSIONS:
        p = ms.fuse(sets, Metric.DotProduct).meta_filter(flt).fetch(50).take(20)
        p = p.rrf(2.0) if fusion == R.RRF else p.dbsf() if fusion == R.DBSF else p.min_max()
        got = p.collect_arrays()
        assert ms._store.last_stats["pruned_chunks"] > 0
        same(got, expect(oracle, rows, inv, sets, Metric.DotProduct, fusion, 20, 50, rrf_k=2.0, mask=keep), ("meta", fusion))
    res = ms.fuse(sets, Metric.DotProduct).meta_filter(flt).fetch(50).take(4).collect()
    assert [len(r.indices) for r in res] == [4, 4] and all(300 <= i < 1500 for r in res for i in r.indices)


# ---- routes -----------------------------------------------------------------------------------------------------------------------------------

def test_routes_and_paths_give_the_same_bits(oracle):
    store, rows, rng, inv = make(128, 3000, seed=7)
    sets = sets_of(rng, 128, (4, 4, 4, 4, 2))
    for fusion in FUSIONS:
        exp = expect(oracle, rows, inv, sets, Metric.Cosine, fusion, 10, 100)
        for fuse_device in (-1, 0, 1):
            store.set_option("fuse_device", fuse_device)
            for path in (Path.Auto, Path.Exact, Path.Mfma):
                got = plan_of(store, sets, Metric.Cosine, fusion, 10, 100, path=path).collect_arrays()
                same(got, exp, (fusion, fuse_device, path))
                if path != Path.Auto:
                    assert store.last_stats["path_used"] == int(path)
    store.close()


@pytest.mark.parametrize("tie_order", [1, 2])
def test_tie_orders_take_the_host_route(oracle, tie_order):
    rng = np.random.default_rng(17 + tie_order)
    rows = quantised(rng, (1500, 8))
    store, rows, _, inv = make(8, 0, rows=rows)
    store.set_chunk_size(128)
    store.set_option("tie_order", tie_order)
    store.set_option("fuse_device", 1)  # asked for, not eligible: the host route
    sets = sets_of(rng, 8, (3, 2))
    legs = np.concatenate(sets)
    lists = []
    for q in legs:  # a leg's list IS ott_query's under this tie order ...
        h, _ = store.query(q, Metric.DotProduct).per_query().take(40).collect_arrays()
        if tie_order == 1:  # ... which is the oracle's literal collector: the scores bit for bit, the rows as a set
            o = oracle.vec_query(rows, q, int(Metric.DotProduct), 1, 40, ties=oracle.TIES_LITERAL, inv=inv)
        else:
            o, _ = oracle.meta_query(rows, 128, q, int(Metric.DotProduct), 1, 40, ties=oracle.TIES_LITERAL, inv=inv)
        assert np.array_equal(h["score"].view(np.uint32), o["score"].view(np.uint32)) and sorted(h["index"].tolist()) == sorted(o["index"].tolist())
        lists.append((h["index"].copy(), h["score"].copy()))
    canon = R.leg_lists(oracle, rows, legs, Metric.DotProduct, 1, 40, inv=inv)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(lists, canon)), "the tie order must show in a list"
    for fusion in FUSIONS:
        got = plan_of(store, sets, Metric.DotProduct, fusion, 30, 40).collect_arrays()
        same(got, expect(oracle, rows, inv, sets, Metric.DotProduct, fusion, 30, 40, lists=lists), (tie_order, fusion))
    store.close()


def test_worker_threads_answer_as_the_serial_run(oracle):
    """eight threads, six calls each, beside one another on one store: every call returns what it returns alone"""
    store, rows, rng, inv = make(33, 3000, seed=8)
    jobs = []
    for t in range(8):
        sets = sets_of(rng, 33, (1 + t % 4, 16 if t == 3 else 2))
        fusion = FUSIONS[t % 3]
        fetch = 512 if t == 3 else 30 + 10 * t
        jobs.append((sets, fusion, fetch, expect(oracle, rows, inv, sets, Metric.Cosine, fusion, 12, fetch)))
    for sets, fusion, fetch, exp in jobs:
        same(plan_of(store, sets, Metric.Cosine, fusion, 12, fetch).collect_arrays(), exp, "serial")
    errors = []
    start = threading.Barrier(len(jobs))

    def work(t):
        sets, fusion, fetch, exp = jobs[t]
        try:
            rf = plan_of(store, sets, Metric.Cosine, fusion, 12, fetch).resolve()
            start.wait()
            for _ in range(6):
                hits, counts, _ = store._run_fuse(rf)
                same((hits, counts), exp, ("thread", t))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(len(jobs))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    store.close()


# ---- refusals that need a store, the stats --------------------------------------------------------------------------------------------------

def raw_call(store, legs, legs_per_request, k, fetch, cap, out, fusion=0, mode=1):
    legs = np.ascontiguousarray(legs, np.float32)
    lp = np.array(legs_per_request, np.uint32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = legs.ctypes.data, legs.shape[0], int(Metric.DotProduct), 1, mode, k, 0
    n_out = C.c_uint64(77)
    per = (C.c_uint64 * len(legs_per_request))(*([77] * len(legs_per_request)))
    st = N.Stats()
    rc = N.lib().ott_query_fuse(store._handle(), C.byref(d), N.ptr(lp), len(legs_per_request), fusion, 60.0, None, fetch,
                                None if out is None else N.ptr(out), cap, C.byref(n_out), per, C.byref(st))
    return rc, N.lib().ott_last_error().decode(), n_out.value, list(per), st.as_dict()


def test_refusals_that_need_a_store_and_the_stats(oracle):
    store, rows, rng, inv = make(8, 300, seed=9)
    legs = quantised(rng, (5, 8))
    out = np.zeros(64, N.HIT_DTYPE)
    # cap: the sum over the requests of min(k, legs x min(fetch, rows)) = min(10, 3 x 4) + min(10, 2 x 4) = 18
    rc, err, n_out, per, _ = raw_call(store, legs, [3, 2], 10, 4, 17, out)
    assert rc == -1 and "output capacity is smaller than the sum over the requests" in err and n_out == 77 and per == [77, 77] and not out["index"].any()
    rc, err, n_out, per, _ = raw_call(store, legs, [3, 2], 10, 4, 18, None)
    assert rc == -1 and "ott_query_fuse: out is NULL" in err and n_out == 77
    rc, err, *_ = raw_call(store, legs, [3, 2], 10, 4, 64, out, mode=0)
    assert rc == -4 and "d->mode must be OTT_MODE_PER_QUERY" in err
    rc, err, n_out, per, st = raw_call(store, legs, [3, 2], 10, 4, 18, out)
    assert rc == 0 and n_out == sum(per) and per == expect(oracle, rows, inv, [legs[:3], legs[3:]], Metric.DotProduct, R.RRF, 10, 4)[1]
    assert st["path_used"] in (int(Path.Exact), int(Path.Mfma)) and st["passes"] >= 1 and st["bytes_scanned"] > 0 and st["vectors_compared"] == 5 * 300
    assert st["merge_ns"] > 0 and st["total_ns"] >= st["merge_ns"]  # the fuse kernel's event time is in merge_ns, the whole call in total_ns
    for fuse_device in (0, 1):
        store.set_option("fuse_device", fuse_device)
        st = raw_call(store, legs, [3, 2], 10, 4, 18, out)[4]
        assert st["merge_ns"] > 0 and st["total_ns"] >= st["merge_ns"] and st["passes"] >= 1
    with pytest.raises(OttersError):
        store.set_option("fuse_device", 2)
    store.close()
    # an empty store: a valid call with no hits, whatever cap is
    class Empty:
        def __init__(self):
            self.h = C.c_void_p()
            N.check(N.lib().ott_store_create(8, 0, C.byref(self.h)))

        def _handle(self):
            return self.h

    empty = Empty()
    rc, err, n_out, per, _ = raw_call(empty, legs, [3, 2], 10, 4, 0, None)
    assert rc == 0 and n_out == 0 and per == [0, 0], (rc, err)
    N.check(N.lib().ott_store_destroy(empty.h))
    multi = VecStore(8, devices=[0, 0])
    multi.add_vectors(rows)
    rc, err, *_ = raw_call(multi, legs, [3, 2], 10, 4, 64, out)
    assert rc == -4 and "a multi-GPU store is not served" in err
    multi.close()
