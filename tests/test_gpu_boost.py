"""GPU: score boosting (ott_query_boost, VecQueryPlan.boost, MetaQueryPlan.boost_by / boost_decay / boost_where).
Bar: query b's hits — index, F's f32 bits, order, count, and `query` = b — are exactly the numpy model's (tests/boost_ref.py: S from
the oracle, the formula one IEEE operation at a time, NaN drop, filter on F, canonical order).  Bit for bit, no tolerances.  Rows
and queries are integers in -2..2, so exact ties in S are frequent and a boost below 1 decides between them."""
import ctypes as C
import threading

import numpy as np
import pytest

import boost_cases as BC
import boost_ref as BR
import masks_ref as MR
from otters_amd import BoostCombine, BoostTerm, Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N
from otters_amd.expr import CmpOp

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
ALL_METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan)
NP_OF = {DataType.Int32: np.int32, DataType.Int64: np.int64, DataType.Float32: np.float32, DataType.Float64: np.float64, DataType.DateTime: np.int64}


def make_store(rows, chunk=None):
    store = VecStore(rows.shape[1])
    if chunk:
        store.set_chunk_size(chunk)
    store.add_vectors(rows)
    return store


class Formula:
    """terms as the API takes them and as the model takes them, side by side"""

    def __init__(self, store):
        self.store, self.api, self.model, self.n_slots = store, [], [], 0

    def value(self, values, dtype, weight, origin=0.0, missing=0.0, nulls=None):
        values = np.asarray(values, NP_OF[dtype])
        self.api.append(BoostTerm.value(self.store.add_column(values, dtype, nulls), weight, origin, missing))
        self.model.append(("value", values, nulls, weight, origin, missing))
        return self

    def decay(self, values, dtype, origin, scale, weight=1.0, missing=0.0, nulls=None):
        values = np.asarray(values, NP_OF[dtype])
        self.api.append(BoostTerm.lin_decay(self.store.add_column(values, dtype, nulls), origin, scale, weight, missing))
        self.model.append(("decay", values, nulls, weight, origin, scale, missing))
        return self

    def mask(self, mask, weight, slot=None):
        slot = self.n_slots if slot is None else slot
        self.store.write_row_mask_slot(slot, mask)
        self.n_slots = max(self.n_slots, slot + 1)
        self.api.append(BoostTerm.mask_slot(slot, weight))
        self.model.append(("mask", np.asarray(mask, bool), weight))
        return self

    def pick(self, idx):
        f = Formula.__new__(Formula)
        f.store, f.api, f.model, f.n_slots = self.store, [self.api[i] for i in idx], [self.model[i] for i in idx], self.n_slots
        return f


def run(store, q, metric, api_terms, take, k, combine=BR.SUM, sw=1.0, flt=None, common=None, chunk_mask=None, use_dev=False, merged=False):
    """one ott_query_boost call: ([hits of query b], stats)"""
    p = store.query(q, metric).boost(api_terms, BoostCombine(combine), sw)
    if not merged:
        p = p.per_query()
    p = p.take_max(k) if take else p.take_min(k)
    if flt is not None:
        p = p.filter(flt[1], flt[0])
    if common is not None:
        p = p.with_row_mask(common)
    hits, counts, stats = store._run(p.resolve(), chunk_mask=chunk_mask, use_device_row_mask=use_dev)
    nq = 1 if q.ndim == 1 else q.shape[0]
    if merged:
        counts = [hits.size]
    assert sum(counts) == hits.size and len(counts) == nq
    out, at = [], 0
    for c in counts:
        out.append(hits[at:at + c])
        at += c
    return out, stats


def same(got, exp, where):
    assert len(got) == len(exp), where
    for b, (g, e) in enumerate(zip(got, exp)):
        w = (where, "query", b)
        assert g.size == e.size, (w, g.size, e.size)
        assert np.array_equal(g["index"].astype(np.int64), e["index"].astype(np.int64)), (w, g["index"][:12], e["index"][:12])
        assert np.array_equal(g["score"].view(np.uint32), e["score"].view(np.uint32)), (w, g["score"][:12], e["score"][:12])
        assert np.array_equal(g["query"].astype(np.int64), e["query"].astype(np.int64)), (w, g["query"][:12], e["query"][:12])


def check(store, S, q, f, metric, take, k, where, combine=BR.SUM, sw=1.0, flt=None, keep=None, **kw):
    exp = BR.expected(S[: q.shape[0]], f.model, take, k, combine, sw, int(flt[0]) if flt else 0, flt[1] if flt else 0.0, keep)
    got, st = run(store, q, metric, f.api, take, k, combine, sw, flt, **kw)
    same(got, exp, where)
    return got, st


def pool_of(store, rng, n):
    """eight terms over every column dtype, NULLs with `missing`, both decays, a written slot shorter than the store and an evaluated one"""
    nulls = rng.random(n) < 0.15
    f = Formula(store)
    f.value(rng.uniform(-1, 1, n), DataType.Float32, 0.3, 0.25, -0.5, nulls)
    f.decay(rng.integers(-15, 16, n), DataType.Int32, 0.0, 10.0, 0.75)
    f.mask(rng.random(n - 70) < 0.4, 0.125)
    f.value(rng.uniform(-1e3, 1e3, n), DataType.Float64, 1e-4, 17.0)
    f.value(2 ** 53 + rng.integers(-40, 40, n), DataType.Int64, 0.003, 2.0 ** 53)
    f.decay(1_700_000_000_123 + rng.integers(-100_000, 100_000, n), DataType.DateTime, 1_700_000_000_123.0, 200_000.0, 0.5, 0.1, rng.random(n) < 0.1)
    # an evaluated slot: the filter `col < 40` over an Int32 column, evaluated on the device
    vals = rng.integers(0, 100, n).astype(np.int32)
    cid = store.add_column(vals, DataType.Int32)
    leaf = N.Leaf()
    leaf.column, leaf.op, leaf.clause, leaf.lit_i64 = cid, int(CmpOp.Lt), 0, 40
    N.check(N.lib().ott_store_eval_row_mask_slot(store._handle(), 9, C.byref(leaf), 1, 1, None))
    f.api.append(BoostTerm.mask_slot(9, -0.2))
    f.model.append(("mask", vals < 40, -0.2))
    f.value(rng.integers(-3, 4, n), DataType.Int32, 0.05, 1.0, 2.0, nulls)
    return f


# ---- 1. the shape and semantics sweep ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ALL_METRICS, ids=lambda m: m.name)
@pytest.mark.parametrize("n", [1000, 4097])
@pytest.mark.parametrize("dim", [8, 43, 128, 1100])
def test_every_metric_take_filter_k_batch_size_and_formula(oracle, dim, n, metric):
    """dims: the lsl4 short row (8), a remainder of dim % 8 (43), several stages (128), rows beyond 1024 floats (1100); n = 4097 is
    no multiple of 64; chunks of 100 rows with two dropped, so tiles straddle mask words and runs"""
    rng, rows, q = BC.int_corpus(n, dim, 1000 * dim + n, nq=9)
    store = make_store(rows, chunk=100)
    S = BR.scores(oracle, rows, q, metric)
    assert np.unique(S[0].view(np.uint32)).size < n  # the corpus really produces ties in S
    n_chunks = (n + 99) // 100
    cm = np.ones(n_chunks, bool)
    cm[[1, n_chunks - 2]] = False
    keep = np.repeat(cm, 100)[:n]
    pool = pool_of(store, rng, n)
    formulas = [pool.pick([]), pool.pick([0]), pool.pick([1, 2]), pool, pool.pick([5, 6]), pool.pick([4, 3, 7])]
    configs = [(1, 10, None), (3, 1, Cmp.Lt), (4, 600, Cmp.Gt), (5, n, Cmp.Lte), (9, 10, Cmp.Gte), (4, 10, Cmp.Eq), (9, 600, None)]
    i = 0
    for take in (0, 1):
        for nq, k, cmp in configs:
            f = formulas[i % len(formulas)]
            combine, sw = (BR.SUM, BR.MULT)[(i // 2) % 2], (1.0, 0.5, -1.0)[i % 3]
            i += 1
            flt = None
            if cmp is not None:
                F0 = BR.final(S[:1], f.model, combine, sw)[0][keep]
                F0 = F0[~np.isnan(F0)]
                flt = (cmp, float(F0[F0.size // 3]) if cmp == Cmp.Eq else float(np.median(F0)))  # a threshold inside F's range; for Eq an F that occurs
            _, st = check(store, S, q[:nq], f, metric, take, k, (dim, n, metric.name, take, nq, k, cmp, len(f.api), combine, sw), combine, sw, flt, keep, chunk_mask=cm)
            assert st["path_used"] == int(Path.Exact) and st["passes"] == -(-nq // 4) and st["vectors_compared"] == int(keep.sum()) * nq
            per_row = dim * 4 + (4 if metric == Metric.Cosine else 0) + sum(m[1].dtype.itemsize for m in f.model if m[0] != "mask")
            assert st["bytes_scanned"] == st["passes"] * int(keep.sum()) * per_row, st


def test_three_hundred_rows_of_4096_floats(oracle):
    n, dim = 300, 4096
    rng, rows, q = BC.int_corpus(n, dim, 50, nq=5)
    store = make_store(rows)
    pool = pool_of(store, rng, n)
    for metric in ALL_METRICS:
        S = BR.scores(oracle, rows, q, metric)
        check(store, S, q, pool, metric, TAKE[metric], 20, ("wide", metric.name), BR.SUM, 1.0)
        check(store, S, q[:1], pool.pick([0, 1]), metric, 1 - TAKE[metric], 400, ("wide, one query", metric.name), BR.MULT, 0.5)


# ---- 2. named cases ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base(oracle):
    """one corpus and its scores under the four metrics, shared by the named cases and never changed"""
    n, dim = 1500, 24
    rng, rows, q = BC.int_corpus(n, dim, 61, nq=9)
    S = {m: BR.scores(oracle, rows, q, m) for m in ALL_METRICS}
    for s in S.values():
        s.setflags(write=False)
    rows.setflags(write=False)
    return n, dim, rows, q, S


def test_anchor_no_terms_and_weight_one_is_ott_query_on_the_exact_path(base):
    n, dim, rows, q, S = base
    store = make_store(rows, chunk=128)
    common = np.random.default_rng(1).random(n) < 0.7
    for metric in ALL_METRICS:
        for take, k, flt in ((1, 10, None), (0, 700, (Cmp.Gt, float(np.median(S[metric])))), (TAKE[metric], n, None)):
            got, _ = run(store, q, metric, [], take, k, flt=flt, common=common)
            p = store.query(q, metric).per_query().with_path(Path.Exact).with_row_mask(common)
            p = p.take_max(k) if take else p.take_min(k)
            if flt:
                p = p.filter(flt[1], flt[0])
            hits, counts = p.collect_arrays()
            exp, at = [], 0
            for c in counts:
                exp.append(hits[at:at + c])
                at += c
            same(got, exp, ("anchor", metric.name, take, k))
            one, _ = run(store, q[3], metric, [], take, k, flt=flt, common=common, merged=True)  # MERGED with one query
            e = exp[3].copy()
            e["query"] = 0
            same(one, [e], ("anchor merged", metric.name, take, k))


def test_every_dtype_nulls_a_nan_value_and_the_decay_at_its_knee(base):
    n, dim, rows, q, S = base
    store = make_store(rows)
    rng = np.random.default_rng(62)
    nulls = rng.random(n) < 0.2
    for dtype in (DataType.Int32, DataType.Int64, DataType.DateTime, DataType.Float32, DataType.Float64):
        v = rng.integers(-50, 50, n) if dtype not in (DataType.Float32, DataType.Float64) else rng.uniform(-50, 50, n)
        f = Formula(store).value(v, dtype, 0.01, 3.0, 7.0, nulls).decay(v, dtype, -4.0, 25.0, 0.5, 0.25, nulls)
        for combine in (BR.SUM, BR.MULT):
            check(store, S[Metric.DotProduct], q[:5], f, Metric.DotProduct, 1, 40, (dtype.name, combine), combine, 1.0)
    # a non-NULL NaN value drops the row; a NULL row's value is never looked at
    v = rng.uniform(-1, 1, n).astype(np.float32)
    v[[3, 500, 1499]] = np.nan
    v[[4, 501]] = np.nan
    nl = np.zeros(n, bool)
    nl[[4, 501]] = True
    for f in (Formula(store).value(v, DataType.Float32, 0.5, 0.0, 0.125, nl), Formula(store).decay(v, DataType.Float32, 0.0, 2.0, 0.5, 0.125, nl)):
        got, _ = check(store, S[Metric.Euclidean], q[:3], f, Metric.Euclidean, 0, n, "nan value")
        for g in got:
            assert g.size == n - 3 and not np.isin([3, 500, 1499], g["index"]).any() and np.isin([4, 501], g["index"]).all()
    # LIN_DECAY with u below, equal to and above 1, on both sides of the origin, and far away
    d = rng.integers(-12, 13, n).astype(np.int32)
    d[:7] = [10, -10, 9, -9, 11, -11, 0]
    f = Formula(store).decay(d, DataType.Int32, 0.0, 10.0, 0.9)
    g = BR.term_g(f.model[0], n)
    assert g[0] == 0 and g[1] == 0 and 0 < g[2] < 0.11 and g[4] == 0 and g[6] == 1 and not np.signbit(g[:7]).any()
    check(store, S[Metric.Cosine], q, f, Metric.Cosine, 1, 300, "decay knee")


def test_mask_terms_evaluated_written_and_shorter_than_the_store(base):
    n, dim, rows, q, S = base
    store = make_store(rows)
    rng = np.random.default_rng(63)
    pool = pool_of(store, rng, n)
    f = pool.pick([2, 6])  # the written slot of n - 70 bits, the evaluated one
    got, _ = check(store, S[Metric.DotProduct], q[:4], f, Metric.DotProduct, 1, n, "slots")
    B = BR.boost_sum(f.model, n)
    assert np.all(B[n - 70:][~f.model[1][1][n - 70:]] == np.float32(0.125))  # rows behind the short slot's end count as set
    # an empty slot, one at the edge of the range, one that was cleared
    with pytest.raises(OttersError, match=r"term 1 \(MASK\): slot 10 was never filled") as ei:
        run(store, q[:1], Metric.DotProduct, [f.api[0], BoostTerm.mask_slot(10, 1.0)], 1, 5)
    assert ei.value.status == -1
    with pytest.raises(OttersError, match="slot 64 is not below OTT_MASK_SLOTS"):
        run(store, q[:1], Metric.DotProduct, [BoostTerm.mask_slot(64, 1.0)], 1, 5)
    store.clear_row_mask_slots()
    with pytest.raises(OttersError, match="slot 0 was never filled"):
        run(store, q[:1], Metric.DotProduct, f.api, 1, 5)


def test_the_three_sharp_cases(oracle):
    """what tests/test_boost_cpu.py proves sharp: the chain order, the f64 subtraction of a datetime, the Int64 conversion"""
    n = 600
    for seed, make in ((71, lambda: BC.chain_order(n)[0]), (72, lambda: BC.datetime_decay(n)[0]), (73, lambda: BC.int64_edges(n))):
        _, rows, q = BC.int_corpus(n, 16, seed)
        store = make_store(rows)
        S = BR.scores(oracle, rows, q, 2)
        f = Formula(store)
        for t in make():
            if t[0] == "value":
                f.value(t[1], {np.dtype(np.float32): DataType.Float32, np.dtype(np.int64): DataType.Int64}[t[1].dtype], t[3], t[4], t[5], t[2])
            else:
                f.decay(t[1], DataType.DateTime, t[4], t[5], t[3], t[6], t[2])
        for k in (10, n):
            check(store, S, q, f, Metric.DotProduct, 1, k, ("sharp", seed, k))
    # the Int64 edge values themselves, as scores: S = 0 (a zero query under dot), F = c_0
    rows = np.ones((BC.I64_EDGE.size, 8), np.float32)
    store = make_store(rows)
    f = Formula(store).value(BC.I64_EDGE, DataType.Int64, 1.0, 2.0 ** 53)
    got, _ = run(store, np.zeros((1, 8), np.float32), Metric.DotProduct, f.api, 1, 100)
    exp = (BC.I64_EDGE_F64 - 2.0 ** 53).astype(np.float32)
    by_row = got[0][np.argsort(got[0]["index"])]
    assert np.array_equal(by_row["score"].view(np.uint32), exp.view(np.uint32))


def test_integer_ties_go_to_the_lower_row_and_signed_zeros_are_ordered(oracle, base):
    n, dim, rows, q, S = base
    store = make_store(rows)
    rng = np.random.default_rng(64)
    f = Formula(store).value(rng.integers(-2, 3, n), DataType.Int32, 1.0).mask(rng.random(n) < 0.5, 2.0)
    F = BR.final(S[Metric.DotProduct], f.model)
    assert np.unique(F[0]).size < n // 10  # integer F: long runs of ties
    got, _ = check(store, S[Metric.DotProduct], q, f, Metric.DotProduct, 1, 200, "integer ties")
    for g in got:
        tied = g["score"][1:] == g["score"][:-1]
        assert tied.any() and np.all(g["index"][1:][tied] > g["index"][:-1][tied])
    # -0.0 against +0.0: rows orthogonal to the query have S = +0; MULT with 1 + B = -1 turns them into -0
    rows0 = rows.copy()
    rows0[:400, :] = 0.0
    rows0[:400, 0] = 1.0
    q0 = np.zeros((2, dim), np.float32)
    q0[:, 1] = [1.0, -1.0]
    store0 = make_store(rows0)
    flip = np.where(np.arange(n) % 3 == 0, -2.0, 0.0)
    f0 = Formula(store0).value(flip, DataType.Float64, 1.0)
    S0 = BR.scores(oracle, rows0, q0, 2)
    F0 = BR.final(S0, f0.model, BR.MULT)
    assert (np.signbit(F0[0, :400]) & (F0[0, :400] == 0)).any() and (~np.signbit(F0[0, :400]) & (F0[0, :400] == 0)).any()
    for take in (0, 1):
        got, _ = check(store0, S0, q0, f0, Metric.DotProduct, take, n, ("signed zeros", take), BR.MULT)
        z = got[0][got[0]["score"] == 0]
        sign = np.signbit(z["score"])
        assert sign.any() and (~sign).any() and np.all(np.diff(sign.astype(int)) >= 0 if take else np.diff(sign.astype(int)) <= 0)  # Max: +0 first


def test_a_denormal_product_an_overflow_and_inf_minus_inf(oracle, base):
    n, dim, rows, q, S = base
    store = make_store(rows)
    rng = np.random.default_rng(65)
    v = rng.uniform(-3, 3, n).astype(np.float32)
    f = Formula(store).value(v, DataType.Float32, 1e-40).value(v, DataType.Float32, 3e38).value(v, DataType.Float32, -3e38)
    c0 = np.float32(1e-40) * v
    assert ((c0 != 0) & (np.abs(c0) < np.finfo(np.float32).tiny)).all()
    zero_q = np.zeros((1, dim), np.float32)
    Sz = BR.scores(oracle, rows, zero_q, 2)
    got, _ = check(store, Sz, zero_q, f.pick([0]), Metric.DotProduct, 1, n, "denormal c_j: F is the denormal itself")
    assert got[0].size == n and np.count_nonzero(got[0]["score"]) == n
    got, _ = check(store, S[Metric.DotProduct], q[:2], f.pick([0, 1]), Metric.DotProduct, 1, n, "overflow to inf")
    assert np.isinf(got[0]["score"]).any() and got[0].size == n
    F = BR.final(S[Metric.DotProduct][:2], f.model)
    dropped = int(np.isnan(F[0]).sum())
    assert dropped > n // 4
    got, _ = check(store, S[Metric.DotProduct], q[:2], f, Metric.DotProduct, 1, n, "inf - inf drops the row")
    assert got[0].size == n - dropped


def test_deleted_rows_a_common_host_mask_and_the_device_mask_as_common(base):
    n, dim, rows, q, S = base
    store = make_store(rows)
    rng = np.random.default_rng(66)
    pool = pool_of(store, rng, n)
    common = rng.random(n - 30) < 0.6
    check(store, S[Metric.Cosine], q[:6], pool, Metric.Cosine, 1, 40, "common mask", keep=MR.keep_of(n, common, None), common=common)
    dead = rng.choice(n, 300, replace=False)
    store.delete_rows(dead)
    alive = np.ones(n, bool)
    alive[dead] = False
    check(store, S[Metric.Cosine], q[:6], pool, Metric.Cosine, 1, 40, "deleted + common", BR.MULT, keep=MR.keep_of(n, common, alive), common=common)
    check(store, S[Metric.Euclidean], q[:6], pool.pick([0, 2]), Metric.Euclidean, 0, 700, "deleted", keep=alive)
    vals = rng.integers(0, 100, n).astype(np.int32)
    leaf = N.Leaf()
    leaf.column, leaf.op, leaf.clause, leaf.lit_i64 = store.add_column(vals, DataType.Int32), int(CmpOp.Lt), 0, 55
    N.check(N.lib().ott_store_eval_row_mask(store._handle(), C.byref(leaf), 1, 1, None))
    check(store, S[Metric.DotProduct], q[:6], pool, Metric.DotProduct, 1, 30, "device mask as common", keep=alive & (vals < 55), use_dev=True)


def test_the_key_table_is_left_clean_for_the_other_query_kinds(base):
    n, dim, rows, q, S = base
    rng = np.random.default_rng(67)
    labels = rng.integers(0, 40, n)
    masks = [rng.random(n) < 0.5 for _ in range(5)]

    def others(store):
        g = store.query(q[:2], Metric.DotProduct).per_query().one_per_group().take(15).collect_arrays()
        store.set_option("masks_sweep", 1)
        m = store.query(q[:5], Metric.DotProduct).per_query().with_row_masks(masks).take(15).collect_arrays()
        return g, m

    used, fresh = make_store(rows), make_store(rows)
    used.set_groups(labels)
    fresh.set_groups(labels)
    pool = pool_of(used, rng, n)
    first, _ = check(used, S[Metric.DotProduct], q[:7], pool, Metric.DotProduct, 1, 30, "once")
    second, _ = check(used, S[Metric.DotProduct], q[:7], pool, Metric.DotProduct, 1, 30, "twice")
    same(second, first, "the same call twice")
    check(used, S[Metric.Euclidean], q[:7], pool, Metric.Euclidean, 0, 600, "through the pair form of the top-k")
    for u, f in zip(others(used), others(fresh)):
        assert np.array_equal(u[0]["index"], f[0]["index"]) and np.array_equal(u[0]["score"].view(np.uint32), f[0]["score"].view(np.uint32))
        assert list(u[1]) == list(f[1])


def test_what_the_store_refuses(base):
    n, dim, rows, q, S = base
    store = make_store(rows)
    cid = store.add_column(np.zeros(n, np.float32), DataType.Float32)

    def refused(status, text, fn):
        with pytest.raises(OttersError, match=text) as ei:
            fn()
        assert ei.value.status == status

    refused(-1, r"term 0 \(VALUE\): unknown column id 5", lambda: run(store, q[:1], Metric.DotProduct, [BoostTerm.value(5, 1.0)], 1, 5))
    L, h = N.lib(), store._handle()
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.mode, d.k = q.ctypes.data, 3, 2, 1, 1, 10
    out = np.zeros(64, dtype=N.HIT_DTYPE)
    assert L.ott_query_boost(h, C.byref(d), 0, 1.0, None, 0, N.ptr(out), 29, None, None, None) == -1 and b"output capacity is smaller than nq * min(k, rows)" in L.ott_last_error()
    assert L.ott_query_boost(h, C.byref(d), 0, 1.0, None, 0, N.ptr(out), 30, None, None, None) == 0
    store.set_tie_order("reference")
    refused(-4, "tie_order 1 and 2 are not served", lambda: run(store, q[:1], Metric.DotProduct, [], 1, 5))
    store.set_tie_order("canonical")
    store.add_vectors(rows[:10])  # the column no longer covers the store
    refused(-1, "the length of column 0 no longer matches the store", lambda: run(store, q[:1], Metric.DotProduct, [BoostTerm.value(cid, 1.0)], 1, 5))
    multi = VecStore(dim, devices=[0, 0])
    multi.add_vectors(rows)
    d.nq = 1
    assert L.ott_query_boost(multi._handle(), C.byref(d), 0, 1.0, None, 0, N.ptr(out), 64, None, None, None) == -4 and b"a multi-GPU store is not served" in L.ott_last_error()


# ---- 3. MetaQueryPlan --------------------------------------------------------------------------------------------------------------------------

def test_meta_boosts_equal_the_model(oracle):
    n, dim, cs = 3000, 16, 200
    rng, rows, q = BC.int_corpus(n, dim, 68, nq=3)
    chunk = np.arange(n) // cs
    pop = rng.uniform(0, 10, n)
    pop_null = rng.random(n) < 0.05
    ts = 1_700_000_000_000 + chunk.astype(np.int64) * 86_400_000 + rng.integers(0, 86_400_000, n)
    ver = ((chunk % 3) + rng.integers(0, 2, n)).astype(np.int32)
    tag = np.array(["title", "body", "note"])[rng.integers(0, 3, n)]
    meta = MetaStore.from_columns([Column.from_numpy("pop", DataType.Float64, pop, pop_null), Column.from_numpy("ts", DataType.DateTime, ts),
                                   Column.from_numpy("version", DataType.Int32, ver), Column.from_numpy("tag", DataType.String, tag)]
                                  ).with_vectors(rows).with_chunk_size(cs).build()
    origin_ms = 1_700_000_000_000 + 7 * 86_400_000  # 2023-11-21T22:13:20Z
    model = [("value", pop, pop_null, 0.1, 0.0, 0.0), ("decay", ts, None, 0.8, float(origin_ms), 5.0 * 86_400_000, 0.0), ("mask", tag == "title", 0.5),
             ("mask", (ver >= 2) | (tag == "note"), 0.25)]
    for metric in (Metric.Cosine, Metric.Euclidean):
        S = BR.scores(oracle, rows, q, metric)
        for b in range(3):
            plan = (meta.query(q[b], metric).boost_by("pop", 0.1).boost_decay("ts", "2023-11-21T22:13:20Z", 5.0 * 86_400_000, weight=0.8)
                    .boost_where(col("tag").eq("title"), 0.5).boost_where(col("version").gte(2) | col("tag").eq("note"), 0.25).take(12))
            got = plan.collect()
            exp = BR.expected(S[b:b + 1], model, TAKE[metric], 12)[0]
            assert got.indices == exp["index"].tolist(), (metric.name, b, got.indices, exp["index"])
            assert np.array_equal(np.array(got.scores, np.float32).view(np.uint32), exp["score"].view(np.uint32)), (metric.name, b)
        # with a meta_filter, a vec_filter on F and the other combine
        keep = (ver >= 1) & ~pop_null & (pop < 8.0)
        F = BR.final(S[:1], model[:2], BR.MULT, 0.5)
        thr = float(np.float32(np.nanmedian(F[0][keep])))
        got = (meta.query(q[0], metric).meta_filter(col("version").gte(1) & col("pop").lt(8.0)).boost_by("pop", 0.1)
               .boost_decay("ts", float(origin_ms), 5.0 * 86_400_000, weight=0.8).boost_combine(BoostCombine.Mult, 0.5).vec_filter(thr, Cmp.Gte).take(25).collect())
        exp = BR.expected(S[:1], model[:2], TAKE[metric], 25, BR.MULT, 0.5, int(Cmp.Gte), thr, keep)[0]
        assert got.indices == exp["index"].tolist() and np.array_equal(np.array(got.scores, np.float32).view(np.uint32), exp["score"].view(np.uint32)), metric.name
        assert meta.last_query_stats() is not None and len(got) > 0


# ---- 4. concurrency ------------------------------------------------------------------------------------------------------------------------------

def test_four_threads_of_boosted_batches_beside_plain_queries_equal_their_serial_answers(base):
    n, dim, rows, q, S = base
    store = make_store(rows)
    pool = pool_of(store, np.random.default_rng(69), n)
    jobs = [(pool, 9, 20, BR.SUM, Metric.DotProduct), (pool.pick([0, 1]), 5, 600, BR.MULT, Metric.Euclidean), (pool.pick([2, 6]), 1, 50, BR.SUM, Metric.Cosine),
            (pool.pick([3, 4, 5]), 4, 10, BR.MULT, Metric.Manhattan)]

    def boosted(j):
        f, nq, k, combine, metric = jobs[j]
        p = store.query(q[:nq], metric).per_query().boost(f.api, BoostCombine(combine), 0.75)
        return store._run((p.take_max(k) if TAKE[metric] else p.take_min(k)).resolve())[:2]

    def plain(j):
        metric = jobs[j][4]
        return store._run(store.query(q[:3], metric).per_query().take(15).resolve())[:2]

    serial = [(boosted(j), plain(j)) for j in range(4)]
    for j, ((hits, counts), _) in enumerate(serial):  # the serial answers are the model's
        f, nq, k, combine, metric = jobs[j]
        exp = np.concatenate(BR.expected(S[metric][:nq], f.model, TAKE[metric], k, combine, 0.75))
        assert np.array_equal(hits["index"], exp["index"]) and np.array_equal(hits["score"].view(np.uint32), exp["score"].view(np.uint32))
    errors = []

    def worker(j):
        try:
            for _ in range(6):
                for got, want in zip((boosted(j), plain(j)), serial[j]):
                    assert np.array_equal(got[0]["index"], want[0]["index"]) and np.array_equal(got[0]["score"].view(np.uint32), want[0]["score"].view(np.uint32))
                    assert np.array_equal(got[0]["query"], want[0]["query"]) and list(got[1]) == list(want[1])
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=worker, args=(j,)) for j in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---- 5. past 2^32 bytes of key table -----------------------------------------------------------------------------------------------------------

def test_a_key_table_past_4_gib(oracle):
    """2^27 + 300 rows of dim 4 (store N of tests/test_gpu_large_offsets.py, with its free-memory guard): the key table of a
    four-query pass is 4 GiB, row ids pass 2^24 and 2^26, a column's byte offsets pass 2^29.  The model answers over the window rows
    K (tests/large_offsets.py), which are the common row mask; five queries, two passes."""
    import large_offsets as LO
    import test_gpu_large_offsets as LOF
    import time
    t0 = time.perf_counter()
    b = LOF.Big(oracle, "N")
    try:
        t1 = time.perf_counter()
        rng = np.random.default_rng(70)
        f = Formula(b.store)
        f.value(rng.random(b.n, dtype=np.float32), DataType.Float32, 0.4, 0.5)
        f.decay(rng.integers(-20, 21, b.n, dtype=np.int32), DataType.Int32, 0.0, 15.0, 0.3)
        bits = np.unpackbits(rng.integers(0, 256, b.n // 8 + 1, dtype=np.uint8))[: b.n - 60].view(bool)
        f.mask(bits, 0.2)  # shorter than the store: the last rows count as set

        def over_k(t):
            """a model term over the compact rows R[K]; K is sorted, so the rows behind a short mask's end stay behind it"""
            if t[0] == "mask":
                return ("mask", t[1][b.K[b.K < t[1].size]], t[2])
            return (t[0], t[1][b.K], None if t[2] is None else t[2][b.K]) + tuple(t[3:])

        model = [over_k(t) for t in f.model]
        t2 = time.perf_counter()
        for metric, combine in ((Metric.DotProduct, BR.SUM), (Metric.Euclidean, BR.MULT)):
            S = BR.scores(oracle, b.R, b.q_pool[:5], metric)
            exp = [b.S(h) for h in BR.expected(S, model, TAKE[metric], 20, combine, 0.5)]
            got, st = run(b.store, b.q_pool[:5], metric, f.api, TAKE[metric], 20, combine, 0.5, common=b.mask)
            same(got, exp, ("4 GiB table", metric.name, combine))
            assert st["passes"] == 2 and st["vectors_compared"] == b.n * 5, st
        assert any(int(g["index"].max()) >= 1 << 26 for g in got) and LO.HALF == 130
        print(f"the store {t1 - t0:.2f} s, the columns and the slot {t2 - t1:.2f} s, two boosted batches and their models {time.perf_counter() - t2:.2f} s")
    finally:
        b.close()
