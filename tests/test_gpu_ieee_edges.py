"""GPU: IEEE edge values (tests/ieee_edges.py) on every query path, against the oracle — index, query and f32 score bits.

Signed-zero scores, subnormal elements / products / sums of squares, finite rows whose products or sums of squares overflow, and
rows that live on half or bf16 subnormals.  tie_order 0 is compared with the oracle's canonical collector; tie_order 1 and 2 with
its literal restatement of the reference's (test_gpu_ties.same_sets: same score sequence, same (index, query) sets) — where the
collector admits by IEEE comparison (-0.0 == +0.0) but positions by total order (+0.0 above -0.0)."""
import numpy as np
import pytest

import ieee_edges as E
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore
from test_gpu_ties import same_sets

pytestmark = pytest.mark.gpu

OPTION_SETS = {"default": {}, "hi_fmt1": {"hi_fmt": 1}, "hi_fmt0": {"hi_fmt": 0}, "no_hi_pass": {"no_hi_pass": 1}, "mfma_f32": {"mfma_f32": 1}}
METRICS = ((Metric.Cosine, 1), (Metric.DotProduct, 1), (Metric.Euclidean, 0), (Metric.Cosine, 0))


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"], ref["query"]), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


MFMA_MAX_K = 484  # the batch path's largest k (a larger k is refused, as is a dim below 8)


def paths_for(dim, k):
    return (Path.Exact, Path.Auto, Path.Mfma) if dim >= 8 and k <= MFMA_MAX_K else (Path.Exact, Path.Auto)


def mfma_or_refused(store, queries, *a, **kw):
    """Path.Mfma forced: the oracle's bits, or — for a batch that holds a query of elements >= 1e10, whose error bound is not
    finite — the library's explicit refusal (Path.Auto answers those on the exact path)"""
    try:
        return run(store, queries, *a, path=Path.Mfma, **kw)
    except OttersError as e:
        assert "non-finite error bound" in str(e), str(e)
        assert np.abs(queries).max() >= 1e10, str(e)
        return None


def run(store, queries, metric, take, k, path=Path.Exact, filt=None, mask=None, perq=False):
    p = store.query(queries, metric)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    p = (p.take_max(k) if take else p.take_min(k)).with_path(path)
    if perq:
        p = p.per_query()
    return p.collect_arrays()


def oracle_ref(oracle, rows, queries, metric, take, k, filt=None, mask=None, perq=False, ties=None):
    ties = oracle.TIES_CANONICAL if ties is None else ties
    fc, ft = (int(filt[1]), filt[0]) if filt else (0, 0.0)
    if not perq:
        return oracle.vec_query(rows, queries, int(metric), take, k, fc, ft, row_mask=mask, ties=ties)
    parts = []
    for qi in range(queries.shape[0]):
        r = oracle.vec_query(rows, queries[qi], int(metric), take, k, fc, ft, row_mask=mask, ties=ties)
        r["query"] = qi
        parts.append(r)
    return np.concatenate(parts)


def edge_corpus(dim, seed=0):
    """families a-c and e at one dim, in one store, with queries from each family"""
    rng = np.random.default_rng(seed + dim)
    parts = [E.signed_zero_cosines(rng, 40, dim), E.subnormal_sums(rng, 64, dim), E.overflow(rng, 48, dim)]
    if dim >= 8:
        parts.append(E.bf16_lo_edges(rng, 64, dim))
    rows = np.concatenate([p[0] for p in parts]).astype(np.float32)
    rows = np.concatenate([rows, rng.uniform(-1, 1, (57, dim)).astype(np.float32)])   # ordinary rows around them
    queries = np.concatenate([p[1] for p in parts]).astype(np.float32)
    return rows, queries


@pytest.mark.parametrize("dim", [1, 7, 8, 33, 768])
def test_inverse_norms_of_edge_rows(oracle, dim):
    """store.inv_norms() == the oracle's on rows whose sums of squares are subnormal, underflow, or overflow — arriving through
    several appends, and through write_rows over resident planes"""
    rows, _ = edge_corpus(dim)
    store = VecStore(dim)
    cut = [0, 5, 41, 120, rows.shape[0]]
    for a, b in zip(cut, cut[1:]):
        store.add_vectors(rows[a:b])
    assert np.array_equal(store.inv_norms().view(np.uint32), oracle.inv_norms(rows).view(np.uint32)), dim
    store.query(rows[:2], Metric.Cosine).take(5).collect_arrays()     # planes resident
    store.set_option("hi_fmt", 1)
    store.query(rows[:64], Metric.Cosine).take(5).with_path(Path.Auto).collect_arrays()
    rows2 = rows.copy()
    rows2[10:110] = rows[::-1][10:110]                                 # edge rows over other edge rows
    store.write_rows(10, rows2[10:110])
    assert np.array_equal(store.inv_norms().view(np.uint32), oracle.inv_norms(rows2).view(np.uint32)), dim
    k = 20
    for path in paths_for(dim, k):
        got, _ = run(store, rows2[:3], Metric.Cosine, 1, k, path)
        bits_equal(got, oracle_ref(oracle, rows2, rows2[:3], Metric.Cosine, 1, k), ("after write_rows", dim, path))
    store.close()


@pytest.mark.parametrize("opt", list(OPTION_SETS))
def test_edge_values_on_every_path_and_tile_width(oracle, opt):
    """Exact / Auto / Mfma under each option set; one query and batches of 16, 32, 64, 256 (every tile width); merged and per
    query; take_max and take_min; k = 1, 10, 600"""
    dim = 33
    rows, qe = edge_corpus(dim, 7)
    rng = np.random.default_rng(11)
    store = VecStore(dim)
    for name, v in OPTION_SETS[opt].items():
        store.set_option(name, v)
    store.add_vectors(rows)
    pool = np.concatenate([qe, rng.uniform(-1, 1, (256, dim)).astype(np.float32)])
    pool[len(qe):len(qe) + 256:7] *= np.float32(1e-22)                 # queries of subnormal sums of squares among them
    for nq in (1, 16, 32, 64, 256):
        queries = pool[:nq] if nq > 1 else pool[[0]]
        for metric, take in METRICS:
            for k in (1, 10, 600):
                for perq in ((False, True) if nq in (1, 16) else (False,)):
                    ref = oracle_ref(oracle, rows, queries, metric, take, k, perq=perq)
                    for path in paths_for(dim, k):
                        where = (opt, nq, metric, take, k, path, perq)
                        if path == Path.Mfma:
                            r = mfma_or_refused(store, queries, metric, take, k, perq=perq)
                            if r is not None:
                                bits_equal(r[0], ref, where)
                            # the same edge rows under queries of finite bounds (subnormal, ordinary)
                            fin = pool[len(qe):len(qe) + nq] if nq > 1 else queries
                            if np.abs(fin).max() < 1e10:
                                got, _ = run(store, fin, metric, take, k, path, perq=perq)
                                bits_equal(got, oracle_ref(oracle, rows, fin, metric, take, k, perq=perq), where + ("finite",))
                            continue
                        got, _ = run(store, queries, metric, take, k, path, perq=perq)
                        bits_equal(got, ref, where)
    store.close()


def test_edge_filter_thresholds_and_row_masks(oracle):
    """filter thresholds 0.0, -0.0, +-inf, +-FLT_MAX, +-2^-149, with each Cmp; with and without a row mask"""
    dim = 8
    rows, qe = edge_corpus(dim, 3)
    store = VecStore(dim)
    store.add_vectors(rows)
    mask = np.random.default_rng(5).random(rows.shape[0]) < 0.7
    queries = qe[:6]
    for thr in E.THRESHOLDS:
        for cmp in (Cmp.Lt, Cmp.Gt, Cmp.Lte, Cmp.Gte, Cmp.Eq):
            for metric, take in METRICS[:3]:
                for m in (None, mask):
                    ref = oracle_ref(oracle, rows, queries, metric, take, 25, filt=(thr, cmp), mask=m)
                    got, _ = run(store, queries, metric, take, 25, Path.Exact, filt=(thr, cmp), mask=m)
                    bits_equal(got, ref, (thr, cmp, metric, m is not None, Path.Exact))
                    r = mfma_or_refused(store, queries, metric, take, 25, filt=(thr, cmp), mask=m)
                    if r is not None:
                        bits_equal(r[0], ref, (thr, cmp, metric, m is not None, Path.Mfma))
    store.close()


def signed_zero_cases():
    """stores whose cosine scores against a huge query are all +-0: the issue's 40 x 8 case and a larger one (several blocks of
    eight, a remainder, zeros of both signs at every cut)"""
    rng = np.random.default_rng(5)
    out = []
    for n in (40, 203, 1000):
        rows = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        q = np.stack([(rng.uniform(-1, 1, 8) * 1e20), rng.uniform(-1, 1, 8) * 1e20, rng.uniform(-1, 1, 8)]).astype(np.float32)
        out.append((rows, q))
    rows, q, _ = E.signed_zero_cosines(rng, 40, 8)
    out.append((rows, q))
    return out


def _zero_boundary(scores):
    """positions where +0.0 turns into -0.0 (take_max order)"""
    s = np.signbit(scores) & (scores == 0)
    return [i for i in range(1, len(s)) if s[i] and not s[i - 1]]


@pytest.mark.parametrize("tie_order", [0, 1])
def test_signed_zero_cut(oracle, tie_order):
    """the cut at take(k) running through cosines of +0.0 and -0.0: canonical order vs the oracle's canonical collector, the
    reference order vs its literal restatement (which admits by IEEE comparison and positions by total_cmp)"""
    ties = oracle.TIES_CANONICAL if tie_order == 0 else oracle.TIES_LITERAL
    for case, (rows, q) in enumerate(signed_zero_cases()):
        store = VecStore(8)
        store.set_option("tie_order", tie_order)
        store.add_vectors(rows)
        n = rows.shape[0]
        for qs in (q[[0]], q[:2], q):
            every = oracle.vec_query(rows, qs, oracle.METRIC_COSINE, oracle.TAKE_MAX, n * len(qs), ties=oracle.TIES_CANONICAL)
            ks = sorted({1, 2, 3, 5, 10, 600} | {b for b in _zero_boundary(every["score"])} | {b + 1 for b in _zero_boundary(every["score"])})
            for k in ks:
                for take, metric in ((1, Metric.Cosine), (0, Metric.Cosine)):
                    for path in paths_for(8, k + tie_order):  # (the reference order asks its passes for k + 1)
                        for perq in (False, True):
                            where = (tie_order, case, len(qs), k, take, path, perq)
                            if path == Path.Mfma:
                                r = mfma_or_refused(store, qs, metric, take, k, perq=perq)
                                if r is None:
                                    continue
                                got = r[0]
                            else:
                                got, _ = run(store, qs, metric, take, k, path, perq=perq)
                            ref = oracle_ref(oracle, rows, qs, metric, take, k, perq=perq, ties=ties)
                            if tie_order == 0:
                                bits_equal(got, ref, where)
                            else:
                                same_sets(got, ref, where)
        store.close()


@pytest.mark.parametrize("cs", [8, 1000, 1021])
def test_signed_zero_cut_per_chunk_collectors(oracle, cs):
    """tie_order 2 (one collector per chunk, then the concat-sort-truncate that treats -0.0 == +0.0) on a MetaStore"""
    rng = np.random.default_rng(cs)
    n = 3000
    rows = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    q = np.stack([rng.uniform(-1, 1, 8) * 1e20, rng.uniform(-1, 1, 8) * 1e20]).astype(np.float32)
    bucket = np.zeros(n, np.int32)
    meta = MetaStore.from_columns([Column.from_numpy("bucket", DataType.Int32, bucket)]).with_vectors(rows).with_chunk_size(cs).build()
    meta.set_tie_order("reference")
    for qs in (q[:1], q):
        for k in (1, 3, 10, 40, 600):
            plan = meta.query_batch(qs, Metric.Cosine) if len(qs) > 1 else meta.query(qs[0], Metric.Cosine)
            res = plan.take(k).collect()
            lit, _ = oracle.meta_query(rows, cs, qs, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, ties=oracle.TIES_LITERAL)
            where = (cs, len(qs), k)
            assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), lit["score"].view(np.uint32)), where
            assert sorted(res.indices) == sorted(lit["index"].tolist()), where


def test_signed_zero_cut_on_three_shards(oracle):
    """tie_order 1 on one store spread over three shards of this process"""
    for case, (rows, q) in enumerate(signed_zero_cases()):
        store = VecStore(8, devices=[0, 0, 0])
        store.set_option("multi_min_shard_rows", 0)
        store.set_tie_order("reference")
        store.add_vectors(rows)
        for k in (1, 3, 10, 37, 600):
            for perq in (False, True):
                got, _ = run(store, q, Metric.Cosine, 1, k, perq=perq)
                same_sets(got, oracle_ref(oracle, rows, q, Metric.Cosine, 1, k, perq=perq, ties=oracle.TIES_LITERAL), (case, k, perq))
        store.close()


def test_half_subnormal_rows_are_certified_exactly(oracle):
    """family d under hi_fmt 1: the batch path (path_used 2) certifies without bound violations and returns the oracle's bits —
    the half plane's rows and query operands carry most of their dot product in half subnormals"""
    rows, q, info = E.half_subnormal_rows(np.random.default_rng(3))
    dim = rows.shape[1]
    store = VecStore(dim)
    store.set_option("hi_fmt", 1)
    store.add_vectors(rows)
    queries = np.repeat(q, 16, axis=0)
    for metric in (Metric.DotProduct, Metric.Cosine):
        for k in (info["k"] + 1, 200):
            got, _ = run(store, queries, metric, 1, k, Path.Mfma, perq=True)
            st = store.last_stats
            assert st["path_used"] == 2 and st["bound_violations"] == 0, (metric, k, st)
            bits_equal(got, oracle_ref(oracle, rows, queries, metric, 1, k, perq=True), (metric, k))
            if metric == Metric.DotProduct and k == info["k"] + 1:  # row 0 first, then every S row ahead of the F rows
                assert sorted(got["index"][:k].tolist()) == sorted([0] + info["s_rows"].tolist())
    store.close()
