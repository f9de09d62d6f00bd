"""CPU: the Manhattan (L1) metric's host side and the reference it is tested against (tests/manhattan_ref.py).

* The numpy restatement of the arithmetic contract is anchored to the pinned oracle: the same loop with the term swapped for
  d*d or q*v equals oracle.l2sq / oracle.dot bit for bit, in both reduce orders, at tail-heavy dims and on IEEE edge rows.
* Its reference tie outcome (the closed form of tests/test_tie_rule_model.py) equals a literal TopKCollector written here.
* The value 3 is the same in the C header, the Python enum, the C++ mirror and the Rust binding; the default take is Min."""
import os
import re
import subprocess

import numpy as np
import pytest

import ieee_edges as E
import manhattan_ref as M
from otters_amd import Column, DataType, MetaStore, Metric, TakeType, VecQueryPlan, VecStore
from otters_amd.meta import MetaQueryPlan
from otters_amd.vec import infer_default_take_type

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_enum(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "otters_hip.h")).read(), flags=re.S)
    vals = {}
    for body in re.findall(r"typedef enum\s*\{(.*?)\}", hdr, flags=re.S):
        for n, v in re.findall(r"(OTT_[A-Z0-9_]+)\s*=\s*(-?\d+)", body):
            vals[n] = int(v)
    return vals[name]


def rust_const(name):
    src = open(os.path.join(ROOT, "bindings", "rust", "otters-hip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub const %s\s*:\s*\w+\s*=\s*(-?\d+)\s*;" % name, src)
    assert m, name
    return int(m.group(1))


# ---- the numpy machinery against the oracle -------------------------------------------------------------------------------

def edge_sets(dim):
    rng = np.random.default_rng(100 + dim)
    out = []
    for gen in (E.signed_zero_cosines, E.subnormal_sums, E.overflow):
        rows, q, _ = gen(rng, dim=dim)
        out.append((gen.__name__, rows.astype(np.float32), np.atleast_2d(q).astype(np.float32)))
    return out


@pytest.mark.parametrize("reduce_mode", [M.REDUCE_AVX, M.REDUCE_SEQ4])
@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 31, 33, 100])
def test_machinery_equals_the_oracle_for_l2_and_dot(oracle, dim, reduce_mode):
    rng = np.random.default_rng(dim * 7 + reduce_mode)
    sets = [("random", rng.uniform(-2, 2, (37, dim)).astype(np.float32), rng.uniform(-2, 2, (3, dim)).astype(np.float32))]
    sets += edge_sets(dim)
    for name, rows, qs in sets:
        qs = qs[:4]
        for kind, fn in (("l2", oracle.l2sq), ("dot", oracle.dot)):
            got = M.scores(rows, qs, kind, reduce_mode)
            want = np.array([[fn(q, r, reduce_mode) for r in rows] for q in qs], np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, kind, dim, reduce_mode)


def test_l1_scores_follow_the_contract():
    """hand-checked values: the order of the adds, the remainder, signed zeros, infinities and NaN"""
    f = np.float32
    # dim 9: eight chains of one element each, then a remainder of one; |q - v| whatever the operand order
    q = np.arange(9, dtype=f)
    v = -np.arange(9, dtype=f)
    assert M.scores(v[None], q)[0, 0] == M.scores(q[None], v)[0, 0] == f(2 * 36)
    # one chain, rounding: 1 + 2^-24 + 2^-24 rounds to 1 at each add in the chain order; the remainder is summed apart
    rows = np.zeros((1, 17), f)
    qq = np.zeros(17, f)
    qq[0], qq[8], qq[16] = 1.0, 2.0 ** -24, 2.0 ** -24
    s = M.scores(rows, qq)[0, 0]
    assert s == (f(1.0) + f(2.0 ** -24)) + f(2.0 ** -24)
    # |-0 - +0| = +0; inf - inf = NaN; an infinite difference is +inf; an overflowing sum is +inf
    assert M.scores(np.array([[0.0]], f), np.array([-0.0], f)).view(np.uint32)[0, 0] == 0
    assert np.isnan(M.scores(np.array([[np.inf]], f), np.array([np.inf], f))[0, 0])
    assert M.scores(np.array([[-np.inf]], f), np.array([np.inf], f))[0, 0] == np.inf
    big = np.full((1, 8), 3e38, f)
    assert M.scores(big, -big[0])[0, 0] == np.inf


def test_selection_filters_nan_and_masks():
    S = np.array([[3.0, np.nan, 1.0, 1.0, 0.0], [1.0, 2.0, np.inf, 5.0, 1.0]], np.float32)
    h = M.select_canonical(S, M.TAKE_MIN, 4)
    assert list(zip(h["index"].tolist(), h["query"].tolist())) == [(4, 0), (0, 1), (2, 0), (3, 0)]
    h = M.select_canonical(S, M.TAKE_MIN, 10, M.CMP_EQ, 1.0)
    assert list(zip(h["index"].tolist(), h["query"].tolist())) == [(0, 1), (2, 0), (3, 0), (4, 1)]
    h = M.select_canonical(S, M.TAKE_MAX, 2, M.CMP_GTE, 2.0, row_mask=[True, True, False])
    assert list(zip(h["index"].tolist(), h["query"].tolist())) == [(3, 1), (0, 0)]
    h = M.select_canonical(S, M.TAKE_MIN, 2, perq=True)
    assert list(zip(h["index"].tolist(), h["query"].tolist())) == [(4, 0), (2, 0), (0, 1), (4, 1)]


# ---- the reference tie outcome: closed form against a literal collector ---------------------------------------------------

def literal_collector(S, take, k, cmp=M.CMP_NONE, thr=0.0, row_mask=None):
    """src/vec_compute.rs:236-288 restated literally: visit order of src/vec.rs:222-303, filter + NaN drop, fill then sort,
    strict-improvement inserts at slice::binary_search_by's position (Ok(i) | Err(i) -> i), pop"""
    nq, n = S.shape
    full = n // 8 * 8
    visits = [(r, q) for b in range(0, full, 8) for q in range(nq) for r in range(b, b + 8)]
    visits += [(r, q) for q in range(nq) for r in range(full, n)]
    key = lambda s: int(M.ordkey(np.array([s], np.float32), take)[0])  # noqa: E731
    buf, thr_k = [], None
    for r, q in visits:
        if row_mask is not None and r < len(row_mask) and not row_mask[r]:
            continue
        s = S[q, r]
        if not M.passes(np.array([s], np.float32), cmp, thr)[0] or k == 0:
            continue
        if len(buf) == k:
            if not (s < thr_k if take == M.TAKE_MIN else s > thr_k):
                continue
            ks, size, base = key(s), len(buf), 0
            while size > 1:
                half = size // 2
                mid = base + half
                base = base if key(buf[mid][0]) > ks else mid
                size -= half
            kb = key(buf[base][0])
            pos = base if kb == ks else base + (1 if kb < ks else 0)
            buf.insert(pos, (s, r, q))
            buf.pop()
            thr_k = buf[-1][0]
        else:
            buf.append((s, r, q))
            if len(buf) == k:
                buf.sort(key=lambda e: key(e[0]))  # (stable: the oracle's restatement of sort_unstable_by)
                thr_k = buf[-1][0]
    buf.sort(key=lambda e: key(e[0]))
    return buf


@pytest.mark.parametrize("seed", range(30))
def test_closed_form_equals_the_literal_collector_on_l1_scores(seed):
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([5, 8, 9, 23, 64, 100, 257]))
    dim = int(rng.choice([1, 2, 3, 8, 11]))
    nq = int(rng.choice([1, 1, 2, 3, 5]))
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    queries = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    S = M.scores(rows, queries)
    take = M.TAKE_MIN if rng.random() < 0.8 else M.TAKE_MAX
    mask = (rng.random(n) < 0.8) if rng.random() < 0.4 else None
    cmp, thr = (0, 0.0)
    if rng.random() < 0.5:
        cmp, thr = int(rng.choice([1, 2, 3, 4, 5])), float(rng.integers(0, 2 * dim + 1))
    for k in (1, 2, 3, 5, 8, 13, 20, 40, n * nq, n * nq + 3):
        lit = literal_collector(S, take, k, cmp, thr, mask)
        got = M.select_reference(S, take, k, cmp, thr, mask)
        assert [(int(r), int(q)) for r, q in zip(got["index"], got["query"])] == [(r, q) for _, r, q in lit], (seed, k)
        assert np.array_equal(got["score"].view(np.uint32), np.array([s for s, _, _ in lit], np.float32).view(np.uint32))


# ---- the value 3 through every layer; the default take --------------------------------------------------------------------

def test_metric_value_is_the_same_in_every_layer():
    assert int(Metric.Manhattan) == 3 == header_enum("OTT_METRIC_MANHATTAN") == rust_const("OTT_METRIC_MANHATTAN")
    # the existing values are untouched
    assert [int(Metric.Cosine), int(Metric.Euclidean), int(Metric.DotProduct)] == [0, 1, 2]
    assert header_enum("OTT_METRIC_DOT") == 2


def test_default_take_is_min():
    assert infer_default_take_type(Metric.Manhattan) == TakeType.Min
    plan = VecQueryPlan.new().with_vector_store(VecStore(4)).with_query_vectors([[1, 2, 3, 4]]).with_metric(Metric.Manhattan).take(3)
    assert plan.take_type == TakeType.Min
    rq = plan.resolve()
    assert rq.take == int(TakeType.Min) and rq.metric == 3
    assert VecStore(4).query([1, 2, 3, 4], Metric.Manhattan).take(2).take_type == TakeType.Min
    meta = MetaStore.from_columns([Column("a", DataType.Int32).from_([1, 2])]).with_vectors([[1.0], [2.0]]).build(_host_only=True)
    mp = MetaQueryPlan(meta, [np.array([1.0], np.float32)], Metric.Manhattan)
    assert mp.take(1).take_type == TakeType.Min
    mp = MetaQueryPlan(meta, [np.array([1.0], np.float32)], Metric.Manhattan)
    mp.take_count = 1  # no take type set: resolve() infers it
    rq, _, _ = mp.resolve()
    assert rq.take == int(TakeType.Min)


def test_cpp_mirror_names_the_same_value(tmp_path):
    src = tmp_path / "manhattan_value.cpp"
    src.write_text('#include "otters.hpp"\n#include "otters_meta.hpp"\n'
                   "static_assert(static_cast<int>(otters::Metric::Manhattan) == OTT_METRIC_MANHATTAN, \"C++ mirror\");\n"
                   "static_assert(OTT_METRIC_MANHATTAN == 3, \"ABI value\");\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
