"""CPU: the host side of late-interaction (MaxSim) search (VecQueryPlan.max_sim, ott_query_maxsim) — the NumPy
expectation of tests/maxsim_ref.py against a plain Python loop and against grouped search's expectation, the argument the 32-bit
table rests on (no non-NaN f32 has ordinal 0), plan resolution and its refusals, the label round trip, and the refusals the library
makes from the descriptor alone."""
import ctypes as C
import struct

import numpy as np
import pytest

import ieee_edges as E
import manhattan_ref as M
import maxsim_ref as R
from otters_amd import Cmp, Metric, Mode, OttersError, Path, VecStore


# ---- the reference ------------------------------------------------------------------------------------------------------------

def total_key(x) -> int:
    b = struct.unpack("<I", struct.pack("<f", float(x)))[0]
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def by_loops(S, gid, keep, k, take, cmp=0, thr=0.0):
    """groups x tokens x rows, one comparison at a time"""
    nq, n = S.shape
    out = []
    for g in range(int(gid.max()) + 1):
        acc, complete = None, True
        for t in range(nq):
            best = None
            for r in range(n):
                if gid[r] != g or not keep[r] or np.isnan(S[t, r]):
                    continue
                s = S[t, r]
                if best is None or (total_key(s) > total_key(best) if take == 1 else total_key(s) < total_key(best)):
                    best = s
            if best is None:
                complete = False
                break
            with np.errstate(all="ignore"):
                acc = np.float32(best) if acc is None else np.float32(acc + np.float32(best))
        if not complete or np.isnan(acc) or not bool(R.holds(np.array([acc], np.float32), cmp, thr)[0]):
            continue
        out.append((total_key(acc), g, acc))
    out.sort(key=lambda e: (-e[0] if take == 1 else e[0], e[1]))
    return out[:k]


def special_scores():
    rng = np.random.default_rng(41)
    n, nq = 40, 3
    S = rng.integers(-2, 3, (nq, n)).astype(np.float32)  # quantised: equal bests and equal sums
    S[:, 7] = np.nan                                   # a NaN row inside a group that has other rows
    S[0, 12] = np.inf
    S[1, 13] = -np.inf
    S[:, 20:24] = np.float32(0.0)
    S[:, 22:24] = -np.float32(0.0)                      # signed zeros in one group: +0.0 beats -0.0 under Max
    S[:, 28:32] = -np.float32(0.0)                      # a group of -0.0 only: its sum is -0.0
    gid = np.arange(n) // 4
    gid[12:14] = 3                                      # +inf for token 0 and -inf for token 1 in one group ...
    S[1, 12], S[1, 14:16] = -np.inf, -np.inf            # ... both its bests under Min / one under Max: NaN or inf sums
    S[:, 36:40] = np.nan                                # a group made only of NaN rows
    S[2, 16:20] = np.nan                                # a group that lacks one token
    return S, gid


@pytest.mark.parametrize("take", [1, 0])
def test_vectorised_reference_is_the_plain_loop(take):
    S, gid = special_scores()
    n = S.shape[1]
    full = M.select_canonical(S, take, S.size)
    rng = np.random.default_rng(42)
    for keep in (np.ones(n, bool), rng.random(n) < 0.6):
        for k in (1, 3, 10):
            for cmp, thr in ((0, 0.0), (int(Cmp.Gte), 0.0), (int(Cmp.Lt), 1.0), (int(Cmp.Eq), 0.0)):
                got = R.expected(full, gid, keep, k, S.shape[0], take, cmp, thr, n_groups=10)
                want = by_loops(S, gid, keep, k, take, cmp, thr)
                assert got["index"].tolist() == [g for _, g, _ in want], (take, k, cmp)
                assert got["score"].view(np.uint32).tolist() == [int(np.float32(a).view(np.uint32)) for _, _, a in want], (take, k, cmp)
                assert not got["query"].any()
    # what the case is there for
    all_rows = R.expected(full, gid, np.ones(n, bool), 10, 3, take, n_groups=10)
    assert 9 not in all_rows["index"] and 4 not in all_rows["index"]          # only NaN rows / a token without a score
    assert 1 in all_rows["index"]                                            # the NaN row does not take its group with it
    minus_zero = all_rows[all_rows["index"] == 7]["score"].view(np.uint32)
    assert minus_zero.tolist() == [0x80000000]                               # -0.0 + -0.0 + -0.0, started from best[0]
    if take == 1:
        assert all_rows[all_rows["index"] == 5]["score"].view(np.uint32).tolist() == [0]  # +0.0 is the best of {+0.0, -0.0}


def test_one_token_is_grouped_searchs_expectation_with_rows_mapped_to_groups():
    """(scores that differ between groups: among EQUAL scores grouped search prefers the lower row, MaxSim the lower group id)"""
    import test_gpu_groups as G
    rng = np.random.default_rng(43)
    n = 300
    S = ((rng.permutation(n) - 150 + 0.5) / 8).astype(np.float32)[None, :]  # no two alike, none zero
    S[0, 5], S[0, 90] = -np.float32(0.0), np.float32(0.0)                    # ... but the two zeros, which the total order tells apart
    S[0, 17] = np.nan
    for take in (1, 0):
        full = M.select_canonical(S, take, n)
        for n_groups in (1, 2, 37, n):
            gid = rng.integers(0, n_groups, n) if n_groups < n else rng.permutation(n)
            keep = rng.random(n) < 0.8
            for k in (1, 10, 64, n):
                ref, _ = G.expected(full, gid, keep, k, 1)
                got = R.expected(full, gid, keep, k, 1, take, n_groups=n_groups)
                assert got["index"].tolist() == gid[ref["index"].astype(np.int64)].tolist(), (take, n_groups, k)
                assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32))


def edge_values():
    rng = np.random.default_rng(44)
    vals = [np.array(E.THRESHOLDS, np.float32), np.array([E.TINY, -E.TINY, E.MIN_NORMAL, -E.MIN_NORMAL, E.FLT_MAX, -E.FLT_MAX, E.HALF_SUB], np.float32)]
    for fam in (E.signed_zero_cosines, E.subnormal_sums, E.overflow, E.half_subnormal_rows, E.bf16_lo_edges):
        rows, q, _ = fam(rng)
        vals += [rows.ravel(), np.asarray(q, np.float32).ravel(), E.seq_sumsq(rows), E.bf16_lo(rows).ravel()]
    # every sign and exponent with the smallest, the largest and a middle mantissa: the corners of the bit patterns
    sign, expo, mant = np.meshgrid(np.arange(2, dtype=np.uint32), np.arange(256, dtype=np.uint32), np.array([0, 1, 0x400000, 0x7FFFFF], np.uint32))
    vals.append(((sign << 31) | (expo << 23) | mant).astype(np.uint32).ravel().view(np.float32))
    v = np.concatenate(vals)
    return v[~np.isnan(v)]


def test_no_number_has_ordinal_zero_so_zero_can_mean_empty():
    v = edge_values()
    assert v.size > 100_000 and np.isinf(v).any() and (v.view(np.uint32) == 0x80000000).any() and (v.view(np.uint32) == 1).any()
    for take_max in (True, False):
        o = R.ord_of(v, take_max)
        assert o.min() >= 1 and o.max() <= 0xFFFFFFFF, take_max
        # the ordinal is a bijection the reduce kernel can undo, and it orders like the total order
        k = np.array([total_key(x) for x in v[:2000]], np.uint64)
        assert np.array_equal(o[:2000], k if take_max else (~k & np.uint64(0xFFFFFFFF)))
    # the two bit patterns that WOULD map to 0 are NaNs
    for bits, take_max in ((0xFFFFFFFF, True), (0x7FFFFFFF, False)):
        x = np.array([bits], np.uint32).view(np.float32)
        assert np.isnan(x[0]) and int(R.ord_of(x, take_max)[0]) == 0


# ---- plans --------------------------------------------------------------------------------------------------------------------

def host_store():
    store = VecStore(4)
    store._n, store._n_groups = 100, 7  # (no GPU: lengths as set_groups would leave them)
    return store


def test_max_sim_resolves_and_defaults_to_the_group_count():
    store = host_store()
    q = np.eye(4, dtype=np.float32)[:3]
    rq = store.query(q, Metric.Cosine).max_sim().resolve()
    assert rq.max_sim and not rq.grouped and rq.k == 7 and rq.take == 1 and rq.mode == int(Mode.Merged) and rq.queries.shape == (3, 4)
    rq = store.query(q, Metric.Euclidean).max_sim().take(3).resolve()
    assert rq.max_sim and rq.k == 3 and rq.take == 0           # take(k) infers Min from the metric
    assert store.query(q, Metric.Manhattan).max_sim().take(3).resolve().take == 0
    assert store.query(q, Metric.Euclidean).max_sim().resolve().take == 1   # a plan without take ranks by Max
    rq = store.query(q, Metric.DotProduct).max_sim().filter(0.5, Cmp.Gte).with_path(Path.Exact).resolve()
    assert rq.filter_cmp == int(Cmp.Gte) and rq.filter_thr == 0.5 and rq.path == int(Path.Exact)
    assert not store.query(q, Metric.Cosine).take(3).resolve().max_sim


def test_max_sim_refusals_at_validate():
    store = host_store()
    q = np.eye(4, dtype=np.float32)[:2]
    with pytest.raises(OttersError, match="max_sim cannot be combined with with_row_ids"):
        store.query(q, Metric.Cosine).max_sim().with_row_ids([1, 2]).validate()
    with pytest.raises(OttersError, match="max_sim cannot be combined with one_per_group"):
        store.query(q, Metric.Cosine).max_sim().one_per_group().validate()
    with pytest.raises(OttersError, match="max_sim cannot be combined with per_query"):
        store.query(q, Metric.Cosine).per_query().max_sim().validate()
    store.query(q, Metric.Cosine).max_sim().with_row_mask(np.ones(100, bool)).validate()


def test_group_labels_round_trip(monkeypatch):
    store = VecStore(4)
    store._n = 6
    sent = {}
    monkeypatch.setattr(VecStore, "_set_dense_groups", lambda self, dense, n_groups: sent.update(dense=dense, n=n_groups))
    assert store.group_labels() is None
    labels = np.array([40, -3, 40, 7, 7, 2 ** 40], dtype=np.int64)
    store.set_groups(labels)
    assert store.group_labels().tolist() == [-3, 7, 40, 2 ** 40] and sent["n"] == 4
    assert np.array_equal(store.group_labels()[sent["dense"]], labels)  # [dense id] = the caller's label
    monkeypatch.undo()
    store.clear_groups()  # (no handle: nothing reaches the library)
    assert store.group_labels() is None and store.group_count() == 0


def test_dense_ids_carry_no_labels(monkeypatch):
    from otters_amd import _native as N

    class Lib:
        def ott_store_set_groups(self, *a):
            return 0

    store = VecStore(4)
    store._n = 3
    store._group_labels = np.array([5, 6])
    monkeypatch.setattr(N, "lib", lambda: Lib())
    monkeypatch.setattr(VecStore, "_handle", lambda self: None)
    store._set_dense_groups(np.array([0, 1, 1], np.uint32), 2)
    assert store.group_labels() is None and store.group_count() == 2


# ---- the library ----------------------------------------------------------------------------------------------------------------

def test_library_refuses_from_the_descriptor_alone_without_a_device():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    out = np.zeros(4, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)
    q = np.zeros(8, np.float32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, 2, int(Metric.Cosine), 1, 4
    d.mode = int(Mode.PerQuery)
    assert L.ott_query_maxsim(None, C.byref(d), N.ptr(out), 4, C.byref(n_out), None) == -4
    assert b"tokens of ONE query" in L.ott_last_error()
    d.mode, d.path = int(Mode.Merged), int(Path.Mfma)
    assert L.ott_query_maxsim(None, C.byref(d), N.ptr(out), 4, C.byref(n_out), None) == -4
    assert b"MFMA path does not serve late-interaction" in L.ott_last_error()
    d.path = int(Path.Auto)
    assert L.ott_query_maxsim(None, C.byref(d), N.ptr(out), 4, C.byref(n_out), None) == -1
    assert b"ott_query_maxsim: store is NULL" in L.ott_last_error()
    assert n_out.value == 9  # nothing was touched
