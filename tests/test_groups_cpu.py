"""CPU: the host side of grouped search (VecQueryPlan.one_per_group, MetaQueryPlan.distinct_by) — plan
validation and its error strings, how labels become dense group ids (NULL rows and String columns included), and the two
arguments the device code rests on, checked in numpy: "the largest candidate key of every group, then the top-k of those" IS
"the full canonical ranking, the first hit of every group, cut at k"; and per-shard top-k lists of group bests, merged with
duplicates removed, give the global answer."""
import numpy as np
import pytest

from otters_amd import Cmp, Column, DataType, MetaStore, Metric, OttersError, VecStore, col
from otters_amd.vec import dense_group_ids


# ---- plans --------------------------------------------------------------------------------------------------------------------

def test_one_per_group_resolves_and_defaults_to_the_group_count():
    store = VecStore(4)
    store._n, store._n_groups = 100, 7  # (no GPU: lengths as set_groups would leave them)
    rq = store.query([1, 0, 0, 0], Metric.Cosine).one_per_group().resolve()
    assert rq.grouped and rq.k == 7
    rq = store.query([1, 0, 0, 0], Metric.Cosine).one_per_group().take(3).resolve()
    assert rq.grouped and rq.k == 3
    rq = store.query([1, 0, 0, 0], Metric.Cosine).take(3).resolve()
    assert not rq.grouped and rq.k == 3
    assert store.query([1, 0, 0, 0], Metric.Cosine).resolve().k == 100


def test_one_per_group_with_row_ids_is_refused_at_validate():
    store = VecStore(4)
    store._n, store._n_groups = 100, 7
    plan = store.query([1, 0, 0, 0], Metric.Cosine).one_per_group().with_row_ids([1, 2])
    with pytest.raises(OttersError, match="one_per_group cannot be combined with with_row_ids"):
        plan.validate()
    store.query([1, 0, 0, 0], Metric.Cosine).one_per_group().with_row_mask(np.ones(100, bool)).validate()


def test_set_groups_checks_the_length_before_the_library():
    store = VecStore(4)
    store._n = 5
    with pytest.raises(OttersError, match="3 group ids for a store of 5 rows"):
        store.set_groups([0, 1, 2])
    assert store.group_count() == 0


# ---- densification ------------------------------------------------------------------------------------------------------------

def test_dense_group_ids():
    ids, n = dense_group_ids(np.array([40, -3, 40, 7, 7, 2 ** 40], dtype=np.int64))
    assert ids.dtype == np.uint32 and n == 4
    assert ids.tolist() == [2, 0, 2, 1, 1, 3]
    ids, n = dense_group_ids(np.zeros(0, np.int32))
    assert ids.size == 0 and n == 0
    ids, n = dense_group_ids([9, 9, 9])
    assert ids.tolist() == [0, 0, 0] and n == 1
    for bad in (np.array([0.5, 1.0]), np.array([True, False]), np.array(["a", "b"])):
        with pytest.raises(OttersError, match="group ids must be integers"):
            dense_group_ids(bad)


def meta_store(n=12):
    doc = Column("doc", DataType.Int64).from_([5, 5, None, 9, 9, 9, None, 2, 5, 2, None, 9])
    tag = Column("tag", DataType.String).from_(["b", "a", "b", None, "c", "a", "a", None, "b", "c", "c", "a"])
    day = Column("day", DataType.DateTime).from_([10, 10, 20, 20, 30, 30, 10, 10, 20, 20, 30, 30])
    i32 = Column("i32", DataType.Int32).from_([1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3])
    f = Column("f", DataType.Float32).from_([0.5] * n)
    # (no vectors: the store is a host-only object here)
    return MetaStore({c.name(): c.dtype() for c in (doc, tag, day, i32, f)}, {c.name(): c for c in (doc, tag, day, i32, f)}, 4, n, 3, 3,
                     None, {}, {}, {})


def same_partition(ids, labels):
    """ids[i] == ids[j] exactly when labels[i] == labels[j] (None = a label of its own)"""
    n = len(labels)
    for i in range(n):
        for j in range(n):
            same = labels[i] is not None and labels[i] == labels[j] or i == j
            assert (ids[i] == ids[j]) == same, (i, j)


def test_distinct_ids_by_value_nulls_are_groups_of_their_own():
    st = meta_store()
    ids, n = st._distinct_ids("doc")
    assert ids.dtype == np.uint32 and n == 3 + 3 and int(ids.max()) == n - 1
    same_partition(ids.tolist(), [5, 5, None, 9, 9, 9, None, 2, 5, 2, None, 9])
    assert st._distinct_ids("doc")[0] is ids  # built once per column name
    ids, n = st._distinct_ids("tag")
    assert n == 3 + 2
    same_partition(ids.tolist(), ["b", "a", "b", None, "c", "a", "a", None, "b", "c", "c", "a"])
    assert st._distinct_ids("day")[1] == 3 and st._distinct_ids("i32")[1] == 3


def test_distinct_by_refusals():
    st = meta_store()
    with pytest.raises(OttersError, match="Float column"):
        st.query([1, 0, 0], Metric.Cosine).distinct_by("f").resolve()
    with pytest.raises(OttersError, match="unknown column 'nope'"):
        st.query([1, 0, 0], Metric.Cosine).distinct_by("nope").resolve()
    with pytest.raises(OttersError, match="one query, not a batch"):
        st.query_batch([[1, 0, 0], [0, 1, 0]], Metric.Cosine).distinct_by("doc").resolve()
    with pytest.raises(OttersError, match="cannot be combined with with_row_ids"):
        st.query([1, 0, 0], Metric.Cosine).distinct_by("doc").with_row_ids([1]).resolve()
    rq, _, _ = st.query([1, 0, 0], Metric.Cosine).distinct_by("doc").resolve()
    assert rq.grouped and rq.k == 6
    rq, _, _ = st.query([1, 0, 0], Metric.Cosine).distinct_by("doc").take(2).vec_filter(0.1, Cmp.Gt).resolve()
    assert rq.grouped and rq.k == 2 and rq.filter_cmp == int(Cmp.Gt)


# ---- the two arguments, in numpy ------------------------------------------------------------------------------------------------

def ord_of(score, take_max):
    b = score.astype(np.float32).view(np.uint32).astype(np.uint64)
    key = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    return key if take_max else (~key & np.uint64(0xFFFFFFFF))


def keys_of(score, rows, take_max):
    return (ord_of(score, take_max) << np.uint64(32)) | (~rows.astype(np.uint64) & np.uint64(0xFFFFFFFF))


def by_ranking(score, gid, keep, k, take_max):
    """full canonical ranking (better score, lower row), first hit of every group, cut at k"""
    rows = np.flatnonzero(keep)
    order = rows[np.lexsort((rows, -ord_of(score[rows], take_max).astype(np.int64)))]
    _, first = np.unique(gid[order], return_index=True)
    return order[np.sort(first)][:k]


def by_table(score, gid, keep, k, take_max, n_groups):
    """the device's way: slot = max key of the group (0 = empty), then the k largest slots"""
    rows = np.flatnonzero(keep)
    table = np.zeros(n_groups, np.uint64)
    np.maximum.at(table, gid[rows], keys_of(score[rows], rows, take_max))
    table = np.sort(table[table != 0])[::-1][:k]
    return (~table & np.uint64(0xFFFFFFFF)).astype(np.int64)


@pytest.mark.parametrize("take_max", [True, False])
def test_max_key_per_group_then_top_k_is_first_of_each_group_of_the_ranking(take_max):
    rng = np.random.default_rng(11)
    n, dim = 400, 6
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)  # quantised: equal scores inside a group and between groups
    q = rng.integers(-2, 3, dim).astype(np.float32)
    score = (rows @ q).astype(np.float32)
    score[[3, 77]] = np.float32(0.0) * np.float32(-1.0)  # signed zeros order by the total order
    for n_groups in (1, 2, 37, n):
        gid = rng.integers(0, n_groups, n) if n_groups < n else rng.permutation(n)
        keep = rng.random(n) < 0.8
        in_group = {g: score[(gid == g) & keep] for g in range(min(n_groups, 37))}
        assert n_groups == n or any(np.unique(s).size < s.size for s in in_group.values())  # ties inside a group occur
        for k in (1, 10, 64, n):
            a, b = by_ranking(score, gid, keep, k, take_max), by_table(score, gid, keep, k, take_max, n_groups)
            assert np.array_equal(a, b), (n_groups, k)
            assert np.unique(gid[a]).size == a.size


def test_shard_lists_of_k_merged_and_deduplicated_are_the_global_answer():
    rng = np.random.default_rng(12)
    n, k_all = 500, (1, 7, 40, 500)
    score = rng.integers(-3, 4, n).astype(np.float32)
    for trial in range(20):
        n_groups = int(rng.choice([1, 2, 13, 90, n]))
        gid = rng.integers(0, n_groups, n)
        keep = rng.random(n) < 0.9
        cuts = np.sort(rng.choice(np.arange(1, n), 3, replace=False))
        bounds = [0, *cuts.tolist(), n]
        for k in k_all:
            want = by_ranking(score, gid, keep, k, True)
            cat = []
            for lo, hi in zip(bounds[:-1], bounds[1:]):  # every shard: its own grouped top-k over its rows
                local = np.zeros(n, bool)
                local[lo:hi] = keep[lo:hi]
                cat.append(by_ranking(score, gid, local, k, True))
            cat = np.concatenate(cat)
            got = by_ranking(score, gid, np.isin(np.arange(n), cat), k, True)  # concatenate, canonical order, first of each group, cut
            assert np.array_equal(got, want), (trial, k)
