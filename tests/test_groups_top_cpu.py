"""CPU: the host side of grouped search with up to m hits per group (VecQueryPlan.per_group, MetaQueryPlan.distinct_by(keep=);
DESIGN.md 3.1g) — plan resolution, defaults and the refusal strings — and the arguments the device code rests on, in numpy:

  - the CASCADE of group_top_sweep_kernel, modelled as threads that take one memory step at a time under randomly drawn
    schedules (loads may return an older value of the slot), always ends with each group's m largest keys, descending;
  - "the first m hits of each group of the canonical ranking, the first k groups, each group's hits contiguous" IS "the m largest
    keys per group, the groups by their largest key", on quantised scores with ties and signed zeros;
  - why a multi-GPU store is refused: per-shard lists of k groups do not contain the answer for m > 1 (a counter-example)."""
import numpy as np
import pytest

from otters_amd import Cmp, Column, DataType, MetaStore, Metric, Mode, OttersError, VecStore


# ---- plans --------------------------------------------------------------------------------------------------------------------

def store_of(n=100, n_groups=7):
    store = VecStore(4)
    store._n, store._n_groups = n, n_groups  # (no GPU: lengths as set_groups would leave them)
    return store


def test_per_group_resolves_and_defaults_to_the_group_count():
    store = store_of()
    rq = store.query([1, 0, 0, 0], Metric.Cosine).per_group(3).resolve()
    assert rq.grouped and rq.group_size == 3 and rq.k == 7 and not rq.max_sim
    rq = store.query([1, 0, 0, 0], Metric.Cosine).per_group(16).take(2).resolve()
    assert rq.grouped and rq.group_size == 16 and rq.k == 2
    rq = store.query([1, 0, 0, 0], Metric.Cosine).per_group(1).resolve()  # per_group(1) is one_per_group(), through the new entry point
    assert rq.grouped and rq.group_size == 1 and rq.k == 7
    rq = store.query([[1, 0, 0, 0], [0, 1, 0, 0]], Metric.Euclidean).per_group(np.int64(2)).per_query().take(3).resolve()
    assert rq.group_size == 2 and rq.mode == int(Mode.PerQuery) and rq.take == 0
    # plans without per_group are what they were
    rq = store.query([1, 0, 0, 0], Metric.Cosine).one_per_group().resolve()
    assert rq.grouped and rq.group_size == 0 and rq.group_of_hit is None
    assert store.query([1, 0, 0, 0], Metric.Cosine).resolve().group_size == 0


def test_per_group_refusals_at_validate():
    store = store_of()
    q = [1, 0, 0, 0]
    for bad in (0, 17, -1, 2.0, "3", True):
        with pytest.raises(OttersError, match=r"per_group: the group size must be an integer 1 \.\. 16"):
            store.query(q, Metric.Cosine).per_group(bad).validate()
    with pytest.raises(OttersError, match="per_group cannot be combined with with_row_ids"):
        store.query(q, Metric.Cosine).per_group(2).with_row_ids([1, 2]).validate()
    with pytest.raises(OttersError, match="max_sim cannot be combined with per_group"):
        store.query(q, Metric.Cosine).per_group(2).max_sim().validate()
    with pytest.raises(OttersError, match="collect_groups needs a per_group"):
        store.query(q, Metric.Cosine).one_per_group().collect_groups()
    store.query(q, Metric.Cosine).per_group(2).with_row_mask(np.ones(100, bool)).filter(0.5, Cmp.Gt).validate()


def test_per_group_on_an_empty_store_returns_three_empty_things():
    store = store_of(0, 0)
    hits, counts, groups = store.query([1, 0, 0, 0], Metric.Cosine).per_group(3).collect_arrays()
    assert hits.size == 0 and counts == [0] and groups.size == 0 and groups.dtype == np.uint32
    assert store.query([1, 0, 0, 0], Metric.Cosine).per_group(3).collect() == []
    assert store.query([1, 0, 0, 0], Metric.Cosine).per_group(3).collect_groups() == []


def meta_store(n=12):
    doc = Column("doc", DataType.Int64).from_([5, 5, None, 9, 9, 9, None, 2, 5, 2, None, 9])
    f = Column("f", DataType.Float32).from_([0.5] * n)
    return MetaStore({c.name(): c.dtype() for c in (doc, f)}, {c.name(): c for c in (doc, f)}, 4, n, 3, 3, None, {}, {}, {})


def test_distinct_by_keep_resolves_and_refuses():
    st = meta_store()
    rq, _, _ = st.query([1, 0, 0], Metric.Cosine).distinct_by("doc").resolve()
    assert rq.grouped and rq.group_size == 0 and rq.k == 6  # keep defaults to 1: the query it always was
    rq, _, _ = st.query([1, 0, 0], Metric.Cosine).distinct_by("doc", keep=1).resolve()
    assert rq.grouped and rq.group_size == 0
    rq, _, _ = st.query([1, 0, 0], Metric.Cosine).distinct_by("doc", keep=3).resolve()
    assert rq.grouped and rq.group_size == 3 and rq.k == 6 and rq.mode == int(Mode.Merged)
    rq, _, _ = st.query([1, 0, 0], Metric.Cosine).distinct_by("doc", keep=16).take(2).vec_filter(0.1, Cmp.Gt).resolve()
    assert rq.group_size == 16 and rq.k == 2 and rq.filter_cmp == int(Cmp.Gt)
    for bad in (0, 17, 1.5, None, True):
        with pytest.raises(OttersError, match=r"distinct_by: keep must be an integer 1 \.\. 16"):
            st.query([1, 0, 0], Metric.Cosine).distinct_by("doc", keep=bad).resolve()
    # today's refusals, unchanged by keep
    with pytest.raises(OttersError, match="Float column"):
        st.query([1, 0, 0], Metric.Cosine).distinct_by("f", keep=2).resolve()
    with pytest.raises(OttersError, match="unknown column 'nope'"):
        st.query([1, 0, 0], Metric.Cosine).distinct_by("nope", keep=2).resolve()
    with pytest.raises(OttersError, match="one query, not a batch"):
        st.query_batch([[1, 0, 0], [0, 1, 0]], Metric.Cosine).distinct_by("doc", keep=2).resolve()
    with pytest.raises(OttersError, match="cannot be combined with with_row_ids"):
        st.query([1, 0, 0], Metric.Cosine).distinct_by("doc", keep=2).with_row_ids([1]).resolve()


# ---- keys and the two formulations ----------------------------------------------------------------------------------------------

def ord_of(score, take_max):
    b = score.astype(np.float32).view(np.uint32).astype(np.uint64)
    key = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    return key if take_max else (~key & np.uint64(0xFFFFFFFF))


def keys_of(score, rows, take_max):
    return (ord_of(score, take_max) << np.uint64(32)) | (~rows.astype(np.uint64) & np.uint64(0xFFFFFFFF))


def rows_of(keys):
    return (~keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def by_ranking(score, gid, keep, k, m, take_max):
    """the contract, literally: walk the canonical ranking (better score, lower row); keep a hit iff fewer than m earlier hits
    have its group; groups by their first hit, the first k of them, each group's hits contiguous in the ranking's order"""
    rows = np.flatnonzero(keep)
    order = rows[np.lexsort((rows, -ord_of(score[rows], take_max).astype(np.int64)))]
    seen, per = [], {}
    for r in order.tolist():
        g = int(gid[r])
        if g not in per:
            per[g] = []
            seen.append(g)
        if len(per[g]) < m:
            per[g].append(r)
    return [(g, per[g]) for g in seen[:k]]


def by_table(table, k):
    """the device's way, from a finished table [m][n_groups] (0 = empty): groups by their level-0 key, the k largest; a group's
    hits are its non-empty slots from level 0 down"""
    top = table[0]
    groups = np.flatnonzero(top != 0)
    groups = groups[np.argsort(top[groups])[::-1]][:k]
    return [(int(g), rows_of(table[:, g][table[:, g] != 0]).tolist()) for g in groups]


def table_by_sort(keys, gid, n_groups, m):
    table = np.zeros((m, n_groups), np.uint64)
    for g in range(n_groups):
        kg = np.sort(keys[gid == g])[::-1][:m]
        table[: kg.size, g] = kg
    return table


def quantised_scores(rng, n, dim=6):
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)  # quantised: equal scores inside a group and between groups
    q = rng.integers(-2, 3, dim).astype(np.float32)
    score = (rows @ q).astype(np.float32)
    zeros = np.flatnonzero(score == 0)[:4]
    score[zeros[::2]] = np.float32(0.0) * np.float32(-1.0)  # signed zeros order by the total order
    return score


@pytest.mark.parametrize("take_max", [True, False])
def test_m_largest_keys_per_group_is_first_m_of_each_group_of_the_ranking(take_max):
    rng = np.random.default_rng(21)
    n = 400
    score = quantised_scores(rng, n)
    assert np.signbit(score[score == 0]).any() and not np.signbit(score[score == 0]).all()
    for n_groups in (1, 2, 37, 200, n):
        gid = rng.integers(0, n_groups, n) if n_groups < n else rng.permutation(n)
        if n_groups == 200:
            gid = np.arange(n) // 2  # groups shorter than m
        keep = rng.random(n) < 0.8
        rows = np.flatnonzero(keep)
        keys = keys_of(score[rows], rows, take_max)
        for m in (1, 2, 3, 8, 16):
            table = table_by_sort(keys, gid[rows], n_groups, m)
            for k in (1, 10, 64, n):
                a, b = by_ranking(score, gid, keep, k, m, take_max), by_table(table, k)
                assert a == b, (n_groups, m, k)
                assert all(1 <= len(h) <= m for _, h in a) and len({g for g, _ in a}) == len(a)
            if m == 1:  # ott_query_groups' answer: the first hit of every group
                flat = [h[0] for _, h in by_ranking(score, gid, keep, 10, 1, take_max)]
                order = rows[np.lexsort((rows, -ord_of(score[rows], take_max).astype(np.int64)))]
                _, first = np.unique(gid[order], return_index=True)
                assert flat == order[np.sort(first)][:10].tolist()


# ---- the cascade under arbitrary interleavings ------------------------------------------------------------------------------------

class Memory:
    """slots that only rise, with their history: a load may return ANY earlier value of the slot (a stale read past a cache), an
    atomic always acts on the current one"""

    def __init__(self, m, n_groups, rng, stale):
        self.hist = [[[0] for _ in range(n_groups)] for _ in range(m)]
        self.rng, self.stale = rng, stale
        self.atomics = 0

    def load(self, j, g):
        h = self.hist[j][g]
        return h[int(self.rng.integers(0, len(h)))] if self.stale else h[-1]

    def atomic_max(self, j, g, key):
        h = self.hist[j][g]
        old = h[-1]
        if key > old:
            h.append(key)
        self.atomics += 1
        return old

    def table(self):
        return np.array([[h[-1] for h in level] for level in self.hist], dtype=np.uint64)


def cascade_thread(mem, key, g, m):
    """group_top_sweep_kernel's epilogue for one passing (row, query) pair, one memory operation per step"""
    if not key > (yield lambda: mem.load(m - 1, g)):  # the group's current m-th best: no cascade for a key that does not beat it
        return
    for j in range(m):
        if key > (yield lambda: mem.load(j, g)):
            old = yield lambda: mem.atomic_max(j, g, key)
            if old < key:  # the slot is this key's now: what it held walks on
                if old == 0:
                    return
                key = old


def run_schedule(keys, gid, n_groups, m, rng, schedule, stale):
    mem = Memory(m, n_groups, rng, stale)
    threads = [cascade_thread(mem, int(k), int(g), m) for k, g in zip(keys.tolist(), gid.tolist())]
    pending = {}
    for i, t in enumerate(threads):  # every thread stands in front of its first memory operation
        pending[i] = next(t)
    live = list(pending)
    pos = 0
    while live:
        if schedule == "random":
            at = int(rng.integers(0, len(live)))
        elif schedule == "round robin":  # everyone passes the pre-check on an empty table, then they all collide
            at = pos % len(live)
        else:  # "one after the other": no concurrency at all
            at = 0
        i = live[at]
        try:
            pending[i] = threads[i].send(pending[i]())
            pos += 1
        except StopIteration:
            live.pop(at)
    return mem


@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_every_schedule_of_the_cascade_ends_with_the_m_largest_keys_descending(m):
    rng = np.random.default_rng(30 + m)
    n = 160
    score = quantised_scores(rng, n)
    rows = np.arange(n)
    for take_max in (True, False):
        keys = keys_of(score, rows, take_max)
        assert np.unique(keys).size == n  # rows are distinct, so keys are
        for n_groups in (1, 5, 80):
            gid = rng.integers(0, n_groups, n) if n_groups != 80 else np.arange(n) // 2
            want = table_by_sort(keys, gid, n_groups, m)
            for order in ("as is", "ascending", "descending"):  # ascending: every key displaces the whole column
                perm = {"as is": rows, "ascending": np.argsort(keys), "descending": np.argsort(keys)[::-1]}[order]
                for schedule, stale, reps in (("one after the other", False, 1), ("round robin", False, 1), ("round robin", True, 2), ("random", True, 4)):
                    for _ in range(reps):
                        mem = run_schedule(keys[perm], gid[perm], n_groups, m, rng, schedule, stale)
                        assert np.array_equal(mem.table(), want), (m, take_max, n_groups, order, schedule, stale)
            # what the pre-check is for: without concurrency and with the best keys first, only the m best of a group reach an atomic
            mem = run_schedule(keys[np.argsort(keys)[::-1]], gid[np.argsort(keys)[::-1]], n_groups, m, rng, "one after the other", False)
            assert mem.atomics == int((want != 0).sum())


# ---- why a multi-GPU store is refused --------------------------------------------------------------------------------------------

def test_shard_lists_of_k_groups_do_not_contain_the_answer_for_m_above_one():
    """Two shards, k = 1, m = 2.  Group A's best row is in shard 0 and its second best in shard 1, where group B's row beats it:
    shard 1's list of k = 1 groups holds B only, so A's second hit is in no shard's list.  (For m = 1 the same lists suffice:
    tests/test_groups_cpu.py.)"""
    #                 shard 0      | shard 1
    score = np.array([9.0, 1.0, 0.5, 8.0, 7.0, 0.25], np.float32)
    gid = np.array([0, 2, 2, 1, 0, 1])  # A = 0, B = 1
    bounds = (0, 3, 6)
    keep = np.ones(6, bool)
    for m, suffices in ((1, True), (2, False)):
        k = 1
        want = by_ranking(score, gid, keep, k, m, True)
        listed = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):  # every shard: its own answer over its rows
            local = np.zeros(6, bool)
            local[lo:hi] = True
            listed += [r for _, hits in by_ranking(score, gid, local, k, m, True) for r in hits]
        got = by_ranking(score, gid, np.isin(np.arange(6), listed), k, m, True)  # the best a merging host can do with the lists
        assert (got == want) == suffices, (m, got, want)
    assert by_ranking(score, gid, keep, 1, 2, True) == [(0, [0, 4])]
