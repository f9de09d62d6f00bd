"""What reaches the native boundary (CPU, no library needed): every ott_query* entry of the Python layer is run against a fake
library that records its arguments and snapshots the ott_query_desc it is handed -- the scalar fields, which pointers are null,
and, for the masks and the query matrix, the words READ THROUGH THE POINTER DURING THE CALL (so an array that was not kept alive
until the call shows as garbage).  The fake leaves n_out at 0.  Expected values are written out here from the plans' arguments.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import pytest

from otters_amd import _native as N
from otters_amd import BoostTerm, Cmp, Column, DataType, Metric, MetaStore, Mode, OttersError, Path, RecommendStrategy, VecStore, col
from otters_amd.dist import Comm, ShardedVecStore

N_ROWS, DIM, CHUNK, N_GROUPS = 40, 8, 16, 5
HANDLE, COMM_HANDLE = 0x5EED, 7
RNG = np.random.default_rng(7)
ROWS = RNG.uniform(-1, 1, (65, DIM)).astype(np.float32)
Q1 = RNG.uniform(-1, 1, (1, DIM)).astype(np.float32)
Q3 = RNG.uniform(-1, 1, (3, DIM)).astype(np.float32)
TARGET = RNG.uniform(-1, 1, DIM).astype(np.float32)
PAIRS = [(1, 2), (3, 4)]
SPARSE1 = ([1, 3], [0.5, 1.0])
SPARSE3 = [([1, 3], [0.5, 1.0]), ([2], [2.0]), ([0, 4, 5], [1.0, 1.0, 1.0])]
EUC, MIN, MAX = int(Metric.Euclidean), 0, 1
DESC_SCALARS = ("nq", "metric", "take", "filter_cmp", "filter_thr", "mode", "k", "row_mask_bits", "use_device_row_mask", "path")
ZERO_STATS = N.Stats().as_dict()


def words_of(bools):
    """bit i of word i // 64 = bools[i], as Python integers; an empty sequence is one zero word"""
    b = [bool(x) for x in bools]
    return [sum(1 << j for j, x in enumerate(b[i:i + 64]) if x) for i in range(0, len(b), 64)] or [0]


def row_mask(size):
    return np.arange(size) % 3 != 1


class FakeLib:
    def __init__(self):
        self.calls, self.queries, self.n_chunks = [], [], 0
        self.fill = False  # True: an ott_query* call reports its output buffer as full (n_out = cap) and notes the buffer's address

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name == "ott_store_create":
                args[2]._obj.value = HANDLE
            if name.startswith("ott_query"):
                self.queries.append((name, args, self._snapshot(args)))
                if self.fill:  # (..., out, cap, &n_out, ...) in every entry
                    at = next(i for i, a in enumerate(args) if type(getattr(a, "_obj", None)) is C.c_uint64)
                    args[at]._obj.value, self.out_address = args[at - 1], args[at - 2].value
            return 0
        return call

    def _read_words(self, address, bits):
        return np.frombuffer(C.string_at(address, 8 * max((bits + 63) // 64, 1)), dtype="<u8").tolist()

    def _snapshot(self, args):
        d = next(a._obj for a in args if isinstance(getattr(a, "_obj", None), N.QueryDesc))
        # a packed mask that nothing references any more has gone back to NumPy's small-block cache: these take it over
        scribble = [np.full(size, 0xFF, dtype=np.uint8) for size in (8, 16) for _ in range(16)]  # noqa: F841
        snap ={f: getattr(d, f) for f in DESC_SCALARS}
        snap["queries"] = None if not d.queries else np.frombuffer(C.string_at(d.queries, 4 * d.nq * DIM), dtype=np.float32).copy()
        snap["chunk_mask"] = None if not d.chunk_mask else self._read_words(d.chunk_mask, self.n_chunks)
        snap["row_mask"] = None if not d.row_mask else self._read_words(d.row_mask, d.row_mask_bits)
        return snap

    def names(self):
        return [name for name, _ in self.calls]


@pytest.fixture
def native(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(N, "lib", lambda: fake)
    made = []

    def store(n=N_ROWS):
        s = VecStore(DIM, device=0)
        s.set_chunk_size(CHUNK)
        s.add_vectors(ROWS[:n])
        s.set_groups(np.arange(n) % N_GROUPS)
        made.append(s)
        fake.n_chunks = -(-n // CHUNK)
        return s

    fake.store = store
    yield fake
    for s in made:  # the handle is the fake's: nothing may reach a real library with it once the patch is undone
        s._h = None


# ---- the plans' own _run* entries ------------------------------------------------------------------------------------------------------
P = "any non-null pointer"


@dataclass
class Kind:
    entry: str
    make: Callable            # store -> plan
    run: str                  # the _run* method of plan.vector_store
    nq: int
    mode: int
    default_take: int         # no take call
    default_k: int            # no take call
    args: Callable            # (resolved, k, cap) -> expected arguments after (store handle, descriptor)
    cap: Callable             # k -> the output capacity the call names
    metric: int = EUC
    inferred_take: int = MIN  # take(n) without a type: Euclidean distances rank ascending
    queries: Optional[np.ndarray] = None
    has_path: bool = True
    forced_take: Optional[int] = None    # a kind that refuses to run without a take
    second: object = None                # the second element of the returned tuple; default: [0] * nq
    n_returned: int = 3
    extra_stats: tuple = ()
    tag: str = ""


def sharded(store):
    comm = Comm(C.c_void_p(COMM_HANDLE), 0, 1)
    comm._fin.detach()  # (the handle is not a real one)
    return ShardedVecStore(store, comm, global_rows=N_ROWS).query(Q1, Metric.Euclidean)


EMPTY_U32 = np.zeros(0, np.uint32)
TAIL = ["n_out", ("per", 1), "stats"]
KINDS = [
    Kind("ott_query", lambda s: s.query(Q1, Metric.Euclidean), "_run", 1, Mode.Merged, MAX, N_ROWS,
         lambda r, k, cap: [P, cap] + TAIL, lambda k: min(k, N_ROWS), queries=Q1),
    Kind("ott_query_ids", lambda s: s.query(Q1, Metric.Euclidean).with_row_ids([3, 1, 7, 3]), "_run", 1, Mode.Merged, MAX, N_ROWS,
         lambda r, k, cap: [r.row_ids, 4, P, cap] + TAIL, lambda k: min(k, 3), queries=Q1),
    Kind("ott_query_groups", lambda s: s.query(Q1, Metric.Euclidean).one_per_group(), "_run", 1, Mode.Merged, MAX, N_GROUPS,
         lambda r, k, cap: [P, cap] + TAIL, lambda k: min(k, N_GROUPS), queries=Q1),
    Kind("ott_query_groups_top", lambda s: s.query(Q1, Metric.Euclidean).per_group(2), "_run", 1, Mode.Merged, MAX, N_GROUPS,
         lambda r, k, cap: [2, P, cap, "n_out", ("per", 1), P, "stats"], lambda k: 2 * min(k, N_GROUPS), queries=Q1),
    Kind("ott_query_maxsim", lambda s: s.query(Q3, Metric.Euclidean).max_sim(), "_run", 3, Mode.Merged, MAX, N_GROUPS,
         lambda r, k, cap: [P, cap, "n_out", "stats"], lambda k: min(k, N_GROUPS), queries=Q3, second=[0, 0, 0]),
    Kind("ott_query_maxsim_groups", lambda s: s.query(Q3, Metric.Euclidean).max_sim().with_groups([4, 1, 1]), "_run", 3, Mode.Merged, MAX, 2,
         lambda r, k, cap: [r.group_list, 3, P, cap, "n_out", "stats"], lambda k: min(k, 2), queries=Q3, second=[0, 0, 0],
         extra_stats=(("group_index_builds", 0),)),
    Kind("ott_query_maxsim_groups_batch", lambda s: s.max_sim_batch([Q3[:2], Q3[2:]], Metric.Euclidean).with_groups([[0, 2], [3, 3, 1, 4]]),
         "_run_maxsim_batch", 3, Mode.Merged, MAX, 3,
         lambda r, k, cap: [r.tokens_per_query, r.listed_per_query, 2, r.groups, P, cap, "n_out", ("per", 2), "stats"],
         lambda k: min(k, 2) + min(k, 3), queries=Q3, has_path=False, second=[0, 0], extra_stats=(("group_index_builds", 0),)),
    Kind("ott_query_mmr", lambda s: s.query(Q1, Metric.Euclidean).mmr(0.5), "_run", 1, Mode.Merged, MIN, 3,
         lambda r, k, cap: [None, 0, min(1024, max(20, 5 * k)), 0.5, P, cap, "n_out", ("per", 1), P, "stats"], lambda k: min(k, N_ROWS),
         queries=Q1, forced_take=3),
    Kind("ott_query_masks", lambda s: s.query(Q3, Metric.Euclidean).per_query().with_row_masks([row_mask(N_ROWS), None, row_mask(N_ROWS)]), "_run",
         3, Mode.PerQuery, MAX, N_ROWS,
         lambda r, k, cap: [P, 1, N_ROWS, P, P, cap, "n_out", ("per", 3), "stats"], lambda k: 3 * min(k, N_ROWS), queries=Q3),
    Kind("ott_query_boost", lambda s: s.query(Q1, Metric.Euclidean).boost([BoostTerm.value(0, 1.0)]), "_run", 1, Mode.Merged, MAX, N_ROWS,
         lambda r, k, cap: [0, 1.0, ("array", 1), 1, P, cap] + TAIL, lambda k: min(k, N_ROWS), queries=Q1),
    Kind("ott_query_recommend", lambda s: s.recommend([1, 2], [3], Metric.Euclidean), "_run_recommend", 0, Mode.Merged, MIN, N_ROWS,
         lambda r, k, cap: [r.positive, 2, r.negative, 1, 1, P, cap, "n_out", P, "stats"], lambda k: min(k, N_ROWS), second=EMPTY_U32),
    Kind("ott_query_recommend", lambda s: s.recommend([1, 2], [], Metric.Euclidean).fill_negative_side(False), "_run_recommend", 0, Mode.Merged, MIN,
         N_ROWS, lambda r, k, cap: [r.positive, 2, None, 0, 0, P, cap, "n_out", P, "stats"], lambda k: min(k, N_ROWS), second=EMPTY_U32,
         tag="no negatives, no fill"),
    Kind("ott_query_recommend_strategy", lambda s: s.recommend([1, 2], [3], Metric.Euclidean, RecommendStrategy.SumScores), "_run_recommend", 0,
         Mode.Merged, MIN, N_ROWS, lambda r, k, cap: [2, r.positive, 2, r.negative, 1, 0, P, cap, "n_out", P, "stats"], lambda k: min(k, N_ROWS),
         second=EMPTY_U32),
    Kind("ott_query_discover", lambda s: s.discover(PAIRS, target=TARGET, metric=Metric.Euclidean), "_run_discover", 1, Mode.Merged, MIN, N_ROWS,
         lambda r, k, cap: [2 ** 64 - 1, r.positive, r.negative, 2, 0, 0, P, cap, "n_out", P, "stats"], lambda k: min(k, N_ROWS), queries=TARGET,
         second=EMPTY_U32, tag="target vector"),
    Kind("ott_query_discover", lambda s: s.discover(PAIRS, target_row=5, metric=Metric.Euclidean).min_wins(1), "_run_discover", 0, Mode.Merged, MIN,
         N_ROWS, lambda r, k, cap: [5, r.positive, r.negative, 2, 1, 0, P, cap, "n_out", P, "stats"], lambda k: min(k, N_ROWS), second=EMPTY_U32,
         tag="target row"),
    Kind("ott_query_discover", lambda s: s.discover(PAIRS, metric=Metric.Euclidean), "_run_discover", 0, Mode.Merged, MIN, N_ROWS,
         lambda r, k, cap: [2 ** 64 - 1, r.positive, r.negative, 2, 0, 0, P, cap, "n_out", P, "stats"], lambda k: min(k, N_ROWS), second=EMPTY_U32,
         tag="context only"),
    Kind("ott_query_fuse", lambda s: s.fuse([Q3[:2], Q3[2:]], Metric.Euclidean), "_run_fuse", 3, Mode.PerQuery, MIN, N_ROWS,
         lambda r, k, cap: [r.legs_per_request, 2, 0, 60.0, None, min(max(4 * k, 32), 512), P, cap, "n_out", ("per", 2), "stats"],
         lambda k: min(k, 2 * min(max(4 * k, 32), N_ROWS)) + min(k, min(max(4 * k, 32), N_ROWS)), queries=Q3, second=[0, 0]),
    Kind("ott_query_sparse", lambda s: s.sparse_query(SPARSE1), "_run_sparse", 1, Mode.Merged, MAX, N_ROWS,
         lambda r, k, cap: [r.indptr, r.indices, r.values, P, cap, "n_out", ("per", 1), "stats"], lambda k: min(k, N_ROWS),
         metric=int(Metric.DotProduct), inferred_take=MAX, tag="one query"),
    Kind("ott_query_sparse", lambda s: s.sparse_query(SPARSE3), "_run_sparse", 3, Mode.PerQuery, MAX, N_ROWS,
         lambda r, k, cap: [r.indptr, r.indices, r.values, P, cap, "n_out", ("per", 3), "stats"], lambda k: 3 * min(k, N_ROWS),
         metric=int(Metric.DotProduct), inferred_take=MAX, tag="three queries"),
    Kind("ott_query_sharded", sharded, "_run", 1, Mode.Merged, MAX, N_ROWS,
         lambda r, k, cap: [P, cap] + TAIL, lambda k: min(k, N_ROWS), queries=Q1, n_returned=2, tag="k clamped to the corpus"),
]


@dataclass
class Scenario:
    tag: str
    mask_size: Optional[int] = None  # with_row_mask(row_mask(size))
    take: Optional[tuple] = None     # (method, count)
    filt: Optional[tuple] = None     # (threshold, Cmp)
    chunk: bool = False              # chunk_mask=[True, False, True]
    exact: bool = False              # with_path(Path.Exact)
    device: bool = False             # use_device_row_mask=True
    mask_sent: bool = False          # the descriptor carries the caller's row mask


SCENARIOS = [
    Scenario("plain"),
    Scenario("mask shorter than the store, take, filter, chunk mask, path", 24, ("take", 5), (0.25, Cmp.Gt), chunk=True, exact=True, mask_sent=True),
    Scenario("mask as long as the store, take_min", N_ROWS, ("take_min", 7), mask_sent=True),
    Scenario("mask of one word and one bit, take_max above the store", 65, ("take_max", 50), mask_sent=True),
    Scenario("mask of exactly one word, filter", 64, None, (-1.5, Cmp.Lte), mask_sent=True),
    Scenario("mask of size 0 is not sent", 0, ("take", 5)),
    Scenario("the device row mask wins over the caller's", N_ROWS, ("take_max", 7), chunk=True, device=True),
]


def kind_of_argument(a):
    obj = getattr(a, "_obj", None)
    if obj is not None:
        return {N.QueryDesc: "desc", N.Stats: "stats", C.c_uint64: "n_out"}[type(obj)]
    if isinstance(a, C.Array):
        return ("per" if a._type_ is C.c_uint64 else "array", len(a))
    if isinstance(a, C.c_void_p):
        return "handle" if a.value == HANDLE else ("ptr", a.value)
    return a


def assert_arguments(args, expected):
    got = [kind_of_argument(a) for a in args]
    assert len(got) == len(expected), (got, expected)
    for i, (g, e) in enumerate(zip(got, expected)):
        if e is P:
            assert isinstance(g, tuple) and g[0] == "ptr" and g[1], (i, g)
        elif isinstance(e, np.ndarray):
            assert g == ("ptr", e.ctypes.data), (i, g)
        else:
            assert type(g) is type(e) and g == e, (i, g, e)


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s.tag for s in SCENARIOS])
@pytest.mark.parametrize("kind", KINDS, ids=[k.entry + (": " + k.tag if k.tag else "") for k in KINDS])
def test_descriptor_and_arguments(native, kind, sc):
    store = native.store()
    plan = kind.make(store)
    if sc.mask_size is not None:
        assert plan.with_row_mask(row_mask(sc.mask_size)) is plan
    if sc.filt is not None:
        assert plan.filter(*sc.filt) is plan
    take = sc.take if sc.take is not None or kind.forced_take is None else ("take", kind.forced_take)
    if take is not None:
        assert getattr(plan, take[0])(take[1]) is plan
    if sc.exact and kind.has_path:
        assert plan.with_path(Path.Exact) is plan
    resolved = plan.resolve()
    native.calls.clear()
    chunk_mask = np.array([True, False, True]) if sc.chunk else None
    ret = getattr(plan.vector_store, kind.run)(resolved, chunk_mask=chunk_mask, use_device_row_mask=sc.device)

    (name, args, snap), = native.queries
    assert name == kind.entry
    k = kind.default_k if take is None else take[1]
    want = {
        "nq": kind.nq, "metric": kind.metric, "mode": int(kind.mode),
        "take": kind.default_take if take is None else {"take": kind.inferred_take, "take_min": MIN, "take_max": MAX}[take[0]],
        "k": min(k, N_ROWS) if kind.entry == "ott_query_sharded" else k,
        "filter_cmp": 0 if sc.filt is None else int(sc.filt[1]), "filter_thr": 0.0 if sc.filt is None else sc.filt[0],
        "path": int(Path.Exact) if sc.exact and kind.has_path else int(Path.Auto),
        "use_device_row_mask": 1 if sc.device else 0,
        "row_mask_bits": sc.mask_size if sc.mask_sent else 0,
        "row_mask": words_of(row_mask(sc.mask_size)) if sc.mask_sent else None,
        "chunk_mask": [0b101] if sc.chunk else None,
    }
    got_queries = snap.pop("queries")
    assert snap == want
    if kind.queries is None:
        assert got_queries is None
    else:
        assert np.array_equal(got_queries, kind.queries.ravel())

    cap = max(kind.cap(k), 1)
    lead = ["handle", ("ptr", COMM_HANDLE), "desc"] if kind.entry == "ott_query_sharded" else ["handle", "desc"]
    assert_arguments(args, lead + kind.args(resolved, want["k"], cap))

    assert len(ret) == kind.n_returned
    assert ret[0].dtype == N.HIT_DTYPE and ret[0].size == 0
    second = [0] * kind.nq if kind.second is None else kind.second
    if isinstance(second, np.ndarray):
        assert ret[1].dtype == second.dtype and ret[1].size == 0
    else:
        assert ret[1] == second
    if kind.n_returned == 3:
        assert ret[2] == {**ZERO_STATS, **dict(kind.extra_stats)}
    else:
        assert store.last_stats == ZERO_STATS


def test_the_full_buffer_comes_back_without_a_copy(native):
    """_run and _run_maxsim_batch return their output buffer itself when the call filled it"""
    store = native.store()
    native.fill = True
    hits, counts, _ = store._run(store.query(Q1, Metric.Euclidean).take(4).resolve())
    assert hits.size == 4 and hits.ctypes.data == native.out_address
    hits, counts, _ = store._run_maxsim_batch(store.max_sim_batch([Q3[:2], Q3[2:]], Metric.Euclidean).with_groups([[0, 2], [3, 3, 1, 4]]).take(2).resolve())
    assert hits.size == 4 and hits.ctypes.data == native.out_address


def test_empty_stores_make_no_query_call(native):
    empty = VecStore(DIM, device=0)
    assert [x if i != 0 else x.size for i, x in enumerate(empty._run(empty.query(Q3, Metric.Cosine).resolve()))] == [0, [0, 0, 0], None]
    hits, counts, stats = empty._run_fuse(empty.fuse([Q3[:2], Q3[2:]], Metric.Cosine).take(3).resolve())
    assert hits.size == 0 and hits.dtype == N.HIT_DTYPE and counts == [0, 0] and stats == ZERO_STATS
    assert native.calls == []


# ---- the four meta wrappers over a small MetaStore -------------------------------------------------------------------------------------
@dataclass
class MetaKind:
    name: str            # the word in the error message
    entry: str
    make: Callable       # meta store -> plan
    empty: object        # the second element of collect_arrays() when every chunk is pruned
    n_results: Optional[int] = None  # collect() / collect_per_query() return a list of this many MetaQueryResults, or (results, list)


META_KINDS = [
    MetaKind("recommend", "ott_query_recommend", lambda ms: ms.recommend([1, 2], [3], Metric.Euclidean), EMPTY_U32),
    MetaKind("fuse", "ott_query_fuse", lambda ms: ms.fuse([Q3[:2], Q3[2:]], Metric.Euclidean), [0, 0], 2),
    MetaKind("sparse_query", "ott_query_sparse", lambda ms: ms.sparse_query(SPARSE3), [0, 0, 0], 3),
    MetaKind("discover", "ott_query_discover", lambda ms: ms.discover(PAIRS, target=TARGET, metric=Metric.Euclidean), EMPTY_U32),
]
META_IDS = [k.name for k in META_KINDS]
CALLER = np.arange(24) % 2 == 0


def meta_store(native, n=N_ROWS, attach=True):
    cols = [Column("a", DataType.Int32).from_(list(range(n))), Column("f", DataType.Float32).from_([float(i) for i in range(n)])]
    ms = MetaStore.from_columns(cols).with_vectors(ROWS[:n]).with_chunk_size(CHUNK).build(_host_only=True)
    if attach:
        ms._store = native.store(n)
        native.calls.clear()
    return ms


def assert_empty(kind, got):
    hits, second = got
    assert hits.dtype == N.HIT_DTYPE and hits.size == 0
    if isinstance(kind.empty, np.ndarray):
        assert second.dtype == kind.empty.dtype and second.size == 0
    else:
        assert second == kind.empty


def materialised(kind, plan):
    """collect() of an empty answer: the rows' columns in sorted order, no rows"""
    out = plan.collect_per_query() if kind.name == "sparse_query" else plan.collect()
    if kind.n_results is None:
        results, extra = out
        assert extra == []
        results = [results]
    else:
        results = out
        assert len(results) == kind.n_results
    for r in results:
        assert r.columns == ["a", "f"] and sorted(r.data) == ["a", "f"] and r.indices == [] and r.scores == [] and len(r) == 0


@pytest.mark.parametrize("kind", META_KINDS, ids=META_IDS)
def test_meta_every_chunk_pruned(native, kind):
    ms = meta_store(native)
    plan = kind.make(ms).meta_filter(col("a").gt(1000)).take(3)
    assert_empty(kind, plan.collect_arrays())
    assert native.calls == []
    materialised(kind, plan)


@pytest.mark.parametrize("kind", META_KINDS, ids=META_IDS)
def test_meta_no_filter_passes_the_callers_mask_through(native, kind):
    ms = meta_store(native)
    plan = kind.make(ms).vec_filter(0.25, Cmp.Lt).take_max(3).with_row_mask(CALLER).with_path(Path.Exact)
    assert_empty(kind, plan.collect_arrays())
    (name, _, snap), = native.queries
    assert name == kind.entry and native.names() == [kind.entry]
    assert (snap["chunk_mask"], snap["use_device_row_mask"], snap["row_mask_bits"], snap["row_mask"]) == (None, 0, 24, words_of(CALLER))
    assert (snap["take"], snap["k"], snap["filter_cmp"], snap["filter_thr"], snap["path"]) == (MAX, 3, int(Cmp.Lt), 0.25, int(Path.Exact))
    assert ms._store.last_stats == ZERO_STATS
    materialised(kind, plan)


@pytest.mark.parametrize("kind", META_KINDS, ids=META_IDS)
def test_meta_filter_decided_by_the_zone_maps(native, kind):
    ms = meta_store(native)
    plan = kind.make(ms).meta_filter(col("a").lt(32)).take(3)  # chunks 0 and 1 pass wholesale, chunk 2 not at all
    assert_empty(kind, plan.collect_arrays())
    (name, _, snap), = native.queries
    assert name == kind.entry and native.names() == [kind.entry]
    assert (snap["chunk_mask"], snap["use_device_row_mask"], snap["row_mask_bits"], snap["row_mask"]) == ([0b011], 0, 0, None)
    # ... and a caller's mask still travels
    native.queries.clear()
    kind.make(ms).meta_filter(col("a").lt(32)).with_row_mask(CALLER).collect_arrays()
    (_, _, snap), = native.queries
    assert (snap["chunk_mask"], snap["use_device_row_mask"], snap["row_mask_bits"], snap["row_mask"]) == ([0b011], 0, 24, words_of(CALLER))


@pytest.mark.parametrize("kind", META_KINDS, ids=META_IDS)
def test_meta_filter_on_the_device(native, kind):
    ms = meta_store(native)
    plan = kind.make(ms).meta_filter(col("f").lt(20.0)).take(3)  # a float column: the zone maps prune chunk 2 and decide no row
    assert_empty(kind, plan.collect_arrays())
    (name, _, snap), = native.queries
    assert name == kind.entry and native.names() == ["ott_store_add_column", "ott_store_eval_row_mask", kind.entry]
    assert (snap["chunk_mask"], snap["use_device_row_mask"], snap["row_mask_bits"], snap["row_mask"]) == ([0b011], 1, 0, None)
    assert ms._store.last_stats == ZERO_STATS
    native.calls.clear()
    native.queries.clear()
    with pytest.raises(OttersError) as e:
        kind.make(ms).meta_filter(col("f").lt(20.0)).with_row_mask(CALLER).take(3).collect_arrays()
    assert str(e.value) == f"{kind.name}: with_row_mask cannot be combined with a meta_filter that needs a row mask of its own"
    assert native.calls == []
    assert ms._mask_lock.acquire(blocking=False)  # (the refusal left the lock free)
    ms._mask_lock.release()


@pytest.mark.parametrize("n", [40, 64, 65])
@pytest.mark.parametrize("kind", META_KINDS, ids=META_IDS)
def test_meta_filter_on_the_host(native, monkeypatch, kind, n):
    monkeypatch.setattr(MetaStore, "_device_mask_ok", lambda self, compiled: False)
    ms = meta_store(native, n)
    passes = np.arange(n) < 20
    chunks = words_of([True, True] + [False] * (-(-n // CHUNK) - 2))
    for caller in (None, CALLER, np.arange(n + 7) % 5 != 0):  # none, shorter than the store, longer than the store
        native.calls.clear()
        native.queries.clear()
        plan = kind.make(ms).meta_filter(col("f").lt(20.0)).take(3)
        want = passes
        if caller is not None:
            plan.with_row_mask(caller)
            padded = np.ones(n, bool)
            padded[: min(caller.size, n)] = caller[:n]
            want = passes & padded
        assert_empty(kind, plan.collect_arrays())
        (name, _, snap), = native.queries
        assert name == kind.entry and native.names() == [kind.entry]
        assert (snap["chunk_mask"], snap["use_device_row_mask"], snap["row_mask_bits"], snap["row_mask"]) == (chunks, 0, n, words_of(want))


@pytest.mark.parametrize("kind", META_KINDS, ids=META_IDS)
def test_meta_refusals_come_in_order(native, kind):
    ms = meta_store(native)
    with pytest.raises(OttersError, match="^meta_filter compile error: "):
        kind.make(ms).meta_filter(col("nope").lt(5)).take(3).collect_arrays()
    assert kind.make(ms).meta_filter(col("nope").lt(5)).meta_filter(col("a").lt(5)).meta_error is None  # a later good filter clears it
    bare = meta_store(native, attach=False)  # no vectors on a device: the forwards still chain, the refusal comes at collect
    plan = kind.make(bare)
    assert plan.vec_filter(0.5, Cmp.Gt).filter(0.5, Cmp.Gt).take(3).take_min(3).take_max(3).with_row_mask(CALLER).with_path(Path.Exact) is plan
    if kind.name == "discover":
        assert plan.min_wins(1) is plan and plan._plan is None
    with pytest.raises(OttersError) as e:
        plan.collect_arrays()
    assert str(e.value) == {"recommend": "recommend: the store holds no vectors, so no row can be an example", "fuse": "fuse: the store holds no vectors",
                            "sparse_query": "sparse_query: the store holds no vectors",
                            "discover": "discover: the store holds no vectors, so no row can be an example"}[kind.name]
    assert native.calls == []
