"""GPU: the life cycle of the cascade's planes (otters_amd/csrc/ott_planes.hip: built on demand, extended after appends, kept in
step by write_rows, dropped by a reallocation / set_batch_image(False) / compact / reserve, declined when the format does not suit
the store).  One store per option set (hi_fmt -1: int8 plane first and a half plane behind it, 1: the half plane alone, 0: a bf16
plane alone) walks through every step that builds, rewrites or drops a plane, and after every step the batch path (Path.Mfma) must
return the oracle's hits bit for bit on the three metrics at k = 10 and k = 130 (above the int8 level's 128: the hi plane serves),
with no bound violation and a measured |approximate - exact| / eps of at most 1.

3000 rows of dim 72: at least 8, and no multiple of 32, 64 or 128, so every plane's padded pitch differs from the row pitch; the
first 2000 rows fill what the store reserved, the next 1000 force a reallocation.

Two more corpora make a from-scratch build REJECT its format (more than 1 row in 64 marked, ott_plane_policy.h); a NumPy check in
f64 on the stored f32 values proves each case before any GPU call:
  A  the half plane's roll-back to bf16: one row of norm 1e3 puts the plane's one factor at 2^-2, and one row in eight is scaled by
     1e-6, deep in half's subnormals.  The elements are bf16 values (all but one row in a hundred), so bf16 itself loses 2^-10 on
     fewer than 1 row in 64 — an ordinary f32 row measures 1.65e-3 under bf16, above 2^-10, whatever its scale;
  B  the int8 plane's removal: one row in sixteen has one element 259 times the magnitude of the rest, which then sit at 0.49 of
     the row's quantisation step and all round to zero.  (The loss is relative to the row's own norm, which the big element
     dominates: at dim 72 a row can lose at most sqrt(71) / 254 = 0.0332, just above 2^-5, and an element 1e4 times the rest
     loses sqrt(71) / 1e4 = 8e-4.)"""
import math

import numpy as np
import pytest

import adversarial_i8 as A8
from otters_amd import Metric, Path, VecStore

pytestmark = pytest.mark.gpu

N, N0, DIM, NQ = 3000, 2000, 72, 9
KS = (10, 130)
METRICS = (Metric.Cosine, Metric.Euclidean, Metric.DotProduct)
TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1}
f32 = np.float32


def to_bf16(x):
    """round to nearest even onto bf16's grid (finite values)"""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(f32).reshape(np.shape(x))


def heavy_rows(rng, n):
    """one element of magnitude M in [0.5, 1), the rest at 0.49 M / 127: they all round to zero in int8"""
    m = rng.uniform(0.5, 1.0, n).astype(f32)
    rows = (rng.choice([-1.0, 1.0], (n, DIM)).astype(f32) * ((f32(0.49) / f32(127)) * m)[:, None]).astype(f32)
    rows[np.arange(n), rng.integers(0, DIM, n)] = m * rng.choice([-1.0, 1.0], n).astype(f32)
    return rows


def rel_loss(x, back):
    e = x.astype(np.float64) - back.astype(np.float64)
    return np.sqrt((e * e).sum(1) / (x.astype(np.float64) ** 2).sum(1)) * 1.0001


class Model:
    """the rows a store holds, and the oracle's ranking of every (row, query) pair of a metric, made once per state of the rows"""

    def __init__(self, oracle, rows, queries):
        self.oracle, self.all, self.q = oracle, rows, queries
        self.rows, self.rank = rows[:0], {}

    def set_rows(self, rows):
        self.rows, self.rank = np.ascontiguousarray(rows), {}

    def expected(self, metric, k):
        if metric not in self.rank:
            self.rank[metric] = self.oracle.vec_query(self.rows, self.q, int(metric), TAKE[metric], self.rows.shape[0] * NQ,
                                                      ties=self.oracle.TIES_CANONICAL)
        return self.rank[metric][:k]


def check_queries(store, model, where):
    for metric in METRICS:
        for k in KS:
            got, _ = store.query(model.q, metric).take(k).with_path(Path.Mfma).collect_arrays()
            ref, st = model.expected(metric, k), store.last_stats
            at = (where, metric, k, st)
            print(where, metric.name, k, {f: st[f] for f in ("passes", "rescored", "refined", "i8_refined", "err_ratio_max", "bound_violations")})
            assert got.size == ref.size, at
            assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), at
            assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), at
            assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), at
            assert st["bound_violations"] == 0, at
            assert st["err_ratio_max"] <= 1.0, at


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(72)
    rows = rng.uniform(-1, 1, (N, DIM)).astype(f32)
    queries = rng.uniform(-1, 1, (NQ, DIM)).astype(f32)
    # the rewrites: an ordinary row, a row int8 does not suit (its mark is taken on the rewrite), a row five times as long
    written = [np.stack([rng.uniform(-1, 1, DIM).astype(f32), heavy_rows(rng, 1)[0], (5 * rng.uniform(-1, 1, DIM)).astype(f32)]) for _ in range(2)]
    dead = np.sort(rng.choice(N, 100, replace=False))
    return rows, queries, written, dead


@pytest.mark.parametrize("hi_fmt", [-1, 1, 0])
def test_every_step_that_builds_rewrites_or_drops_a_plane(oracle, corpus, hi_fmt):
    rows, queries, written, dead = corpus
    rows = rows.copy()
    model = Model(oracle, rows, queries)
    store = VecStore(DIM)
    store.set_option("hi_fmt", hi_fmt)
    store.reserve(N0)  # (an append to an empty store allocates 3072 rows: the second append would fit.  2000 exactly, so that it does not)
    store.add_vectors(rows[:N0])  # 1
    model.set_rows(rows[:N0])
    store.prepare_batch()  # 2
    assert store.batch_ready()
    check_queries(store, model, (hi_fmt, "prepared"))  # 3
    store.add_vectors(rows[N0:])  # 4: past the 2000 rows allocated, the store reallocates and the planes go
    assert not store.batch_ready()
    model.set_rows(rows)
    check_queries(store, model, (hi_fmt, "appended"))  # 5
    for first, new in zip((500, N0 - 1), written):  # 6: inside the old 2000 rows, and across their end
        store.write_rows(first, new)
        rows[first:first + 3] = new
    model.set_rows(rows)
    check_queries(store, model, (hi_fmt, "rewritten"))  # 7
    store.set_batch_image(False)  # 8
    assert not store.batch_ready()
    check_queries(store, model, (hi_fmt, "no planes"))  # 9
    assert not store.batch_ready()
    store.set_batch_image(True)  # 10
    check_queries(store, model, (hi_fmt, "planes again"))  # 11
    assert store.delete_rows(dead) == dead.size  # 12
    new_index = store.compact()
    keep = np.ones(N, bool)
    keep[dead] = False
    assert np.array_equal(new_index >= 0, keep) and store.len() == N - dead.size
    assert not store.batch_ready()
    model.set_rows(rows[keep])
    check_queries(store, model, (hi_fmt, "compacted"))  # 13
    store.reserve(8000)  # 14
    assert not store.batch_ready()
    check_queries(store, model, (hi_fmt, "reserved"))  # 15
    assert np.array_equal(store.rows().view(np.uint32), model.rows.view(np.uint32))
    store.close()


def half_factor(max_norm):
    """the half plane's one factor (hi_plane_format, ott_plane_policy.h): 2^-(e / 4), max_norm = m 2^e with m in [0.5, 1)"""
    e = math.frexp(max_norm)[1]
    return math.ldexp(1.0, -int(e / 4))


def corpus_a(rng):
    rows = rng.uniform(-1, 1, (N, DIM)).astype(f32)
    rows[7] *= f32(1000.0 / np.linalg.norm(rows[7].astype(np.float64)))
    rows[3::8] *= f32(1e-6)
    exact = np.arange(N) % 100 != 50  # all but one row in a hundred hold bf16 values
    rows[exact] = to_bf16(rows[exact])
    return rows


def corpus_b(rng):
    rows = rng.uniform(-1, 1, (N, DIM)).astype(f32)
    rows[5::16] = heavy_rows(rng, rows[5::16].shape[0])
    return rows


def prove_a(rows):
    for n in (N0, N):  # each build from scratch: the first 2000 rows, and all of them after the reallocation
        part = rows[:n]
        max_norm = float(np.sqrt((part.astype(np.float64) ** 2).sum(1)).max())
        assert 1e-3 <= max_norm <= 1e6, max_norm
        factor = half_factor(max_norm)
        assert factor == 0.25, (max_norm, factor)
        scaled = part * f32(factor)  # a power of two: exact
        with np.errstate(over="ignore"):
            half_lost = rel_loss(scaled, scaled.astype(np.float16).astype(f32)) > 2.0 ** -10
        bf16_lost = rel_loss(part, to_bf16(part)) > 2.0 ** -10
        assert int(half_lost.sum()) * 64 > n, (n, int(half_lost.sum()))
        assert int(bf16_lost.sum()) * 64 < n, (n, int(bf16_lost.sum()))
        assert bf16_lost.any()  # (the bf16 plane still measures a loss: the rows that hold ordinary f32 values)


def prove_b(rows):
    for n in (N0, N):
        _, _, rel = A8.i8_plane(rows[:n])
        lost = rel * 1.0001 > 2.0 ** -5
        assert int(lost.sum()) * 64 > n, (n, int(lost.sum()))
        assert not lost[np.arange(n) % 16 != 5].any()  # the ordinary rows suit int8


@pytest.mark.parametrize("name,make,prove,hi_fmt", [("A", corpus_a, prove_a, 1), ("B", corpus_b, prove_b, -1)])
def test_a_build_from_scratch_rejects_its_format(oracle, corpus, name, make, prove, hi_fmt):
    rows = make(np.random.default_rng(ord(name)))
    prove(rows)
    model = Model(oracle, rows, corpus[1])
    store = VecStore(DIM)
    store.set_option("hi_fmt", hi_fmt)
    store.reserve(N0)  # (as above: the second append reallocates)
    store.add_vectors(rows[:N0])
    model.set_rows(rows[:N0])
    check_queries(store, model, (name, "first build"))
    store.add_vectors(rows[N0:])
    model.set_rows(rows)
    check_queries(store, model, (name, "built again after the reallocation"))
    store.close()
