"""GPU: deleted rows on ONE store over several GPUs of this process, and through ott_query_sharded.

The multi-GPU store routes delete / restore / live_len / read_live_mask by row range (every shard owns the live bits of its
rows; a row move between shards carries them along), so after the same deletions device lists [0]*4 and [0]*8 return the hits
of the single store bit for bit — in every exchange mode (fixture `exchange_mode`), and in a child process under the
device-affinity audit build of the library.  ott_store_compact is refused there.  The sharded path: two ranks as threads of one
process over the host transport, rows deleted on one rank only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from otters_amd import Metric, OttersError, Path, VecStore

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIT_LIB = os.path.join(ROOT, "otters_amd", "csrc", "libotters_hip_audit.so")
DEVS = [[0, 0, 0, 0], [0] * 8]


def same_hits(a, b, where=None):
    assert a.shape == b.shape, (where, a.shape, b.shape)
    assert np.array_equal(a["index"], b["index"]), (where, a[:8], b[:8])
    assert np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)), (where, a[:8], b[:8])
    assert np.array_equal(a["query"], b["query"]), (where, a[:8], b[:8])


def compare(one, many, rng, dim, where):
    n = one.len()
    q1 = rng.uniform(-1, 1, dim).astype(np.float32)
    q5 = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    q40 = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    mask = rng.random(n - n // 9) < 0.5
    for metric in (Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan):
        for k in (1, 10, 100, 600, None):
            for q in (q1, q5):
                for caller in (None, mask):
                    for perq in ((False, True) if q.ndim == 2 else (False,)):
                        def go(s):
                            p = s.query(q, metric)
                            p = p.with_row_mask(caller) if caller is not None else p
                            p = p.take(k) if k is not None else p
                            p = p.per_query() if perq else p
                            return p.collect_arrays()
                        (a, ca), (b, cb) = go(one), go(many)
                        same_hits(b, a, (where, metric, k, q.shape, caller is not None, perq))
                        assert ca == cb
    for path in (Path.Mfma, Path.Auto):
        a, _ = one.query(q40, Metric.Cosine).take(50).with_path(Path.Exact).collect_arrays()
        b, _ = many.query(q40, Metric.Cosine).take(50).with_path(path).collect_arrays()
        same_hits(b, a, (where, "cascade", path))
    for order in ("reference", "reference_chunked", "canonical"):
        one.set_tie_order(order)
        many.set_tie_order(order)
        a, _ = one.query(q5, Metric.DotProduct).take(30).collect_arrays()
        b, _ = many.query(q5, Metric.DotProduct).take(30).collect_arrays()
        same_hits(b, a, (where, "tie order", order))


@pytest.mark.usefixtures("exchange_mode")
@pytest.mark.parametrize("devs", DEVS, ids=lambda d: f"x{len(d)}")
def test_multi_equals_single_store_after_the_same_deletions(oracle, devs):
    n, dim = 50_000, 96
    rng = np.random.default_rng(41)
    one, many = VecStore(dim), VecStore(dim, devices=devs)
    for s in (one, many):
        s.reserve(n)
        s.append_random(n, 21)
    assert len([c for _, _, c in many.shards() if c]) == len(devs)
    # random rows of every shard, a block that covers one shard's whole range and runs into the next, duplicates
    first = many.shards()[1][1]
    dead = np.concatenate([rng.choice(n, 700, replace=False), np.arange(first - 5, first + many.shards()[1][2] + 100), [3, 3, n - 1]])
    ca, cb = one.delete_rows(dead), many.delete_rows(dead)
    assert ca == cb == np.unique(dead).size
    assert one.live_len() == many.live_len() == n - ca and many.len() == n
    assert np.array_equal(one.live_mask(), many.live_mask())
    compare(one, many, rng, dim, "deleted")
    # against the oracle outright
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    keep = np.ones(n, bool)
    keep[dead] = False
    rows = oracle.rand_rows(0, n, dim, 21)
    got, _ = many.query(q, Metric.Cosine).take(40).collect_arrays()
    same_hits(got, oracle.vec_query(rows, q, 0, 1, 40, row_mask=keep, ties=oracle.TIES_CANONICAL), "oracle")
    # an out-of-range index changes nothing on any shard; repeats change nothing; restore routes the same way
    with pytest.raises(OttersError) as e:
        many.delete_rows([1, n])
    assert e.value.status == -1 and many.live_len() == n - ca
    assert many.delete_rows(dead[:50]) == 0
    part = dead[::3]
    assert one.restore_rows(part) == many.restore_rows(part) == np.unique(part).size
    assert np.array_equal(one.live_mask(), many.live_mask())
    compare(one, many, rng, dim, "partly restored")
    # compaction is not for a multi-GPU store (the shards' ranges are pinned to chunk multiples)
    with pytest.raises(OttersError) as e:
        many.compact()
    assert e.value.status == -4 and many.len() == n
    for s in (one, many):
        s.close()


@pytest.mark.usefixtures("exchange_mode")
def test_deleted_rows_follow_their_rows_when_the_shards_are_rebalanced():
    """no reserve: the rows land in the first shard, are deleted there, and move between the shards before the next query"""
    dim, devs = 33, [0, 0, 0, 0]
    rng = np.random.default_rng(17)
    rows = rng.uniform(-1, 1, (20_000, dim)).astype(np.float32)
    one, many = VecStore(dim), VecStore(dim, devices=devs)
    for s in (one, many):
        s.add_vectors(rows[:9000])
    assert [c for _, _, c in many.shards()] == [9000, 0, 0, 0]
    dead = np.concatenate([rng.choice(9000, 900, replace=False), np.arange(2000, 4500)])
    assert one.delete_rows(dead) == many.delete_rows(dead)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    for k in (25, 600):
        a, _ = one.query(q, Metric.Cosine).take(k).collect_arrays()
        b, _ = many.query(q, Metric.Cosine).take(k).collect_arrays()
        same_hits(b, a, ("first balance", k))
    assert sum(1 for _, _, c in many.shards() if c) == 4
    assert np.array_equal(one.live_mask(), many.live_mask()) and many.live_len() == one.live_len()
    for s in (one, many):
        s.add_vectors(rows[9000:])
    more = rng.choice(20_000, 1500, replace=False)
    assert one.delete_rows(more) == many.delete_rows(more)
    for k in (25, 600):
        a, _ = one.query(q, Metric.DotProduct).take(k).collect_arrays()
        b, _ = many.query(q, Metric.DotProduct).take(k).collect_arrays()
        same_hits(b, a, ("second balance", k))
    assert np.array_equal(one.live_mask(), many.live_mask())
    for s in (one, many):
        s.close()


def test_the_same_under_the_device_affinity_audit_build():
    """every HIP call of delete / restore / read_live_mask / the mask composition on a shard thread is made with that shard's
    device selected: this file's multi-store tests in a child process over libotters_hip_audit.so, shards as distinct devices"""
    assert os.path.exists(AUDIT_LIB), "libotters_hip_audit.so is missing: __graft_entry__.build() makes it"
    if os.environ.get("OTT_LIB_PATH") == AUDIT_LIB:
        return  # (this IS the child)
    env = dict(os.environ, OTT_TEST_MULTI_MODE="remote", HSA_ENABLE_IPC_MODE_LEGACY="0", OTT_LIB_PATH=AUDIT_LIB)
    for var in ("OTT_MULTI_FAKE_DISTINCT", "OTT_MULTI_TRANSPORT", "OTT_RCCL_LIBRARY", "OTT_TEST_HOOKS"):
        env.pop(var, None)
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_tombstone_multi.py",
           "-k", "multi_equals_single or rebalanced"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    tail = out.stdout[-3000:] + "\n" + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "OTT_DEVICE_AUDIT violation" not in out.stderr, tail


def test_sharded_query_with_rows_deleted_on_one_rank_only(oracle):
    import threading
    from otters_amd.dist import Comm, ShardedVecStore, shard_ranges
    n, dim, world = 30_000, 40, 2
    rows = oracle.rand_rows(0, n, dim, 19)
    qs = np.random.default_rng(3).uniform(-1, 1, (4, dim)).astype(np.float32)
    ranges = shard_ranges(n, 8, world)
    rng = np.random.default_rng(8)
    # rank 1 only: its best rows for the first query and a random tenth (indices counted from the SHARD's first row)
    base1, cnt1 = ranges[1]
    best = oracle.vec_query(rows[base1:base1 + cnt1], qs[0], 0, 1, 50, ties=oracle.TIES_CANONICAL)["index"].astype(np.int64)
    dead_local = np.unique(np.concatenate([best, rng.choice(cnt1, cnt1 // 10, replace=False)]))
    keep = np.ones(n, bool)
    keep[base1 + dead_local] = False
    barrier = threading.Barrier(world)
    slots = [None] * world
    lock = threading.Lock()

    def make_allgather(rank):
        def allgather(b: bytes) -> bytes:
            with lock:
                slots[rank] = b
            barrier.wait(timeout=60)
            out = b"".join(slots)
            barrier.wait(timeout=60)
            return out
        return allgather
    results, errs = [None] * world, []

    def worker(rank):
        try:
            base, cnt = ranges[rank]
            store = VecStore(dim)
            store.set_base_offset(base)
            store.append_random(cnt, 19)
            if rank == 1:
                assert store.delete_rows(dead_local) == dead_local.size
            sh = ShardedVecStore(store, Comm.host(rank, world, make_allgather(rank)))
            out = []
            for metric, k in ((Metric.Cosine, 10), (Metric.Euclidean, 100), (Metric.DotProduct, 600)):
                hits, _ = sh.query(qs, metric).take(k).collect_arrays()
                out.append(hits.copy())
                hits, _ = sh.query(qs, metric).per_query().take(7).collect_arrays()
                out.append(hits.copy())
            results[rank] = out
            sh.comm.close()
            store.close()
        except Exception as e:  # noqa: BLE001
            errs.append((rank, e))
            barrier.abort()
    ths = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in ths]
    [t.join(timeout=120) for t in ths]
    assert not errs, errs
    i = 0
    for metric, k in ((0, 10), (1, 100), (2, 600)):
        take = 0 if metric == 1 else 1
        ref = oracle.vec_query(rows, qs, metric, take, k, row_mask=keep, ties=oracle.TIES_CANONICAL)
        for r in range(world):
            got = results[r][i]
            assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (metric, k, r)
            got = results[r][i + 1]
            for qi in range(4):
                rq = oracle.vec_query(rows, qs[qi], metric, take, 7, row_mask=keep, ties=oracle.TIES_CANONICAL)
                g = got[qi * 7:(qi + 1) * 7]
                assert np.array_equal(g["index"], rq["index"]) and np.array_equal(g["score"].view(np.uint32), rq["score"].view(np.uint32)), (metric, qi, r)
        i += 2
