"""GPU: the Manhattan (L1) metric on several stores at once — bit for bit against one single-GPU store and tests/manhattan_ref.py.
 * one store over 4 and 8 shards of this process (ott_store_create_multi), in the exchange modes of tests/conftest.py ("local",
   "remote"); k up to 512 and beyond, per query, host row masks, MetaStore chunk pruning;
 * the same tests once more in child processes: over tests/fake_rccl (mode "fake_rccl") and under the device-affinity audit
   build of the library (mode "remote"), with the environment tests/test_gpu_multi_modes.py builds;
 * ott_query_sharded: two ranks (threads, host all-gather), both shards on GPU 0;
 * the C++ mirror (include/otters.hpp) and a plain-C host on one Manhattan query."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import manhattan_ref as M
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, VecStore, col
from test_gpu_multi_modes import child_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAN = Metric.Manhattan


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"].astype(np.int64), ref["index"].astype(np.int64)), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["query"].astype(np.int64), ref["query"].astype(np.int64)), where
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def run(store, q, k, mask=None, perq=False, filt=None):
    p = store.query(q, MAN)
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    p = p.take(k)
    if perq:
        p = p.per_query()
    return p.collect_arrays()[0]


@pytest.mark.parametrize("shards", [4, 8])
def test_multi_store_equals_one_store(exchange_mode, shards):
    rng = np.random.default_rng(shards)
    for n, dim in ((5000, 33), (90_000, 24)):
        rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
        mask = rng.random(n) < 0.6
        one = VecStore(dim)
        one.add_vectors(rows)
        many = VecStore(dim, devices=[0] * shards)
        many.add_vectors(rows)
        assert len(many.shards()) == shards
        S = M.scores(rows, q)
        for nq in (1, 5):
            for k in (1, 10, 100, 512, 513, 3000):
                for perq in (False, True):
                    for m in (None, mask):
                        where = (exchange_mode, shards, n, nq, k, perq, m is not None)
                        got = run(many, q[:nq], k, mask=m, perq=perq)
                        bits_equal(got, run(one, q[:nq], k, mask=m, perq=perq), where)
                        bits_equal(got, M.select_canonical(S[:nq], M.TAKE_MIN, k, row_mask=m, perq=perq), where)
        thr = float(np.sort(S.ravel())[n // 2])
        bits_equal(run(many, q, 200, filt=(thr, Cmp.Lte)), run(one, q, 200, filt=(thr, Cmp.Lte)), (exchange_mode, shards, "filter"))
        many.close()
        one.close()


def test_multi_metastore_chunk_pruning(exchange_mode):
    n, dim, cs = 20_000, 16, 512
    rng = np.random.default_rng(5)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    bucket = ((np.arange(n) // cs) % 3).astype(np.int32)
    val = rng.integers(0, 10, n).astype(np.int32)
    q = rng.uniform(-1, 1, (3, dim)).astype(np.float32)
    S = M.scores(rows, q)
    keep = (bucket != 1) & (val > 3)
    for devices in (None, [0] * 4):
        meta = (MetaStore.from_columns([Column.from_numpy("bucket", DataType.Int32, bucket), Column.from_numpy("val", DataType.Int32, val)],
                                       devices=devices).with_vectors(rows).with_chunk_size(cs).build())
        for k in (10, 600):
            res = meta.query_batch(q, MAN).meta_filter(col("bucket").neq(1) & col("val").gt(3)).take(k).collect()
            ref = M.select_canonical(S, M.TAKE_MIN, k, row_mask=keep)
            assert res.indices == ref["index"].tolist(), (devices, k)
            assert np.array_equal(np.array(res.scores, np.float32).view(np.uint32), ref["score"].view(np.uint32)), (devices, k)


@pytest.mark.parametrize("mode,audit", [("fake_rccl", False), ("remote", True)], ids=["fake_rccl", "audit-remote"])
def test_multi_store_manhattan_in_a_child_process(mode, audit):
    env = child_env(mode, audit)
    me = "tests/test_gpu_multi_manhattan.py"
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           me + "::test_multi_store_equals_one_store", me + "::test_multi_metastore_chunk_pruning"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + "\n" + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "OTT_DEVICE_AUDIT violation" not in out.stderr, tail


def test_sharded_query_two_ranks_equals_one_store(oracle):
    from otters_amd.dist import Comm, ShardedVecStore, shard_ranges
    n, dim, world, seed = 30_000, 40, 2, 23
    rows = oracle.rand_rows(0, n, dim, seed)
    qs = np.random.default_rng(3).uniform(-1, 1, (4, dim)).astype(np.float32)
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
    cases = ((10, False), (100, False), (600, False), (7, True))

    def worker(rank):
        try:
            base, cnt = shard_ranges(n, 8, world)[rank]
            store = VecStore(dim)
            store.set_base_offset(base)
            store.append_random(cnt, seed)
            sh = ShardedVecStore(store, Comm.host(rank, world, make_allgather(rank)))
            out = []
            for k, perq in cases:
                p = sh.query(qs, MAN).take(k)
                if perq:
                    p = p.per_query()
                out.append(p.collect_arrays()[0].copy())
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
    single = VecStore(dim)
    single.append_random(n, seed)
    S = M.scores(rows, qs)
    for i, (k, perq) in enumerate(cases):
        want = run(single, qs, k, perq=perq)
        bits_equal(want, M.select_canonical(S, M.TAKE_MIN, k, perq=perq), ("single", k, perq))
        for r in range(world):
            bits_equal(results[r][i], want, ("rank", r, k, perq))
    single.close()


CPP = r"""
#include <cstdio>
#include "otters.hpp"
int main() {
    otters::VecStore store(3);
    store.add_vectors({{0, 0, 0}, {5, 5, 5}, {1, -1, 0}, {-4, 0, 4}, {0.5f, 0, 0}});
    // no take type: the plan infers Min for Manhattan (the nearest rows first)
    auto hits = store.query(std::vector<float>{0, 0, 0}, otters::Metric::Manhattan).take(3).collect();
    for (const auto& h : hits) std::printf("hit %zu score %g\n", h.index, h.score);
    return 0;
}
"""

C_HOST = r"""
#include <stdio.h>
#include "otters_hip.h"
int main(void) {
    static const float rows[5 * 3] = {0, 0, 0, 5, 5, 5, 1, -1, 0, -4, 0, 4, 0.5f, 0, 0};
    static const float q[3] = {0, 0, 0};
    ott_store* s = NULL;
    ott_query_desc d = {0};
    ott_hit hits[3];
    ott_stats st;
    uint64_t n = 0, i;
    if (ott_store_create(3, 0, &s) || ott_store_append(s, rows, 5)) return 1;
    d.queries = q; d.nq = 1; d.metric = OTT_METRIC_MANHATTAN; d.take = OTT_TAKE_MIN; d.k = 3; d.path = OTT_PATH_AUTO;
    if (ott_query(s, &d, hits, 3, &n, NULL, &st)) { fprintf(stderr, "%s\n", ott_last_error()); return 1; }
    for (i = 0; i < n; i++) printf("hit %llu score %g\n", (unsigned long long)hits[i].index, hits[i].score);
    printf("path %u\n", st.path_used);
    d.path = OTT_PATH_MFMA;
    if (ott_query(s, &d, hits, 3, &n, NULL, NULL) != OTT_ERR_UNSUPPORTED) return 2;
    ott_store_destroy(s);
    return 0;
}
"""


@pytest.mark.parametrize("lang", ["cpp", "c"])
def test_cpp_mirror_and_plain_c_host(tmp_path, lang):
    src = tmp_path / ("m.cpp" if lang == "cpp" else "m.c")
    src.write_text(CPP if lang == "cpp" else C_HOST)
    exe = tmp_path / "m"
    lib = os.path.join(ROOT, "otters_amd", "csrc")
    cc = ["g++", "-std=c++17"] if lang == "cpp" else ["gcc", "-std=c11", "-Wall", "-Werror"]
    subprocess.check_call(cc + ["-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L" + lib, "-lotters_hip",
                                "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    env = dict(os.environ)
    env.pop("OTTERS_HIP_DEVICES", None)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[:3] == ["hit 0 score 0", "hit 4 score 0.5", "hit 2 score 2"], lines
    if lang == "c":
        assert lines[3] == "path 1"
