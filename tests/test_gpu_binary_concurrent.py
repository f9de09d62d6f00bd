"""GPU: ott_query_binary from two threads at once on one store.  The first caller runs on the store's own context, the overlapping
one on a worker that aliases the bit rows and owns its stream, its call block (chunk runs, query words, gate words, pair cursor), its
key table and its pair arrays; each call must return what it returns alone (tests/binary_ref.py), bit for bit, on the table route, on
the gated route and under automatic.  The C calls go through ctypes on descriptors and buffers made BEFORE the threads start; tests/overlap.py finds
calls of different threads that overlapped by half of the shorter one — none observed is a failure, as in
tests/test_gpu_concurrent_kinds.py."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import binary_ref as BR
import manhattan_ref as M
import overlap
from otters_amd import Metric, Mode, VecStore
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

N_ROWS, N_BITS, NQ, K, CALLS = 60000, 1024, 5, 10, 25


class Slot:
    """one thread's queries, descriptor and output buffers"""

    def __init__(self, rng, take):
        self.take = take
        self.q = rng.integers(0, 2 ** 64, (NQ, N_BITS // 64), dtype=np.uint64)
        self.d = N.QueryDesc()
        self.d.nq, self.d.metric, self.d.take, self.d.mode, self.d.k = NQ, int(Metric.Manhattan), take, int(Mode.PerQuery), K
        self.out = np.zeros(NQ * K, dtype=N.HIT_DTYPE)
        self.n_out, self.per = C.c_uint64(0), (C.c_uint64 * NQ)()
        self.results, self.intervals, self.rc = [], [], []

    def call(self, L, handle, tid):
        t0 = time.perf_counter_ns()
        rc = L.ott_query_binary(handle, C.byref(self.d), N.ptr(self.q), N.ptr(self.out), NQ * K, C.byref(self.n_out), self.per, None)
        t1 = time.perf_counter_ns()
        self.rc.append(rc)
        self.intervals.append((tid, t0, t1))
        self.results.append((self.out[: self.n_out.value].copy(), list(self.per)))


def test_two_callers_at_once_get_the_serial_answers():
    rng = np.random.default_rng(31)
    words = rng.integers(0, 2 ** 64, (N_ROWS, N_BITS // 64), dtype=np.uint64)
    store = VecStore(1)
    store.add_vectors(np.zeros((N_ROWS, 1), np.float32))
    store.set_binary(words, N_BITS)
    L, handle = N.lib(), store._handle()
    for gate in (0, 1, -1):
        store.set_option("binary_gate", gate)
        before = store.binary_counters()
        slots = [Slot(rng, M.TAKE_MIN), Slot(rng, M.TAKE_MAX)]
        want = [np.concatenate(BR.query(words, s.q, s.take, K)) for s in slots]
        start = threading.Barrier(2)

        def work(tid):
            start.wait()
            for _ in range(CALLS):
                slots[tid].call(L, handle, tid)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for s, w in zip(slots, want):
            assert s.rc == [0] * CALLS, (gate, L.ott_last_error())
            for hits, per in s.results:
                assert per == [K] * NQ and hits.size == w.size
                assert np.array_equal(hits["index"], w["index"]) and np.array_equal(hits["score"].view(np.uint32), w["score"].view(np.uint32))
                assert np.array_equal(hits["query"], w["query"])
        after = store.binary_counters()
        assert BR.gate_eligible(N_BITS, NQ, K, N_ROWS)  # so binary_gate = 1 must have taken the gated route in every call
        assert after["gated_calls"] - before["gated_calls"] == (2 * CALLS if gate == 1 else 0), (gate, before, after)
        assert after["table_calls"] - before["table_calls"] == (0 if gate == 1 else 2 * CALLS), (gate, before, after)
        assert overlap.pairs(slots[0].intervals + slots[1].intervals), ("no two calls overlapped: no worker context ran", gate)
    assert store.binary_counters()["overflows"] == 0
    store.close()
