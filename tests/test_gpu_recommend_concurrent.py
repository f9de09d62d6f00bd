"""GPU: eight threads mix recommend(), plain queries and grouped queries on one store at once (ott_query_recommend; DESIGN.md
3.1k).  Overlapping calls run on worker contexts with their own stream and scratch — the rows' states and the key table belong to
the context — so every answer equals its serial answer, bit for bit; the serial recommend answers are the host model's."""
import threading

import numpy as np
import pytest

import recommend_ref as R
from otters_amd import Metric, VecStore

pytestmark = pytest.mark.gpu

THREADS = 8
ROUNDS = 3


def test_eight_threads_mix_recommend_plain_and_grouped_queries(oracle):
    n, dim = 2000, 24
    rng = np.random.default_rng(12200)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (THREADS, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_groups(np.arange(n) // 7)  # grouped search shares the key table's buffer with recommend, per context
    inv = store.inv_norms()
    ids = [rng.choice(n, 9, replace=False) for _ in range(THREADS)]
    ex = [(i[:5].tolist(), i[5:].tolist()) for i in ids]  # five positives and four negatives per thread

    def job(t):  # half of the threads recommend — with a second round, without one, without the flag, one pass —, the others query
        metric = Metric.Cosine if t % 2 else Metric.Euclidean
        pos, neg = ex[t]
        if t % 4 == 0:
            return store.recommend(pos, neg, metric).take(n).collect_arrays       # two rounds, the sort path
        if t % 4 == 1:
            return store.recommend(pos[:1], neg, metric).take(10).collect_arrays  # no second round: the memset
        if t == 2:
            return store.recommend(pos, neg, metric).take(20).fill_negative_side(False).collect_arrays
        if t == 6:
            return store.recommend(pos[:1], [], metric).take(20).collect_arrays   # the NQ = 1 kernel
        if t == 3:
            return store.query(q[t], metric).take(20).collect_arrays
        return store.query(q[t], metric).one_per_group().take(20).collect_arrays

    def flat(res):
        return tuple(np.asarray(a).tobytes() for a in res)

    serial = [flat(job(t)()) for t in range(THREADS)]
    # the serial recommend answers are the model's
    for t, (pos_of, k, flags) in {0: (slice(None), n, 1), 1: (slice(1), 10, 1), 2: (slice(None), 20, 0), 4: (slice(None), n, 1), 5: (slice(1), 10, 1), 6: (slice(1), 20, 1)}.items():
        metric = Metric.Cosine if t % 2 else Metric.Euclidean
        exp = R.recommend(oracle, rows, inv, ex[t][0][pos_of], [] if t == 6 else ex[t][1], metric, 1 if t % 2 else 0, k, flags=flags)  # (thread 6 lists no negatives)
        R.same(job(t)(), exp, t)
    gate = threading.Barrier(THREADS)
    got, errors = [[None] * ROUNDS for _ in range(THREADS)], []

    def work(t):
        try:
            run = job(t)
            gate.wait()
            for r in range(ROUNDS):
                got[t][r] = flat(run())
        except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(THREADS):
        for r in range(ROUNDS):
            assert got[t][r] == serial[t], (t, r)
    store.close()
