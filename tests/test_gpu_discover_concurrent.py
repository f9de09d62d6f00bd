"""GPU: six threads mix discover() with and without a target, with different pair counts, and plain queries on one store at once
(ott_query_discover).  Overlapping calls run on worker contexts with their own stream and scratch — the rows'
states, the key table, the level counters and the list above the cut level belong to the context — so every answer equals its
serial answer, bit for bit; the serial discover answers are the host model's."""
import threading

import numpy as np
import pytest

import discover_ref as D
import mmr_ref as MR
from otters_amd import Metric, VecStore

pytestmark = pytest.mark.gpu

THREADS = 6
ROUNDS = 3


def test_six_threads_mix_discover_context_and_plain_queries(oracle):
    n, dim = 2000, 24
    rng = np.random.default_rng(12300)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (THREADS, dim)).astype(np.float32)
    store = VecStore(dim)
    store.add_vectors(rows)
    inv = store.inv_norms()
    n_pairs = [7, 1, 4, 2, 12, 3]
    ctx = [[tuple(rng.choice(n, 2, replace=False).tolist()) for _ in range(c)] for c in n_pairs]
    # thread:  0 vector target, the sort path   1 context search, one pass   2 row target   3 plain query   4 context search, the sort path   5 vector target, min_wins
    kind = {0: dict(target=q[0], k=n), 1: dict(k=10), 2: dict(target_row=77, k=20), 4: dict(k=n), 5: dict(target=q[5], k=15, min_wins=2)}

    def job(t):
        metric = Metric.Cosine if t % 2 else Metric.Euclidean
        if t == 3:
            return store.query(q[t], metric).take(20).collect_arrays
        kw = kind[t]
        return store.discover(ctx[t], target=kw.get("target"), target_row=kw.get("target_row"), metric=metric).take(kw["k"]).min_wins(kw.get("min_wins", 0)).collect_arrays

    def flat(res):
        return tuple(np.asarray(a).tobytes() for a in res)

    serial = [flat(job(t)()) for t in range(THREADS)]
    # the serial discover answers are the model's
    for t, kw in kind.items():
        metric = Metric.Cosine if t % 2 else Metric.Euclidean
        P = np.stack([MR.pair_row(oracle, rows, inv, e, metric) for pair in ctx[t] for e in pair])
        T = D.target_scores(oracle, rows, inv, kw["target"], metric) if "target" in kw else MR.pair_row(oracle, rows, inv, kw["target_row"], metric) if "target_row" in kw else None
        ex = sorted({e for pair in ctx[t] for e in pair} | ({kw["target_row"]} if "target_row" in kw else set()))
        D.same(job(t)(), D.discover(P, 1 if t % 2 else 0, kw["k"], T=T, examples=ex, min_wins=kw.get("min_wins", 0)), t)
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
