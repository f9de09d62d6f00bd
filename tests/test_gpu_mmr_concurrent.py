"""GPU: eight threads mix mmr(), plain queries and with_row_ids on one store at once (ott_query_mmr).  Overlapping
calls run on worker contexts with their own stream and scratch — the pair scores and the candidate block belong to the context —
so every answer equals its serial answer, bit for bit; the serial MMR answers are the host model's."""
import threading

import numpy as np
import pytest

import mmr_ref as R
from otters_amd import Metric, VecStore

pytestmark = pytest.mark.gpu

THREADS = 8
ROUNDS = 3


@pytest.fixture(scope="module", autouse=True)
def collect_the_models_garbage():
    """The host model makes millions of short-lived Python objects (one oracle call per pair score).  They are collected here, when
    the module is done, so that the interpreter's next full collection does not fall into a test of another module that holds its
    own work to the host clock."""
    yield
    import gc
    gc.collect()


def test_eight_threads_mix_mmr_plain_and_id_list_queries(oracle):
    n, dim = 3000, 24
    rng = np.random.default_rng(12100)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (THREADS, dim)).astype(np.float32)
    ids = rng.choice(n, 400, replace=False)
    store = VecStore(dim)
    store.add_vectors(rows)
    inv = store.inv_norms()

    def job(t):  # a third of the threads each: MMR (two sizes of pair scratch), plain top-k, an id list with and without MMR
        base = store.query(q[t], Metric.Cosine if t % 2 else Metric.Euclidean)
        if t % 4 == 0:
            return base.take(10).mmr(0.5, 200).collect_mmr
        if t % 4 == 1:
            return base.take(20).collect_arrays
        if t % 4 == 2:
            return base.with_row_ids(ids).take(5).mmr(0.3, 64).collect_mmr
        return base.with_row_ids(ids).take(20).collect_arrays

    def flat(res):
        return tuple(np.asarray(a).tobytes() for a in res)

    serial = [flat(job(t)()) for t in range(THREADS)]
    # the serial MMR answers are the model's
    exp = R.mmr(oracle, rows, q[0], Metric.Euclidean, 0, 10, 200, 0.5, inv=inv)
    got = job(0)()
    R.same(got[0], got[2], exp[0], exp[2])
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
