"""GPU: the first listed MaxSim query on a freshly grouped store, issued by four threads at once (ott_query_maxsim_groups; DESIGN.md
3.1h).  The group-to-rows index is built by lock_shared_clean's clean step under the store's exclusive lock: whoever comes first
builds it, the others find it there.  Every answer equals the serial one, bit for bit, and the index was built once."""
import threading

import numpy as np
import pytest

import maxsim_ref as R
from otters_amd import Metric, VecStore
from otters_amd import _native as N
from test_gpu_maxsim_groups import bits_equal, reference

pytestmark = pytest.mark.gpu

THREADS = 4


def test_four_threads_issue_the_first_listed_query_at_once(oracle):
    n, dim, nq, ng = 2000, 24, 5, 250
    rng = np.random.default_rng(11900)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    gid = rng.integers(0, ng, n)
    gid[:ng] = np.arange(ng)
    lists = [rng.choice(ng, 40 + 10 * t, replace=False) for t in range(THREADS)]
    full = R.ranking(oracle, rows, q, Metric.Cosine, 1)
    refs = [reference(full, gid, ng, np.ones(n, bool), lists[t], 10, nq, 1) for t in range(THREADS)]
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_option("group_gather", 1)
    builds = lambda: int(N.lib().ott_store_group_index_builds(store._handle()))  # noqa: E731
    for round_ in range(2):  # a second set_groups drops the index: the race runs twice
        store.set_groups(gid)
        assert builds() == round_
        rqs = [store.query(q, Metric.Cosine).max_sim().with_groups(lists[t]).take(10).resolve() for t in range(THREADS)]
        gate = threading.Barrier(THREADS)
        got, errors = [None] * THREADS, []

        def work(t):
            try:
                gate.wait()
                got[t] = store._run(rqs[t])
            except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
                errors.append((t, repr(e)))

        threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for t in range(THREADS):
            hits, _, st = got[t]
            bits_equal(hits, refs[t], (round_, t))
            assert st["vectors_compared"] == int(np.isin(gid, lists[t]).sum()) * nq  # the gather answered
        assert builds() == round_ + 1                                              # built once, by one of the four
        serial = store._run(rqs[0])[0]
        bits_equal(serial, refs[0], "serial")
        assert builds() == round_ + 1
    store.close()
