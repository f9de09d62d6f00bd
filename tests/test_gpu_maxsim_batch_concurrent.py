"""GPU: batches and single calls of MaxSim re-ranking issued by four threads at once on one freshly grouped store
(ott_query_maxsim_groups_batch, ott_query_maxsim_groups).  All of them take the store shared through
lock_shared_clean: whoever comes first builds the group-to-rows index in the clean step, the others find it there, and every call runs
on a query context of its own.  Every answer equals the serial one and the reference, bit for bit, and the index was built once."""
import threading

import numpy as np
import pytest

import maxsim_ref as R
from otters_amd import Metric, VecStore
from otters_amd import _native as N
from test_gpu_maxsim_batch import batch_equal, batch_reference, token_sets_of
from test_gpu_maxsim_groups import bits_equal, reference

pytestmark = pytest.mark.gpu

THREADS = 4


def test_four_threads_issue_batches_and_single_calls_at_once(oracle):
    n, dim, ng = 2000, 24, 250
    rng = np.random.default_rng(12900)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    gid = rng.integers(0, ng, n)
    gid[:ng] = np.arange(ng)
    keep = np.ones(n, bool)
    # threads 0 and 2 issue batches (of different shapes), threads 1 and 3 single calls
    batches = {}
    for t, sizes in ((0, (5, 1, 9, 3)), (2, (2, 32, 4, 7, 1, 8))):
        sets = token_sets_of(rng.uniform(-1, 1, (sum(sizes), dim)).astype(np.float32), sizes)
        lists = [rng.choice(ng, 20 + 15 * b, replace=False) for b in range(len(sizes))]
        refs = batch_reference([R.ranking(oracle, rows, s, Metric.Cosine, 1) for s in sets], sets, gid, ng, keep, lists, 10, 1)
        batches[t] = (sets, lists, refs)
    singles = {}
    for t in (1, 3):
        q = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
        listed = rng.choice(ng, 40 + 10 * t, replace=False)
        singles[t] = (q, listed, reference(R.ranking(oracle, rows, q, Metric.Cosine, 1), gid, ng, keep, listed, 10, 5, 1))
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_option("group_gather", 1)
    builds = lambda: int(N.lib().ott_store_group_index_builds(store._handle()))  # noqa: E731
    for round_ in range(2):  # a second set_groups drops the index: the race runs twice
        store.set_groups(gid)
        assert builds() == round_
        plans = {t: store.max_sim_batch(sets, Metric.Cosine).with_groups(lists).take(10).resolve() for t, (sets, lists, _) in batches.items()}
        plans.update({t: store.query(q, Metric.Cosine).max_sim().with_groups(listed).take(10).resolve() for t, (q, listed, _) in singles.items()})
        gate = threading.Barrier(THREADS)
        got, errors = [None] * THREADS, []

        def work(t):
            try:
                gate.wait()
                got[t] = store._run_maxsim_batch(plans[t]) if t in batches else store._run(plans[t])
            except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
                errors.append((t, repr(e)))

        threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for t in range(THREADS):
            hits, counts, st = got[t]
            if t in batches:
                batch_equal(hits, counts, batches[t][2], (round_, t))
                assert st["passes"] == 1  # the batched gather answered
            else:
                bits_equal(hits, singles[t][2], (round_, t))
        assert builds() == round_ + 1  # built once, by one of the four
        for t in batches:  # ... and the serial answers
            hits, counts, _ = store._run_maxsim_batch(plans[t])
            batch_equal(hits, counts, batches[t][2], ("serial", t))
        assert builds() == round_ + 1
    store.close()
