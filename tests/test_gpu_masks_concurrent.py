"""GPU: four threads run with_row_masks batches with different masks on ONE store, 20 times each, next to a thread of plain queries
(ott_query_masks).  Every call takes the store shared and runs on a query context of its own — its own upload of
the masks, its own union buffer and key table — so every answer equals its serial answer (and the oracle's), bit for bit, on both
routes."""
import threading

import numpy as np
import pytest

import masks_ref as MR
from otters_amd import Metric, VecStore
from test_gpu_masks import corpus, same

pytestmark = pytest.mark.gpu

THREADS, REPEATS = 4, 20


def split(hits, counts):
    out, at = [], 0
    for c in counts:
        out.append(hits[at:at + c])
        at += c
    return out


@pytest.mark.parametrize("route", [1, 0], ids=["sweep", "by_mask_group"])
def test_four_threads_with_different_masks_next_to_plain_queries(oracle, route):
    n, dim = 3000, 24
    rng, rows, q = corpus(n, dim, 41 + route, nq=9)
    store = VecStore(dim)
    store.add_vectors(rows)
    store.set_option("masks_sweep", route)
    jobs = []
    for t in range(THREADS):
        nq = (5, 9, 4, 7)[t]
        pool = [rng.random(n) < (0.1 + 0.2 * t) for _ in range(3)]
        masks = [None if b % 4 == 3 else pool[b % 3] for b in range(nq)]
        qs = np.ascontiguousarray(q[:nq][::-1]) if t % 2 else q[:nq]
        plan = store.query(qs, Metric.DotProduct).per_query().with_row_masks(masks).take_max(15).resolve()
        serial = split(*store._run(plan)[:2])
        same(serial, MR.expected(oracle, rows, qs, masks, Metric.DotProduct, 1, 15), ("serial", t))
        jobs.append((plan, serial))
    plain = store.query(q[:3], Metric.DotProduct).per_query().take_max(15).resolve()
    plain_serial = split(*store._run(plain)[:2])

    gate = threading.Barrier(THREADS + 1)
    errors = []

    def work(t):
        try:
            gate.wait()
            for i in range(REPEATS):
                if t == THREADS:
                    same(split(*store._run(plain)[:2]), plain_serial, ("plain", i))
                else:
                    same(split(*store._run(jobs[t][0])[:2]), jobs[t][1], (t, i))
        except BaseException as e:  # noqa: BLE001 -- reported by the asserting thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS + 1)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    store.close()
