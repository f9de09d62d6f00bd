"""GPU: the pruned exact sweep on the sharp corpora of tests/prune_sharp.py.  The other pruned-sweep files draw their
rows from uniform(-1, 1): a uniform row's bound lies some 0.06 |q| |v| above its score and the hits lie far above the gate, so a
device bound that is too low by less than that passes them.  Here the seed's k-th best — the gate — is exactly the score of a tight
row A, whose bound is nearly its score, and the required hits are challengers that beat A by 1 .. 1024 f32 steps: a device bound
that falls short by more than a tight row's own small slack (tests/test_exact_prune_sharp_cpu.py prints it) drops a hit.
  * every form — the head, c = 1 with the integer decode, three bits, one bit, 7/8 without a sketch — on its own family of rows,
    against the oracle and against the full sweep of the same store: indices, order and score bits, no tolerance;
  * cosine and dot, Take Max and Take Min (the negated corpus), k = 1, 10, 64, 100, 256, a row mask that removes every other copy of
    A (at k = 256 the seed's gate is then a filler row's), a score filter AT the gate with Gte / Lte (the copies pass) and with Gt /
    Lt (only challengers pass: the seed lists nothing and the gate stays open);
  * challengers in lanes 0 and 63 of the first gated tile, in 72 consecutive rows (a wave's queue of 64 survivors flushes with rows
    still to come), in adjacent tiles and in the short last tile; 20 000 rows at the line lengths 96, 256, 773 and 896;
  * the staircase: 140 000 x 96 with four challengers in every gated tile, ascending over the store, so that a wave that takes a
    further tile finds rows that barely beat its own k-th best.  (A device of 256 CUs sweeps with 2048 waves and this store has 1969
    gated tiles: there each wave meets one tile and the staircase is held within the tile; the test prints both numbers.)
  * three corpora for what the tight families cannot see.  They keep stage 0 on the line's levels, where the head's rho_all is the
    line's rho: "clamp0" multiplies stage 0 by four, so that the score needs rho_all.  And rows along a uniform query's signs meet
    the quantised query's middle digit and its error with random signs: "qdigit" sets every odd dim along the middle digit, so
    that K needs its 16 K1 term; "qerr" pairs a query that is mostly quantisation error with edge codes along that error, so that
    the score needs 15 a qe1 (these two on the four-bit forms, whose decode they are);
  * the loose direction: at k = 10 the rows the device finishes are at most those whose HEADER bound, taken on the CPU from
    host-made lines, reaches the seed's gate, plus 1 % of the gated rows (the rising gate only lowers the device's count)."""
import numpy as np
import pytest

import prune_sharp as S
from otters_amd import Cmp, Metric, Path, VecStore
from test_exact_prune_sharp_cpu import form_bounds, load_drivers

pytestmark = pytest.mark.gpu

CASES = [(shape, form) for shape in S.SHAPES for form in S.forms_of(shape)]  # shape by shape: the corpora and the oracle's answers are shared
_refs = {"shape": None}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return load_drivers(tmp_path_factory.mktemp("sharp_gpu"))


@pytest.fixture(scope="module")
def sweep_waves():
    """the waves of the sweep's persistent grid: two workgroups of four per CU (tests/test_gpu_exact_prune_overlap.py: waves() asks
    the device the same way and sizes its stores for three per CU)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4


def bits_equal(got, ref, where):
    assert got.size == ref.size, (where, got.size, ref.size)
    assert np.array_equal(got["index"], ref["index"]), (where, got["index"][:12], ref["index"][:12])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32)), (where, got["score"][:12], ref["score"][:12])


def make_store(rows, form):
    store = VecStore(rows.shape[1])
    store.set_option("exact_small", 0)
    store.set_option("exact_prune", 1)
    for name, v in S.FORMS[form].items():
        store.set_option(name, v)
    store.add_vectors(rows)
    return store


def run(store, q, metric, take, k, filt=None, mask=None):
    p = store.query(q, Metric(metric))
    if mask is not None:
        p = p.with_row_mask(mask)
    if filt is not None:
        p = p.filter(*filt)
    got = (p.take_max(k) if take else p.take_min(k)).with_path(Path.Exact).collect_arrays()[0]
    assert store.last_stats["path_used"] == int(Path.Exact)
    return got, store.last_stats["rescored"]


def oracle_ref(oracle, key, rows, q, metric, take, k, filt, mask):
    """the oracle's answer, once per family and query: the two four-bit forms ask for the same"""
    if _refs["shape"] != key[1]:
        _refs.clear()
        _refs["shape"] = key[1]
    if key not in _refs:
        fc, ft = (int(filt[1]), filt[0]) if filt else (0, 0.0)
        _refs[key] = oracle.vec_query(rows, q, metric, take, k, fc, ft, row_mask=mask, ties=oracle.TIES_CANONICAL)
    return _refs[key]


@pytest.mark.parametrize("shape,form", CASES, ids=[f"{s[1]}x{s[0]}-{s[2]}-{f}" for s, f in CASES])
def test_hits_a_few_steps_beyond_the_gate(oracle, libs, sweep_waves, shape, form):
    dim, n, variant, staircase = shape
    seed = S.seed_rows(n)
    if staircase:
        print("staircase:", (n + 63) // 64 - seed // 64, "gated tiles,", sweep_waves, "waves in the sweep's grid")
    for metric in S.METRICS:
        c = S.sharp_corpus(form, dim, n, metric, variant, staircase)
        q, gate = c["q"], float(c["gate"])
        mask = np.ones(n, bool)
        mask[c["copies"][::2]] = False
        for take in (1, 0):
            rows = c["rows"] if take else -c["rows"]
            thr = gate if take else -gate
            store = make_store(rows, form)
            cases = [(k, None, None) for k in S.KS]
            cases += [(100, None, mask), (256, None, mask)]
            cases += [(64, (thr, Cmp.Gte if take else Cmp.Lte), None), (64, (thr, Cmp.Gt if take else Cmp.Lt), None)]
            finished = {}
            for i, (k, filt, m) in enumerate(cases):
                where = (form, shape, metric, take, k, filt, m is not None)
                ref = oracle_ref(oracle, (S.FAMILY[form], shape, metric, take, i), rows, q, metric, take, k, filt, m)
                got, finished[i] = run(store, q, metric, take, k, filt, m)
                bits_equal(got, ref, ("oracle",) + where)
                store.set_option("exact_prune", 0)
                full, none = run(store, q, metric, take, k, filt, m)
                store.set_option("exact_prune", 1)
                bits_equal(got, full, ("full sweep",) + where)
                assert none == 0, where
                if filt is not None and filt[1] in (Cmp.Gt, Cmp.Lt):  # the seed lists nothing: an open gate finishes every gated row
                    assert ref.size == min(k, c["slots"].size), where
                    assert finished[i] == n - seed, (where, finished[i])
                elif m is None or k <= S.COPIES // 2:  # the gate is A's score: the pruned sweep ran, and it pruned
                    assert 0 < finished[i] < n - seed, (where, finished[i])
                else:  # (the gate is a filler row's: the loose rows of "clamp0" may all reach it)
                    assert 0 < finished[i] <= n - seed, (where, finished[i])
                if m is None and filt is None and not staircase:  # every challenger a required hit, as far as k reaches
                    assert np.isin(got["index"][:min(k, c["slots"].size)].astype(np.int64), c["slots"]).all(), where
            # the loose direction, k = 10: the device finishes no more rows than the header's bound keeps at the seed's gate
            b = form_bounds(libs, oracle, form, q, rows[seed:], metric == 0, bool(take))
            key = S.tkey(b) if take else 0xFFFFFFFF - S.tkey(b)
            gkey = int(S.tkey(np.float32(thr))) if take else 0xFFFFFFFF - int(S.tkey(np.float32(thr)))
            host = int(np.count_nonzero(np.isnan(b) | (key >= gkey)))
            print(f"{form} {n}x{dim} {variant} metric {metric} take {take}: k = 10 finished {finished[1]} rows, the header's bound keeps {host} of {n - seed}")
            assert c["slots"].size <= host, (form, shape, metric, take, host)
            assert finished[1] <= host + (n - seed) // 100, (form, shape, metric, take, finished[1], host)
            store.close()
