"""GPU: every kind of query on WORKER contexts (ctx_acquire, ott_store.hip).  ott_query and its siblings are re-entrant on one store: the
first caller runs on the store's own context, every overlapping caller on a worker that aliases the corpus (alias_corpus) and owns its
stream, events and scratch — the lazily made tables of grouped, per-group and MaxSim search, the id-list mask and gather buffers, the
composed live mask, the pruned sweep's gate, the sort path's buffers.  The header promises that a call returns what it returns alone.
Bar: bit for bit — index, query, score bits, order, per-query counts, group ids — no tolerances.

How the expectation is made (tests/grouped_ref.py): ONE full canonical ranking per (store, metric, queries, take) from the oracle
(Manhattan: tests/manhattan_ref.py), restricted to the kept rows and cut by the kind's own rule; MaxSim sums the same ranking's scores
(tests/maxsim_ref.py).  Nothing is taken from the library; test_serial_answers_are_the_oracles is a second, independent check.
The two reference tie orders have no canonical ranking: their expectation is the oracle's literal collector (one over the store, or
one per chunk), compared as tests/test_gpu_ties.py does — the score sequence bit for bit and the (index, query) pairs as a set (per
chunk: the rows as a multiset, the reference drops the query id there) — and the calls of one thread must agree byte for byte.

How a worker is known to have run: the C calls go through ctypes on descriptors and buffers made BEFORE the threads start, one set per
thread, time.perf_counter_ns() brackets the C call alone, and tests/overlap.py finds calls of different threads that overlapped by half
of the shorter one.  `mu` is held from acquire to release, so one of two such calls ran on a worker.  No overlap observed is a FAILURE.

Stores (module scope).  A: 6037 rows (95 tiles, a short last one) x dim 44 (one full stage, one part stage, dim % 8 = 4), integers
-2..2 so that ties occur, 37 random group labels, 5 % of the rows deleted and some restored, default options.  A': its twin with
contiguous groups of 8 and id_gather = 0.  B: 20 000 uniform rows x dim 264 (9 stages), exact_small 0, exact_prune 1, exact_sketch 1,
a few hundred rows deleted.  C, C2: 3000 rows x dim 8 quantised, tie_order 1 and tie_order 2 with chunks of 128 rows.

OTT_CONCURRENCY_REPORT=<path>: the figures of the run (per kind the median call time, the overlapping pairs, the calls per thread, the
peak number of calls in flight) as JSON, for profiles/concurrency_kinds/README.md."""
import copy
import ctypes as C
import json
import os
import threading
import time

import numpy as np
import pytest

import maxsim_ref as MX
import overlap
from grouped_ref import Rankings, bits_equal, dense, expected, ids_expected, plain_expected
from otters_amd import Cmp, Column, DataType, MetaStore, Metric, Path, VecStore, col
from otters_amd import _native as N

pytestmark = pytest.mark.gpu

TAKE = {Metric.Cosine: 1, Metric.Euclidean: 0, Metric.DotProduct: 1, Metric.Manhattan: 0}
SLOTS = 8           # threads of the same-kind test: every slot has queries, id lists and buffers of its own
CALLS = 6           # calls per thread and kind
CALLS_FOR = {}      # kinds that showed no overlap at 6 calls on the GPU get more here (at most 30)
REPORT = []


def list_E(k):
    """ott_internal.h: register list entries per lane for k <= 512; a merge block is 64 * list_E(k) slots wide"""
    return 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8


def quantised(rng, shape):
    a = rng.integers(-2, 3, shape).astype(np.float32)
    flat = a.reshape(-1, a.shape[-1])
    flat[np.all(flat == 0, axis=1)] = 1.0
    return a


# ---- a store with what its expectations need ---------------------------------------------------------------------------------------

class Bundle:
    def __init__(self, oracle, store, rows, q, alive=None, mask=None, gid=None, id_limit=None, tie=None):
        self.oracle, self.store, self.rows, self.q = oracle, store, rows, q
        self.n = rows.shape[0]
        self.alive = np.ones(self.n, bool) if alive is None else alive
        self.mask = mask  # the caller's row mask of the kinds that carry one (rows past its end are kept)
        self.gid = gid
        self.n_groups = 0 if gid is None else int(gid.max()) + 1
        self.id_limit = self.n if id_limit is None else id_limit
        self.tie = tie    # (tie_order, chunk size) of a store in a reference tie order
        self.ranks = [Rankings(oracle, rows, q[s]) for s in range(q.shape[0])]
        self.memo = {}

    def variant(self, **changes):
        """the same store and rankings with other group ids or another live set"""
        b = copy.copy(self)
        b.memo = {}
        for key, val in changes.items():
            setattr(b, key, val)
        if "gid" in changes:
            b.n_groups = int(b.gid.max()) + 1
        return b

    def h(self):
        return self.store._handle()

    def kept(self, masked=False):
        keep = self.alive.copy()
        if masked:
            keep[:self.mask.size] &= self.mask[:self.n]
        return keep

    def full(self, slot, metric, nq, take):
        return self.ranks[slot % SLOTS].get(metric, nq, take)

    def queries(self, slot, nq):
        return self.q[slot % SLOTS][:nq]  # (a contiguous view: the descriptor points into self.q)

    def ids(self, slot):
        rng = np.random.default_rng(5000 + slot % SLOTS)
        base = rng.choice(self.id_limit, 260, replace=False)
        return np.ascontiguousarray(rng.permutation(np.concatenate([base, base[:40]])).astype(np.uint64))  # 300 ids, 40 of them twice


def make_desc(q, metric, take, k, perq=False, cmp=0, thr=0.0, mask=None, path=Path.Auto):
    d = N.QueryDesc()
    keep = [q]
    d.queries, d.nq, d.metric, d.take, d.k = q.ctypes.data, q.shape[0], int(metric), int(take), int(k)
    d.mode, d.filter_cmp, d.filter_thr, d.path = (1 if perq else 0), int(cmp), float(thr), int(path)
    if mask is not None:
        words = N.pack_bits(mask)
        keep.append(words)
        d.row_mask, d.row_mask_bits = words.ctypes.data, int(mask.size)
    return d, keep


class Out:
    """the host output of one prepared call"""

    def __init__(self, cap, nq, perq, gids=False):
        self.hits = np.empty(max(cap, 1), N.HIT_DTYPE)
        self.n = C.c_uint64(0)
        self.per = (C.c_uint64 * nq)()
        self.perq = perq
        self.st = N.Stats()
        self.gids = np.empty(max(cap, 1), np.uint32) if gids else None

    def reset(self):
        self.hits.view(np.uint8).fill(0x5A)
        self.n.value = 0

    def read(self):
        n = int(self.n.value)
        return (self.hits[:n].copy(), [int(x) for x in self.per] if self.perq else None,
                None if self.gids is None else self.gids[:n].copy(), int(self.st.rescored))


class Call:
    """one prepared C call: run() times the call alone, read() copies its result out"""

    def __init__(self, where, fn, args, keep, read, reset):
        self.where, self.fn, self.args, self.keep, self.read, self.reset = where, fn, args, keep, read, reset

    def run(self):
        self.reset()
        t0 = time.perf_counter_ns()
        rc = self.fn(*self.args)
        t1 = time.perf_counter_ns()
        if rc != 0:
            raise AssertionError((self.where, rc, N.lib().ott_last_error()))
        return t0, t1


def same_hits(got, want, where):
    bits_equal(got[0], want[0], where)
    if want[1] is not None:
        assert got[1] == list(want[1]), (where, got[1], want[1])
    if want[2] is not None:
        assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2]), (where, got[2][:12], want[2][:12])


class Kind:
    def __init__(self, name, bundle, make, want, same=same_hits):
        self.name, self.bundle, self.make, self.want, self.same = name, bundle, make, want, same

    def prepared(self, B, slot):
        """(the call with buffers of its own, its expectation) — the expectation once per (store state, slot)"""
        key = (self.name, slot % SLOTS)
        if key not in B.memo:
            B.memo[key] = self.want(B, slot)
        return self.make(B, slot), B.memo[key]


# ---- the kinds -----------------------------------------------------------------------------------------------------------------------

def thr_of(B, slot, metric, nq, take, flt):
    """a filter threshold that cuts the ranking at a given position: (Cmp, position) -> (cmp, the score there)"""
    if flt is None:
        return 0, 0.0
    return int(flt[0]), float(B.full(slot, metric, nq, take)["score"][flt[1]])


def kind_plain(name, bundle, metric, nq, k, perq=False, flt=None, masked=False, path=Path.Auto, stats=False):
    """ott_query; k None: the default take (every pair, ranked by Max)"""
    take = 1 if k is None else TAKE[metric]

    def make(B, slot):
        q, kk = B.queries(slot, nq), (B.n * nq if k is None else k)
        cmp, thr = thr_of(B, slot, metric, nq, take, flt)
        d, keep = make_desc(q, metric, take, kk, perq, cmp, thr, B.mask if masked else None, path)
        cap = min(kk, B.n) * nq if perq else min(kk, B.n * nq)
        o = Out(cap, nq, perq)
        args = (B.h(), C.byref(d), N.ptr(o.hits), cap, C.byref(o.n), o.per if perq else None, C.byref(o.st) if stats else None)
        return Call((name, slot), N.lib().ott_query, args, keep + [d, o], o.read, o.reset)

    def want(B, slot):
        cmp, thr = thr_of(B, slot, metric, nq, take, flt)
        hits, counts = plain_expected(B.full(slot, metric, nq, take), B.kept(masked), B.n * nq if k is None else k, nq, perq, cmp, thr)
        return hits, counts if perq else None, None

    def same(got, ref, where):
        same_hits(got, ref, where)
        if stats:  # the field the sketch tests read: the pruned sweep ran, and rows got past its checkpoint
            assert got[3] > 0, (where, "stats.rescored", got[3])

    return Kind(name, bundle, make, want, same)


def kind_ids(name, bundle, metric, nq, k, perq):
    take = TAKE[metric]

    def make(B, slot):
        q, ids = B.queries(slot, nq), B.ids(slot)
        d, keep = make_desc(q, metric, take, k, perq)
        unique = int(np.unique(ids).size)
        cap = min(k, unique) * nq if perq else min(k, unique * nq)
        o = Out(cap, nq, perq)
        args = (B.h(), C.byref(d), N.ptr(ids), ids.size, N.ptr(o.hits), cap, C.byref(o.n), o.per if perq else None, None)
        return Call((name, slot), N.lib().ott_query_ids, args, keep + [d, o, ids], o.read, o.reset)

    def want(B, slot):
        hits, counts = ids_expected(B.full(slot, metric, nq, take), B.kept(), B.ids(slot), k, nq, perq)
        return hits, counts if perq else None, None

    return Kind(name, bundle, make, want)


def kind_scores(name, bundle, metric, nq):
    """ott_store_score_rows: raw scores in the list's order, deleted rows included"""
    def make(B, slot):
        q, ids = B.queries(slot, nq), B.ids(slot)
        out = np.empty((nq, ids.size), np.float32)

        def reset():
            out.view(np.uint32).fill(0x5A5A5A5A)
        args = (B.h(), N.ptr(q), nq, int(metric), N.ptr(ids), ids.size, N.ptr(out))
        return Call((name, slot), N.lib().ott_store_score_rows, args, [q, ids, out], lambda: (out.copy(),), reset)

    def want(B, slot):
        full = B.full(slot, metric, nq, TAKE[metric])
        assert full.size == B.n * nq  # no pair without a score in these corpora: the ranking holds every score
        S = np.empty((nq, B.n), np.float32)
        S[full["query"].astype(np.int64), full["index"].astype(np.int64)] = full["score"]
        return (S[:, B.ids(slot).astype(np.int64)],)

    def same(got, ref, where):
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (where, got[0][0, :8], ref[0][0, :8])

    return Kind(name, bundle, make, want, same)


def kind_groups(name, bundle, metric, nq, k, flt=None, masked=False):
    """ott_query_groups; k None: every group, ranked by Max (above 512 groups: through the pair sort)"""
    perq = nq > 1
    take = 1 if k is None else TAKE[metric]

    def make(B, slot):
        q, kk = B.queries(slot, nq), (B.n_groups if k is None else k)
        cmp, thr = thr_of(B, slot, metric, nq, take, flt)
        d, keep = make_desc(q, metric, take, kk, perq, cmp, thr, B.mask if masked else None)
        cap = min(kk, B.n_groups) * nq
        o = Out(cap, nq, perq)
        args = (B.h(), C.byref(d), N.ptr(o.hits), cap, C.byref(o.n), o.per if perq else None, None)
        return Call((name, slot, B.n_groups), N.lib().ott_query_groups, args, keep + [d, o], o.read, o.reset)

    def want(B, slot):
        cmp, thr = thr_of(B, slot, metric, nq, take, flt)
        hits, counts, _ = expected(B.full(slot, metric, nq, take), B.gid, B.kept(masked), B.n_groups if k is None else k, nq, 1, cmp, thr)
        return hits, counts if perq else None, None

    return Kind(name, bundle, make, want)


def kind_groups_top(name, bundle, metric, nq, k, m):
    perq = nq > 1
    take = TAKE[metric]

    def make(B, slot):
        q = B.queries(slot, nq)
        d, keep = make_desc(q, metric, take, k, perq)
        cap = min(k, B.n_groups) * nq * m
        o = Out(cap, nq, perq, gids=True)
        args = (B.h(), C.byref(d), m, N.ptr(o.hits), cap, C.byref(o.n), o.per if perq else None, N.ptr(o.gids), None)
        return Call((name, slot, B.n_groups), N.lib().ott_query_groups_top, args, keep + [d, o], o.read, o.reset)

    def want(B, slot):
        hits, counts, groups = expected(B.full(slot, metric, nq, take), B.gid, B.kept(), k, nq, m)
        return hits, counts if perq else None, groups

    return Kind(name, bundle, make, want)


def kind_maxsim(name, bundle, metric, nq, take, k, masked=False):
    def make(B, slot):
        q = B.queries(slot, nq)
        d, keep = make_desc(q, metric, take, k, False, 0, 0.0, B.mask if masked else None)
        cap = min(k, B.n_groups)
        o = Out(cap, nq, False)
        args = (B.h(), C.byref(d), N.ptr(o.hits), cap, C.byref(o.n), None)
        return Call((name, slot, B.n_groups), N.lib().ott_query_maxsim, args, keep + [d, o], o.read, o.reset)

    def want(B, slot):
        return MX.expected(B.full(slot, metric, nq, take), B.gid, B.kept(masked), k, nq, take, n_groups=B.n_groups), None, None

    return Kind(name, bundle, make, want)


def kind_ties(name, bundle, nq, k, perq):
    """ott_query on a store in one of the reference's tie orders, against the oracle's literal collectors"""
    metric, take = Metric.DotProduct, 1

    def make(B, slot):
        q = B.queries(slot, nq)
        d, keep = make_desc(q, metric, take, k, perq)
        cap = k * nq if perq else k
        o = Out(cap, nq, perq)
        args = (B.h(), C.byref(d), N.ptr(o.hits), cap, C.byref(o.n), o.per if perq else None, None)
        return Call((name, slot), N.lib().ott_query, args, keep + [d, o], o.read, o.reset)

    def literal(B, q):
        O = B.oracle
        if B.tie[0] == 1:
            return O.vec_query(B.rows, q, int(metric), take, k, ties=O.TIES_LITERAL)
        return O.meta_query(B.rows, B.tie[1], q, int(metric), take, k, ties=O.TIES_LITERAL)[0]

    def want(B, slot):
        q = B.queries(slot, nq)
        return [literal(B, q[qi:qi + 1]) for qi in range(nq)] if perq else [literal(B, q)]

    def same(got, ref, where):
        hits, counts = got[0], got[1]
        assert hits.size == sum(r.size for r in ref), (where, hits.size)
        if perq:
            assert counts == [r.size for r in ref], (where, counts)
        o = 0
        for qi, lit in enumerate(ref):
            g = hits[o:o + lit.size]
            o += lit.size
            assert np.array_equal(g["score"].view(np.uint32), lit["score"].view(np.uint32)), (where, qi, "score sequence")
            if perq:
                assert np.all(g["query"] == qi), (where, qi)
                assert sorted(g["index"].tolist()) == sorted(lit["index"].tolist()), (where, qi)
            elif B_TIE_PAIRS[name]:  # one collector over the store keeps the query of every pair
                assert sorted(zip(g["index"].tolist(), g["query"].tolist())) == sorted(zip(lit["index"].tolist(), lit["query"].tolist())), where
            else:  # per chunk the reference drops the query id: the rows as a multiset
                assert sorted(g["index"].tolist()) == sorted(lit["index"].tolist()), where

    return Kind(name, bundle, make, want, same)


B_TIE_PAIRS = {"ties reference merged": True, "ties reference per query": True, "ties per chunk merged": False, "ties per chunk per query": False}


def kind_device(name, bundle, metric, nq, k, shape):
    """ott_query_device into a torch buffer of cap + 64 slots prefilled with 0x5A.  shape: "merged" (cap = k), "in place" (PER_QUERY, cap /
    nq = 64 * list_E(k): the merge kernel's own geometry, written without a copy), "k+37" (PER_QUERY, cap / nq = k + 37)"""
    take = TAKE[metric]
    perq = shape != "merged"
    groups = nq if perq else 1
    cap = {"merged": k, "in place": nq * 64 * list_E(k), "k+37": nq * (k + 37)}[shape]

    def make(B, slot):
        import torch
        q = B.queries(slot, nq)
        d, keep = make_desc(q, metric, take, k, perq)
        buf = torch.empty((cap + 64) * 16, dtype=torch.uint8, device="cuda:0")
        nout = torch.zeros(1, dtype=torch.int64, device="cuda:0")

        def reset():
            buf.fill_(0x5A)
            nout.fill_(-1)
            torch.cuda.current_stream().synchronize()

        def read():
            return buf.cpu().numpy().copy(), int(nout.cpu()[0])
        args = (B.h(), C.byref(d), C.c_void_p(buf.data_ptr()), cap, C.c_void_p(nout.data_ptr()), None)
        return Call((name, slot), N.lib().ott_query_device, args, keep + [d, buf, nout], read, reset)

    def want(B, slot):
        hits, counts = plain_expected(B.full(slot, metric, nq, take), B.kept(), k, nq, perq)
        return hits, counts if perq else [hits.size]

    def same(got, ref, where):
        raw, total = got
        hits, counts = ref
        assert raw.size == (cap + 64) * 16
        slots, gstride, o = raw.view(N.HIT_DTYPE), cap // groups, 0
        for g in range(groups):
            c = counts[g]
            assert c <= gstride, (where, g, c, gstride)
            bits_equal(slots[g * gstride:g * gstride + c], hits[o:o + c], (where, "group", g))
            pad = raw[(g * gstride + c) * 16:(g + 1) * gstride * 16]
            assert np.all(pad == 0xFF), (where, "a slot behind the hits of group", g, "is no sentinel", np.flatnonzero(pad != 0xFF)[:4])
            o += c
        past = raw[cap * 16:]
        assert past.size == 64 * 16 and np.all(past == 0x5A), (where, "written past cap", np.flatnonzero(past != 0x5A)[:4])
        assert total == sum(counts), (where, total, counts)

    return Kind(name, bundle, make, want, same)


COS, L2, DOT, MAN = Metric.Cosine, Metric.Euclidean, Metric.DotProduct, Metric.Manhattan
KINDS = [
    kind_plain("l2 top-10, row mask and deleted rows", "A", L2, 1, 10, masked=True),
    kind_plain("manhattan 5 queries top-100 lte", "A", MAN, 5, 100, perq=True, flt=(Cmp.Lte, 300)),
    kind_plain("cosine k=700 sort path", "A", COS, 1, 700),
    kind_plain("default take 2 queries", "A", COS, 2, None),
    kind_ids("id list gather", "A", DOT, 3, 10, perq=True),
    kind_ids("id list mask route", "A2", COS, 3, 10, perq=False),
    kind_scores("score rows", "A", COS, 3),
    kind_groups("groups 1 query cosine gte", "A", COS, 1, 10, flt=(Cmp.Gte, 200)),
    kind_groups("groups 6 queries dot gt", "A", DOT, 6, 10, flt=(Cmp.Gt, 2000)),
    kind_groups_top("per group m=3", "A2", COS, 1, 10, 3),
    kind_groups_top("per group m=16 5 queries", "A2", L2, 5, 10, 16),
    kind_maxsim("maxsim 6 tokens cosine", "A", COS, 6, 1, 10),
    kind_maxsim("maxsim 3 tokens l2 take-min", "A", L2, 3, 0, 10, masked=True),
    kind_plain("pruned sweep", "B", COS, 1, 10, stats=True),
    kind_plain("batch 16 mfma", "B", COS, 16, 10, perq=True, path=Path.Mfma),
    kind_plain("batch 16 auto", "B", COS, 16, 10),
    kind_ties("ties reference merged", "C", 3, 50, False),
    kind_ties("ties reference per query", "C", 3, 50, True),
    kind_ties("ties per chunk merged", "C2", 3, 50, False),
    kind_ties("ties per chunk per query", "C2", 3, 50, True),
    kind_device("device merged cap=k A", "A", COS, 3, 10, "merged"),
    kind_device("device in place A", "A", COS, 3, 100, "in place"),
    kind_device("device k+37 A", "A", COS, 3, 100, "k+37"),       # 137 slots per query: wider than the merge block of 128
    kind_device("device k=600 staged A", "A", COS, 2, 600, "merged"),
    kind_device("device merged cap=k B", "B", COS, 3, 10, "merged"),
    kind_device("device in place B", "B", COS, 3, 10, "in place"),
    kind_device("device k+37 B", "B", COS, 3, 10, "k+37"),        # 47 slots per query: narrower than the merge block of 64
]
BY_NAME = {kd.name: kd for kd in KINDS}
# what test_groups_replaced_between_concurrent_rounds runs on A under every layout: the three table users and two kinds without a table
REGROUPED = [
    BY_NAME["groups 1 query cosine gte"], BY_NAME["groups 6 queries dot gt"], kind_groups("groups every group", "A", DOT, 1, None),
    kind_groups_top("per group m=3 on A", "A", COS, 1, 10, 3), kind_groups_top("per group m=16 5 queries on A", "A", L2, 5, 10, 16),
    BY_NAME["maxsim 6 tokens cosine"], BY_NAME["maxsim 3 tokens l2 take-min"],
    BY_NAME["l2 top-10, row mask and deleted rows"], BY_NAME["id list gather"],
]


# ---- stores --------------------------------------------------------------------------------------------------------------------------

class World:
    def __init__(self, oracle):
        rng = np.random.default_rng(7100)
        n, dim = 6037, 44
        rows = quantised(rng, (n, dim))
        q = quantised(rng, (SLOTS, 6, dim))
        self.labels37 = rng.integers(0, 37, n) * 1000 - 5
        self.labels8 = np.arange(n) // 8
        dead = rng.choice(n, 302, replace=False)  # 5 % of the rows
        back = dead[:40]
        alive = np.ones(n, bool)
        alive[dead[40:]] = False
        mask = rng.random(n) < 0.85
        stores = []
        for labels in (self.labels37, self.labels8):
            s = VecStore(dim)
            if labels is self.labels8:
                s.set_option("id_gather", 0)
            s.add_vectors(rows)
            s.set_groups(labels)
            assert s.delete_rows(dead) == dead.size and s.restore_rows(back) == back.size
            stores.append(s)
        self.A = Bundle(oracle, stores[0], rows, q, alive, mask, dense(self.labels37))
        self.A2 = Bundle(oracle, stores[1], rows, q, alive, mask, dense(self.labels8))
        self.A2.ranks = self.A.ranks  # (the same rows and queries: one ranking serves both)

        n, dim = 20_000, 264
        rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        q = rng.uniform(-1, 1, (SLOTS, 16, dim)).astype(np.float32)
        s = VecStore(dim)
        for name, value in (("exact_small", 0), ("exact_prune", 1), ("exact_sketch", 1)):
            s.set_option(name, value)
        s.add_vectors(rows)
        dead = rng.choice(n, 400, replace=False)
        assert s.delete_rows(dead) == dead.size
        alive = np.ones(n, bool)
        alive[dead] = False
        self.B = Bundle(oracle, s, rows, q, alive)

        n, dim = 3000, 8
        rows = quantised(rng, (n, dim))
        q = quantised(rng, (SLOTS, 3, dim))
        c1, c2 = VecStore(dim), VecStore(dim)
        c1.set_tie_order("reference")
        c2.set_chunk_size(128)
        c2.set_tie_order("reference_chunked")
        c1.add_vectors(rows)
        c2.add_vectors(rows)
        self.C = Bundle(oracle, c1, rows, q, tie=(1, 0))
        self.C2 = Bundle(oracle, c2, rows, q, tie=(2, 128))

    def bundle(self, kind):
        return getattr(self, kind.bundle)

    def close(self):
        for b in (self.A, self.A2, self.B, self.C, self.C2):
            b.store.close()


@pytest.fixture(scope="module")
def world(oracle):
    w = World(oracle)
    yield w
    w.close()
    path = os.environ.get("OTT_CONCURRENCY_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


# ---- threads -------------------------------------------------------------------------------------------------------------------------

def run_threads(plans):
    """plans[t]: the prepared (kind, call, expectation) triples thread t runs in order.  All threads start at a barrier.  Returns
    (intervals as (thread, t0, t1, kind name), results[t] as (kind, result, expectation)); raises on the first error of a thread."""
    barrier = threading.Barrier(len(plans))
    errs, intervals, results = [], [[] for _ in plans], [[] for _ in plans]

    def body(t):
        try:
            barrier.wait()
            for kind, call, ref in plans[t]:
                t0, t1 = call.run()
                intervals[t].append((t, t0, t1, kind.name))
                results[t].append((kind, call.where, call.read(), ref))
        except BaseException as e:  # noqa: BLE001
            errs.append((t, repr(e)))

    threads = [threading.Thread(target=body, args=(t,)) for t in range(len(plans))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs[:3]
    return [iv for per in intervals for iv in per], results


def check_all(results):
    for per_thread in results:
        for kind, where, got, ref in per_thread:
            kind.same(got, ref, where)


def peak_in_flight(intervals):
    events = sorted([(iv[1], 1) for iv in intervals] + [(iv[2], -1) for iv in intervals])
    level = peak = 0
    for _, step in events:
        level += step
        peak = max(peak, level)
    return peak


def report(test, name, intervals, calls_per_thread):
    pairs = overlap.pairs([iv[:3] for iv in intervals])
    entry = {"test": test, "kind": name, "calls": len(intervals), "calls_per_thread": calls_per_thread,
             "median_call_us": round(float(np.median([iv[2] - iv[1] for iv in intervals])) / 1000.0, 1),
             "overlapping_pairs": len(pairs), "peak_calls_in_flight": peak_in_flight(intervals)}
    REPORT.append(entry)
    print(entry)
    return pairs


def rotation(items, t):
    t %= len(items)
    return items[t:] + items[:t]


# ---- tests ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [kd.name for kd in KINDS])
def test_serial_answers_are_the_oracles(world, name):
    """every kind alone, on the store's own context, with every slot's queries: a later concurrent failure is not the expectation's"""
    kind = BY_NAME[name]
    B = world.bundle(kind)
    for slot in range(SLOTS):
        call, ref = kind.prepared(B, slot)
        call.run()
        kind.same(call.read(), ref, ("serial",) + tuple(call.where))


@pytest.mark.parametrize("name", [kd.name for kd in KINDS])
def test_same_kind_from_eight_threads(world, name):
    kind = BY_NAME[name]
    B = world.bundle(kind)
    n_calls = CALLS_FOR.get(name, CALLS)
    plans = []
    for t in range(SLOTS):
        call, ref = kind.prepared(B, t)
        plans.append([(kind, call, ref)] * n_calls)
    intervals, results = run_threads(plans)
    check_all(results)
    for per_thread in results:  # what one thread got, call after call, is the same bytes
        first = [np.asarray(x).tobytes() for x in per_thread[0][2] if isinstance(x, np.ndarray)]
        for _, where, got, _ in per_thread[1:]:
            assert [np.asarray(x).tobytes() for x in got if isinstance(x, np.ndarray)] == first, where
    pairs = report("same kind", name, intervals, n_calls)
    assert pairs, (name, "no two calls of different threads overlapped by half of the shorter one: no worker context is known to have run",
                   n_calls, "calls per thread")


def test_mixed_kinds_share_worker_contexts(world):
    """20 threads on at most 16 contexts (the wait-at-the-limit branch of ContextPool::acquire); every thread walks all kinds of A and
    A' in a rotation of its own, twice: one worker serves grouped, then MaxSim, then per-group, then id-list calls in orders no
    serial test produces.  Then every kind once more, alone: a table left dirty on the own context shows there."""
    kinds = [kd for kd in KINDS if kd.bundle in ("A", "A2")]
    plans = []
    for t in range(20):
        prepared = [(kd,) + kd.prepared(world.bundle(kd), t) for kd in kinds]
        plans.append(rotation(prepared, t * 3) * 2)
    intervals, results = run_threads(plans)
    check_all(results)
    pairs = report("mixed kinds, 20 threads", "all kinds of A and A'", intervals, 2 * len(kinds))
    assert pairs, "no overlap observed among 20 threads"
    for kd in kinds:
        call, ref = kd.prepared(world.bundle(kd), 0)
        call.run()
        kd.same(call.read(), ref, ("serial after the mixed round",) + tuple(call.where))


def test_groups_replaced_between_concurrent_rounds(world):
    """workers keep tables sized for the n_groups they last saw: 37 groups, then 6037 singleton groups (above 512: every group through
    the pair sort), then the 37 again.  Every result follows the layout that is set."""
    A = world.A
    singles = np.random.default_rng(7200).permutation(A.n)
    layouts = [A, A.variant(gid=dense(singles)), A]

    def one_round(B, r):
        plans = []
        for t in range(SLOTS):
            prepared = [(kd,) + kd.prepared(B, t) for kd in REGROUPED]
            plans.append(rotation(prepared, t + r))
        intervals, results = run_threads(plans)
        check_all(results)
        report("groups replaced, round %d (%d groups)" % (r, B.n_groups), "grouped kinds of A", intervals, len(REGROUPED))

    try:
        one_round(layouts[0], 0)
        A.store.set_groups(singles)
        assert A.store.group_count() == A.n
        one_round(layouts[1], 1)
        A.store.clear_groups()
        A.store.set_groups(world.labels37)
        one_round(layouts[2], 2)
    finally:
        A.store.set_groups(world.labels37)  # (the module's other tests find A as it was)


def test_queries_while_a_single_gpu_store_grows(oracle):
    """One appender, four readers, a store without a reserve: every block of 700 rows reallocates and moves the rows, the sketch and
    the live mask.  The store passes through 7 states (2000 rows, then one more block each); before every block the appender deletes
    rows that lead the readers' current answers, which is a mutation of its own: between two blocks a reader may also see the old
    rows without them (6 states in between).  Every answer equals the expectation of one of these states, the states one reader
    sees never go back, and the call after the last append sees the last state."""
    rng = np.random.default_rng(7300)
    dim, n0, block, n_blocks, readers = 44, 2000, 700, 6, 4
    rows = quantised(rng, (n0 + block * n_blocks, dim))
    q = quantised(rng, (SLOTS, 6, dim))
    mask = rng.random(n0) < 0.85
    kinds = [BY_NAME["l2 top-10, row mask and deleted rows"], BY_NAME["id list gather"]]
    store = VecStore(dim)
    store.add_vectors(rows[:n0])
    # the states and their expectations, before any thread runs
    states, deletions = [], []
    cur = Bundle(oracle, store, rows[:n0], q, None, mask, id_limit=n0)
    states.append(cur)
    for b in range(n_blocks):
        lead = [int(kd.prepared(cur, t)[1][0]["index"][0]) for kd in kinds for t in range(readers)]  # the best row of every reader's answers
        doomed = np.unique(np.array(lead + rng.choice(n0, 20, replace=False).tolist()))
        doomed = doomed[cur.alive[doomed]]  # (the random ones may name a row an earlier round deleted)
        alive = cur.alive.copy()
        alive[doomed] = False
        states.append(cur.variant(alive=alive))
        deletions.append(doomed)
        n = n0 + block * (b + 1)
        cur = Bundle(oracle, store, rows[:n], q, np.concatenate([alive, np.ones(block, bool)]), mask, id_limit=n0)
        states.append(cur)
    wants = {(kd.name, t): [kd.prepared(st, t)[1] for st in states] for kd in kinds for t in range(readers)}
    calls = {(kd.name, t): kd.make(states[0], t) for kd in kinds for t in range(readers)}
    done = threading.Event()
    errs, seen = [], [[] for _ in range(readers)]

    def reader(t):
        try:
            last = False
            while not last:
                last = done.is_set()  # (read BEFORE the calls: the last pass starts after the last append)
                for kd in kinds:
                    call = calls[(kd.name, t)]
                    call.run()
                    seen[t].append((kd, call.read(), last))
        except BaseException as e:  # noqa: BLE001
            errs.append((t, repr(e)))

    def appender():
        try:
            for b in range(n_blocks):
                assert store.delete_rows(deletions[b]) == deletions[b].size
                store.add_vectors(rows[n0 + block * b:n0 + block * (b + 1)])
        except BaseException as e:  # noqa: BLE001
            errs.append(("appender", repr(e)))
        finally:
            done.set()

    threads = [threading.Thread(target=reader, args=(t,)) for t in range(readers)] + [threading.Thread(target=appender)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs[:3]

    def matches(kd, got, ref):
        try:
            kd.same(got, ref, "")
            return True
        except AssertionError:
            return False

    states_seen = set()
    for t in range(readers):
        at = {kd.name: 0 for kd in kinds}
        assert seen[t] and seen[t][-1][2]
        for i, (kd, got, last) in enumerate(seen[t]):
            fits = [s for s, ref in enumerate(wants[(kd.name, t)]) if matches(kd, got, ref)]
            assert fits, (t, kd.name, i, "the answer of no state", got[0][:5])
            ahead = [s for s in fits if s >= at[kd.name]]
            assert ahead, (t, kd.name, i, "an earlier state than the one before", fits, at[kd.name])
            at[kd.name] = ahead[0]
            states_seen.add(ahead[0])
            if last:
                assert len(states) - 1 in fits, (t, kd.name, "the call after the last append does not see the last state", fits)
    REPORT.append({"test": "store grows under its readers", "calls": sum(len(x) for x in seen), "states_seen": sorted(states_seen), "states": len(states)})
    print(REPORT[-1])
    assert store.len() == rows.shape[0] and np.array_equal(store.rows(), rows)
    store.close()


def test_meta_store_filters_from_threads(oracle):
    """the evaluated device row mask is store-global; MetaStore._mask_lock makes building it and querying with it one critical section.
    Six threads, each with a predicate and a query of its own: an answer scored with another thread's mask has the wrong rows."""
    rng = np.random.default_rng(7400)
    n, dim, cs, n_threads, rounds = 4000, 24, 256, 6, 8
    rows = quantised(rng, (n, dim))
    a = rng.integers(0, 100, n).astype(np.int32)
    b = (rng.integers(-8, 9, n) / 8.0).astype(np.float32)  # (eighths: every literal below is exact in f32)
    meta = (MetaStore.from_columns([Column.from_numpy("a", DataType.Int32, a), Column.from_numpy("b", DataType.Float32, b)])
            .with_vectors(rows).with_chunk_size(cs).build())
    q = quantised(rng, (n_threads, dim))
    cases = [
        (col("a").gte(50), a >= 50),
        (col("a").lt(30), a < 30),
        (col("b").lt(0.25), b < 0.25),
        (col("a").gte(20) & col("b").gte(-0.5), (a >= 20) & (b >= -0.5)),
        (col("a").lt(80) | col("b").gt(0.5), (a < 80) | (b > 0.5)),
        (col("a").gte(40) & col("a").lt(60), (a >= 40) & (a < 60)),
    ]
    k = 10
    refs = []
    for t, (_, keep) in enumerate(cases):
        full = oracle.vec_query(rows, q[t], oracle.METRIC_COSINE, oracle.TAKE_MAX, n, ties=oracle.TIES_CANONICAL)
        refs.append(plain_expected(full, keep, k, 1)[0])
    assert len({r["index"].tobytes() for r in refs}) == n_threads  # another thread's mask gives another answer
    barrier = threading.Barrier(n_threads)
    errs, got = [], [[] for _ in range(n_threads)]

    def body(t):
        try:
            barrier.wait()
            for _ in range(rounds):
                res = meta.query(q[t], Metric.Cosine).meta_filter(cases[t][0]).take(k).collect()
                got[t].append((list(res.indices), np.array(res.scores, np.float32)))
        except BaseException as e:  # noqa: BLE001
            errs.append((t, repr(e)))

    threads = [threading.Thread(target=body, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs[:3]
    for t in range(n_threads):
        assert len(got[t]) == rounds
        for r, (idx, sc) in enumerate(got[t]):
            assert idx == refs[t]["index"].astype(np.int64).tolist(), (t, r, idx, refs[t]["index"])
            assert np.array_equal(sc.view(np.uint32), refs[t]["score"].view(np.uint32)), (t, r)
