"""GPU: bit rows and ott_query_binary on stores past 2^24 rows and 2^32 bytes of layout, as
tests/test_gpu_large_offsets.py does it for the other kinds.  tests/test_gpu_binary.py and tests/test_gpu_binary_edges.py stop at
200 000 rows and 34 MB.  Bar: index, order, count, `query` and the f32 score bits equal to tests/binary_ref.py, no tolerance, the
route asserted from binary_counters() (test_gpu_binary.gated).

How the model answers for a store it cannot score whole: tests/large_offsets.py.  A binary query applies its row mask first and a
pair's score depends on its two rows alone, so the model over the window rows words[K], mapped through K, is the answer under the row
mask K; K is 130 rows at both ends of the store and on either side of every boundary row.  Masked sweeps skip whole slices, so every
store is also swept once unmasked, with twelve planted rows at K's window edges that win by construction (the precondition asserted).

The stores, the smallest that cross each line; one is alive at a time:
  N   2^24 + 130 rows x 128 bits from host words (268 MB of layout: nine staging batches): row ids and slice numbers pass 2^24.
      Measured: the host words 0.06 s, set_binary 0.04 s
  W   2^21 + 130 rows x 16384 bits from host words (4 GiB, 128 staging batches): row 2^20 starts at byte 2^31 of the layout, row 2^21
      at byte 2^32.  The host array is zeros but for K's windows: a zero row lies at distance popcount(q), about 8192.  Measured:
      set_binary of the 4 GiB 0.74 s
  S4  dim 4, 2^24 + 130 rows filled on the device, set_binary_sign: the kernel's word index n * W and its row ids pass 2^24.
      Measured: set_binary_sign under 0.01 s
  SW  dim 2048, 2^20 + 130 rows (8 GiB of dense rows), set_binary_sign: row 2^19 starts at byte 2^32 of the dense rows, row 2^20
      at float offset 2^31.  Measured: the fill 0.38 s, set_binary_sign under 0.01 s
The times are an MI355X's when the file was written; every run prints its own (pytest -s).  No test of the file took more than 1 s
there but the first, whose 13 s are the process's first use of the device."""
import time

import numpy as np
import pytest

import binary_ref as BR
import large_offsets as LO
from otters_amd import OttersError, VecStore
from test_gpu_binary import GATES, MAX, MIN, gated, rows_at_distance, run, same

pytestmark = pytest.mark.gpu

SEED = 0xB17
HALF = LO.HALF
SHAPES = {  # name: (dim of the dense rows, n_bits, rows, boundary rows, host words or None = sign bits of rows filled on the device)
    "N": (1, 128, (1 << 24) + HALF, (1 << 24,), True),
    "W": (1, 16384, (1 << 21) + HALF, (1 << 20, 1 << 21), True),
    "S4": (4, 4, (1 << 24) + HALF, (1 << 24,), False),
    "SW": (2048, 2048, (1 << 20) + HALF, (1 << 19, 1 << 20), False),
}


def free_or_skip(name, need):
    """(the first call may be the process's first use of torch's device runtime: its time is printed apart from the store's)"""
    import torch
    t0 = time.perf_counter()
    free = torch.cuda.mem_get_info(0)[0]
    print(f"store {name}: asking for the free device memory took {time.perf_counter() - t0:.2f} s")
    if free < need:
        pytest.skip(f"store {name} needs {need} bytes of device memory (rows, bit rows, tables and a quarter more), {free} are free")


def planted_positions(n, boundaries):
    """(near, far): twelve rows at K's window edges — the store's first and last row, both sides of every boundary, the slices' edges
    beside them, the windows' outer edges — and twelve more beside them, all distinct, each sorted"""
    b0, b1 = boundaries[0], boundaries[-1]
    want = [0, n - 1, b0 - 1, b0, b1 - 1, b1, HALF - 1, b0 - HALF, b1 + 64, b0 - 64, b0 - 65, b1 + 63, b0 + 1, n - 2, b0 + HALF - 1, b1 - HALF]
    near = list(dict.fromkeys(int(r) for r in want))[:12]
    beside = [r + d for d in (1, -1, 2, -2, 3, -3) for r in near]
    inside = lambda r: any(a <= r < a + c for a, c in LO.spans(n, boundaries))  # noqa: E731
    far = [r for r in dict.fromkeys(beside) if inside(r) and r not in near][:12]
    assert len(near) == len(far) == 12
    return np.array(sorted(near), np.int64), np.array(sorted(far), np.int64)


class Big:
    """one store with its bit rows, the window rows K and their words: made once, never changed"""

    def __init__(self, oracle, name):
        self.name = name
        self.dim, self.n_bits, self.n, self.boundaries, from_host = SHAPES[name]
        n, n_bits, W = self.n, self.n_bits, BR.words(self.n_bits)
        self.K, mask_words = LO.windows(n, self.boundaries)
        self.mask = LO.mask_bool(mask_words, n)  # the plans take bool[n]
        self.near, self.far = planted_positions(n, self.boundaries)
        assert np.isin(self.near, self.K).all() and np.isin(self.far, self.K).all() and not np.isin(self.near, self.far).any()
        rng = np.random.default_rng(SEED + n_bits)
        self.q_bits = rng.integers(0, 2, (5, n_bits)).astype(bool)
        self.q = BR.pack(self.q_bits)
        free_or_skip(name, int(1.25 * (n * (self.dim * 4 + 5) + BR.layout_bytes(n, n_bits) + 5 * n * 8 + 5 * n * 24 // 8)))
        t0 = time.perf_counter()
        self.store = VecStore(self.dim)
        self.store.reserve(n)
        self.store.append_random(n, SEED)
        self.store.inv_norms(n - 1, 1)  # (waits for the fill)
        t1 = time.perf_counter()
        if from_host:
            self.words_all = self.host_words(rng)
            t2 = time.perf_counter()
            self.store.set_binary(self.words_all, n_bits)
            self.words = np.ascontiguousarray(self.words_all[self.K])
            what = f"the host words {t2 - t1:.2f} s, set_binary {time.perf_counter() - t2:.2f} s"
        else:
            self.words_all = None
            self.store.set_binary_sign()
            t2 = time.perf_counter()
            self.R = LO.window_rows(oracle, self.K, self.dim, SEED)
            self.words = BR.pack(BR.sign_bits(self.R))
            what = f"set_binary_sign {t2 - t1:.2f} s, the window rows {time.perf_counter() - t2:.2f} s"
        self.words.setflags(write=False)
        assert self.words.shape == (self.K.size, W)
        assert self.store.binary_info() == {"n_bits": n_bits, "bytes": BR.layout_bytes(n, n_bits)}
        print(f"store {name}: {n} rows x {n_bits} bits, {BR.layout_bytes(n, n_bits)} bytes of layout; the dense rows {t1 - t0:.2f} s, {what}")

    def host_words(self, rng):
        """N: i.i.d. words.  W: zeros but for K's windows (the pages of the rows between them are never written).  Both: twelve rows
        at distances 0 .. 11 from query 0 and twelve at n_bits - 0 .. 11"""
        n, n_bits, W = self.n, self.n_bits, BR.words(self.n_bits)
        if self.name == "N":
            words = rng.integers(0, 2 ** 64, (n, W), dtype=np.uint64)
        else:
            try:
                words = np.zeros((n, W), np.uint64)
            except MemoryError:
                self.store.close()
                pytest.skip(f"store {self.name} needs {n * W * 8} bytes of host memory for its words")
            for a, c in LO.runs_of(self.K):
                words[a:a + c] = rng.integers(0, 2 ** 64, (c, W), dtype=np.uint64)
        words[self.near] = BR.pack(rows_at_distance(self.q_bits[0], np.arange(12), rng))
        words[self.far] = BR.pack(rows_at_distance(self.q_bits[0], n_bits - np.arange(12), rng))
        return words

    def S(self, hits):
        return [LO.to_store_index(self.K, h) for h in hits]

    def close(self):
        self.store.close()
        self.words_all = None


class Stores:
    def __init__(self, oracle):
        self.oracle, self.name, self.big = oracle, None, None

    def get(self, name):
        if self.name != name:
            self.drop()
            self.big, self.name = Big(self.oracle, name), name
        return self.big

    def drop(self):
        if self.big is not None:
            self.big.close()
        self.big, self.name = None, None


@pytest.fixture(scope="module")
def stores(oracle):
    s = Stores(oracle)
    yield s
    s.drop()
    import gc
    gc.collect()


TOO_MANY_PAIRS = 1 << 26  # ott_binary_plan.h: BINARY_MAX_SORT_PAIRS: k_eff above 512 is served up to this many (query, row) pairs


def case_masked_by_the_windows(stores, name, nqs):
    """the row mask is K: the model over words[K], its indices mapped through K.  k = 513 is more than the table route's block lists
    hold: the pair form, which a call of more than 2^26 (query, row) pairs is refused (ott_binary_plan.h: binary_check_cap) — the
    store's rows count there, not the mask's, so on N five queries are refused and three are the most that are served"""
    b = stores.get(name)
    Sc = BR.scores(b.words, b.q)
    for nq in nqs:
        for k in (10, 513):
            for tk in (MIN, MAX):
                if k > 512 and nq * b.n > TOO_MANY_PAIRS:
                    with pytest.raises(OttersError, match="ott_query_binary: k above 512 is served only up to 2\\^26") as ei:
                        run(b.store, b.q[:nq], b.n_bits, tk, k, mask=b.mask)
                    assert ei.value.status == -4
                    continue
                exp = b.S(BR.expected(Sc[:nq], tk, k))
                assert exp[0].size == min(k, b.K.size) and exp[0]["index"].max() >= b.boundaries[-1] > exp[0]["index"].min()
                for gate in GATES:
                    got, stats = gated(b.store, gate, lambda: run(b.store, b.q[:nq], b.n_bits, tk, k, mask=b.mask), b.n_bits, k)
                    same(got, exp, (name, "masked", nq, k, tk, gate))
                    assert stats["vectors_compared"] == b.n * nq and stats["bytes_scanned"] == stats["passes"] * BR.layout_bytes(b.n, b.n_bits)


def case_read_binary_of_every_window(stores, name):
    b = stores.get(name)
    at = 0
    for a, c in LO.runs_of(b.K):
        assert np.array_equal(b.store.read_binary(a, c), b.words[at:at + c]), (name, a, c)
        at += c
    for r in [0, b.n - 1] + [x for bd in b.boundaries for x in (bd - 1, bd)]:  # single rows on both sides of every boundary
        assert np.array_equal(b.store.read_binary(r, 1), b.words[LO.compact_of(b.K, [r])]), (name, r)


def min_and_max_distance_outside(words, q0, planted, block=1 << 20):
    """over every row but the planted ones: the least and the greatest Hamming distance from q0, by the model, in blocks"""
    lo, hi = 1 << 30, -1
    for a in range(0, words.shape[0], block):
        d = BR.distances(words[a:a + block], q0[None])[0].astype(np.int64)
        inside = planted[(planted >= a) & (planted < a + block)] - a
        d[inside] = -1
        d = d[d >= 0]
        if d.size:
            lo, hi = min(lo, int(d.min())), max(hi, int(d.max()))
    return lo, hi


def case_unmasked_sweep_returns_the_planted_rows(stores, name, nqs):
    """no mask: every slice is read.  The twelve best rows of query 0 are the planted ones, in distance order, with the model's bits,
    because no other row lies within 20 bits of them (asserted).  N: from the model's distances over ALL rows, in blocks; the chance
    that i.i.d. rows of 128 bits break it is below 1e-8; query 0 alone is asked.  W: every row outside K is the zero row, so the model
    over K and the twelve lowest rows outside it (a zero row that is a hit is one of these: ties go to the lower row) is the whole
    store's answer for every query"""
    b = stores.get(name)
    planted = np.sort(np.r_[b.near, b.far])
    if name == "N":
        Kp, words_p = b.K, b.words
        lo, hi = min_and_max_distance_outside(b.words_all, b.q[0], planted)
    else:
        outside = np.setdiff1d(np.arange(HALF + 12, dtype=np.int64), b.K)[:12]
        assert outside.size == 12 and not b.words_all[outside].any()
        Kp = np.sort(np.r_[b.K, outside])
        words_p = b.words_all[Kp]
        d = BR.distances(words_p, b.q[:1])[0].astype(np.int64)[~np.isin(Kp, planted)]
        lo, hi = int(d.min()), int(d.max())
    assert 20 < lo and hi < b.n_bits - 20, (lo, hi)
    Sc = BR.scores(words_p, b.q)
    for nq in nqs:
        for tk, rows in ((MIN, b.near), (MAX, b.far)):
            exp = [LO.to_store_index(Kp, h) for h in BR.expected(Sc[:nq], tk, 12)]
            assert exp[0]["index"].tolist() == rows.tolist() and exp[0]["score"].tolist() == [float(d if tk == MIN else b.n_bits - d) for d in range(12)]
            for gate in (0, 1):
                got, stats = gated(b.store, gate, lambda: run(b.store, b.q[:nq], b.n_bits, tk, 12), b.n_bits, 12)
                same(got, exp, (name, "planted", nq, tk, gate))
                assert stats["vectors_compared"] == b.n * nq and stats["bytes_scanned"] == stats["passes"] * BR.layout_bytes(b.n, b.n_bits)


def case_sign_store(stores, name):
    """set_binary_sign over dense rows filled on the device: every window read back equals the sign bits of the oracle's rows, and
    one masked sign query equals the model"""
    b = stores.get(name)
    case_read_binary_of_every_window(stores, name)
    q = np.random.default_rng(SEED).uniform(-1, 1, (2, b.dim)).astype(np.float32)
    qw = BR.pack(BR.sign_bits(q))
    p = b.store.binary_query_sign(q).take(10).resolve()
    assert np.array_equal(p.words, qw)
    Sc = BR.scores(b.words, qw)
    for tk in (MIN, MAX):
        exp = b.S(BR.expected(Sc, tk, 10))
        for gate in GATES:
            got, stats = gated(b.store, gate, lambda: run(b.store, qw, b.n_bits, tk, 10, mask=b.mask), b.n_bits, 10)
            same(got, exp, (name, "sign, masked", tk, gate))
            assert stats["vectors_compared"] == b.n * 2


# ---- the cases in the stores' order: one store is alive at a time --------------------------------------------------------------------
def test_n_masked_by_the_windows(stores):
    case_masked_by_the_windows(stores, "N", (1, 3, 5))


def test_n_read_binary(stores):
    case_read_binary_of_every_window(stores, "N")


def test_n_unmasked_with_planted_rows(stores):
    case_unmasked_sweep_returns_the_planted_rows(stores, "N", (1,))


def test_w_masked_by_the_windows(stores):
    case_masked_by_the_windows(stores, "W", (1, 2))


def test_w_read_binary(stores):
    case_read_binary_of_every_window(stores, "W")


def test_w_unmasked_with_planted_rows(stores):
    case_unmasked_sweep_returns_the_planted_rows(stores, "W", (1, 2))


def test_sign_rows_of_4_floats_past_2_24_rows(stores):
    case_sign_store(stores, "S4")


def test_sign_rows_of_2048_floats_past_2_32_bytes(stores):
    case_sign_store(stores, "SW")
    stores.drop()
