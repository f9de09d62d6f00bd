"""Sharp inputs for the pruned exact sweep: rows whose score bound is nearly their score, and corpora whose required
hits sit a few f32 steps beyond the gate.  Builders only: numpy and the CPU oracle, no GPU and no compiled driver.  The conditions
the builders promise — a small slack of the tight rows, a margin of at most 1024 steps of every challenger — are proved with the
header's own bound in tests/test_exact_prune_sharp_cpu.py; tests/test_gpu_exact_prune_sharp.py runs the corpora on the device.

A tight row, per form of the sweep (FORMS):
  head, c1  four bits per dim: every value of the row on a reconstruction level a (2 code + 1), a a power of two, and one tail value
            of 16 a, which sets the cell width 2 a and clips, so the line's a is the row's a and the remainder is that one a;
  sk3       three bits: the same with codes -4 .. 3 and one value of 8 a;
  sk1       one bit: every sketched value +-a, so the mean magnitude is a and the remainder is zero;
  7/8       no sketch: the tail behind the checkpoint is c q_t with c = +-2^s, so the Cauchy-Schwarz step holds with equality on the
            side of the take that c's sign names.
A corpus (sharp_corpus): copies of one tight row A in the seed, challengers behind it — A with one stage-0 element moved by a few
f32 ulps, so that the oracle's score lies 1 .. 1024 ordinals beyond A's — and low-scoring filler of the same family."""
import functools
import math

import numpy as np

FORMS = {  # name -> the store options that select it (exact_small = 0 and exact_prune = 1 besides)
    "head": dict(exact_sketch=1, exact_sketch_bits=4, exact_sketch_head=-1),
    "c1": dict(exact_sketch=1, exact_sketch_bits=4, exact_sketch_head=0),
    "sk3": dict(exact_sketch=1, exact_sketch_bits=3, exact_sketch_head=-1),
    "sk1": dict(exact_sketch=1, exact_sketch_bits=1, exact_sketch_head=-1),
    "7/8": dict(exact_sketch=0, exact_sketch_bits=4, exact_sketch_head=-1),
}
FAMILY = {"head": "sk4", "c1": "sk4", "sk3": "sk3", "sk1": "sk1", "7/8": "7/8"}  # the two four-bit forms share their rows
VARIANTS = ("aligned", "against", "2^-60", "2^40", "edge", "stage0")
# not a tight row, and outside the quarter rule: "aligned" with stage 0 times four, so that in the four-bit forms most of stage 0's
# codes clamp and the head's remainder over ALL stages, rho_all, is many times the line's rho — and lies along the query, so the
# score needs nearly all of it.  The other variants keep stage 0 on the levels, where rho_all is rho: they cannot tell the two apart
LOOSE_VARIANTS = ("clamp0",)
# the four-bit forms decode a line against the QUANTISED query (ott_prune.h: prune_query_quant): q_i = 2^e qhat_i + e_i, qhat = 256 d2 +
# 16 d1 + d0.  Rows along a uniform query's signs see the middle digit and the error e_i with random signs, and what they add stays
# inside the row's slack.  "qdigit": every odd dim takes the sign of the query's middle digit d1 (the even dims the query's own sign,
# so that the row still scores high): K needs its 16 K1 term.  "qerr": a query of one large element and many small ones, whose
# quantisation error is most of it; every code at the range's edge with the sign of e_i: the score needs nearly all of 15 a qe1
QUANT_VARIANTS = ("qdigit", "qerr")
MAX_STEPS = 1024  # the cap on a challenger's margin, in f32 ordinals
COPIES = 256      # copies of A in the seed: at least k for every k the tests use, so the seed's k-th best is A's score exactly
KS = (1, 10, 64, 100, 256)
METRICS = (0, 2)  # cosine, dot product (the oracle's and the library's numbers)
# the corpora of the GPU file: (dim, rows, variant, staircase).  20 000 rows = 312 tiles and one of 32 rows, at the line lengths of
# the existing tests; 140 000 x 96: four challengers in every gated tile, ascending over the whole store; and the rows that need rho_all
SHAPES = ((96, 20_000, "aligned", False), (256, 20_000, "2^-60", False), (773, 20_000, "edge", False), (896, 20_000, "stage0", False),
          (96, 140_000, "2^40", True), (256, 20_000, "clamp0", False), (256, 20_000, "qdigit", False), (896, 20_000, "qerr", False))


def forms_of(shape):
    """the quantised query is the four-bit forms' alone"""
    return ("head", "c1") if shape[2] in QUANT_VARIANTS else tuple(FORMS)


def stages(dim):
    return ((dim + 3) // 4 * 4 + 31) // 32


def checkpoint(form, dim):
    """the first dim the form's bound covers without reading it: the sketch's first dim, or 7/8 of the stages (ott_exact_plan.h:
    prune_plan, ott_prune.h: prune_sketchb_stage0).  The head form's own checkpoint is 0; its LINE starts here"""
    nst, fam = stages(dim), FAMILY.get(form, form)
    if fam == "sk4":
        c = 1
    elif fam == "sk3":
        c = max(1, nst - (5 * nst + 7) // 8)
    elif fam == "sk1":
        c = nst - (nst + 3) // 4
    else:
        c = nst * 7 // 8
        while c > 0 and c * 32 > dim - dim % 8:
            c -= 1
    assert 1 <= c < nst and 32 * c <= dim - dim % 8, (form, dim, c)
    return 32 * c


def tkey(x):
    """f32::total_cmp as an unsigned key (the library's total_key); arrays too"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def query(dim, seed=0, variant="aligned"):
    q = np.random.default_rng(1000 + 7 * dim + seed).uniform(-1, 1, dim).astype(np.float32)
    if variant == "qerr":  # 2^e = 2^-10 from the one large element: the others quantise to 0 or +-1
        q *= np.float32(1e-3)
        q[3] = 1.0
    return q


def quantised(q):
    """prune_query_quant and prune_quant_digits restated: qhat, its middle balanced base-16 digit, and the error q - 2^e qhat"""
    mx = float(np.abs(q).max())
    e = math.frexp(mx)[1] - 11
    if math.ldexp(mx, -e) > 1911:
        e += 1
    qhat = np.clip(np.rint((q * np.float32(2.0 ** -e)).astype(np.float32)), -1911, 1911).astype(np.int64)
    d0 = ((qhat + 8) & 15) - 8
    d1 = ((((qhat - d0) >> 4) + 8) & 15) - 8
    return qhat, d1, q.astype(np.float64) - 2.0 ** e * qhat


def _scale(variant):
    return np.float32(2.0 ** {"2^-60": -60, "2^40": 40}.get(variant, -3))


def tight_rows(form, dim, q, n, rng, variant="aligned", signs=None):
    """n tight rows of the form's family.  signs: per row +1 (along the query's signs: a high score), -1 (against them), or 0 = random
    signs, the filler.  Default: +1, or -1 for the variant "against".  The other variants: the scale a = 2^-60 or 2^40 in place of
    2^-3, every code at the range's edge, a stage 0 that holds most of the norm (edge codes there, the two smallest behind it)"""
    fam = FAMILY.get(form, form)
    assert variant in VARIANTS + LOOSE_VARIANTS + QUANT_VARIANTS
    if signs is None:
        signs = np.full(n, -1 if variant == "against" else 1)
    signs = np.asarray(signs).astype(np.int8)
    a = _scale(variant)
    first = checkpoint(form, dim)
    sq = np.where(np.signbit(q), -1, 1).astype(np.int8)
    if variant in QUANT_VARIANTS:
        _, d1, err = quantised(q)
        follow = np.where(np.arange(dim) % 2 == 1, d1, 0) if variant == "qdigit" else err
        sq = np.where(follow != 0, np.sign(follow), sq).astype(np.int8)
    s = np.where(signs[:, None] == 0, (2 * rng.integers(0, 2, (n, dim), dtype=np.int8) - 1), signs[:, None] * sq[None, :]).astype(np.int8)
    top = 7 if fam == "sk3" else 15  # the largest |2 code + 1| of the levels used
    if variant == "qerr":  # (the filler: against the query's one large element, so that it scores low)
        big = int(np.argmax(np.abs(q)))
        s[signs == 0, big] = -sq[big]
    if variant in ("edge", "qerr"):
        kap = np.full((n, dim), top, np.int8)
    elif variant == "stage0":
        kap = (2 * rng.integers(0, 2, (n, dim), dtype=np.int8) + 1).astype(np.int8)
        kap[:, :32] = top
    else:
        kap = (2 * rng.integers(0, (top + 1) // 2, (n, dim), dtype=np.int8) + 1).astype(np.int8)
    rows = (s * kap).astype(np.float32)
    rows *= a  # (a small odd integer times a power of two: exact)
    if variant == "clamp0":
        rows[:, :32] *= np.float32(4)
    if fam in ("sk4", "sk3"):
        rows[:, first + 1] = a * np.float32(top + 1) * s[:, first + 1].astype(np.float32)  # 16 a (8 a): the cell width is 2 a, the value clips
    elif fam == "sk1":
        rows[:, first:] = a * s[:, first:].astype(np.float32)
    else:  # c q_t with c = +-2^s: the prefix on levels of a sixteenth of it, so that its values are the size of the tail's
        c = np.where(signs == 0, (2.0 * rng.integers(0, 2, n) - 1) * 0.5 ** rng.integers(0, 3, n), signs).astype(np.float32) * (a * np.float32(16))
        rows[:, first:] = c[:, None] * q[None, first:]
        if variant == "stage0":
            rows[:, :32] *= np.float32(4)
    return rows


def scores(oracle, rows, q, metric):
    """the oracle's bit-exact score of every row"""
    h = oracle.vec_query(rows, q, metric, oracle.TAKE_MAX, rows.shape[0], 0, 0.0, ties=oracle.TIES_CANONICAL)
    assert h.size == rows.shape[0]
    out = np.empty(rows.shape[0], np.float32)
    out[h["index"].astype(np.int64)] = h["score"]
    return out


def _bump(x, ulps):
    """x moved by `ulps` f32 steps of its magnitude (never through zero)"""
    b = int(np.float32(x).view(np.uint32))
    mag = (b & 0x7FFFFFFF) + int(ulps)
    assert 0x00800000 <= mag < 0x7F800000, (x, ulps)
    return np.uint32((b & 0x80000000) | mag).view(np.float32)


def nudge_pool(oracle, A, q, metric, two=False):
    """Challengers of A: copies with ONE stage-0 element moved by t ulps of its magnitude, t on a geometric grid of both signs, that
    the oracle scores 1 .. MAX_STEPS ordinals above A (Take Max; the negated rows are Take Min's).  With `two`, a second element is
    moved beforehand — the finer search for a family whose single nudges miss the window.
    -> (rows [p, dim], steps [p]) in ascending steps, one entry per distinct step"""
    grid = np.unique(np.round(1.19 ** np.arange(1, 90)).astype(np.int64))
    grid = grid[grid < (1 << 22)]
    grid = np.concatenate([grid, -grid])
    base = A
    if two:
        base = A.copy()
        base[31] = _bump(A[31], -(1 << 12))
    js = range(31 if two else 32)
    cand = np.repeat(base[None, :], 1 + len(js) * grid.size, axis=0)
    at = 1
    for j in js:
        for t in grid:
            cand[at, j] = _bump(base[j], t)
            at += 1
    cand[0] = A
    key = tkey(scores(oracle, cand, q, metric))
    steps = key[1:] - key[0]
    ok = np.flatnonzero((steps >= 1) & (steps <= MAX_STEPS))
    _, pick = np.unique(steps[ok], return_index=True)
    ok = ok[pick]
    return cand[1:][ok], steps[ok]


def seed_rows(n):
    """prune_plan's seed of a store this small: a tenth of the rows in whole tiles"""
    return max(64, (n // 10 + 63) // 64 * 64)


def challenger_slots(n, staircase=False):
    """the rows that hold challengers, behind the seed: where the device code branches.  Plain: lanes 0 and 63 of the first gated tile,
    72 consecutive rows across two tiles (a wave queues 64 survivors and flushes with rows still to come), lanes of two adjacent
    tiles, the first and last row of the last tile (a short one when n is no multiple of 64).  Staircase: four lanes of every tile"""
    s, last = seed_rows(n), (n - 1) // 64 * 64
    if staircase:
        return np.concatenate([np.array([t, t + 21, t + 42, t + 63]) for t in range(s, n - 63, 64)])
    slots = [s, s + 63, last, n - 1]
    slots += list(range(s + 64 * 5, s + 64 * 5 + 72))
    slots += [s + 64 * 9 + 1, s + 64 * 9 + 62, s + 64 * 10, s + 64 * 10 + 33, s + 64 * 10 + 63]
    slots = np.unique(np.array(slots))
    assert slots[0] >= s and slots[-1] < n
    return slots


@functools.lru_cache(maxsize=4)
def _base(fam, dim, n, variant, seed):
    """the query, A and the filler: what the two metrics share"""
    rng = np.random.default_rng(dim * 131 + n + seed)
    q = query(dim, seed, variant)
    A = tight_rows(fam, dim, q, 1, rng, variant)[0]
    return q, A, tight_rows(fam, dim, q, n, rng, variant, signs=np.zeros(n, np.int8))


@functools.lru_cache(maxsize=8)
def _corpus(fam, dim, n, metric, variant, staircase, seed):
    import oracle
    oracle.build()
    q, A, filler = _base(fam, dim, n, variant, seed)
    rows = filler.copy()
    sc = scores(oracle, np.concatenate([A[None, :], rows]), q, metric)
    assert sc[0] > 0
    high = sc[1:] > np.float32(0.9) * sc[0]
    rows[high] = -rows[high]
    pool, steps = nudge_pool(oracle, A, q, metric)
    if pool.shape[0] < 8:
        pool, steps = nudge_pool(oracle, A, q, metric, two=True)
    assert pool.shape[0] >= 8, (fam, dim, metric, variant, pool.shape)
    s = seed_rows(n)
    copies = np.unique(np.linspace(0, s - 1, COPIES).astype(np.int64))
    assert copies.size == COPIES and copies[-1] == s - 1
    rows[copies] = A
    slots = challenger_slots(n, staircase)
    which = (np.arange(slots.size) * pool.shape[0]) // slots.size  # ascending: a later slot never scores lower
    rows[slots] = pool[which]
    rows.setflags(write=False)
    return dict(rows=rows, q=q, A=A, copies=copies, slots=slots, steps=steps[which], pool=pool.shape[0], gate=sc[0])


def sharp_corpus(form, dim, n, metric, variant="aligned", staircase=False, seed=0):
    """-> dict(rows, q, A, gate, copies, slots, steps, pool); shared and read-only.  Take Max; for Take Min negate the rows (every
    score negates exactly, so the margins are the same on the other side).  The seed — the first tenth of the rows in whole tiles —
    holds COPIES copies of the tight row A spread over its tiles, so its k-th best is A's score `gate` for every k <= COPIES;
    the slots hold challengers in ascending score order (the pool's steps spread over them, lowest first); every other row is filler
    of the family with random signs, negated where it would come within a tenth of A's score"""
    assert variant != "against"
    return _corpus(FAMILY[form], dim, n, metric, variant, staircase, seed)
