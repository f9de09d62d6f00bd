"""IEEE edge-value corpora for every query path (test infrastructure; numpy only, no GPU).

The fuzz corpora (tests/test_gpu_fuzz.py) keep elements, products and sums of squares inside the normal f32 range.  These do
not.  Every builder returns (rows, queries, info): f32 arrays and a dict that names the edge the family aims at.  The verdict of
every test that uses them is the oracle's; this module only chooses the data and restates, in numpy, what a precondition needs.

  a  signed-zero cosines: queries / rows whose f32 sum of squares overflows although every element is finite (q_inv = 0 or
     inv = 0: every cosine is dot * 0 = +0.0, -0.0 or NaN), and rows of one large element plus subnormal multiples of 2^-149;
  b  subnormal sums of squares: norms in [3e-22, 1e-19], rows of subnormal elements only, rows where some squares underflow,
     rows whose squares all underflow (a nonzero row of norm 0);
  c  overflow: dot products that overflow to +-inf (and inf - inf = NaN, dropped), squared-L2 differences that overflow to +inf;
  d  rows exact in IEEE half with most of their dot product in half subnormals, for the hi pass (hi_fmt 1);
  e  rows whose bf16 lo part falls below 2^-126, for hi_fmt 0 and the split pass."""
import numpy as np

f32 = np.float32
TINY = f32(2.0 ** -149)     # smallest f32 subnormal
MIN_NORMAL = f32(2.0 ** -126)
FLT_MAX = np.finfo(np.float32).max

# filter thresholds at the edges (each with every Cmp)
THRESHOLDS = [0.0, -0.0, float("inf"), float("-inf"), float(FLT_MAX), -float(FLT_MAX), float(TINY), -float(TINY)]


def seq_sumsq(x: np.ndarray) -> np.ndarray:
    """sequential f32 sum of squares per row (the reference's norm, src/vec.rs:387-397)"""
    x = np.atleast_2d(np.asarray(x, f32))
    s = np.zeros(x.shape[0], f32)
    with np.errstate(over="ignore", under="ignore"):
        for j in range(x.shape[1]):
            s = s + x[:, j] * x[:, j]
    return s


def signed_zero_cosines(rng, n=40, dim=8):
    """family a.  Query 0 (x 1e20): its sum of squares overflows, q_inv = 0, every cosine is +-0.  Rows n-8.. : rows whose own
    norm overflows (inv = 0).  Rows n-16..n-9: one large element plus subnormal multiples of 2^-149 (+-0 and +-2^-149 cosines
    against query 1, which has no component along the large element)."""
    rows = rng.uniform(-1, 1, (n, dim)).astype(f32)
    rows[n - 8:] = (rng.uniform(-1, 1, (8, dim)) * 1e20).astype(f32)
    sub = rows[n - 16:n - 8]
    sub[:] = (rng.integers(-3, 4, (8, dim)) * TINY).astype(f32)
    sub[:, 0] = f32(1.0)
    q = np.empty((2, dim), f32)
    q[0] = (rng.uniform(-1, 1, dim) * 1e20).astype(f32)
    q[1] = rng.uniform(-1, 1, dim).astype(f32)
    q[1, 0] = 0.0
    return rows, q, {"family": "a", "huge_query": 0, "huge_rows": list(range(n - 8, n)), "subnormal_rows": list(range(n - 16, n - 8))}


def subnormal_sums(rng, n=64, dim=8):
    """family b: every row's f32 sum of squares (sequential) is below 2^-126 or underflows in part."""
    rows = np.empty((n, dim), f32)
    q4 = n // 4
    # norms in [3e-22, 1e-19]: the sum of squares is subnormal (1e-43 .. 1e-38) and sqrtf gets a subnormal input
    u = rng.uniform(-1, 1, (q4, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rows[:q4] = (u * 10.0 ** rng.uniform(-21.5, -19, (q4, 1))).astype(f32)
    # subnormal elements only
    rows[q4:2 * q4] = (rng.integers(-2 ** 20, 2 ** 20, (q4, dim)) * TINY).astype(f32)
    # some squares underflow to 0, the norm does not
    rows[2 * q4:3 * q4] = (rng.uniform(-1, 1, (q4, dim)) * 1e-30).astype(f32)
    rows[2 * q4:3 * q4, 0] = f32(1e-10)
    # every square underflows: a nonzero row of norm 0
    rows[3 * q4:] = (rng.uniform(-1, 1, (n - 3 * q4, dim)) * 1e-25).astype(f32)
    q = rng.uniform(-1, 1, (3, dim)).astype(f32)
    q[1] *= f32(1e-22)   # a query of subnormal sum of squares
    q[2] = rows[q4]      # a query of subnormal elements
    return rows, q, {"family": "b", "blocks": q4}


def overflow(rng, n=48, dim=8):
    """family c: dots that overflow to +-inf (and inf - inf = NaN), squared-L2 differences that overflow to +inf (many equal
    +inf scores)."""
    rows = rng.uniform(-1, 1, (n, dim)).astype(f32)
    h = n // 3
    rows[:h] = (np.sign(rng.uniform(-1, 1, (h, dim))) * 1e30).astype(f32)      # dot with a 1e10 query: inf - inf = NaN
    rows[:4] = f32(1e30)                                                        # ... +inf
    rows[4:8] = f32(-1e30)                                                      # ... -inf
    rows[h:2 * h, :] = f32(3e38)                                                # L2 against a negative query: +inf
    rows[h:2 * h, 1::2] = f32(-3e38)
    q = np.empty((3, dim), f32)
    q[0] = f32(1e10)
    q[1] = (rng.uniform(-1, 1, dim) * 1e10).astype(f32)
    q[2] = f32(-3e38)
    return rows, q, {"family": "c"}


HALF_SUB = 2.0 ** -24      # IEEE half: subnormals are multiples of 2^-24 below 2^-14


def half_subnormal_rows(rng, dim=768, n_sub=64, n_fill=700, n_rand=2000):
    """family d.  Row 0 carries the store's largest norm (1.0: the hi plane's power-of-two factor stays 1).  The n_sub "S" rows
    are exact in half: one large element on axis 0 and half subnormals (multiples of 2^-24 below 2^-14) on every other axis, all
    of the query's sign.  The query has a small component on axis 0 and the rest on the subnormal axes, so an S row's dot is
    mostly subnormal products.  The n_fill "F" rows are exact half normals and score between "S with subnormals flushed" and
    "S as it is": a unit that flushed the subnormals would list the F rows first and leave the S rows outside a certified
    top-k.  The rest is random filler of lower score."""
    rows = np.zeros((1 + n_sub + n_fill + n_rand, dim), f32)
    rows[0, 0] = 1.0
    q = np.zeros(dim, f32)
    q[0] = f32(0.25)
    q[1:] = f32(np.sqrt((1 - 0.0625) / (dim - 1)))
    q = q.astype(np.float16).astype(f32)
    big = f32(0.5)
    sub_m = rng.integers(600, 1023, (n_sub, dim - 1))
    S = np.zeros((n_sub, dim), f32)
    S[:, 0] = big
    S[:, 1:] = (sub_m * HALF_SUB).astype(f32)
    s_exact = S.astype(np.float64) @ q.astype(np.float64)
    s_flushed = np.float64(big) * np.float64(q[0])
    # F: exact half normals (on axis 0 only), score in between
    lo, hi = s_flushed, s_exact.min()
    fvals = np.linspace(lo + 0.2 * (hi - lo), lo + 0.8 * (hi - lo), n_fill) / np.float64(q[0])
    Fr = np.zeros((n_fill, dim), f32)
    Fr[:, 0] = fvals.astype(np.float16).astype(f32)
    R = (rng.uniform(-1, 1, (n_rand, dim)) * 0.001).astype(np.float16).astype(f32)
    R[:, 0] = f32(2.0 ** -7)
    rows[1:1 + n_sub] = S
    rows[1 + n_sub:1 + n_sub + n_fill] = Fr
    rows[1 + n_sub + n_fill:] = R
    # shuffle (row 0 stays: it is only there for the factor)
    perm = 1 + rng.permutation(rows.shape[0] - 1)
    rows[1:] = rows[perm]
    s_idx = np.where(np.isin(perm, np.arange(1, 1 + n_sub)))[0] + 1
    return rows, q[None, :], {"family": "d", "s_rows": s_idx, "s_exact": s_exact, "s_flushed": float(s_flushed), "k": n_sub}


def bf16_lo_edges(rng, n=512, dim=96):
    """family e: rows of norm >= 1e-18 (not flagged irregular) whose elements' bf16 lo parts (x - bf16(x)) fall below 2^-126."""
    rows = (rng.uniform(-1, 1, (n, dim)) * 1e-17).astype(f32)
    # elements in [2^-126, 2^-119): normal in f32, their bf16 rounding residue is below 2^-126
    m = rng.integers(2 ** 23, 2 ** 24, (n, dim)).astype(np.float64)
    e = rng.integers(-149, -142, (n, dim)).astype(np.float64)
    tail = (np.sign(rng.uniform(-1, 1, (n, dim))) * m * 2.0 ** e).astype(f32)
    rows[:, dim // 2:] = tail[:, dim // 2:]
    q = rng.uniform(-1, 1, (4, dim)).astype(f32)
    return rows, q, {"family": "e"}


def bf16_lo(x: np.ndarray) -> np.ndarray:
    """x - bf16(x) (round to nearest even), the split pass's second plane"""
    u = np.asarray(x, f32).view(np.uint32).astype(np.uint64)
    hi = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(f32)
    return (np.asarray(x, f32) - hi).astype(f32)
