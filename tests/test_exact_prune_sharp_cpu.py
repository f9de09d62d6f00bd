"""CPU: the conditions that tests/prune_sharp.py promises, proved with the header's own bound (otters_amd/csrc/ott_prune.h) through the
drivers the *_bound.py files compile — the same sources with one loop over rows added — and the oracle's bit-exact scores.
  1. the quarter rule: per form and dim, the largest slack (bound - score) / (|q| |v|) of the tight rows, over every variant, both
     metrics and the side of the take the row is built for, is at most a quarter of the median slack of uniform(-1, 1) rows.  The
     score is taken in float64.  Both figures are printed, and every form keeps the rule at every dim (the three variants outside
     it, prune_sharp.LOOSE_VARIANTS and QUANT_VARIANTS, are printed beside them);
  2. the cap: in every corpus the GPU file uses, each challenger's score ordinal lies strictly beyond the gate's by at most 1024 f32
     steps on the winning side of the take, Max and Min; the seed's k-th best is the gate for every k; no filler row reaches it; and
     the oracle's hits are the challengers in score order, then the lowest-index copies of A.  Every corpus's margins are printed.
The GPU half is tests/test_gpu_exact_prune_sharp.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import prune_sharp as S
import test_exact_prune_bound as plain_file
import test_exact_prune_head_bound as head_file
import test_exact_prune_sketch3_bound as sketch3_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "otters_amd", "csrc")
P = C.POINTER(C.c_float)

# one loop over rows behind each file's driver: out[r] = the form's bound of row r at its own checkpoint
LOOPS = {
    "head": r"""
extern "C" void sharp_rows(int form, const float* q, const float* rows, unsigned long long n, unsigned dim, unsigned, float qinv, const float* vinv, int cosine,
                           int upper, float* out) {
    for (unsigned long long r = 0; r < n; r++)
        out[r] = form == 0 ? hd_bound(q, rows + r * dim, dim, qinv, vinv[r], cosine, upper) : c1_bound(q, rows + r * dim, dim, qinv, vinv[r], cosine, upper);
}
""",
    "sketch": r"""
extern "C" void sharp_rows(int form, const float* q, const float* rows, unsigned long long n, unsigned dim, unsigned first, float qinv, const float* vinv,
                           int cosine, int upper, float* out) {
    for (unsigned long long r = 0; r < n; r++)
        out[r] = form == 3 ? skb_bound(q, rows + r * dim, dim, first, first, 3, qinv, vinv[r], cosine, upper)
                           : sk_bound(q, rows + r * dim, dim, first, first, qinv, vinv[r], cosine, upper);
}
""",
    "plain": r"""
extern "C" void sharp_rows(int, const float* q, const float* rows, unsigned long long n, unsigned dim, unsigned first, float qinv, const float* vinv, int cosine,
                           int upper, float* out) {
    for (unsigned long long r = 0; r < n; r++) out[r] = prune_bound(q, rows + r * dim, dim, first, qinv, vinv[r], cosine, upper);
}
""",
}
SOURCES = {"head": head_file.DRIVER, "sketch": sketch3_file.DRIVER, "plain": plain_file.DRIVER}
DRIVER_OF = {"head": ("head", 0), "c1": ("head", 1), "sk3": ("sketch", 3), "sk1": ("sketch", 1), "7/8": ("plain", 0)}


def load_drivers(tmp):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    libs = {}
    for name, src_text in SOURCES.items():
        src, so = tmp / f"{name}.cpp", tmp / f"{name}.so"
        src.write_text(src_text + LOOPS[name])
        subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HDR, str(src), "-o", str(so)])
        L = C.CDLL(str(so))
        L.sharp_rows.argtypes = [C.c_int, P, P, C.c_ulonglong, C.c_uint, C.c_uint, C.c_float, P, C.c_int, C.c_int, P]
        L.sharp_rows.restype = None
        libs[name] = L
    return libs


def form_bounds(libs, oracle, form, q, rows, cosine, upper):
    """the header's bound of every row in the given form, at the form's own checkpoint (the kernel's state: restated by the drivers)"""
    q = np.ascontiguousarray(q, np.float32)
    rows = np.ascontiguousarray(rows, np.float32)
    inv_v = np.ascontiguousarray(oracle.inv_norms(rows), np.float32)
    inv_q = np.float32(oracle.inv_norms(q[None, :])[0])
    out = np.empty(rows.shape[0], np.float32)
    name, code = DRIVER_OF[form]
    libs[name].sharp_rows(code, q.ctypes.data_as(P), rows.ctypes.data_as(P), rows.shape[0], q.size, S.checkpoint(form, q.size), inv_q, inv_v.ctypes.data_as(P),
                          int(cosine), int(upper), out.ctypes.data_as(P))
    return out


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return load_drivers(tmp_path_factory.mktemp("sharp"))


def slack(libs, oracle, form, q, rows, upper):
    """(bound - score) / (|q| |v|) per row on the given side, the larger of the two metrics; the score in float64"""
    q64, r64 = q.astype(np.float64), rows.astype(np.float64)
    dot = r64 @ q64
    scale = np.linalg.norm(q64) * np.linalg.norm(r64, axis=1)
    side = 1.0 if upper else -1.0
    out = []
    for cosine in (True, False):
        b = form_bounds(libs, oracle, form, q, rows, cosine, upper).astype(np.float64)
        assert not np.isnan(b).any(), (form, cosine)
        s = side * (b - (dot / scale if cosine else dot)) / (1.0 if cosine else scale)
        assert (s > -1e-6).all(), (form, cosine, s.min())  # (the float64 score against an f32 bound of the f32 score)
        out.append(s)
    return np.maximum(out[0], out[1])


@pytest.mark.parametrize("dim", [96, 256, 768, 773, 896])
@pytest.mark.parametrize("form", list(S.FORMS))
def test_tight_rows_keep_the_quarter_rule(libs, oracle, form, dim):
    """the figures of every form and dim: profiles/prune_sharp/README.md (head, dim 96 / 256 / 768: 0.0105 / 0.0116 / 0.0109 against 0.064)"""
    rng = np.random.default_rng(dim)
    q = S.query(dim)
    uniform = rng.uniform(-1, 1, (200, dim)).astype(np.float32)
    med = float(np.median(slack(libs, oracle, form, q, uniform, True)))
    worst = {}
    for variant in S.VARIANTS:
        rows = S.tight_rows(form, dim, q, 6, rng, variant)
        worst[variant] = float(slack(libs, oracle, form, q, rows, variant != "against").max())
    tight = max(worst.values())
    for variant in S.LOOSE_VARIANTS + S.QUANT_VARIANTS:  # printed, not held to the rule: see prune_sharp.LOOSE_VARIANTS, QUANT_VARIANTS
        qv = S.query(dim, 0, variant)
        worst[variant] = float(slack(libs, oracle, form, qv, S.tight_rows(form, dim, qv, 6, rng, variant), True).max())
    print(f"slack {form:>4} dim {dim:>3}: tight max {tight:.6f} uniform median {med:.4f} ratio 1/{med / tight:.1f}  "
          + " ".join(f"{v}={worst[v]:.6f}" for v in worst))
    assert tight <= med / 4, (form, dim, worst, med)


def expected_hits(c, rows, oracle, metric, take, k):
    """what the layout says the hits are: the challengers best first (equal scores by index), then the lowest-index copies of A"""
    sc = S.scores(oracle, rows[c["slots"]], c["q"], metric)
    key = S.tkey(sc) if take else 0xFFFFFFFF - S.tkey(sc)
    order = np.lexsort((c["slots"], -key))
    idx = np.concatenate([c["slots"][order], c["copies"]])[:k]
    return idx


CORPORA = [(fam, shape) for shape in S.SHAPES for fam in ("head", "sk3", "sk1", "7/8") if fam in S.forms_of(shape)]


@pytest.mark.parametrize("fam,shape", CORPORA, ids=[f"{s[1]}x{s[0]}-{s[2]}-{f}" for f, s in CORPORA])
def test_challengers_sit_within_1024_steps_of_the_gate(oracle, fam, shape):
    dim, n, variant, staircase = shape
    for metric in S.METRICS:
        c = S.sharp_corpus(fam, dim, n, metric, variant, staircase)
        seed = S.seed_rows(n)
        assert (c["copies"] < seed).all() and (c["slots"] >= seed).all()
        assert (c["steps"] >= 1).all() and (c["steps"] <= S.MAX_STEPS).all() and (np.diff(c["steps"]) >= 0).all()
        if not staircase:  # a wave's queue holds 64 survivors: 72 consecutive challengers
            run = np.flatnonzero(np.diff(c["slots"]) != 1)
            assert np.diff(np.concatenate([[-1], run, [c["slots"].size - 1]])).max() >= 70
        for take in (1, 0):
            rows = c["rows"] if take else -c["rows"]
            sc = S.scores(oracle, rows, c["q"], metric)
            key = S.tkey(sc) if take else 0xFFFFFFFF - S.tkey(sc)  # larger = better
            gate = int(key[c["copies"][0]])
            assert (key[c["copies"]] == gate).all()
            margin = key[c["slots"]] - gate
            assert np.array_equal(margin, c["steps"]), (fam, shape, metric, take)
            assert margin.min() >= 1 and margin.max() <= S.MAX_STEPS
            other = np.ones(n, bool)
            other[c["copies"]] = False
            other[c["slots"]] = False
            assert key[other].max() < gate
            assert np.sort(key[:seed])[::-1][S.COPIES - 1] == gate and np.sort(key[:seed])[::-1][0] == gate  # the seed's k-th best, every k
            for k in S.KS:
                ref = oracle.vec_query(rows, c["q"], metric, take, k, 0, 0.0, ties=oracle.TIES_CANONICAL)
                assert np.array_equal(ref["index"].astype(np.int64), expected_hits(c, rows, oracle, metric, take, k)), (fam, shape, metric, take, k)
        print(f"margin {fam:>4} {n}x{dim} {variant} {'cosine' if metric == 0 else 'dot'}, Max and Min: {c['slots'].size} challengers from a pool of {c['pool']}, "
              f"{int(margin.min())} .. {int(margin.max())} f32 steps beyond the gate; best filler {gate - int(key[other].max())} steps below it")
