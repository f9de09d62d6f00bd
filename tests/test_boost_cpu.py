"""CPU: score boosting (ott_query_boost, VecQueryPlan.boost, MetaQueryPlan.boost_by / boost_decay / boost_where)
without a GPU — the header's declarations, the struct's layout in C, ctypes and Rust, the ABI's device-free refusals, the planners'
refusals and lowering, a walk of the plan header (ott_boost_plan.h) by a stand-alone C++ program under AddressSanitizer + UBSan
whose formula must equal the numpy model (tests/boost_ref.py) bit for bit, the model against the oracle, and the preconditions that
make the GPU file's three sharp cases sharp."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import boost_cases as BC
import boost_ref as BR
import manhattan_ref as M
import test_rust_binding as RB
from otters_amd import BoostCombine, BoostTerm, Cmp, Column, DataType, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N
from otters_amd.meta import _lower_boosts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")


# ---- the header and the struct ------------------------------------------------------------------------------------------------------

def test_header_declares_the_call_and_the_defines_and_keeps_abi_4():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ott_query_boost\s*\(", code)
    assert re.search(r"ott_query_boost\s*\([^;]*const\s+void\s*\*\s*terms", code)  # const void* on purpose: the binding test's type map
    defs = dict(re.findall(r"#define\s+(OTT_[A-Z0-9_]+)\s+(\d+)", code))
    assert int(defs["OTT_BOOST_MAX_TERMS"]) == 8 == N.BOOST_MAX_TERMS
    assert int(defs["OTT_BOOST_MAX_QUERIES"]) == 1024 == N.BOOST_MAX_QUERIES
    assert int(defs["OTT_ABI_VERSION"]) == 4 == N.ABI_VERSION == N.lib().ott_abi_version()
    enums = dict(re.findall(r"(OTT_BOOST_[A-Z_]+)\s*=\s*(\d+)", code))
    assert {k: int(v) for k, v in enums.items()} == {"OTT_BOOST_SUM": 0, "OTT_BOOST_MULT": 1, "OTT_BOOST_VALUE": 0, "OTT_BOOST_LIN_DECAY": 1, "OTT_BOOST_MASK": 2}
    assert (N.BOOST_SUM, N.BOOST_MULT, N.BOOST_VALUE, N.BOOST_LIN_DECAY, N.BOOST_MASK) == (0, 1, 0, 1, 2)
    assert (int(BoostCombine.Sum), int(BoostCombine.Mult)) == (0, 1)
    assert "ott_boost.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert hasattr(N.lib(), "ott_query_boost")


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "otters_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ott_boost_term), offsetof(ott_boost_term, kind), offsetof(ott_boost_term, source),
           offsetof(ott_boost_term, weight), offsetof(ott_boost_term, scale), offsetof(ott_boost_term, origin), offsetof(ott_boost_term, missing),
           offsetof(ott_boost_term, reserved));
    return 0;
}
"""
FIELDS = ("kind", "source", "weight", "scale", "origin", "missing", "reserved")


def test_the_term_struct_has_one_layout_in_c_ctypes_and_rust(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call([cc, "-std=c11", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 0, 4, 8, 12, 16, 24, 28]
    assert C.sizeof(N.BoostTerm) == got[0] and [n for n, _ in N.BoostTerm._fields_] == list(FIELDS)
    assert [getattr(N.BoostTerm, f).offset for f in FIELDS] == got[1:]
    rust = RB.rust_structs(RB.rust_source())
    assert [n for n, _ in rust["ott_boost_term"]] == list(FIELDS)
    offs, size = RB.c_layout_of(rust["ott_boost_term"])
    assert size == got[0] and [offs[f] for f in FIELDS] == got[1:]
    assert re.search(r"size_of::<ott_boost_term>\(\)\s*==\s*32", RB.rust_source())


# ---- the ABI's refusals: all before any device work -----------------------------------------------------------------------------------

def desc(nq=1, mode=1, dim=4, path=0):
    q = np.zeros((max(nq, 1), dim), np.float32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, nq, int(Metric.DotProduct), 1, mode, 3, path
    return d, q


def term(kind=0, source=0, weight=1.0, scale=0.0, origin=0.0, missing=0.0, reserved=0):
    t = N.BoostTerm()
    t.kind, t.source, t.weight, t.scale, t.origin, t.missing, t.reserved = kind, source, weight, scale, origin, missing, reserved
    return t


def test_argument_refusals_need_no_device():
    L = N.lib()
    out = np.zeros(8, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)
    inf, nan = float("inf"), float("nan")

    def call(d, terms=(), combine=0, sw=1.0, n_terms=None, null_terms=False):
        arr = (N.BoostTerm * max(len(terms), 1))(*terms)
        n = len(terms) if n_terms is None else n_terms
        return L.ott_query_boost(None, C.byref(d[0]), combine, sw, None if null_terms or not n else arr, n, N.ptr(out), out.size, C.byref(n_out), None, None)

    def err():
        return L.ott_last_error()

    assert call(desc()) == -1 and b"ott_query_boost: store is NULL" in err()  # nothing wrong with the arguments: the store is next
    assert call(desc(nq=0)) == -1 and b"No queries provided" in err()
    assert call(desc(nq=1025)) == -1 and b"1025 queries are above OTT_BOOST_MAX_QUERIES (1024)" in err()
    assert call(desc(nq=2, mode=0)) == -1 and b"a batch needs OTT_MODE_PER_QUERY" in err()
    assert call(desc(nq=1, mode=0)) == -1 and b"store is NULL" in err()  # MERGED with one query is served
    assert call(desc(), [term()] * 9) == -1 and b"9 terms are above OTT_BOOST_MAX_TERMS (8)" in err()
    assert call(desc(), n_terms=2, null_terms=True) == -1 and b"terms is NULL" in err()
    assert call(desc(), combine=2) == -1 and b"unknown combine" in err()
    for bad in (inf, -inf, nan):
        assert call(desc(), sw=bad) == -1 and b"score_weight is not finite" in err()
        assert call(desc(), [term(), term(weight=bad)]) == -1 and b"term 1 (VALUE): weight is not finite" in err()
        assert call(desc(), [term(kind=1, scale=1.0, origin=bad)]) == -1 and b"term 0 (LIN_DECAY): origin is not finite" in err()
        assert call(desc(), [term(missing=bad)]) == -1 and b"term 0 (VALUE): missing is not finite" in err()
        assert call(desc(), [term(kind=1, scale=bad)]) == -1 and b"term 0 (LIN_DECAY): scale must be finite and above 0" in err()
    assert call(desc(), [term(kind=1, scale=0.0)]) == -1 and b"scale must be finite and above 0" in err()
    assert call(desc(), [term(kind=1, scale=-1.0)]) == -1 and b"scale must be finite and above 0" in err()
    assert call(desc(), [term(kind=3)]) == -1 and b"term 0: unknown kind 3" in err()
    assert call(desc(), [term(), term(reserved=1)]) == -1 and b"term 1 (VALUE): reserved must be 0" in err()
    assert call(desc(), [term(kind=2, source=64)]) == -1 and b"term 0 (MASK): slot 64 is not below OTT_MASK_SLOTS (64)" in err()
    assert call(desc(), [term(kind=2, source=63, origin=nan, missing=inf)]) == -1 and b"store is NULL" in err()  # a MASK term reads neither
    assert call(desc(path=2)) == -4 and b"the MFMA path does not serve boosted queries" in err()
    assert L.ott_query_boost(None, None, 0, 1.0, None, 0, None, 0, None, None, None) == -1 and b"desc is NULL" in err()
    assert n_out.value == 9 and not out["index"].any()  # nothing was touched


# ---- VecQueryPlan.boost ---------------------------------------------------------------------------------------------------------------

def plan_of(nq=1, dim=4, **kw):
    store = VecStore(dim, **kw)
    return store.query(np.ones((nq, dim), np.float32), Metric.DotProduct).take(5)


def test_vec_plan_refusals_and_lowering():
    terms = [BoostTerm.value(3, 0.1, origin=2.0, missing=-1.0), BoostTerm.lin_decay(4, 1.7e12, 86400e3, weight=0.5), BoostTerm.mask_slot(7, 0.25)]

    def refused(p, text):
        with pytest.raises(OttersError) as ei:
            p.validate()
        assert text in str(ei.value), str(ei.value)

    refused(plan_of().boost(terms).with_row_ids([1]), "boost cannot be combined with with_row_ids")
    refused(plan_of(2).per_query().boost(terms).with_row_masks([None, None]), "boost cannot be combined with with_row_masks")
    refused(plan_of().boost(terms).one_per_group(), "boost cannot be combined with one_per_group")
    refused(plan_of().boost(terms).per_group(2), "boost cannot be combined with per_group")
    refused(plan_of().boost(terms).max_sim(), "boost cannot be combined with max_sim")
    refused(plan_of().boost(terms).mmr(0.5), "boost cannot be combined with mmr")
    refused(plan_of().boost(terms).with_path(Path.Mfma), "boost cannot be combined with Path.Mfma")
    refused(plan_of(3).boost(terms), "a batch needs per_query()")
    refused(plan_of(devices=[0, 0]).boost(terms), "a multi-GPU store is not served")
    refused(plan_of().boost([BoostTerm.value(0, 1.0)] * 9), "9 terms are above the 8")
    refused(plan_of().boost([(0, 1)]), "a sequence of BoostTerm")
    refused(plan_of().boost(5), "a sequence of BoostTerm")
    refused(plan_of().boost(terms, combine=7), "combine must be BoostCombine.Sum or BoostCombine.Mult")
    refused(plan_of().boost(terms, score_weight=float("inf")), "score_weight is not finite")
    refused(plan_of().boost([BoostTerm.value(0, float("nan"))]), "term 0: weight, origin and missing must be finite")
    refused(plan_of().boost([BoostTerm.lin_decay(0, 0.0, 0.0)]), "term 0: scale must be finite and above 0")
    plan_of(3).per_query().boost(terms).with_row_mask(np.ones(3, bool)).filter(0.5, Cmp.Gt).with_path(Path.Exact).validate()  # all of these combine
    rq = plan_of().boost(terms, BoostCombine.Mult, 2.0).resolve()
    arr, n, combine, sw = rq.boost
    assert (n, combine, sw) == (3, 1, 2.0)
    assert [(t.kind, t.source, t.weight, t.scale, t.origin, t.missing, t.reserved) for t in arr] == [
        (0, 3, np.float32(0.1), 0.0, 2.0, -1.0, 0), (1, 4, 0.5, np.float32(86400e3), 1.7e12, 0.0, 0), (2, 7, 0.25, 0.0, 0.0, 0.0, 0)]
    assert plan_of().boost([]).resolve().boost[:2] == (None, 0)  # no terms: score_weight x S alone
    assert plan_of().resolve().boost is None  # a plan without boost is what it was


# ---- MetaQueryPlan.boost_by / boost_decay / boost_where ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def meta():
    n = 40
    cols = [Column("age", DataType.Int32).from_(list(range(n))), Column("lang", DataType.String).from_(["en", "de"] * (n // 2)),
            Column.from_numpy("ts", DataType.DateTime, 1_700_000_000_000 + np.arange(n, dtype=np.int64) * 1000)]
    return MetaStore.from_columns(cols).with_vectors(np.ones((n, 3), np.float32).tolist()).with_chunk_size(10).build(_host_only=True)


def test_meta_plan_refusals_and_lowering(meta):
    q = np.ones(3, np.float32)

    def refused(p, text, how="collect"):
        with pytest.raises(OttersError) as ei:
            getattr(p, how)()
        assert text in str(ei.value), str(ei.value)

    new = lambda: meta.query(q, Metric.DotProduct)  # noqa: E731
    refused(new().boost_by("lang", 0.1), "boost_by: column 'lang' is a String column")
    refused(new().boost_decay("lang", 0, 1.0), "boost_decay: column 'lang' is a String column")
    refused(new().boost_by("nope", 0.1), "boost_by: unknown column 'nope'")
    refused(new().boost_where(col("nope").lt(5), 0.5), "boost_where compile error: Unknown column 'nope'")
    refused(new().boost_where(5, 0.5), "boost_where takes an Expr")
    refused(new().boost_decay("ts", "yesterday", 1.0), "origin 'yesterday' is not a datetime string")
    refused(new().boost_by("age", 0.1, origin="2023-11-20"), "a datetime string is an origin for a DateTime column")
    refused(new().boost_by("age", 0.1).with_row_ids([1]), "boost cannot be combined with with_row_ids")
    refused(new().boost_by("age", 0.1).distinct_by("age"), "boost cannot be combined with distinct_by")
    refused(new().boost_by("age", 0.1).take(3).mmr(), "boost cannot be combined with mmr")
    refused(new().boost_by("age", 0.1).with_path(Path.Mfma), "boost cannot be combined with Path.Mfma")
    refused(new().boost_combine(3), "combine must be BoostCombine.Sum or BoostCombine.Mult")
    refused(new().boost_decay("age", 0, 0.0), "scale must be finite and above 0")
    refused(meta.query_batch(np.ones((2, 3), np.float32), Metric.DotProduct).boost_by("age", 0.1), "boost takes one query, not a batch")
    refused(meta.query_batch(np.ones((2, 3), np.float32), Metric.DotProduct).meta_filters([None, None]).boost_where(col("age").lt(5), 1.0),
            "meta_filters cannot be combined with boost_by, boost_decay or boost_where", how="collect_per_query")
    p = new()
    for _ in range(9):
        p = p.boost_by("age", 0.1)
    refused(p, "9 terms are above the 8")
    # lowering: names to column ids, an Expr to a slot, a datetime origin to epoch milliseconds; the order is the caller's
    ids, slots = {"age": 11, "ts": 12}, []
    young, english = col("age").lt(5), col("lang").eq("en").compile(meta.schema())
    plan = (new().boost_by("age", 0.1, origin=3, missing=-2.0).boost_where(young, 0.5).boost_decay("ts", "2023-11-14T22:13:20Z", 5000.0, weight=0.7)
            .boost_where(english, 0.25).boost_combine(BoostCombine.Mult, 0.5).meta_filter(col("age").gt(1)).vec_filter(0.5, Cmp.Gt).take(4))
    terms = _lower_boosts(plan, column_id=ids.__getitem__, fill_slot=lambda slot, compiled: slots.append((slot, compiled)))
    assert terms == [BoostTerm.value(11, 0.1, 3.0, -2.0), BoostTerm.mask_slot(0, 0.5), BoostTerm.lin_decay(12, 1_700_000_000_000.0, 5000.0, 0.7),
                     BoostTerm.mask_slot(1, 0.25)]
    assert [s for s, _ in slots] == [0, 1] and slots[1][1] is english and slots[0][1].clauses == young.compile(meta.schema()).clauses
    rq, chunk_mask, compiled = plan.resolve()  # meta_filter and vec_filter work as before
    assert rq.k == 4 and rq.filter_cmp == int(Cmp.Gt) and compiled is not None and rq.mode == 0


# ---- the plan header: a stand-alone program under ASan + UBSan; its formula against the numpy model --------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ott_boost_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static bool has(BoostRefusal r, uint32_t nq, uint32_t n_terms, uint32_t bad, const BoostTerm* t, const char* text, int status) {
    const std::string s = boost_refusal_text(r, nq, n_terms, bad, t);
    if (s.find(text) == std::string::npos || s.empty()) { fprintf(stderr, "text of %d is '%s'\n", (int)r, s.c_str()); return false; }
    return boost_refusal_status(r) == status;
}
static BoostTerm T(uint32_t kind, uint32_t source, float weight = 1.f, float scale = 0.f, double origin = 0, float missing = 0.f, uint32_t reserved = 0) {
    BoostTerm t;
    t.kind = kind; t.source = source; t.weight = weight; t.scale = scale; t.origin = origin; t.missing = missing; t.reserved = reserved;
    return t;
}
// the formula over a case file: [u32 n, n_terms, combine, f32 score_weight] then per term [BoostTerm (32 B), u32 dtype, u32 has_nulls,
// u64 mask_bits, values (n elements) or mask words, n NULL bytes if has_nulls] then S (n f32); writes F (n f32)
static int formula(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    uint32_t n, n_terms, combine;
    float sw;
    CHECK(fread(&n, 4, 1, f) == 1 && fread(&n_terms, 4, 1, f) == 1 && fread(&combine, 4, 1, f) == 1 && fread(&sw, 4, 1, f) == 1);
    std::vector<BoostTerm> terms(n_terms);
    std::vector<uint32_t> dtype(n_terms), has_nulls(n_terms);
    std::vector<uint64_t> mask_bits(n_terms);
    std::vector<std::vector<char>> vals(n_terms), nulls(n_terms);
    for (uint32_t j = 0; j < n_terms; j++) {
        CHECK(fread(&terms[j], 32, 1, f) == 1 && fread(&dtype[j], 4, 1, f) == 1 && fread(&has_nulls[j], 4, 1, f) == 1 && fread(&mask_bits[j], 8, 1, f) == 1);
        const size_t bytes = terms[j].kind == BOOST_MASK ? (size_t)((mask_bits[j] + 63) / 64) * 8 : (size_t)n * boost_elem_size(dtype[j]);
        vals[j].resize(bytes + 8);  // (+ 8: an empty mask still has a buffer)
        if (bytes) CHECK(fread(vals[j].data(), 1, bytes, f) == bytes);
        if (has_nulls[j]) {
            nulls[j].resize(n);
            CHECK(fread(nulls[j].data(), 1, n, f) == n);
        }
    }
    std::vector<float> S(n), F(n), g(n_terms ? n_terms : 1);
    CHECK(fread(S.data(), 4, n, f) == n);
    fclose(f);
    for (uint32_t r = 0; r < n; r++) {
        for (uint32_t j = 0; j < n_terms; j++)
            g[j] = terms[j].kind == BOOST_MASK ? boost_g_mask((const uint64_t*)vals[j].data(), mask_bits[j], r)
                                                : boost_g_value(terms[j], has_nulls[j] && nulls[j][r], boost_column_f64(dtype[j], vals[j].data(), r));
        F[r] = boost_final(combine, sw, S[r], n_terms, n_terms ? boost_sum(terms.data(), g.data(), n_terms) : 0.0f);
    }
    f = fopen(out, "wb");
    if (!f) return 2;
    CHECK(fwrite(F.data(), 4, n, f) == n);
    fclose(f);
    return 0;
}
int main(int argc, char** argv) {
    if (argc == 3) return formula(argv[1], argv[2]);
    CHECK(BOOST_MAX_TERMS == 8 && BOOST_MAX_QUERIES == 1024 && BOOST_NQ == 4 && BOOST_SLOTS == 64 && BOOST_MAX_ROWS == 0xFFFFFFF0ull);
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    uint32_t bad = 99;
    // ---- the refusals the arguments decide, in the order the call makes them: every later fault is present too
    const BoostTerm junk[3] = {T(7, 0, nan, 0, 0, 0, 1), T(BOOST_MASK, 64), T(BOOST_VALUE, 0)};
    CHECK(boost_check_args(0, 0, 2, 9, nan, nullptr, 9, &bad) == BOOST_NO_QUERIES);
    CHECK(boost_check_args(1025, 0, 2, 9, nan, nullptr, 9, &bad) == BOOST_TOO_MANY_QUERIES);
    CHECK(boost_check_args(2, 0, 2, 9, nan, nullptr, 9, &bad) == BOOST_MERGED);
    CHECK(boost_check_args(2, 1, 2, 9, nan, nullptr, 9, &bad) == BOOST_TOO_MANY_TERMS);
    CHECK(boost_check_args(1, 0, 2, 9, nan, nullptr, 3, &bad) == BOOST_NULL_TERMS);  // MERGED with one query is served
    CHECK(boost_check_args(1, 0, 2, 9, nan, junk, 3, &bad) == BOOST_BAD_COMBINE);
    CHECK(boost_check_args(1, 0, 2, 1, nan, junk, 3, &bad) == BOOST_BAD_SCORE_WEIGHT && boost_check_args(1, 0, 2, 1, -inf, junk, 3, &bad) == BOOST_BAD_SCORE_WEIGHT);
    CHECK(boost_check_args(1, 0, 2, 1, 1.f, junk, 3, &bad) == BOOST_BAD_KIND && bad == 0);
    CHECK(boost_check_args(1, 0, 2, 1, 1.f, junk + 1, 2, &bad) == BOOST_BAD_SLOT && bad == 0);
    CHECK(boost_check_args(1, 0, 2, 1, 1.f, junk + 2, 1, &bad) == BOOST_MFMA && boost_check_args(1, 0, 1, 1, 1.f, junk + 2, 1, &bad) == BOOST_OK);
    CHECK(boost_check_args(1024, 1, 0, 0, -3.f, nullptr, 0, &bad) == BOOST_OK);
    {
        BoostTerm t[2] = {T(BOOST_VALUE, 5), T(BOOST_LIN_DECAY, 5, nan, -1.f, inf, nan, 1)};
        CHECK(boost_check_args(1, 1, 0, 0, 1.f, t, 2, &bad) == BOOST_RESERVED && bad == 1);
        t[1].reserved = 0;
        CHECK(boost_check_args(1, 1, 0, 0, 1.f, t, 2, &bad) == BOOST_BAD_WEIGHT && bad == 1);
        t[1].weight = 1.f;
        CHECK(boost_check_args(1, 1, 0, 0, 1.f, t, 2, &bad) == BOOST_BAD_ORIGIN);
        t[1].origin = 0;
        CHECK(boost_check_args(1, 1, 0, 0, 1.f, t, 2, &bad) == BOOST_BAD_MISSING);
        t[1].missing = 0;
        CHECK(boost_check_args(1, 1, 0, 0, 1.f, t, 2, &bad) == BOOST_BAD_SCALE);
        for (float s : {0.f, -0.f, inf, nan}) {
            t[1].scale = s;
            CHECK(boost_check_args(1, 1, 0, 0, 1.f, t, 2, &bad) == BOOST_BAD_SCALE);
        }
        t[1].scale = 1e-45f;  // the smallest denormal is above 0
        CHECK(boost_check_args(1, 1, 0, 0, 1.f, t, 2, &bad) == BOOST_OK);
        const BoostTerm m = T(BOOST_MASK, 63, 1.f, nan, nan, nan);  // a MASK term reads neither scale, origin nor missing
        CHECK(boost_check_args(1, 1, 0, 0, 1.f, &m, 1, &bad) == BOOST_OK);
    }
    // ---- ... and the ones the store decides
    CHECK(boost_check_store(true, 1, BOOST_MAX_ROWS) == BOOST_MULTI_GPU && boost_check_store(false, 1, BOOST_MAX_ROWS) == BOOST_TIE_ORDER);
    CHECK(boost_check_store(false, 2, 5) == BOOST_TIE_ORDER && boost_check_store(false, 0, BOOST_MAX_ROWS) == BOOST_TOO_MANY_ROWS);
    CHECK(boost_check_store(false, 0, BOOST_MAX_ROWS - 1) == BOOST_OK && boost_check_store(false, 0, 0) == BOOST_OK);
    {
        const uint64_t column_rows[3] = {100, 90, 100};
        uint64_t slot_bits[BOOST_SLOTS] = {};
        slot_bits[2] = 40;
        const BoostTerm t[4] = {T(BOOST_VALUE, 0), T(BOOST_MASK, 2), T(BOOST_LIN_DECAY, 2, 1.f, 1.f), T(BOOST_VALUE, 3)};
        CHECK(boost_check_sources(t, 4, column_rows, 3, 100, slot_bits, &bad) == BOOST_UNKNOWN_COLUMN && bad == 3);
        CHECK(boost_check_sources(t, 3, column_rows, 3, 100, slot_bits, &bad) == BOOST_OK);
        CHECK(boost_check_sources(t, 3, column_rows, 3, 101, slot_bits, &bad) == BOOST_COLUMN_LENGTH && bad == 0);
        const BoostTerm u[2] = {T(BOOST_VALUE, 1), T(BOOST_MASK, 3)};
        CHECK(boost_check_sources(u, 2, column_rows, 3, 100, slot_bits, &bad) == BOOST_COLUMN_LENGTH && bad == 0);
        CHECK(boost_check_sources(u + 1, 1, column_rows, 3, 100, slot_bits, &bad) == BOOST_EMPTY_SLOT && bad == 0);
        CHECK(boost_check_sources(nullptr, 0, nullptr, 0, 100, slot_bits, &bad) == BOOST_OK);
    }
    CHECK(boost_check_cap(29, 3, 10, 1000) == BOOST_CAP && boost_check_cap(30, 3, 10, 1000) == BOOST_OK && boost_check_cap(0, 3, 0, 1000) == BOOST_OK);
    CHECK(boost_check_cap(1u << 30, 1024, 513, 1u << 16) == BOOST_OK && boost_check_cap(1u << 30, 1024, 513, (1u << 16) + 1) == BOOST_TOO_MANY_PAIRS);
    CHECK(boost_check_cap(1u << 30, 1024, 512, 1u << 20) == BOOST_OK);
    // ---- every refusal has its own text and its status
    {
        const BoostTerm t = T(BOOST_MASK, 64), v = T(BOOST_LIN_DECAY, 9), k = T(7, 0);
        CHECK(has(BOOST_NO_QUERIES, 0, 0, 0, nullptr, "No queries provided", -1));
        CHECK(has(BOOST_TOO_MANY_QUERIES, 1025, 0, 0, nullptr, "1025 queries are above OTT_BOOST_MAX_QUERIES (1024)", -1));
        CHECK(has(BOOST_MERGED, 2, 0, 0, nullptr, "a batch needs OTT_MODE_PER_QUERY", -1));
        CHECK(has(BOOST_TOO_MANY_TERMS, 1, 9, 0, nullptr, "9 terms are above OTT_BOOST_MAX_TERMS (8)", -1));
        CHECK(has(BOOST_NULL_TERMS, 1, 2, 0, nullptr, "terms is NULL", -1));
        CHECK(has(BOOST_BAD_COMBINE, 1, 0, 0, nullptr, "unknown combine", -1));
        CHECK(has(BOOST_BAD_SCORE_WEIGHT, 1, 0, 0, nullptr, "score_weight is not finite", -1));
        CHECK(has(BOOST_BAD_KIND, 1, 3, 2, &k, "term 2: unknown kind 7", -1));
        CHECK(has(BOOST_RESERVED, 1, 3, 1, &v, "term 1 (LIN_DECAY): reserved must be 0", -1));
        CHECK(has(BOOST_BAD_WEIGHT, 1, 3, 1, &v, "term 1 (LIN_DECAY): weight is not finite", -1));
        CHECK(has(BOOST_BAD_ORIGIN, 1, 3, 1, &v, "origin is not finite", -1));
        CHECK(has(BOOST_BAD_MISSING, 1, 3, 1, &v, "missing is not finite", -1));
        CHECK(has(BOOST_BAD_SCALE, 1, 3, 1, &v, "scale must be finite and above 0", -1));
        CHECK(has(BOOST_BAD_SLOT, 1, 1, 0, &t, "term 0 (MASK): slot 64 is not below OTT_MASK_SLOTS (64)", -1));
        CHECK(has(BOOST_MFMA, 1, 0, 0, nullptr, "the MFMA path does not serve boosted queries", -4));
        CHECK(has(BOOST_MULTI_GPU, 1, 0, 0, nullptr, "a multi-GPU store is not served", -4));
        CHECK(has(BOOST_TIE_ORDER, 1, 0, 0, nullptr, "tie_order 1 and 2 are not served", -4));
        CHECK(has(BOOST_TOO_MANY_ROWS, 1, 0, 0, nullptr, "2^32 - 16 rows or more", -4));
        CHECK(has(BOOST_UNKNOWN_COLUMN, 1, 1, 0, &v, "term 0 (LIN_DECAY): unknown column id 9", -1));
        CHECK(has(BOOST_COLUMN_LENGTH, 1, 1, 0, &v, "the length of column 9 no longer matches the store", -1));
        CHECK(has(BOOST_EMPTY_SLOT, 1, 1, 0, &t, "slot 64 was never filled, or was dropped", -1));
        CHECK(has(BOOST_CAP, 1, 0, 0, nullptr, "output capacity is smaller than nq * min(k, rows)", -1));
        CHECK(has(BOOST_TOO_MANY_PAIRS, 1, 0, 0, nullptr, "k above 512 is served only up to 2^26 (query, row) pairs", -4));
        CHECK(boost_refusal_status(BOOST_OK) == 0 && boost_refusal_text(BOOST_OK, 1, 0, 0, nullptr).empty());
    }
    // ---- passes and bytes
    CHECK(boost_passes(1) == 1 && boost_passes(4) == 1 && boost_passes(5) == 2 && boost_passes(9) == 3 && boost_passes(1024) == 256);
    CHECK(boost_elem_size(BOOST_DT_INT32) == 4 && boost_elem_size(BOOST_DT_FLOAT32) == 4 && boost_elem_size(BOOST_DT_INT64) == 8 &&
          boost_elem_size(BOOST_DT_FLOAT64) == 8 && boost_elem_size(BOOST_DT_DATETIME) == 8);
    {
        const uint32_t dt[3] = {BOOST_DT_FLOAT32, BOOST_DT_DATETIME, BOOST_DT_INT32};
        const BoostTerm t[4] = {T(BOOST_VALUE, 0), T(BOOST_MASK, 1), T(BOOST_LIN_DECAY, 1, 1.f, 1.f), T(BOOST_VALUE, 2)};
        CHECK(boost_bytes_scanned(3, 1000, 128, false, t, 4, dt) == 3ull * 1000 * (512 + 4 + 8 + 4));
        CHECK(boost_bytes_scanned(2, 10, 8, true, nullptr, 0, nullptr) == 2ull * 10 * 36);
    }
    // ---- the formula's corners
    {
        const BoostTerm v = T(BOOST_VALUE, 0, 1.f, 0.f, 1.0, -7.f), d = T(BOOST_LIN_DECAY, 0, 1.f, 2.f, 10.0, 0.5f);
        CHECK(boost_g_value(v, true, 99.0) == -7.f && boost_g_value(v, false, 3.5) == 2.5f && boost_g_value(d, true, 10.0) == 0.5f);
        CHECK(boost_g_value(d, false, 10.0) == 1.f && boost_g_value(d, false, 11.0) == 0.5f && boost_g_value(d, false, 8.0) == 0.f && boost_g_value(d, false, 1e30) == 0.f);
        CHECK(!__builtin_signbit(boost_g_value(d, false, 12.0)));  // u == 1: +0
        const float gn = boost_g_value(d, false, (double)nan);
        CHECK(gn != gn);
        const uint64_t w[2] = {0x5ull, 0x1ull};
        CHECK(boost_g_mask(w, 70, 0) == 1.f && boost_g_mask(w, 70, 1) == 0.f && boost_g_mask(w, 70, 64) == 1.f && boost_g_mask(w, 70, 65) == 0.f && boost_g_mask(w, 70, 70) == 1.f);
        CHECK(boost_g_mask(nullptr, 0, 5) == 1.f);
        CHECK(boost_final(BOOST_SUM, 1.f, -0.f, 0, 0.f) == 0.f && __builtin_signbit(boost_final(BOOST_SUM, 1.f, -0.f, 0, 0.f)));  // no terms: F = Sw, the sign of a zero kept
        const int64_t odd = 9007199254740993ll;  // 2^53 + 1: ties to even
        CHECK(boost_column_f64(BOOST_DT_INT64, &odd, 0) == 9007199254740992.0);
    }
    puts("ok");
    return 0;
}
"""


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("boost_walk")
    src, exe = d / "walk.cpp", d / "walk"
    src.write_text(WALK)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    return exe


def test_plan_header_walk_under_asan_ubsan(walk):
    out = subprocess.run([str(walk)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


DT = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}


def plan_formula(walk, tmp_path, S, terms, combine, sw, name):
    """F of the plan header's host formula for one query's scores"""
    n = S.size
    blob = [struct.pack("<IIIf", n, len(terms), combine, sw)]
    for t in terms:
        if t[0] == "mask":
            m = np.asarray(t[1], bool).ravel()
            blob.append(struct.pack("<IIffdfIIIQ", 2, 0, t[2], 0.0, 0.0, 0.0, 0, 0, 0, m.size))
            blob.append(N.pack_bits(m)[: (m.size + 63) // 64].tobytes())
            continue
        values, nulls, weight, origin = t[1], t[2], t[3], t[4]
        scale, missing = (0.0, t[5]) if t[0] == "value" else (t[5], t[6])
        blob.append(struct.pack("<IIffdfIIIQ", 0 if t[0] == "value" else 1, 0, weight, scale, origin, missing, 0, DT[values.dtype], nulls is not None, 0))
        blob.append(np.ascontiguousarray(values).tobytes())
        if nulls is not None:
            blob.append(np.asarray(nulls, bool).astype(np.uint8).tobytes())
    blob.append(np.ascontiguousarray(S, np.float32).tobytes())
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    fin.write_bytes(b"".join(blob))
    out = subprocess.run([str(walk), str(fin), str(fout)], capture_output=True, text=True)
    assert out.returncode == 0, (name, out.stderr)
    return np.frombuffer(fout.read_bytes(), np.float32)


def edge_terms(n, rng):
    """every dtype, NULLs, NaN and inf values, a denormal product, an overflow, inf - inf, decay at u below / equal to / above 1,
    masks shorter than the rows and of no bits"""
    f32 = rng.uniform(-3, 3, n).astype(np.float32)
    f32[:6] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40]
    f64 = rng.uniform(-1e6, 1e6, n)
    f64[:5] = [1e300, -1e300, np.nan, 5e-324, 2.0 ** 60]
    i32 = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    i64 = rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64)
    i64[: BC.I64_EDGE.size] = BC.I64_EDGE
    dist = rng.integers(-30, 30, n).astype(np.int32)
    dist[:4] = [10, -10, 0, 11]  # with scale 10: u = 1 on both sides, 0, just above 1
    nulls = rng.random(n) < 0.2
    return [("value", f32, nulls, 0.5, 0.25, -1.5), ("value", f64, None, 1e-3, 17.0, 0.0), ("value", i32, nulls, 2.0 ** -20, -5.0, 3.0),
            ("value", i64, None, 2.0 ** -50, 2.0 ** 53, 0.0), ("decay", dist, None, 0.75, 0.0, 10.0, 0.0), ("decay", f64, nulls, -0.5, 100.0, 2e5, 0.25),
            ("mask", rng.random(n - 37) < 0.5, 0.125), ("mask", np.zeros(0, bool), 4.0),
            ("value", f32, None, 1e-40, 0.0, 0.0),   # denormal c_j
            ("value", f32, None, 3e38, 0.0, 0.0),    # overflow to inf
            ("value", f64, None, -3e38, 0.0, 0.0)]   # ... and inf - inf behind it


def test_plan_formula_equals_the_numpy_model_bit_for_bit(walk, tmp_path):
    rng = np.random.default_rng(5)
    n = 1500
    S = rng.uniform(-4, 4, n).astype(np.float32)
    S[:8] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, 3e38, -3e38]
    pool = edge_terms(n, rng)
    picks = [[], [0], [6], [4, 1], [0, 1, 2, 3, 4, 5, 6, 7], [8, 6], [9, 1], [9, 10, 0], [3, 2], [5, 7, 4]]
    picks += [sorted(rng.choice(len(pool), int(rng.integers(1, 9)), replace=False).tolist()) for _ in range(12)]
    n_cases = 0
    for i, pick in enumerate(picks):
        terms = [pool[j] for j in pick]
        for combine in (BR.SUM, BR.MULT):
            for sw in (1.0, -0.375, 0.0):
                got = plan_formula(walk, tmp_path, S, terms, combine, sw, f"c{i}_{combine}_{n_cases}")
                exp = BR.final(S[None], terms, combine, sw)[0]
                # (a NaN F drops the row: which NaN it is, sign and payload, is not part of the contract)
                differ = np.where(np.isnan(exp), ~np.isnan(got), got.view(np.uint32) != exp.view(np.uint32))
                assert not differ.any(), (pick, combine, sw, np.flatnonzero(differ)[:8])
                n_cases += 1
    # the edge inputs did what they are there for
    F = BR.final(S[None], [pool[9], pool[10]], BR.SUM, 1.0)[0]
    assert np.isnan(F).sum() > 10 and np.isinf(BR.boost_sum([pool[9]], n)).any()
    c = np.float32(1e-40) * pool[8][1]
    assert ((c != 0) & (np.abs(c) < np.finfo(np.float32).tiny)).any()


# ---- the model against the oracle ----------------------------------------------------------------------------------------------------------

def test_the_model_without_terms_is_the_oracle(oracle):
    rng, rows, q = BC.int_corpus(700, 19, 11, nq=3)
    rows[[4, 90], 2] = np.nan
    keep = rng.random(700) < 0.8
    for metric in (0, 1, 2, 3):
        S = BR.scores(oracle, rows, q, metric)
        for take, k, cmp, thr in ((1, 10, 0, 0.0), (0, 700, 0, 0.0), (1, 50, 2, float(np.nanmedian(S))), (0, 50, 3, float(np.nanmedian(S))), (1, 9, 5, float(S[0, 7]))):
            got = BR.expected(S, [], take, k, cmp=cmp, thr=thr, keep=keep)
            for b in range(3):
                if metric == 3:
                    exp = M.query(rows, q[b], take, k, cmp, thr, row_mask=keep)
                else:
                    exp = oracle.vec_query(rows, q[b][None], metric, take, k, cmp, thr, row_mask=keep, ties=oracle.TIES_CANONICAL)
                assert np.array_equal(got[b]["index"].astype(np.int64), exp["index"].astype(np.int64)), (metric, take, k, cmp, b)
                assert np.array_equal(got[b]["score"].view(np.uint32), exp["score"].view(np.uint32)), (metric, take, k, cmp, b)


# ---- the preconditions that make the GPU cases sharp ------------------------------------------------------------------------------------------

def test_chain_order_case_a_different_summation_order_gives_a_different_top_k(oracle):
    _, rows, q = BC.int_corpus(600, 16, 71)
    S = BR.scores(oracle, rows, q, 2)
    terms, wrong = BC.chain_order(600)
    B, B_wrong = BR.boost_sum(terms, 600), BR.boost_sum(terms, 600, wrong)
    assert set(np.unique(B).tolist()) <= {0.0, 8.0} and np.array_equal(B_wrong, terms[1][1])  # (1e8 + x) - 1e8 against x
    assert BC.topk_rows(BR.final(S, terms), 10) != BC.topk_rows(BR.final(S, terms, order=wrong), 10)


def test_datetime_case_an_f32_subtraction_gives_a_different_top_k(oracle):
    _, rows, q = BC.int_corpus(600, 16, 72)
    S = BR.scores(oracle, rows, q, 2)
    terms, g32 = BC.datetime_decay(600)
    g = BR.term_g(terms[0], 600)
    assert (g != g32).mean() > 0.5 and (g > 0).sum() > 100
    with np.errstate(all="ignore"):
        F32 = S + (np.float32(terms[0][3]) * g32)[None, :]
    assert BC.topk_rows(BR.final(S, terms), 10) != BC.topk_rows(F32, 10)


def test_int64_case_the_edge_values_round_as_the_model_says():
    terms = BC.int64_edges(600)
    v = terms[0][1]
    assert np.array_equal(v[: BC.I64_EDGE.size].astype(np.float64), BC.I64_EDGE_F64)  # numpy's conversion is the IEEE one
    g = BR.term_g(terms[0], 600)
    exp = (BC.I64_EDGE_F64 - 2.0 ** 53).astype(np.float32)
    assert np.array_equal(g[: exp.size].view(np.uint32), exp.view(np.uint32))
    assert g[0] == 0.0 and g[2] == 4.0 and g[3] == np.float32(2.0 ** 63 - 2.0 ** 53) and g[4] == np.float32(-(2.0 ** 63) - 2.0 ** 53)
    exact = (v[8:].astype(object) - 2 ** 53).astype(np.float64)  # integer arithmetic: what an i64 subtraction would give
    assert (g[8:] != exact).any() and np.all(g[8:][g[8:] > 0] % 2 == 0)  # above 2^53 f64 holds only even integers
