"""CPU: sparse rows and ott_query_sparse without a GPU — the header's declarations against ctypes and Rust, the
ABI's device-free refusals, a walk of the plan header (ott_sparse_plan.h) by a stand-alone C++ program under AddressSanitizer +
UBSan (every refusal with its text, the sliced-ELL layout arithmetic with 64-bit offsets, the form of the weight lookup and its
passes), the header's C statement of the score held to the numpy model (tests/sparse_ref.py) bit for bit — the definition and the
"multiply everything by a dense table" evaluation the kernel uses — and the host objects' lowering."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sparse_cases as SC
import sparse_ref as SR
import test_rust_binding as RB
from otters_amd import Cmp, Column, DataType, MetaStore, OttersError, Path, SparseQueryPlan, VecStore
from otters_amd import _native as N
from otters_amd.vec import sparse_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")
NAMES = ("ott_store_set_sparse", "ott_store_clear_sparse", "ott_store_sparse_info", "ott_store_read_sparse", "ott_query_sparse")


# ---- the header, ctypes and Rust --------------------------------------------------------------------------------------------------------

def test_header_declares_the_calls_the_defines_and_the_option():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(N.lib(), name), name
    defs = dict(re.findall(r"#define\s+(OTT_[A-Z0-9_]+)\s+(\d+)", code))
    assert int(defs["OTT_SPARSE_MAX_VOCAB"]) == 1 << 20 == N.SPARSE_MAX_VOCAB
    assert int(defs["OTT_SPARSE_MAX_QUERIES"]) == 1024 == N.SPARSE_MAX_QUERIES
    assert int(defs["OTT_ABI_VERSION"]) == 4 == N.ABI_VERSION == N.lib().ott_abi_version()  # the ABI grew at the end only
    assert "ott_sparse.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert '"sparse_table"' in open(os.path.join(CSRC, "ott_store.hip")).read() and "OTT_SPARSE_TABLE" in src
    for out_of_scope in ("ott_query_fuse", "BM25", "2^20", "multi-GPU", "reordering rows", "ompaction"):
        assert out_of_scope in src.split("sparse vectors: a sparse row per stored row")[1], out_of_scope


def test_ctypes_and_rust_declarations_match_the_header():
    protos, rust = RB.c_prototypes(), RB.rust_externs()
    scalar = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    for name in NAMES:
        ret, args = protos[name]
        fn = getattr(N.lib(), name)
        assert ret == "int" and fn.restype is C.c_int, name
        assert len(fn.argtypes) == len(args), (name, args)
        for a, ct in zip(args, fn.argtypes):
            assert ct is (C.c_void_p if a.endswith("*") else scalar[a]), (name, a, ct)
        rret, rargs = rust[name]
        assert rret == "c_int" and [RB.C2RUST[a] for a in args] == rargs, (name, args, rargs)
    assert protos["ott_query_sparse"][1] == ["ott_store*", "const ott_query_desc*", "const uint64_t*", "const void*", "const float*", "ott_hit*", "uint64_t",
                                             "uint64_t*", "uint64_t*", "ott_stats*"]
    assert protos["ott_store_set_sparse"][1] == ["ott_store*", "const uint64_t*", "const void*", "const float*", "uint64_t", "uint32_t"]
    assert protos["ott_store_read_sparse"][1] == ["const ott_store*", "uint64_t", "uint64_t", "uint64_t*", "void*", "float*", "uint64_t"]
    consts = dict(re.findall(r"pub const (OTT_SPARSE_[A-Z_]+)\s*:\s*u32\s*=\s*(\d+)", RB.rust_source()))
    assert consts == {"OTT_SPARSE_MAX_VOCAB": "1048576", "OTT_SPARSE_MAX_QUERIES": "1024"}


# ---- the ABI's refusals that need no device -----------------------------------------------------------------------------------------------

def desc(nq=1, mode=1, metric=2, path=0):
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = None, nq, metric, 1, mode, 3, path
    return d


def test_argument_refusals_need_no_device():
    L = N.lib()
    out = np.zeros(8, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)
    idx, val = np.array([3, 1], np.uint32), np.array([1.0, 2.0], np.float32)

    def call(d, ptr=(0, 2), no_ptr=False, no_entries=False):
        p = np.array(list(ptr) + [ptr[-1]] * max(d.nq + 1 - len(ptr), 0), np.uint64)
        return L.ott_query_sparse(None, C.byref(d), None if no_ptr else N.ptr(p), None if no_entries else N.ptr(idx), None if no_entries else N.ptr(val), N.ptr(out),
                                  out.size, C.byref(n_out), None, None)

    def err():
        return L.ott_last_error()

    assert call(desc()) == -1 and b"ott_query_sparse: store is NULL" in err()  # nothing wrong with the arguments: the store is next
    assert call(desc(nq=0)) == -1 and b"No queries provided" in err()
    assert call(desc(nq=1025)) == -1 and b"1025 queries are above OTT_SPARSE_MAX_QUERIES (1024)" in err()
    assert call(desc(nq=2, mode=0)) == -1 and b"a batch needs OTT_MODE_PER_QUERY" in err()
    assert call(desc(nq=1, mode=0)) == -1 and b"store is NULL" in err()  # MERGED with one query is served
    for metric in (0, 1, 3):
        assert call(desc(metric=metric)) == -1 and b"the metric must be OTT_METRIC_DOT" in err()
    assert call(desc(metric=9)) == -1 and b"ott_query_sparse: unknown metric" in err()
    assert call(desc(path=2)) == -4 and b"the MFMA path does not serve sparse queries" in err()
    assert call(desc(), no_ptr=True) == -1 and b"q_indptr, q_indices or q_values is NULL" in err()
    assert call(desc(), no_entries=True) == -1 and b"q_indptr, q_indices or q_values is NULL" in err()
    assert call(desc(), ptr=(0, 0), no_entries=True) == -1 and b"store is NULL" in err()  # an empty query needs no entries
    assert call(desc(), ptr=(1, 2)) == -1 and b"q_indptr[0] is 1, not 0" in err()
    assert call(desc(nq=3), ptr=(0, 2, 1, 2)) == -1 and b"q_indptr decreases at query 1" in err()
    assert L.ott_query_sparse(None, None, None, None, None, None, 0, None, None, None) == -1 and b"desc is NULL" in err()
    assert n_out.value == 9 and not out["index"].any()  # nothing was touched
    assert L.ott_store_set_sparse(None, None, None, None, 0, 1) == -1 and b"ott_store_set_sparse: store is NULL" in err()
    assert L.ott_store_clear_sparse(None) == -1 and b"ott_store_clear_sparse: store is NULL" in err()
    assert L.ott_store_sparse_info(None, None, None, None, None) == -1 and b"ott_store_sparse_info: store is NULL" in err()
    assert L.ott_store_read_sparse(None, 0, 0, None, None, None, 0) == -1 and b"ott_store_read_sparse: store is NULL" in err()
    assert L.ott_store_set_option(None, b"sparse_table", 1) != 0 and b"NULL" in err()


# ---- the plan header, walked by a stand-alone program ------------------------------------------------------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ott_sparse_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static bool has(SparseRefusal r, uint64_t a, uint64_t b, const char* text, int status) {
    const std::string s = sparse_refusal_text(r, a, b);
    if (s.find(text) == std::string::npos || s.empty()) { fprintf(stderr, "text of %d is '%s'\n", (int)r, s.c_str()); return false; }
    return sparse_refusal_status(r) == status;
}
// the score over a case file: [u32 n, vocab, nq] indptr (n + 1 u64) indices values, then per query [u32 len] indices weights; writes per
// query S (n f32) and the overlap (n bytes) of the definition, then the same of the dense evaluation
static int score(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    uint32_t n, vocab, nq;
    CHECK(fread(&n, 4, 1, f) == 1 && fread(&vocab, 4, 1, f) == 1 && fread(&nq, 4, 1, f) == 1);
    std::vector<uint64_t> ptr(n + 1);
    CHECK(fread(ptr.data(), 8, n + 1, f) == n + 1);
    const uint64_t nnz = ptr[n];
    std::vector<uint32_t> idx(nnz + 1);
    std::vector<float> val(nnz + 1);
    if (nnz) CHECK(fread(idx.data(), 4, nnz, f) == nnz && fread(val.data(), 4, nnz, f) == nnz);
    uint64_t a = 0, b = 0;
    CHECK(sparse_check_set(false, ptr.data(), idx.data(), val.data(), n, vocab, n, &a, &b) == SPARSE_OK);
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    std::vector<float> S(n + 1), table(vocab);
    std::vector<uint8_t> ov(n + 1), present(vocab);
    for (uint32_t q = 0; q < nq; q++) {
        uint32_t len;
        CHECK(fread(&len, 4, 1, f) == 1);
        std::vector<uint32_t> qi(len + 1);
        std::vector<float> qw(len + 1);
        if (len) CHECK(fread(qi.data(), 4, len, f) == len && fread(qw.data(), 4, len, f) == len);
        const uint64_t qptr[2] = {0, len};
        CHECK(sparse_check_query(1, qptr, qi.data(), qw.data(), vocab, &a, &b) == SPARSE_OK);
        for (int dense = 0; dense < 2; dense++) {
            if (dense) {
                std::fill(table.begin(), table.end(), 0.0f);
                std::fill(present.begin(), present.end(), (uint8_t)0);
                for (uint32_t e = 0; e < len; e++) {
                    table[qi[e]] = qw[e];
                    present[qi[e]] = 1;
                }
            }
            for (uint32_t r = 0; r < n; r++) {
                bool o = false;
                const uint64_t L = ptr[r + 1] - ptr[r];
                S[r] = dense ? sparse_score_dense(idx.data() + ptr[r], val.data() + ptr[r], L, table.data(), present.data(), &o)
                             : sparse_score(idx.data() + ptr[r], val.data() + ptr[r], L, qi.data(), qw.data(), len, &o);
                ov[r] = o;
            }
            if (n) CHECK(fwrite(S.data(), 4, n, g) == n && fwrite(ov.data(), 1, n, g) == n);
        }
    }
    fclose(f);
    fclose(g);
    return 0;
}
int main(int argc, char** argv) {
    if (argc == 3) return score(argv[1], argv[2]);
    CHECK(SPARSE_MAX_VOCAB == (1u << 20) && SPARSE_MAX_QUERIES == 1024 && SPARSE_SLICE == 64 && SPARSE_LDS_MAX_VOCAB == 32768 && SPARSE_TABLE_NQ == 4 &&
          SPARSE_MAX_ROWS == 0xFFFFFFF0ull);
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    uint64_t a = 99, b = 99;
    // ---- ott_store_set_sparse's checks, in the order the call makes them: every later fault is present too
    {
        const uint64_t bad_ptr[4] = {1, 3, 2, 4};
        uint64_t ptr[4] = {0, 2, 2, 5};
        uint32_t idx[5] = {4, 9, 0, 3, 7};
        float val[5] = {1.f, -0.f, 0.f, 1e-45f, -3e38f};
        CHECK(sparse_check_set(true, nullptr, nullptr, nullptr, 3, 0, 4, &a, &b) == SPARSE_SET_MULTI_GPU);
        CHECK(sparse_check_set(false, nullptr, nullptr, nullptr, 3, 0, 4, &a, &b) == SPARSE_SET_VOCAB && a == 0);
        CHECK(sparse_check_set(false, nullptr, nullptr, nullptr, 3, (1u << 20) + 1, 4, &a, &b) == SPARSE_SET_VOCAB && a == (1u << 20) + 1);
        CHECK(sparse_check_set(false, nullptr, nullptr, nullptr, 3, 1u << 20, 4, &a, &b) == SPARSE_SET_LENGTH && a == 3 && b == 4);
        CHECK(sparse_check_set(false, nullptr, nullptr, nullptr, 3, 10, 3, &a, &b) == SPARSE_SET_NULL);
        CHECK(sparse_check_set(false, bad_ptr, nullptr, nullptr, 3, 10, 3, &a, &b) == SPARSE_SET_INDPTR0 && a == 1);
        CHECK(sparse_check_set(false, bad_ptr + 1, nullptr, nullptr, 0, 10, 0, &a, &b) == SPARSE_SET_INDPTR0 && a == 3);  // even for an empty store
        ptr[2] = 1;
        CHECK(sparse_check_set(false, ptr, nullptr, nullptr, 3, 10, 3, &a, &b) == SPARSE_SET_INDPTR_ORDER && a == 1);
        ptr[2] = 2;
        CHECK(sparse_check_set(false, ptr, nullptr, val, 3, 10, 3, &a, &b) == SPARSE_SET_NULL && sparse_check_set(false, ptr, idx, nullptr, 3, 10, 3, &a, &b) == SPARSE_SET_NULL);
        CHECK(sparse_check_set(false, ptr, idx, val, 3, 10, 3, &a, &b) == SPARSE_OK && a == 0 && b == 0);  // -0.0, 0.0, a subnormal and -3e38 are stored values
        CHECK(sparse_check_set(false, ptr, idx, val, 3, 9, 3, &a, &b) == SPARSE_SET_INDEX_RANGE && a == 0 && b == 9);
        idx[4] = 3;  // a duplicate inside row 2
        val[4] = nan;
        CHECK(sparse_check_set(false, ptr, idx, val, 3, 10, 3, &a, &b) == SPARSE_SET_INDEX_ORDER && a == 2 && b == 2);
        idx[4] = 2;  // descending
        CHECK(sparse_check_set(false, ptr, idx, val, 3, 10, 3, &a, &b) == SPARSE_SET_INDEX_ORDER && a == 2 && b == 2);
        idx[4] = 7;
        for (float v : {nan, inf, -inf}) {
            val[4] = v;
            CHECK(sparse_check_set(false, ptr, idx, val, 3, 10, 3, &a, &b) == SPARSE_SET_VALUE && a == 2 && b == 2);
        }
        const uint64_t none[1] = {0};
        CHECK(sparse_check_set(false, none, nullptr, nullptr, 0, 1, 0, &a, &b) == SPARSE_OK);  // an empty store
        const uint64_t empty_rows[3] = {0, 0, 0};
        CHECK(sparse_check_set(false, empty_rows, nullptr, nullptr, 2, 1, 2, &a, &b) == SPARSE_OK);  // rows without entries
    }
    // ---- ott_query_sparse: what the arguments decide
    {
        const uint64_t ptr[4] = {0, 2, 2, 3}, ptr1[2] = {1, 3}, down[4] = {0, 2, 1, 3}, empty[2] = {0, 0};
        const uint32_t idx[3] = {7, 2, 7};
        const float w[3] = {1.f, -0.f, 2.f};
        CHECK(sparse_check_query_args(0, 0, 0, 2, nullptr, nullptr, nullptr, &a) == SPARSE_Q_NO_QUERIES);
        CHECK(sparse_check_query_args(1025, 0, 0, 2, nullptr, nullptr, nullptr, &a) == SPARSE_Q_TOO_MANY_QUERIES && a == 1025);
        CHECK(sparse_check_query_args(2, 0, 0, 2, nullptr, nullptr, nullptr, &a) == SPARSE_Q_MERGED);
        CHECK(sparse_check_query_args(2, 1, 0, 2, nullptr, nullptr, nullptr, &a) == SPARSE_Q_METRIC && sparse_check_query_args(1, 0, 3, 2, nullptr, nullptr, nullptr, &a) == SPARSE_Q_METRIC);
        CHECK(sparse_check_query_args(1, 0, 2, 2, nullptr, nullptr, nullptr, &a) == SPARSE_Q_MFMA);
        CHECK(sparse_check_query_args(1, 0, 2, 0, nullptr, idx, w, &a) == SPARSE_Q_NULL);
        CHECK(sparse_check_query_args(1, 0, 2, 1, ptr1, idx, w, &a) == SPARSE_Q_INDPTR0 && a == 1);
        CHECK(sparse_check_query_args(3, 1, 2, 0, down, idx, w, &a) == SPARSE_Q_INDPTR_ORDER && a == 1);
        CHECK(sparse_check_query_args(3, 1, 2, 0, ptr, nullptr, w, &a) == SPARSE_Q_NULL && sparse_check_query_args(3, 1, 2, 0, ptr, idx, nullptr, &a) == SPARSE_Q_NULL);
        CHECK(sparse_check_query_args(3, 1, 2, 0, ptr, idx, w, &a) == SPARSE_OK && sparse_check_query_args(1, 0, 2, 1, empty, nullptr, nullptr, &a) == SPARSE_OK);
        CHECK(sparse_check_query_args(1024, 1, 2, 0, nullptr, nullptr, nullptr, &a) == SPARSE_Q_NULL);
        // ... and what the store decides
        CHECK(sparse_check_store(true, false, 0, 5, 1, &a, &b) == SPARSE_Q_MULTI_GPU && sparse_check_store(false, false, 0, 5, 1, &a, &b) == SPARSE_Q_NO_ROWS);
        CHECK(sparse_check_store(false, true, 4, 5, 1, &a, &b) == SPARSE_Q_STALE && a == 4 && b == 5);
        CHECK(sparse_check_store(false, true, 5, 5, 1, &a, &b) == SPARSE_Q_TIE_ORDER && sparse_check_store(false, true, 5, 5, 2, &a, &b) == SPARSE_Q_TIE_ORDER);
        CHECK(sparse_check_store(false, true, SPARSE_MAX_ROWS, SPARSE_MAX_ROWS, 0, &a, &b) == SPARSE_Q_TOO_MANY_ROWS);
        CHECK(sparse_check_store(false, true, SPARSE_MAX_ROWS - 1, SPARSE_MAX_ROWS - 1, 0, &a, &b) == SPARSE_OK && sparse_check_store(false, true, 0, 0, 0, &a, &b) == SPARSE_OK);
        CHECK(sparse_check_query(3, ptr, idx, w, 7, &a, &b) == SPARSE_Q_INDEX_RANGE && a == 0 && b == 7);
        CHECK(sparse_check_query(3, ptr, idx, w, 8, &a, &b) == SPARSE_OK);  // 7 in query 0 and in query 2: two queries may share an index; order is free
        const uint64_t one[2] = {0, 3};
        CHECK(sparse_check_query(1, one, idx, w, 8, &a, &b) == SPARSE_Q_INDEX_DUP && a == 0 && b == 7);
        const uint32_t ok_idx[3] = {7, 2, 0};
        for (float v : {nan, inf, -inf}) {
            const float bad[3] = {1.f, v, 2.f};
            CHECK(sparse_check_query(1, one, ok_idx, bad, 8, &a, &b) == SPARSE_Q_WEIGHT && a == 0 && b == 2);
        }
        const float fine[3] = {0.f, -0.f, 1e-45f};
        CHECK(sparse_check_query(1, one, ok_idx, fine, 8, &a, &b) == SPARSE_OK);
        CHECK(sparse_check_cap(29, 3, 10, 1000) == SPARSE_Q_CAP && sparse_check_cap(30, 3, 10, 1000) == SPARSE_OK && sparse_check_cap(0, 3, 0, 1000) == SPARSE_OK);
        CHECK(sparse_check_cap(1u << 30, 1024, 513, 1u << 16) == SPARSE_OK && sparse_check_cap(1u << 30, 1024, 513, (1u << 16) + 1) == SPARSE_Q_TOO_MANY_PAIRS);
        CHECK(sparse_check_cap(1u << 30, 1024, 512, 1u << 20) == SPARSE_OK);
    }
    // ---- every refusal has its own text and its status
    CHECK(has(SPARSE_SET_MULTI_GPU, 0, 0, "ott_store_set_sparse: a multi-GPU store is not served", -4));
    CHECK(has(SPARSE_SET_VOCAB, 0, 0, "vocab 0 is not in 1 .. OTT_SPARSE_MAX_VOCAB (1048576); remap the indices", -1));
    CHECK(has(SPARSE_SET_LENGTH, 3, 4, "3 sparse rows for a store of 4 rows", -1));
    CHECK(has(SPARSE_SET_NULL, 0, 0, "indptr, indices or values is NULL", -1));
    CHECK(has(SPARSE_SET_INDPTR0, 1, 0, "indptr[0] is 1, not 0", -1));
    CHECK(has(SPARSE_SET_INDPTR_ORDER, 17, 0, "indptr decreases at row 17", -1));
    CHECK(has(SPARSE_SET_INDEX_RANGE, 5, 40, "index 40 of row 5 is not below vocab", -1));
    CHECK(has(SPARSE_SET_INDEX_ORDER, 5, 2, "the indices of row 5 are not strictly ascending at entry 2", -1));
    CHECK(has(SPARSE_SET_VALUE, 5, 2, "the value of entry 2 of row 5 is not finite", -1));
    CHECK(has(SPARSE_Q_NO_QUERIES, 0, 0, "No queries provided", -1));
    CHECK(has(SPARSE_Q_TOO_MANY_QUERIES, 1025, 0, "1025 queries are above OTT_SPARSE_MAX_QUERIES (1024)", -1));
    CHECK(has(SPARSE_Q_MERGED, 0, 0, "a batch needs OTT_MODE_PER_QUERY", -1));
    CHECK(has(SPARSE_Q_METRIC, 0, 0, "the metric must be OTT_METRIC_DOT", -1));
    CHECK(has(SPARSE_Q_MFMA, 0, 0, "the MFMA path does not serve sparse queries", -4));
    CHECK(has(SPARSE_Q_NULL, 0, 0, "q_indptr, q_indices or q_values is NULL", -1));
    CHECK(has(SPARSE_Q_INDPTR0, 2, 0, "q_indptr[0] is 2, not 0", -1));
    CHECK(has(SPARSE_Q_INDPTR_ORDER, 3, 0, "q_indptr decreases at query 3", -1));
    CHECK(has(SPARSE_Q_MULTI_GPU, 0, 0, "ott_query_sparse: a multi-GPU store is not served", -4));
    CHECK(has(SPARSE_Q_NO_ROWS, 0, 0, "no sparse rows are set (ott_store_set_sparse)", -1));
    CHECK(has(SPARSE_Q_STALE, 100, 101, "the sparse rows cover 100 rows, the store holds 101 (rows were appended since ott_store_set_sparse: set them again)", -1));
    CHECK(has(SPARSE_Q_TIE_ORDER, 0, 0, "tie_order 1 and 2 are not served", -4));
    CHECK(has(SPARSE_Q_TOO_MANY_ROWS, 0, 0, "2^32 - 16 rows or more", -4));
    CHECK(has(SPARSE_Q_INDEX_RANGE, 1, 40, "index 40 of query 1 is not below the store's vocab", -1));
    CHECK(has(SPARSE_Q_INDEX_DUP, 0, 5, "index 5 appears twice in query 0", -1));
    CHECK(has(SPARSE_Q_WEIGHT, 0, 2, "the weight of index 2 of query 0 is not finite", -1));
    CHECK(has(SPARSE_Q_CAP, 0, 0, "output capacity is smaller than nq * min(k, rows)", -1));
    CHECK(has(SPARSE_Q_TOO_MANY_PAIRS, 0, 0, "k above 512 is served only up to 2^26 (query, row) pairs", -4));
    CHECK(has(SPARSE_READ_RANGE, 1, 201, "rows 1 .. 201 are beyond the sparse rows", -1));
    CHECK(has(SPARSE_READ_CAP, 777, 0, "entry_cap is too small: the range holds 777 entries", -1));
    CHECK(sparse_refusal_status(SPARSE_OK) == 0 && sparse_refusal_text(SPARSE_OK, 0, 0).empty());
    {
        std::vector<std::string> seen;  // no two refusals share a text
        for (int r = SPARSE_SET_MULTI_GPU; r <= SPARSE_READ_CAP; r++) {
            const std::string t = sparse_refusal_text((SparseRefusal)r, 1, 2);
            CHECK(!t.empty());
            for (const std::string& s : seen) CHECK(s != t);
            seen.push_back(t);
        }
    }
    // ---- the layout: slices, bases, offsets
    CHECK(sparse_slices(0) == 0 && sparse_slices(1) == 1 && sparse_slices(64) == 1 && sparse_slices(65) == 2 && sparse_slices(129) == 3);
    CHECK(sparse_slices(0xFFFFFFF0ull) == 0x3FFFFFFull + 1 && sparse_slices(1ull << 40) == 1ull << 34);
    {
        // 130 rows: slice 0 has lengths 0..63 (L = 63), slice 1 is all empty, slice 2 has two rows of 5 and 2 entries
        std::vector<uint64_t> ptr(131);
        ptr[0] = 0;
        for (int r = 0; r < 130; r++) ptr[r + 1] = ptr[r] + (r < 64 ? r : r == 128 ? 5 : r == 129 ? 2 : 0);
        uint64_t base[4];
        CHECK(sparse_slice_len(ptr.data(), 130, 0) == 63 && sparse_slice_len(ptr.data(), 130, 1) == 0 && sparse_slice_len(ptr.data(), 130, 2) == 5);
        CHECK(sparse_slice_bases(ptr.data(), 130, base) == 64 * 68 && base[0] == 0 && base[1] == 64 * 63 && base[2] == 64 * 63 && base[3] == 64 * 68);
        const SparseLayout l = sparse_layout(130, 64 * 68);
        CHECK(l.n_slices == 3 && l.padded_entries == 4352 && l.off_values == 4352 * 4 && l.off_bases == 4352 * 8 && l.off_lengths == 4352 * 8 + 32 &&
              l.bytes == 4352 * 8 + 32 + 3 * 256);
        CHECK(sparse_entry_offset(base[2], 0, 128) == base[2] && sparse_entry_offset(base[2], 4, 129) == base[2] + 4 * 64 + 1 && sparse_entry_offset(0, 62, 63) == 62 * 64 + 63);
        CHECK(sparse_entry_offset(base[2], 4, 129) < base[3]);
        CHECK(sparse_slice_bytes(base, 0, 3) == 4352 * 8 + 3 * 264 && sparse_slice_bytes(base, 1, 2) == 264 && sparse_slice_bytes(base, 2, 2) == 0);
        CHECK(sparse_bytes_scanned(5, sparse_slice_bytes(base, 0, 3)) == 5 * (4352ull * 8 + 3 * 264));
        // counts beyond 2^32: two rows of 2^31 entries each in different slices (the row pointer alone says so: nothing that long is allocated)
        std::vector<uint64_t> big(67, 0);
        for (int r = 0; r < 66; r++) big[r + 1] = big[r] + (r == 3 || r == 65 ? (1ull << 31) : 1);
        uint64_t bb[3];
        CHECK(sparse_slice_bases(big.data(), 66, bb) == (1ull << 38) && bb[1] == (1ull << 37) && bb[2] == (1ull << 38));
        CHECK(sparse_entry_offset(bb[1], (1ull << 31) - 1, 65) == (1ull << 37) + ((1ull << 31) - 1) * 64 + 1 && sparse_entry_offset(bb[1], (1ull << 31) - 1, 65) < bb[2]);
        const SparseLayout L2 = sparse_layout(0xFFFFFFEFull, 1ull << 40);  // the most rows a query serves, 2^40 entries
        CHECK(L2.n_slices == 0x3FFFFFFull + 1 && L2.off_values == (1ull << 42) && L2.off_bases == (1ull << 43) && L2.off_lengths == (1ull << 43) + (0x4000000ull + 1) * 8 &&
              L2.bytes == (1ull << 43) + (0x4000000ull + 1) * 8 + (0x4000000ull << 8));
        // the 2^22 + 64 rows of 130 entries of a layout past 2^32 bytes
        const uint64_t rows = (1ull << 22) + 64, padded = rows * 130;
        const SparseLayout L3 = sparse_layout(rows, padded);
        CHECK(padded * 8 > (1ull << 32) && L3.n_slices == (1u << 16) + 1 && L3.off_bases == padded * 8 && L3.bytes == padded * 8 + ((1u << 16) + 2) * 8 + rows * 4);
        CHECK(sparse_entry_offset(((1ull << 16)) * 130 * 64, 129, rows - 1) == padded - 1);
    }
    // ---- the form of the lookup, its passes and sizes
    CHECK(sparse_lds_eligible(1) && sparse_lds_eligible(32768) && !sparse_lds_eligible(32769) && !sparse_lds_eligible(1u << 20));
    for (uint32_t nq : {1u, 4u, 64u, 1024u}) {
        CHECK(sparse_take_table(1, 1, nq) && sparse_take_table(1, 32768, nq) && sparse_take_table(1, 32769, nq));            // 1: always the table
        CHECK(!sparse_take_table(0, 1, nq) && !sparse_take_table(0, 32768, nq) && sparse_take_table(0, 32769, nq));          // 0: LDS wherever eligible
        CHECK(sparse_take_table(-1, 32769, nq) && sparse_take_table(-1, 1u << 20, nq));                                        // automatic: no choice above 32768
        CHECK(sparse_take_table(-1, 30522, nq) == sparse_take_table(-1, 31, nq));                                              // ... and one rule per nq class below
    }
    // automatic below 32769, as measured (profiles/sparse/README.md): the LDS form up to three queries, the table form from four on
    CHECK(SPARSE_AUTO_TABLE_FROM_NQ == 4);
    CHECK(!sparse_take_table(-1, 30522, 1) && !sparse_take_table(-1, 30522, 3) && sparse_take_table(-1, 30522, 4) && sparse_take_table(-1, 1, 64) && sparse_take_table(-1, 32768, 1024));
    CHECK(sparse_passes(false, 1) == 1 && sparse_passes(false, 5) == 5 && sparse_passes(false, 1024) == 1024);
    CHECK(sparse_passes(true, 1) == 1 && sparse_passes(true, 4) == 1 && sparse_passes(true, 5) == 2 && sparse_passes(true, 9) == 3 && sparse_passes(true, 1024) == 256);
    CHECK(sparse_vocab_pad(1) == 32 && sparse_vocab_pad(32) == 32 && sparse_vocab_pad(33) == 64 && sparse_vocab_pad(32768) == 32768);
    CHECK(sparse_lds_bytes(1) == 132 && sparse_lds_bytes(30522) == 30528 * 4 + 3816 && sparse_lds_bytes(32768) == 128 * 1024 + 4096 && sparse_lds_bytes(32768) <= 160 * 1024);
    CHECK(sparse_table_bytes(1) == 20 && sparse_table_bytes(9) == 9 * 16 + 8 && sparse_table_bytes(1u << 20) == (16u << 20) + (512u << 10));
    // ---- the score's corners
    {
        const uint32_t idx[4] = {1, 4, 6, 9}, qi[3] = {9, 1, 5};
        const float val[4] = {3e38f, 1.f, 2.f, 3e38f}, qw[3] = {-3e38f, 3e38f, 7.f};
        bool o = false;
        const float s = sparse_score(idx, val, 4, qi, qw, 3, &o);  // inf + -inf
        CHECK(s != s && o);
        CHECK(sparse_score(idx + 1, val + 1, 2, qi, qw, 3, &o) == 0.f && !o);  // shares nothing
        CHECK(sparse_score(idx, val, 0, qi, qw, 3, &o) == 0.f && !o && sparse_score(idx, val, 4, qi, qw, 0, &o) == 0.f && !o);
        const float zv[2] = {-0.f, 0.f}, zw[2] = {1.f, -2.f};
        const uint32_t zi[2] = {3, 8};
        const float z = sparse_score(zi, zv, 2, zi, zw, 2, &o);
        CHECK(z == 0.f && !__builtin_signbit(z) && o);  // -0.0 products never make S -0.0; the row is a candidate
        const float sub = sparse_score(zi, qw + 2, 1, zi, val + 3, 1, &o);  // 7 * 3e38 = inf
        CHECK(sub == inf && o);
        const float tiny_v[1] = {1e-20f}, tiny_w[1] = {1e-25f};
        CHECK(sparse_score(zi, tiny_v, 1, zi, tiny_w, 1, &o) == 1e-45f && o);  // a subnormal product is kept: no flush to zero
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
    d = tmp_path_factory.mktemp("sparse_walk")
    src, exe = d / "walk.cpp", d / "walk"
    src.write_text(WALK)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    return exe


def test_plan_header_walk_under_asan_ubsan(walk):
    out = subprocess.run([str(walk)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def plan_scores(walk, tmp_path, name, rows, vocab, queries):
    """(S, overlap) of the header's definition and of its dense evaluation: [2][nq, n]"""
    ptr, idx, val = SR.csr(rows)
    n = len(rows)
    blob = [struct.pack("<III", n, vocab, len(queries)), ptr.tobytes(), idx.tobytes(), val.tobytes()]
    for qi, qw in queries:
        blob += [struct.pack("<I", len(qi)), np.asarray(qi, np.uint32).tobytes(), np.asarray(qw, np.float32).tobytes()]
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    fin.write_bytes(b"".join(blob))
    out = subprocess.run([str(walk), str(fin), str(fout)], capture_output=True, text=True)
    assert out.returncode == 0, (name, out.stderr)
    raw = fout.read_bytes()
    res, at = [], 0
    for _ in queries:
        for _ in range(2):
            S = np.frombuffer(raw, np.float32, n, at)
            ov = np.frombuffer(raw, np.uint8, n, at + 4 * n).astype(bool)
            res.append((S, ov))
            at += 5 * n
    assert at == len(raw)
    return res


def same_bits(got, exp):
    """equal f32 bits; a NaN equals any NaN (which NaN an inf - inf gives is not part of the contract: the row is dropped)"""
    return not np.where(np.isnan(exp), ~np.isnan(got), got.view(np.uint32) != exp.view(np.uint32)).any()


def test_the_c_score_and_its_dense_evaluation_equal_the_model_bit_for_bit(walk, tmp_path):
    seen_nan = seen_inf = seen_sub = seen_cancel = seen_order = 0
    for name, rows, vocab, queries in SC.cpu_cases():
        ptr, idx, val = SR.csr(rows)
        S, cand = SR.scores(ptr, idx, val, queries, vocab)
        Sd, candd = SR.scores(ptr, idx, val, queries, vocab, dense=True)
        assert same_bits(Sd, S) and np.array_equal(cand, candd), name  # the proof that lets the kernel drop the branch, on the model
        got = plan_scores(walk, tmp_path, name.replace("^", "_"), rows, vocab, queries)
        for b in range(len(queries)):
            for form in (0, 1):  # the definition, the dense evaluation
                Sc, ovc = got[2 * b + form]
                assert same_bits(Sc, S[b]), (name, b, form, np.flatnonzero(Sc.view(np.uint32) != S[b].view(np.uint32))[:8])
                assert np.array_equal(ovc, cand[b]), (name, b, form)
            for r in range(0, len(rows), max(len(rows) // 40, 1)):  # ... and the one-row-at-a-time statement of the definition
                s1, o1 = SR.score_row(rows[r][0], rows[r][1], *queries[b])
                assert o1 == cand[b, r] and same_bits(np.array([s1], np.float32), S[b, r:r + 1]), (name, b, r)
        seen_nan += int(np.isnan(S).sum())
        seen_inf += int(np.isinf(S).sum())
        with np.errstate(all="ignore"):
            seen_sub += int(((S != 0) & (np.abs(S) < np.finfo(np.float32).tiny)).sum())
        seen_cancel += int((cand & (S == 0)).sum())
        if name == "rounding":  # the summation order shows in the bits: the reversed order gives other sums
            rev = [(i[::-1], v[::-1]) for i, v in rows]
            rptr, ridx, rval = SR.csr(rev)
            Sr, _ = SR.scores(rptr, ridx, rval, queries, vocab)
            seen_order = int((Sr.view(np.uint32) != S.view(np.uint32)).sum())
    # the edge inputs did what they are there for
    assert seen_nan >= 1 and seen_inf >= 2 and seen_sub >= 1 and seen_cancel >= 10 and seen_order >= 20, (seen_nan, seen_inf, seen_sub, seen_cancel, seen_order)
    S = SR.scores(*SR.csr(SC.ieee_case()[0]), SC.ieee_case()[2], 31)[0]
    assert not (S.view(np.uint32) == 0x80000000).any()  # S is never -0.0


def test_the_model_selects_as_the_contract_says():
    rows, vocab, queries = SC.ieee_case()
    ptr, idx, val = SR.csr(rows)
    hits = SR.query(ptr, idx, val, queries, vocab, 1, 100)
    assert hits[0]["index"].tolist()[0] == 0 and hits[0]["index"].tolist()[-1] == 2  # +inf first, -inf last
    assert 1 not in hits[0]["index"] and 9 not in hits[0]["index"] and 10 not in hits[0]["index"]
    zeros = hits[0][hits[0]["score"] == 0]["index"].tolist()
    assert zeros == [4, 5, 6, 7, 8, 13]  # equal S: the lower row first
    assert (hits[0]["query"] == 0).all() and (hits[1]["query"] == 1).all()
    low = SR.query(ptr, idx, val, queries, vocab, 0, 3)
    assert low[0]["index"].tolist() == [2, 11, 4] and low[0].size == 3
    keep = np.ones(len(rows), bool)
    keep[[0, 4]] = False
    masked = SR.query(ptr, idx, val, queries, vocab, 1, 100, cmp=int(Cmp.Gte), thr=0.0, keep=keep)
    assert masked[0]["index"].tolist() == [12, 3, 5, 6, 7, 8, 13]


# ---- the host objects ----------------------------------------------------------------------------------------------------------------------

def test_sparse_csr_and_the_plans_lowering():
    ptr, idx, val = sparse_csr([([3, 1], [1.0, 2.0]), ([], []), (np.array([7]), np.array([0.5]))])
    assert ptr.dtype == np.uint64 and ptr.tolist() == [0, 2, 2, 3] and idx.dtype == np.uint32 and idx.tolist() == [3, 1, 7] and val.dtype == np.float32
    ptr, idx, val = sparse_csr([])
    assert ptr.tolist() == [0] and idx.size == 0 and val.size == 0
    for bad, text in (([([1, 2], [1.0])], "sparse vector 0: 2 indices for 1 values"), ([([1], [1.0]), ([-1], [1.0])], "sparse vector 1: an index is not a 32-bit unsigned integer"),
                      ([([2 ** 32], [1.0])], "not a 32-bit unsigned integer")):
        with pytest.raises(OttersError) as ei:
            sparse_csr(bad)
        assert text in str(ei.value)
    store = VecStore(1)
    one = store.sparse_query(([5, 2], [1.0, -1.0]))
    assert isinstance(one, SparseQueryPlan) and len(one.queries) == 1
    assert len(store.sparse_query(([], [])).queries) == 1 and len(store.sparse_query((([1], [1.0]), ([2], [1.0]))).queries) == 2
    assert len(store.sparse_query([([1], [1.0]), ([], []), ([2, 3], [1.0, 1.0])]).queries) == 3
    rs = one.filter(0.5, Cmp.Gt).take_min(7).with_row_mask([True, False]).with_path(Path.Exact).resolve()
    assert (rs.indptr.tolist(), rs.indices.tolist(), rs.values.tolist()) == ([0, 2], [5, 2], [1.0, -1.0])
    assert (rs.take, rs.k, rs.filter_cmp, rs.filter_thr, rs.path, rs.row_mask.tolist()) == (0, 7, int(Cmp.Gt), 0.5, int(Path.Exact), [True, False])
    rs = store.sparse_query(([5], [1.0])).take(3).resolve()
    assert rs.take == 1 and rs.k == 3 and rs.filter_cmp == 0 and rs.row_mask is None  # a dot product: the larger the better
    with pytest.raises(OttersError) as ei:
        store.sparse_query([]).resolve()
    assert "No queries provided" in str(ei.value)
    with pytest.raises(OttersError) as ei:
        store.sparse_query([([1], [1.0]), ([2], [1.0])]).take(3).collect()
    assert "a batch needs OTT_MODE_PER_QUERY" in str(ei.value)
    assert store.sparse_info() is None  # no native store yet: nothing is set
    store.clear_sparse()
    for args, text in ((([0, 2], [1], [1.0, 2.0], 5), "indptr ends at 2, 1 indices and 2 values were given"), (([0, 1], [-4], [1.0], 5), "not a 32-bit unsigned integer"),
                       (([0, 1], [4], [1.0], -1), "vocab -1 is not in 1 .. OTT_SPARSE_MAX_VOCAB")):
        with pytest.raises(OttersError) as ei:
            store.set_sparse(*args)
        assert text in str(ei.value), str(ei.value)


def test_meta_builder_takes_sparse_rows_and_the_plan_defers_its_errors():
    from otters_amd import col
    n = 6
    cols = [Column("age", DataType.Int32).from_(list(range(n)))]
    ptr, idx, val = sparse_csr([([1], [1.0])] * n)
    b = MetaStore.from_columns(cols).with_vectors(np.zeros((n, 1), np.float32)).with_sparse(ptr, idx, val, 10)
    assert b.sparse[3] == 10
    ms = b.build(_host_only=True)
    with pytest.raises(OttersError) as ei:
        MetaStore.from_columns(cols).with_vectors(np.zeros((n, 1), np.float32)).with_sparse(ptr[:-1], idx, val, 10).build(_host_only=True)
    assert "with_sparse: indptr has 6 entries for 6 rows" in str(ei.value)
    p = ms.sparse_query(([1], [1.0])).meta_filter(col("nope").lt(5)).vec_filter(0.0, Cmp.Gt).take(3)
    with pytest.raises(OttersError) as ei:
        p.collect()
    assert "meta_filter compile error: Unknown column 'nope'" in str(ei.value)
    with pytest.raises(OttersError) as ei:
        ms.sparse_query(([1], [1.0])).take(3).collect()
    assert "sparse_query: the store holds no vectors" in str(ei.value)
