"""CPU: rank fusion (ott_query_fuse, VecStore.fuse, MetaStore.fuse) without a GPU — the header's declarations, the
ABI's device-free refusals with the same texts in C and Python, a walk of the plan header (ott_fuse_plan.h) by a stand-alone C++
program under AddressSanitizer + UBSan whose formulas must equal the numpy model (tests/fuse_ref.py) bit for bit, the sharp cases
(tests/fuse_cases.py) proved sharp in numpy, and the planners' refusals and lowering."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as R
from otters_amd import Cmp, Column, DataType, FusePlan, Fusion, MetaStore, Metric, OttersError, Path, VecStore, col
from otters_amd import _native as N
from otters_amd.vec import fuse_args, fuse_default_fetch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")


# ---- the header -----------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_call_the_enum_and_the_defines_and_keeps_abi_4():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ott_query_fuse\s*\(", code)
    assert re.search(r"ott_query_fuse\s*\([^;]*const\s+void\s*\*\s*legs_per_request", code)  # const void* on purpose: the binding test's type map
    defs = dict(re.findall(r"#define\s+(OTT_[A-Z0-9_]+)\s+(\d+)", code))
    assert int(defs["OTT_FUSE_MAX_LEGS"]) == 16 == N.FUSE_MAX_LEGS
    assert int(defs["OTT_FUSE_MAX_FETCH"]) == 512 == N.FUSE_MAX_FETCH
    assert int(defs["OTT_FUSE_MAX_ENTRIES"]) == 8192 == N.FUSE_MAX_ENTRIES
    assert int(defs["OTT_FUSE_MAX_REQUESTS"]) == 1024 == N.FUSE_MAX_REQUESTS
    assert int(defs["OTT_ABI_VERSION"]) == 4 == N.ABI_VERSION == N.lib().ott_abi_version()
    enums = dict(re.findall(r"(OTT_FUSE_[A-Z]+)\s*=\s*(\d+)", code))
    assert {k: int(v) for k, v in enums.items()} == {"OTT_FUSE_RRF": 0, "OTT_FUSE_DBSF": 1, "OTT_FUSE_MINMAX": 2}
    assert (N.FUSE_RRF, N.FUSE_DBSF, N.FUSE_MINMAX) == (0, 1, 2) == (int(Fusion.Rrf), int(Fusion.Dbsf), int(Fusion.MinMax)) == (R.RRF, R.DBSF, R.MINMAX)
    assert "ott_fuse.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert hasattr(N.lib(), "ott_query_fuse")
    for scope in ("per leg", "multi-GPU", "nested prefetches", "stored rows"):  # what the header comment leaves out, by name
        assert scope in src


# ---- the ABI's refusals: all before any device work, the same texts in C and Python -----------------------------------------------------

def desc(nq=2, mode=1, k=3, dim=4):
    q = np.zeros((max(nq, 1), dim), np.float32)
    d = N.QueryDesc()
    d.queries, d.nq, d.metric, d.take, d.mode, d.k, d.path = q.ctypes.data, nq, int(Metric.DotProduct), 1, mode, k, 0
    return d, q


def test_argument_refusals_need_no_device_and_python_says_the_same():
    L = N.lib()
    out = np.zeros(8, dtype=N.HIT_DTYPE)
    n_out = C.c_uint64(9)
    inf, nan = float("inf"), float("nan")

    def both(text, status=-1, nq=2, mode=1, k=3, legs=(2,), fusion=0, rrf_k=60.0, weights=None, fetch=4, null_legs=False, python=True):
        d = desc(nq, mode, k)
        la = np.array(legs if len(legs) else [0], np.uint32)
        wa = None if weights is None else np.array(weights, np.float32)
        rc = L.ott_query_fuse(None, C.byref(d[0]), None if null_legs else N.ptr(la), len(legs), fusion, rrf_k, None if wa is None else N.ptr(wa), fetch,
                              N.ptr(out), out.size, C.byref(n_out), None, None)
        assert rc == status and text.encode() in L.ott_last_error(), (rc, L.ott_last_error())
        if python:
            with pytest.raises(OttersError) as ei:
                fuse_args(list(legs), nq, fetch, fusion, rrf_k, weights, k)
            assert str(ei.value) == L.ott_last_error().decode()

    both("ott_query_fuse: the legs are ranked one by one: d->mode must be OTT_MODE_PER_QUERY", status=-4, mode=0, python=False)
    both("ott_query_fuse: n_requests must be at least 1", legs=())
    both("ott_query_fuse: 1025 requests are above OTT_FUSE_MAX_REQUESTS (1024)", legs=(1,) * 1025, nq=1025)
    both("ott_query_fuse: legs_per_request is NULL", null_legs=True, python=False)
    both("ott_query_fuse: fetch must lie between 1 and OTT_FUSE_MAX_FETCH (512)", fetch=0)
    both("ott_query_fuse: fetch must lie between 1 and OTT_FUSE_MAX_FETCH (512)", fetch=513)
    both("ott_query_fuse: request 1 has 0 legs; a request takes 1 to OTT_FUSE_MAX_LEGS (16)", legs=(2, 0))
    both("ott_query_fuse: request 0 has 17 legs; a request takes 1 to OTT_FUSE_MAX_LEGS (16)", legs=(17,), nq=17)
    # (legs x fetch above OTT_FUSE_MAX_ENTRIES cannot bind while 16 x 512 is the most the two other rules let through: the walk holds its text)
    both("ott_query_fuse: legs_per_request adds up to 3, not to d->nq", legs=(2, 1), nq=2)
    both("ott_query_fuse: unknown fusion (OTT_FUSE_RRF, OTT_FUSE_DBSF or OTT_FUSE_MINMAX)", fusion=3)
    for bad in (inf, nan, -1.0):
        both("ott_query_fuse: rrf_k must be finite and at least 0", rrf_k=bad)
    for bad in (inf, -inf, nan):
        both("ott_query_fuse: the weight of leg 1 is not finite", weights=[1.0, bad])
    both("ott_query_fuse: k must be at least 1", k=0)
    # nothing wrong with the arguments: the store is next (rrf_k is read by RRF alone; 0 is a valid rrf_k; 16 x 512 entries fit)
    both("ott_query: store is NULL", fusion=1, rrf_k=nan, python=False)
    both("ott_query: store is NULL", rrf_k=0.0, weights=[0.0, -2.5], python=False)
    both("ott_query: store is NULL", legs=(16,), nq=16, fetch=512, python=False)
    assert L.ott_query_fuse(None, None, None, 0, 0, 0.0, None, 0, None, 0, None, None, None) == -1 and b"desc is NULL" in L.ott_last_error()
    assert n_out.value == 9 and not out["index"].any()  # nothing was touched
    fuse_args([16], 16, 512, 2, nan, None, 1)  # the same three in Python
    fuse_args([2], 2, 4, 0, 0.0, [0.0, -2.5], 3)


# ---- the plan header: a stand-alone program under ASan + UBSan; its formulas against the numpy model --------------------------------------

WALK = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "ott_fuse_plan.h"
using namespace ott;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static bool has(FuseRefusal r, uint64_t bad, uint64_t v, const char* text, int status) {
    const std::string s = fuse_refusal_text(r, bad, v);
    if (s.find(text) == std::string::npos || s.empty()) { fprintf(stderr, "text of %d is '%s'\n", (int)r, s.c_str()); return false; }
    return fuse_refusal_status(r) == status;
}
// the formulas over a case file: [u32 fusion, take_max, f32 rrf_k, u32 n_legs] then per leg [f32 w, u32 n, n u64 rows, n f32 scores];
// writes [u32 count] then per distinct row, ascending, [u64 row, f32 F] — through the kernel's own steps: keys, a sort, runs summed in leg order
static int formula(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    uint32_t fusion, take_max, n_legs;
    float rrf_k;
    CHECK(fread(&fusion, 4, 1, f) == 1 && fread(&take_max, 4, 1, f) == 1 && fread(&rrf_k, 4, 1, f) == 1 && fread(&n_legs, 4, 1, f) == 1);
    CHECK(n_legs <= FUSE_MAX_LEGS);
    std::vector<uint64_t> keys;
    std::vector<std::vector<float>> con(n_legs);
    for (uint32_t l = 0; l < n_legs; l++) {
        float w;
        uint32_t n;
        CHECK(fread(&w, 4, 1, f) == 1 && fread(&n, 4, 1, f) == 1 && n <= FUSE_MAX_FETCH);
        std::vector<uint64_t> rows(n + 1);
        std::vector<float> sc(n + 1);
        if (n) CHECK(fread(rows.data(), 8, n, f) == n && fread(sc.data(), 4, n, f) == n);
        const FuseLegStats st = fuse_leg_stats(fusion, take_max != 0, sc.data(), n);
        for (uint32_t r = 0; r < n; r++) {
            CHECK(fuse_key_fits(rows[r]));
            keys.push_back(fuse_key(rows[r], l, r));
            con[l].push_back(fuse_contribution(fusion, take_max != 0, rrf_k, w, st, r, sc[r]));
        }
    }
    fclose(f);
    std::sort(keys.begin(), keys.end());
    f = fopen(out, "wb");
    if (!f) return 2;
    std::vector<char> body;
    uint32_t count = 0;
    for (size_t i = 0; i < keys.size();) {
        float F = 0.0f;
        size_t j = i;
        for (; j < keys.size() && fuse_key_row(keys[j]) == fuse_key_row(keys[i]); j++) F = fuse_add(F, con[fuse_key_leg(keys[j])][fuse_key_pos(keys[j])]);
        const uint64_t row = fuse_key_row(keys[i]);
        body.insert(body.end(), (const char*)&row, (const char*)&row + 8);
        body.insert(body.end(), (const char*)&F, (const char*)&F + 4);
        count++;
        i = j;
    }
    CHECK(fwrite(&count, 4, 1, f) == 1 && (body.empty() || fwrite(body.data(), 1, body.size(), f) == body.size()));
    fclose(f);
    return 0;
}
int main(int argc, char** argv) {
    if (argc == 3) return formula(argv[1], argv[2]);
    CHECK(FUSE_MAX_LEGS == 16 && FUSE_MAX_FETCH == 512 && FUSE_MAX_ENTRIES == 8192 && FUSE_MAX_REQUESTS == 1024 && FUSE_ENTRY_LDS == 12);
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    uint64_t bad = 99, v = 99;
    // ---- the refusals the arguments decide, in the order the call makes them: every later fault is present too
    const uint32_t zero_legs[2] = {2, 0}, many[1] = {17}, wide[2] = {1, 16}, three[2] = {2, 1}, ok[2] = {2, 1};
    const float wbad[3] = {1.f, nan, inf}, wok[3] = {0.f, -2.5f, 1e30f};
    CHECK(fuse_check_args(false, nullptr, 0, 9, 0, 9, nan, wbad, 0, &bad, &v) == FUSE_NOT_PER_QUERY);
    CHECK(fuse_check_args(true, nullptr, 0, 9, 0, 9, nan, wbad, 0, &bad, &v) == FUSE_NO_REQUESTS);
    CHECK(fuse_check_args(true, nullptr, 1025, 9, 0, 9, nan, wbad, 0, &bad, &v) == FUSE_TOO_MANY_REQUESTS && v == 1025);
    CHECK(fuse_check_args(true, nullptr, 2, 9, 0, 9, nan, wbad, 0, &bad, &v) == FUSE_NULL_LEGS);
    CHECK(fuse_check_args(true, zero_legs, 2, 9, 0, 9, nan, wbad, 0, &bad, &v) == FUSE_BAD_FETCH && fuse_check_args(true, zero_legs, 2, 9, 513, 9, nan, wbad, 0, &bad, &v) == FUSE_BAD_FETCH);
    CHECK(fuse_check_args(true, zero_legs, 2, 9, 4, 9, nan, wbad, 0, &bad, &v) == FUSE_BAD_LEGS && bad == 1 && v == 0);
    CHECK(fuse_check_args(true, many, 1, 9, 4, 9, nan, wbad, 0, &bad, &v) == FUSE_BAD_LEGS && bad == 0 && v == 17);
    CHECK(fuse_check_args(true, wide, 2, 9, 513 - 1, 9, nan, wbad, 0, &bad, &v) == FUSE_LEG_SUM);  // 16 x 512 = 8192 entries fit
    CHECK(fuse_check_args(true, three, 2, 2, 4, 9, nan, wbad, 0, &bad, &v) == FUSE_LEG_SUM && v == 3);
    CHECK(fuse_check_args(true, ok, 2, 3, 4, 3, nan, wbad, 0, &bad, &v) == FUSE_BAD_FUSION);
    CHECK(fuse_check_args(true, ok, 2, 3, 4, FUSE_RRF, nan, wbad, 0, &bad, &v) == FUSE_BAD_RRF_K && fuse_check_args(true, ok, 2, 3, 4, FUSE_RRF, inf, wbad, 0, &bad, &v) == FUSE_BAD_RRF_K);
    CHECK(fuse_check_args(true, ok, 2, 3, 4, FUSE_RRF, -1e-45f, wbad, 0, &bad, &v) == FUSE_BAD_RRF_K);
    CHECK(fuse_check_args(true, ok, 2, 3, 4, FUSE_RRF, -0.f, wbad, 0, &bad, &v) == FUSE_BAD_WEIGHT && bad == 1);  // -0 is not below 0
    CHECK(fuse_check_args(true, ok, 2, 3, 4, FUSE_DBSF, nan, wbad, 0, &bad, &v) == FUSE_BAD_WEIGHT);        // rrf_k is read by RRF alone
    CHECK(fuse_check_args(true, ok, 2, 3, 4, FUSE_MINMAX, nan, wok, 0, &bad, &v) == FUSE_BAD_K);
    CHECK(fuse_check_args(true, ok, 2, 3, 4, FUSE_MINMAX, nan, wok, 1, &bad, &v) == FUSE_OK && fuse_check_args(true, ok, 2, 3, 4, FUSE_RRF, 0.f, nullptr, 1, &bad, &v) == FUSE_OK);
    // (the entries rule needs a fetch the fetch rule lets through: 16 legs x 512 is the most, so it can only bind together with it)
    CHECK((uint64_t)FUSE_MAX_LEGS * FUSE_MAX_FETCH == FUSE_MAX_ENTRIES);
    // ---- ... and the ones the store decides
    CHECK(fuse_check_store(true, FUSE_ROW_LIMIT) == FUSE_MULTI_GPU && fuse_check_store(false, FUSE_ROW_LIMIT) == FUSE_TOO_MANY_ROWS);
    CHECK(fuse_check_store(false, FUSE_ROW_LIMIT - 1) == FUSE_OK && fuse_check_store(false, 0) == FUSE_OK);
    // ---- every refusal has its text and its status
    CHECK(has(FUSE_NOT_PER_QUERY, 0, 0, "d->mode must be OTT_MODE_PER_QUERY", -4) && has(FUSE_NO_REQUESTS, 0, 0, "n_requests must be at least 1", -1));
    CHECK(has(FUSE_TOO_MANY_REQUESTS, 0, 1025, "1025 requests are above OTT_FUSE_MAX_REQUESTS (1024)", -1) && has(FUSE_NULL_LEGS, 0, 0, "legs_per_request is NULL", -1));
    CHECK(has(FUSE_BAD_FETCH, 0, 0, "fetch must lie between 1 and OTT_FUSE_MAX_FETCH (512)", -1) && has(FUSE_BAD_LEGS, 3, 17, "request 3 has 17 legs", -1));
    CHECK(has(FUSE_TOO_MANY_ENTRIES, 2, 9000, "request 2 has 9000 entries (legs x fetch), above OTT_FUSE_MAX_ENTRIES (8192)", -1));
    CHECK(has(FUSE_LEG_SUM, 0, 3, "adds up to 3, not to d->nq", -1) && has(FUSE_BAD_FUSION, 0, 0, "unknown fusion", -1));
    CHECK(has(FUSE_BAD_RRF_K, 0, 0, "rrf_k must be finite and at least 0", -1) && has(FUSE_BAD_WEIGHT, 5, 0, "the weight of leg 5 is not finite", -1));
    CHECK(has(FUSE_BAD_K, 0, 0, "k must be at least 1", -1) && has(FUSE_MULTI_GPU, 0, 0, "a multi-GPU store is not served", -4));
    CHECK(has(FUSE_TOO_MANY_ROWS, 0, 0, "2^51 rows or more", -4) && has(FUSE_CAP, 0, 0, "output capacity is smaller than the sum over the requests", -1));
    CHECK(has(FUSE_NULL_OUT, 0, 0, "out is NULL", -1) && fuse_refusal_text(FUSE_OK, 0, 0).empty());
    // ---- the capacity rule
    {
        const uint32_t legs[3] = {1, 16, 2};
        CHECK(fuse_stride(512, 300) == 300 && fuse_stride(7, 300) == 7 && fuse_stride(7, 0) == 0);
        CHECK(fuse_cap_needed(legs, 3, 10, 7, 3000) == 7 + 10 + 10 && fuse_cap_needed(legs, 3, 1, 7, 3000) == 3 && fuse_cap_needed(legs, 3, 1000, 512, 300) == 300 + 1000 + 600);
        CHECK(fuse_cap_needed(legs, 3, 5, 7, 0) == 0);  // an empty store needs no room
        int slot;
        CHECK(fuse_check_cap(&slot, 9, 10) == FUSE_CAP && fuse_check_cap(nullptr, 10, 10) == FUSE_NULL_OUT && fuse_check_cap(nullptr, 0, 0) == FUSE_OK && fuse_check_cap(&slot, 10, 10) == FUSE_OK);
    }
    // ---- the key: a round trip for rows up to 2^51 - 1, the refusal beyond, the order the sort relies on
    {
        const uint64_t rows[] = {0, 1, 8191, (1ull << 32) - 1, 1ull << 32, (1ull << 51) - 2, (1ull << 51) - 1};
        for (uint64_t row : rows)
            for (uint32_t leg : {0u, 1u, 15u})
                for (uint32_t pos : {0u, 1u, 511u}) {
                    const uint64_t k = fuse_key(row, leg, pos);
                    CHECK(fuse_key_fits(row) && fuse_key_row(k) == row && fuse_key_leg(k) == leg && fuse_key_pos(k) == pos);
                    CHECK(k != FUSE_PAD_KEY || (row == (1ull << 51) - 1 && leg == 15 && pos == 511));  // the one key the store check keeps out
                }
        CHECK(!fuse_key_fits(1ull << 51) && !fuse_key_fits(~0ull));
        CHECK(fuse_key(5, 15, 511) < fuse_key(6, 0, 0) && fuse_key(5, 2, 511) < fuse_key(5, 3, 0) && fuse_key(5, 2, 3) < FUSE_PAD_KEY);
    }
    // ---- padded counts, threads, LDS
    {
        const uint32_t e[] = {1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 8191, 8192}, p[] = {64, 64, 64, 128, 512, 512, 1024, 1024, 1024, 2048, 8192, 8192};
        for (int i = 0; i < 12; i++) CHECK(fuse_padded(e[i]) == p[i]);
        CHECK(fuse_threads(64) == 64 && fuse_threads(512) == 512 && fuse_threads(1024) == 1024 && fuse_threads(8192) == 1024);
        CHECK(fuse_lds_bytes(8192) == 96 * 1024 && fuse_lds_bytes(1024) == 12 * 1024 && fuse_lds_bytes(64) == 768);
    }
    // ---- the layout: nothing overlaps, the uploads are contiguous, the result block is one piece
    for (uint32_t nq : {1u, 19u, 1024u})
        for (uint32_t nr : {1u, 3u, 1024u})
            for (uint64_t stride : {1ull, 7ull, 512ull})
                for (uint64_t k : {1ull, 10ull, 100000ull})
                    for (uint32_t ml : {1u, 16u}) {
                        if (nr > nq) continue;
                        const FuseLayout L = fuse_layout(nq, nr, stride, k, ml);
                        CHECK(L.off_blocks == 0 && L.block_bytes == (size_t)nq * stride * 16 && L.off_first == L.block_bytes && L.off_legs == L.off_first + 4u * nr);
                        CHECK(L.off_weights == L.off_legs + 4u * nr && L.meta_bytes == 8u * nr + 4u * nq && L.upload_bytes == L.off_weights + 4u * nq);
                        CHECK(L.off_counts >= L.upload_bytes && L.off_counts % 256 == 0 && L.off_hits >= L.off_counts + 4u * nr && L.off_hits % 256 == 0);
                        CHECK(L.kout == (k < ml * stride ? k : ml * stride) && L.total == L.off_hits + (size_t)nr * L.kout * 16 && L.result_bytes == L.total - L.off_counts);
                    }
    // ---- the route
    CHECK(!fuse_take_device(-1, 0, 512) && fuse_take_device(1, 0, 512) && fuse_take_device(1, 0, 1) && !fuse_take_device(0, 0, 512) && !fuse_take_device(1, 1, 7) && !fuse_take_device(-1, 2, 7));
    CHECK(fuse_device_eligible(0, 512) && !fuse_device_eligible(0, 513) && !fuse_device_eligible(1, 5));
    // ---- the formulas at their edges
    {
        const FuseLegStats none{0.0, 0.0};
        CHECK(fuse_contribution(FUSE_RRF, true, 0.f, 1.f, none, 0, 5.f) == 1.f && fuse_contribution(FUSE_RRF, true, 60.f, 1.f, none, 0, 5.f) == 1.f / 61.f);
        CHECK(fuse_contribution(FUSE_RRF, false, 0.5f, -3.f, none, 1, nan) == -3.f / 2.5f);
        const float same[3] = {2.f, 2.f, 2.f}, one[1] = {7.f}, up[3] = {3.f, 2.f, 1.f}, down[3] = {1.f, 2.f, 3.f}, over[2] = {inf, 1.f};
        for (uint32_t fu : {FUSE_DBSF, FUSE_MINMAX}) {
            CHECK(fuse_contribution(fu, true, 0.f, 4.f, fuse_leg_stats(fu, true, same, 3), 1, 2.f) == 2.f);  // !(span > 0): 0.5
            CHECK(fuse_contribution(fu, false, 0.f, 4.f, fuse_leg_stats(fu, false, one, 1), 0, 7.f) == 2.f);
            const float c = fuse_contribution(fu, true, 0.f, 1.f, fuse_leg_stats(fu, true, over, 2), 0, inf);
            CHECK(fu == FUSE_MINMAX ? c != c : c == 0.5f);  // MINMAX: inf / inf is NaN and the row is dropped; DBSF: a NaN span, so 0.5 for all
        }
        const FuseLegStats mx = fuse_leg_stats(FUSE_MINMAX, true, up, 3), mn = fuse_leg_stats(FUSE_MINMAX, false, down, 3);
        CHECK(mx.worst == 1.0 && mx.span == 2.0 && mn.worst == 3.0 && mn.span == 2.0);
        CHECK(fuse_contribution(FUSE_MINMAX, true, 0.f, 1.f, mx, 0, 3.f) == 1.f && fuse_contribution(FUSE_MINMAX, true, 0.f, 1.f, mx, 2, 1.f) == 0.f);
        CHECK(fuse_contribution(FUSE_MINMAX, false, 0.f, 2.f, mn, 0, 1.f) == 2.f && fuse_contribution(FUSE_MINMAX, false, 0.f, 2.f, mn, 1, 2.f) == 1.f);
        const FuseLegStats e = fuse_leg_stats(FUSE_DBSF, true, nullptr, 0);
        CHECK(e.span == 0.0);
        CHECK(fuse_add(0.0f, -0.0f) == 0.0f && !__builtin_signbit(fuse_add(0.0f, -0.0f)));  // F starts at +0: it is never -0
        CHECK(fuse_sum64(3, [&](uint32_t i) { return (double)up[i]; }) == 6.0);
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
    d = tmp_path_factory.mktemp("fuse_walk")
    src, exe = d / "walk.cpp", d / "walk"
    src.write_text(WALK)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    return exe


def test_plan_header_walk_under_asan_ubsan(walk):
    out = subprocess.run([str(walk)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def plan_fused(walk, tmp_path, lists, fusion, take, rrf_k, weights, name):
    """{row: F} of the plan header's host formulas for one request"""
    blob = [struct.pack("<IIfI", fusion, int(take) == 1, rrf_k, len(lists))]
    for l, (rows, scores) in enumerate(lists):
        blob.append(struct.pack("<fI", 1.0 if weights is None else weights[l], len(rows)))
        blob.append(np.ascontiguousarray(rows, np.uint64).tobytes())
        blob.append(np.ascontiguousarray(scores, np.float32).tobytes())
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    fin.write_bytes(b"".join(blob))
    out = subprocess.run([str(walk), str(fin), str(fout)], capture_output=True, text=True)
    assert out.returncode == 0, (name, out.stderr)
    raw = fout.read_bytes()
    n = struct.unpack("<I", raw[:4])[0]
    rec = np.frombuffer(raw[4:], np.dtype([("row", "<u8"), ("F", "<f4")]), n)
    return rec["row"].copy(), rec["F"].copy()


def random_lists(rng, n_legs, n_rows, fetch, kind):
    """leg lists as a first stage would return them: distinct rows, scores best first under `take`"""
    lists = []
    for l in range(n_legs):
        n = int(rng.integers(0, fetch + 1)) if kind != "full" else fetch
        rows = rng.choice(n_rows, size=min(n, n_rows), replace=False).astype(np.uint64)
        if kind == "ints":
            s = rng.integers(-40, 40, rows.size).astype(np.float32)
        elif kind == "wide":
            s = (rng.standard_normal(rows.size) * 10.0 ** rng.integers(-20, 20, rows.size)).astype(np.float32)
        else:
            s = rng.standard_normal(rows.size).astype(np.float32)
        lists.append((rows, s))
    return lists


@pytest.mark.parametrize("fusion", [R.RRF, R.DBSF, R.MINMAX])
@pytest.mark.parametrize("take", [0, 1])
def test_plan_header_formulas_equal_the_model_bit_for_bit(walk, tmp_path, fusion, take):
    rng = np.random.default_rng(100 + 2 * fusion + take)
    cases = [(1, 40, 1, "ints"), (3, 30, 20, "ints"), (16, 600, 512, "full"), (5, 200, 130, "wide"), (16, 50, 40, "normal"), (2, 9, 9, "ints")]
    for i, (n_legs, n_rows, fetch, kind) in enumerate(cases):
        lists = random_lists(rng, n_legs, n_rows, fetch, kind)
        lists = [(r, np.sort(s)[::-1] if take == 1 else np.sort(s)) for r, s in lists]
        if i == 1:
            lists[0] = (lists[0][0], np.full(lists[0][0].size, 2.0, np.float32))  # a leg whose scores are all equal
        if i == 3 and lists[1][1].size:
            lists[1][1][0] = np.inf if take == 1 else -np.inf  # an infinite best score: NaN contributions
        weights = None if i % 2 == 0 else rng.choice(np.array([0.0, 1.0, -1.5, 0.3, 2.0 ** 20], np.float32), n_legs).tolist()
        rrf_k = 60.0 if i % 3 else 0.0
        rows, F = plan_fused(walk, tmp_path, lists, fusion, take, rrf_k, weights, f"c{i}")
        keep = ~np.isnan(F)
        exp = R.fuse_request(lists, fusion, take, 10 ** 9, rrf_k, weights)
        o = np.argsort(exp["index"])
        assert np.array_equal(rows[keep], exp["index"][o]), (fusion, take, i)
        assert np.array_equal(F[keep].view(np.uint32), exp["score"][o].view(np.uint32)), (fusion, take, i)
        union = np.unique(np.concatenate([r for r, _ in lists])) if lists else np.zeros(0, np.uint64)
        assert np.array_equal(rows, union)  # every listed row has one F; the NaN ones are the model's dropped rows


# ---- the sharp cases: a wrong implementation returns another top-k ----------------------------------------------------------------------

def case_lists(oracle, c):
    return R.leg_lists(oracle, c["rows"], c["legs"], Metric.DotProduct, 1, c["fetch"])


def test_leg_order_case_is_sharp(oracle):
    c = FC.leg_order()
    lists = case_lists(oracle, c)
    assert [l[0].tolist() for l in lists] == [[0, 2], [0, 1], [0, 2]]
    right = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"])
    wrong = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"], **c["wrong"])
    assert right["index"].tolist() == [1] and right["score"].tolist() == [0.5]
    assert wrong["index"].tolist() == [0] and wrong["score"].tolist() == [1.0]


def test_rrf_rank_case_is_sharp(oracle):
    c = FC.rrf_rank()
    lists = case_lists(oracle, c)
    assert [l[0].tolist() for l in lists] == [[0, 1], [2, 1]]
    right = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"])
    wrong = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"], **c["wrong"])
    assert right["index"].tolist() == [1] and wrong["index"].tolist() == [0]


def test_equal_f_goes_to_the_lower_row(oracle):
    c = FC.equal_f()
    right = R.fuse_request(case_lists(oracle, c), c["fusion"], 1, c["k"], c["rrf_k"], c["weights"])
    assert right["index"].tolist() == [1, 0, 2]
    assert right["score"][1].view(np.uint32) == right["score"][2].view(np.uint32)  # the same bits: only the row decides


def test_dbsf_mean_case_is_sharp(oracle):
    c = FC.dbsf_mean()
    lists = case_lists(oracle, c)
    n = c["rows"].shape[0]
    assert np.array_equal(lists[0][1], c["scores"]) and lists[0][0][-2:].tolist() == [0, n - 1]  # the probes close leg 0's list
    assert lists[1][0].tolist() == list(range(1, 513)) and not lists[1][1].any()                  # leg 1: the fillers, all 0
    right = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"])
    assert right["index"].tolist() == [0, 1] and (right["score"] == c["target"]).all()
    for w in c["wrong"]:
        wrong = R.fuse_request(lists, c["fusion"], 1, c["k"], c["rrf_k"], c["weights"], **w)
        assert wrong["index"].tolist() != right["index"].tolist(), w
        assert wrong["index"].tolist() in ([0, n - 1], [1, 2]), w  # the probes moved up, or down


# ---- VecStore.fuse and MetaStore.fuse: refusals and lowering ----------------------------------------------------------------------------

def refused(p, text, how="validate"):
    with pytest.raises(OttersError) as ei:
        getattr(p, how)()
    assert text in str(ei.value), str(ei.value)


def test_vec_plan_refusals_and_lowering():
    store = VecStore(4)
    legs = [np.ones((2, 4), np.float32), np.ones((3, 4), np.float32)]
    new = lambda sets=legs: store.fuse(sets, Metric.DotProduct).take(5)  # noqa: E731
    assert isinstance(new(), FusePlan)
    refused(store.fuse([], Metric.DotProduct).take(5), "n_requests must be at least 1")
    refused(new([np.ones((1, 4), np.float32)] * 1025), "1025 requests are above OTT_FUSE_MAX_REQUESTS (1024)")
    refused(new([np.ones((17, 4), np.float32)]), "request 0 has 17 legs")
    refused(new([np.ones((2, 4), np.float32), np.ones((0, 4), np.float32)]), "request 1 has 0 legs")
    refused(new().fetch(0), "fetch must lie between 1 and OTT_FUSE_MAX_FETCH (512)")
    refused(new().fetch(513), "fetch must lie between 1 and OTT_FUSE_MAX_FETCH (512)")
    refused(new([np.ones((9, 4), np.float32)]).fetch(1000), "fetch must lie between")
    refused(new().rrf(float("nan")), "rrf_k must be finite and at least 0")
    refused(new().rrf(-1), "rrf_k must be finite and at least 0")
    refused(new().weights([[1, 2], [1, 2, float("inf")]]), "the weight of leg 4 is not finite")
    refused(new().weights([[1, 2]]), "weights takes one list per request with one weight per leg")
    refused(new().weights([[1, 2], [1, 2]]), "weights takes one list per request with one weight per leg")
    refused(new().take(0), "k must be at least 1")
    refused(new([np.ones((2, 5), np.float32)]), "Query vector length 5 does not match expected dimension 4")
    refused(store.fuse(legs, Metric.Manhattan).take(5).with_path(Path.Mfma), "the MFMA path does not score the Manhattan metric")
    refused(VecStore(4, devices=[0, 0]).fuse(legs, Metric.DotProduct).take(5), "a multi-GPU store is not served")
    new().dbsf().rrf(float("nan")).min_max().validate()  # rrf_k is read by RRF alone
    assert (fuse_default_fetch(1), fuse_default_fetch(8), fuse_default_fetch(10), fuse_default_fetch(128), fuse_default_fetch(4000)) == (32, 32, 40, 512, 512)
    rf = new().resolve()
    assert (rf.fusion, rf.rrf_k, rf.weights, rf.fetch, rf.k, rf.take, rf.metric, rf.filter_cmp, rf.path) == (0, 60.0, None, 32, 5, 1, int(Metric.DotProduct), 0, 0)
    assert rf.queries.shape == (5, 4) and rf.queries.dtype == np.float32 and rf.legs_per_request.tolist() == [2, 3] and rf.legs_per_request.dtype == np.uint32
    rf = (store.fuse(legs, Metric.Euclidean).min_max().weights([[1, 0.5], [0, -1, 2]]).fetch(7).take(3).filter(0.25, Cmp.Lt).with_row_mask([True, False])
          .with_path(Path.Exact).resolve())
    assert (rf.fusion, rf.fetch, rf.k, rf.take, rf.filter_cmp, rf.filter_thr, rf.path) == (2, 7, 3, 0, int(Cmp.Lt), 0.25, int(Path.Exact))
    assert rf.weights.tolist() == [1, 0.5, 0, -1, 2] and rf.weights.dtype == np.float32 and rf.row_mask.tolist() == [True, False]
    assert store.fuse(legs, Metric.Euclidean).dbsf().take_max(3).resolve().take == 1 and store.fuse(legs, Metric.Cosine).rrf(0).take_min(3).resolve().rrf_k == 0.0
    hits, counts = new().collect_arrays()  # an empty store: a valid call with no hits, and no native store is made
    assert hits.size == 0 and counts == [0, 0] and new().collect() == [[], []]


def test_meta_plan_refusals_and_lowering():
    n = 40
    cols = [Column("age", DataType.Int32).from_(list(range(n))), Column("lang", DataType.String).from_(["en", "de"] * (n // 2))]
    meta = MetaStore.from_columns(cols).with_vectors(np.ones((n, 3), np.float32).tolist()).with_chunk_size(10).build(_host_only=True)
    legs = [np.ones((2, 3), np.float32)]
    refused(meta.fuse(legs, Metric.DotProduct).meta_filter(col("nope").lt(5)).take(3), "meta_filter compile error: Unknown column 'nope'", "collect")
    refused(meta.fuse(legs, Metric.DotProduct).take(0), "fuse: the store holds no vectors", "collect")  # (a host-only store: nothing to rank)
    # the plan underneath is VecStore.fuse's: the same refusals, the same lowering
    store = VecStore(3)
    meta._store = store
    try:
        refused(meta.fuse(legs, Metric.DotProduct).take(0), "k must be at least 1", "collect")
        refused(meta.fuse(legs, Metric.DotProduct).fetch(600).take(3), "fetch must lie between 1 and OTT_FUSE_MAX_FETCH (512)")
        refused(meta.fuse([np.ones((2, 4), np.float32)], Metric.DotProduct).take(3), "Query vector length 4 does not match expected dimension 3")
        p = meta.fuse(legs).dbsf().weights([[1, 2]]).fetch(9).vec_filter(0.5, Cmp.Gt).meta_filter(col("age").gt(1)).take_min(4).with_path(Path.Exact)
        p.validate()
        rf = p._plan.resolve()
        assert (rf.fusion, rf.fetch, rf.k, rf.take, rf.metric, rf.filter_cmp, rf.path) == (1, 9, 4, 0, int(Metric.Cosine), int(Cmp.Gt), int(Path.Exact))
        assert rf.weights.tolist() == [1, 2] and p._meta_filter is not None
        hits, counts = meta.fuse(legs).meta_filter(col("age").gt(1000)).take(3).collect_arrays()  # every chunk pruned: nothing runs
        assert hits.size == 0 and counts == [0]
    finally:
        meta._store = None
