"""CPU: bit rows and ott_query_binary without a GPU.  The numpy model (tests/binary_ref.py) checks itself; the plan header
(otters_amd/csrc/ott_binary_plan.h) is compiled into a small host program under AddressSanitizer + UBSan and held to the model:
unit counts, (row, unit) offsets (past 2^32 bytes too: pure arithmetic), route eligibility, the capacity rule, Hamming and the
sign rule; a simulation of the gated sweep never drops a row the model's top-k needs; and what binary_query hands the native
boundary is what its arguments say."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import binary_ref as BR
import manhattan_ref as M
from otters_amd import _native as N
from otters_amd import BinaryQueryPlan, Cmp, Column, DataType, Metric, MetaStore, Mode, OttersError, Path, VecStore, col
from otters_amd.vec import binary_words, sign_bits
from test_native_calls_cpu import CHUNK, DIM, HANDLE, N_ROWS, ROWS, native, words_of  # noqa: F401 (native: the fake library fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "otters_amd", "csrc")


# ---- the model's self-checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [1, 63, 64, 65, 127, 128, 129, 1000])
def test_pack_unpack_round_trip_and_padding(n_bits):
    rng = np.random.default_rng(n_bits)
    bits = rng.integers(0, 2, (37, n_bits)).astype(bool)
    w = BR.pack(bits)
    assert w.dtype == np.uint64 and w.shape == (37, BR.words(n_bits))
    assert np.array_equal(BR.unpack(w, n_bits), bits)
    assert BR.padding_ok(w, n_bits).all()
    for r, j in ((0, 0), (5, n_bits - 1), (36, n_bits // 2)):  # bit j of a row is bit j % 64 of word j // 64
        assert bool((int(w[r, j // 64]) >> (j % 64)) & 1) == bool(bits[r, j])
    if n_bits % 64:
        bad = w.copy()
        bad[3, -1] |= np.uint64(1) << np.uint64(n_bits % 64)
        assert BR.padding_ok(bad, n_bits).tolist() == [i != 3 for i in range(37)]
    # the Python layer packs the same words
    pw, nb = binary_words(bits)
    assert nb == n_bits and np.array_equal(pw, w)
    pw2, nb2 = binary_words(w, n_bits)
    assert nb2 == n_bits and np.array_equal(pw2, w)


def test_popcount_by_table_equals_popcount_by_unpackbits():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 2 ** 63, (50, 7), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (50, 7), dtype=np.uint64)
    x[0, 0], x[0, 1] = np.uint64(0), np.uint64(2 ** 64 - 1)
    assert np.array_equal(BR.popcount_table(x), BR.popcount_unpack(x))
    assert BR.popcount_table(x)[0, :2].tolist() == [0, 64]
    bits = rng.integers(0, 2, (20, 129)).astype(bool)
    q = rng.integers(0, 2, (3, 129)).astype(bool)
    d = BR.distances(BR.pack(bits), BR.pack(q))
    assert np.array_equal(d, (bits[None] != q[:, None]).sum(axis=2))
    assert BR.scores(BR.pack(bits), BR.pack(q)).dtype == np.float32


def test_sign_rule_on_nan_zeros_and_denormals():
    den = np.float32(1e-45)  # the smallest positive denormal
    x = np.array([np.nan, -np.nan, 0.0, -0.0, den, -den, 1.0, -1.0, np.inf, -np.inf, np.float32(1.1754942e-38)], np.float32)
    want = [False, False, False, False, True, False, True, False, True, False, True]
    assert BR.sign_bits(x).tolist() == want
    assert sign_bits(x).tolist() == want  # the Python layer's host rule


def test_select_canonical_ties_go_to_the_lower_row():
    S = np.array([[3, 1, 1, 2, 1, 3]], np.float32)
    assert BR.expected(S, M.TAKE_MIN, 2)[0]["index"].tolist() == [1, 2]
    assert BR.expected(S, M.TAKE_MAX, 2)[0]["index"].tolist() == [0, 5]
    assert BR.expected(S, M.TAKE_MIN, 4, keep=[1, 0, 1, 1, 1, 1])[0]["index"].tolist() == [2, 4, 3, 0]
    h = BR.expected(np.vstack([S, S]), M.TAKE_MIN, 1, M.CMP_GT, 1.0)
    assert [x["index"].tolist() for x in h] == [[3], [3]] and [x["query"].tolist() for x in h] == [[0], [1]]


# ---- the plan header against the model ---------------------------------------------------------------------------------------------------
PROBE = r"""
#include <stdio.h>
#include <vector>
#include "ott_binary_plan.h"
using namespace ott;
int main(int argc, char** argv) {
    printf("{");
    const uint32_t bits[] = {1, 127, 128, 129, 16384};
    printf("\"units\": [");
    for (int i = 0; i < 5; i++) printf("%s[%u, %u]", i ? ", " : "", binary_words(bits[i]), binary_units(bits[i]));
    printf("], \"offsets\": [");
    const uint64_t rows[] = {0, 1, 63, 64, 65, 4097, 40000000ull, 4294967279ull};
    const uint32_t un[] = {1, 2, 8, 128};
    bool first = true;
    for (uint64_t r : rows)
        for (uint32_t u : un) {
            printf("%s[%llu, %u, %llu, %llu]", first ? "" : ", ", (unsigned long long)r, u, (unsigned long long)binary_unit_offset(r, u - 1, u),
                   (unsigned long long)binary_word_offset(r, 2 * u - 1, u));
            first = false;
        }
    printf("], \"bytes\": [%llu, %llu, %llu, %llu, %llu]", (unsigned long long)binary_layout_bytes(0, 128), (unsigned long long)binary_layout_bytes(65, 129),
           (unsigned long long)binary_layout_bytes(10000000, 1024), (unsigned long long)binary_range_bytes(63, 65, 8), (unsigned long long)binary_range_bytes(64, 64, 8));
    printf(", \"tiles\": [");
    const uint32_t tb[] = {1, 1024, 4094, 4095, 8190, 8191, 16382, 16383, 16384};
    for (int i = 0; i < 9; i++) printf("%s[%u, %u, %u]", i ? ", " : "", binary_gate_tile(tb[i], 1), binary_gate_tile(tb[i], 2), binary_gate_tile(tb[i], 9));
    printf("], \"eligible\": [%d, %d, %d, %d, %d, %d, %d]", (int)binary_gate_eligible(1024, 1, 512, 1000000, 0), (int)binary_gate_eligible(1024, 1, 513, 1000000, 0),
           (int)binary_gate_eligible(16382, 1, 10, 1000, 0), (int)binary_gate_eligible(16383, 1, 10, 1000, 0), (int)binary_gate_eligible(1024, 1, 0, 1000, 0),
           (int)binary_gate_eligible(128, 1024, 10, 4294967000ull, 0), (int)binary_gate_eligible(128, 8, 10, 4294967000ull, 0));
    printf(", \"caps\": [%llu, %llu, %llu, %llu, %llu, %llu, %llu]", (unsigned long long)binary_gate_capacity(0, 1024, 10000000), (unsigned long long)binary_gate_capacity(0, 1, 200000), (unsigned long long)binary_gate_capacity(0, 4, 1000000),
           (unsigned long long)binary_gate_capacity(0, 64, 10000000), (unsigned long long)binary_gate_capacity(1024, 1, 200000),
           (unsigned long long)binary_gate_capacity(1024, 1, 100), (unsigned long long)binary_gate_capacity(0, 9, 0));
    printf(", \"take\": [%d, %d, %d, %d]", (int)binary_take_gate(1, 1024, 1, 10, 1000, 0), (int)binary_take_gate(0, 1024, 1, 10, 1000, 0),
           (int)binary_take_gate(1, 1024, 1, 513, 1000, 0), (int)binary_take_gate(-1, 1024, 1, 10, 1000, 0) == (int)BINARY_AUTO_GATE);
    printf(", \"lds\": [%zu, %zu]", binary_gate_lds_bytes(1024, 4), binary_gate_query_lds(16384));
    // refusals: status and the entry point in the text
    uint64_t a, b;
    const uint64_t w2[] = {0, 4, 0, 3};  // two rows of 65 bits: row 0's last word has bit 2 set
    printf(", \"refusals\": [");
    const BinaryRefusal rs[] = {binary_check_set(true, w2, 2, 65, 2, &a, &b), binary_check_set(false, w2, 2, 0, 2, &a, &b), binary_check_set(false, w2, 2, 16385, 2, &a, &b),
                                binary_check_set(false, w2, 3, 65, 2, &a, &b), binary_check_set(false, nullptr, 2, 65, 2, &a, &b), binary_check_set(false, w2, 2, 65, 2, &a, &b),
                                binary_check_set(false, w2, 2, 67, 2, &a, &b), binary_check_sign(false, 16385, &a), binary_check_sign(false, 16384, &a),
                                binary_check_query_args(0, 1, 3, 0, w2, &a), binary_check_query_args(1025, 1, 3, 0, w2, &a), binary_check_query_args(2, 0, 3, 0, w2, &a),
                                binary_check_query_args(1, 0, 2, 0, w2, &a), binary_check_query_args(1, 0, 3, 2, w2, &a), binary_check_query_args(1, 0, 3, 0, nullptr, &a),
                                binary_check_query_args(1, 0, 3, 1, w2, &a), binary_check_store(false, false, 0, 5, 0, &a, &b), binary_check_store(false, true, 4, 5, 0, &a, &b),
                                binary_check_store(false, true, 5, 5, 1, &a, &b), binary_check_store(false, true, 4294967280ull, 4294967280ull, 0, &a, &b),
                                binary_check_store(false, true, 5, 5, 0, &a, &b), binary_check_query(w2, 2, 65, &a, &b), binary_check_cap(9, 2, 5, 100),
                                binary_check_cap(10, 2, 5, 100), binary_check_cap(1 << 30, 2, 513, 1ull << 26)};
    for (size_t i = 0; i < sizeof(rs) / sizeof(rs[0]); i++) printf("%s[%d, %d]", i ? ", " : "", (int)rs[i], binary_refusal_status(rs[i]));
    printf("], \"texts\": [\"%s\", \"%s\", \"%s\"]", binary_refusal_text(BINARY_SET_PADDING, 7, 65).c_str(), binary_refusal_text(BINARY_Q_STALE, 4, 5).c_str(),
           binary_refusal_text(BINARY_SIGN_DIM, 16385, 0).c_str());
    // Hamming and the sign rule on the caller's data: argv[1] = a file of u32 n_bits, u32 n, rows, one query; u32 m, m floats
    if (argc > 2) {
        FILE* f = fopen(argv[1], "rb");
        uint32_t nb = 0, n = 0, m = 0;
        if (!f || fread(&nb, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1) return 2;
        const uint32_t W = binary_words(nb);
        std::vector<uint64_t> rowsv((size_t)n * W), q(W);
        if (fread(rowsv.data(), 8, rowsv.size(), f) != rowsv.size() || fread(q.data(), 8, W, f) != W || fread(&m, 4, 1, f) != 1) return 2;
        std::vector<float> x(m);
        if (fread(x.data(), 4, m, f) != m) return 2;
        fclose(f);
        printf(", \"hamming\": [");
        for (uint32_t r = 0; r < n; r++) printf("%s%u", r ? ", " : "", binary_hamming(q.data(), rowsv.data() + (size_t)r * W, nb));
        printf("], \"sign\": [");
        for (uint32_t i = 0; i < m; i++) printf("%s%u", i ? ", " : "", binary_sign_bit(x[i]));
        printf("], \"bad_padding\": %llu", (unsigned long long)binary_first_bad_padding(rowsv.data(), n, nb));
    }
    // binary_run_bytes on the caller's run sets: argv[3] = a file of u32 n_sets, then per set u32 units, u32 n_runs, (start, count) u64 pairs
    if (argc > 3) {
        FILE* f = fopen(argv[3], "rb");
        uint32_t n_sets = 0;
        if (!f || fread(&n_sets, 4, 1, f) != 1) return 3;
        printf(", \"run_bytes\": [");
        for (uint32_t i = 0; i < n_sets; i++) {
            uint32_t units = 0, n_runs = 0;
            if (fread(&units, 4, 1, f) != 1 || fread(&n_runs, 4, 1, f) != 1) return 3;
            std::vector<uint64_t> runs((size_t)n_runs * 2);  // (exactly n_runs pairs: a read past them is the sanitizer's to find)
            if (fread(runs.data(), 8, runs.size(), f) != runs.size()) return 3;
            printf("%s%llu", i ? ", " : "", (unsigned long long)binary_run_bytes(runs.data(), n_runs, units));
        }
        fclose(f);
        printf("]");
    }
    printf("}\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("binary_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src),
                           "-o", str(exe)])
    rng = np.random.default_rng(5)
    nb, n = 129, 70
    rows, q = BR.pack(rng.integers(0, 2, (n, nb)).astype(bool)), BR.pack(rng.integers(0, 2, (1, nb)).astype(bool))
    x = np.array([np.nan, 0.0, -0.0, 1e-45, -1e-45, 2.5, -2.5, np.inf, -np.inf], np.float32)
    fin = d / "data.bin"
    fin.write_bytes(np.array([nb, n], "<u4").tobytes() + rows.tobytes() + q.tobytes() + np.array([x.size], "<u4").tobytes() + x.tobytes())
    sets = run_sets(np.random.default_rng(6))
    frun = d / "runs.bin"
    frun.write_bytes(np.array([len(sets)], "<u4").tobytes() + b"".join(np.array([u, r.shape[0]], "<u4").tobytes() + r.astype("<u8").tobytes() for u, r in sets))
    out = subprocess.run([str(exe), str(fin), "data", str(frun)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    got = json.loads(out.stdout)
    got["_data"] = (rows, q, x, nb)
    got["_run_sets"] = sets
    return got


def runs_from(counts, gaps, first=0):
    """(start, count) runs [n, 2], ascending: run i holds counts[i] rows, gaps[i] >= 1 rows lie between run i - 1 and run i"""
    counts, gaps = np.asarray(counts, np.int64), np.asarray(gaps, np.int64)
    assert (counts >= 1).all() and (gaps[1:] >= 1).all()
    ends = np.cumsum(counts + gaps) + first
    return np.stack([ends - counts, counts], axis=1)


def run_sets(rng):
    """[(units, runs)]: hand-made run sets that name each case, then random ones.  Runs are what make_run_plan gives: ascending,
    disjoint, at least one row apart"""
    sets = [(1, np.zeros((0, 2), np.int64)),                                            # no run
            (3, np.array([[0, 1]])), (3, np.array([[63, 1]])), (3, np.array([[63, 2]])),  # single rows; a run that crosses a slice edge
            (2, np.array([[0, 64]])), (2, np.array([[1, 64]])), (2, np.array([[64, 64], [130, 1]])),
            (5, np.array([[0, 8], [16, 8], [32, 8], [48, 8]])),                          # four runs share slice 0
            (5, np.array([[60, 8], [70, 1], [72, 1], [127, 2], [129, 1]])),              # every slice shared with the run before
            (1, np.array([[10, 1], [12, 300], [313, 1], [1000, 1]])),                    # a long run between single rows of its own slices
            (128, np.array([[0, 5000]])), (128, np.array([[2 ** 32 - 17 - 64, 64]])),    # the widest row; the last rows a store may hold
            (7, runs_from(np.full(313, 8), np.full(313, 8))),                            # every second chunk of 8 rows: 313 runs
            (7, runs_from(np.full(50, 100), np.full(50, 600), first=3)), (7, runs_from(np.full(5, 1021), np.full(5, 1021)))]
    for _ in range(60):
        n = int(rng.integers(1, 40))
        kind = int(rng.integers(4))
        counts = (np.ones(n, np.int64), rng.integers(1, 10, n), rng.integers(1, 200, n), rng.integers(1, 3000, n))[kind]
        gaps = rng.integers(1, (3, 20, 200, 70)[kind], n)
        sets.append((int(rng.integers(1, 129)), runs_from(counts, gaps, first=int(rng.integers(0, 200)) + (2 ** 32 - 2 ** 20 if kind == 3 and n % 2 else 0))))
    return sets


def test_plan_header_unit_counts_and_offsets(probe):
    assert probe["units"] == [[BR.words(b), BR.units(b)] for b in (1, 127, 128, 129, 16384)] == [[1, 1], [2, 1], [2, 1], [3, 2], [256, 128]]
    seen_big = False
    for r, u, unit_off, word_off in probe["offsets"]:
        assert unit_off == BR.unit_offset(r, u - 1, u) and word_off == BR.word_offset(r, 2 * u - 1, u), (r, u)
        assert unit_off % 16 == 0 and word_off == unit_off + 8 and unit_off + 16 <= BR.layout_bytes(r + 1, 128 * u)
        seen_big = seen_big or unit_off >= 2 ** 32
    assert seen_big  # rows whose offset lies past 2^32 bytes: 64-bit arithmetic
    assert BR.unit_offset(4294967279, 127, 128) == (4294967279 // 64 * 128 + 127) * 1024 + (4294967279 % 64) * 16 > 2 ** 42
    assert probe["bytes"] == [0, BR.layout_bytes(65, 129), BR.layout_bytes(10000000, 1024), BR.range_bytes(63, 65, 8), 0] == [0, 4096, 1280000000, 16384, 0]


def test_plan_header_layout_is_the_transposed_slice():
    rng = np.random.default_rng(9)
    nb = 300
    w = BR.pack(rng.integers(0, 2, (70, nb)).astype(bool))
    img = BR.layout_image(w, nb).view(np.uint64).reshape(2, BR.units(nb), 64, 2)  # [slice][unit][row in slice][half]
    for r in (0, 1, 63, 64, 69):
        flat = img[r // 64, :, r % 64, :].reshape(-1)[: BR.words(nb)]
        assert np.array_equal(flat, w[r])
    assert not img[1, :, 6:, :].any()  # the last slice's padding rows are zero


def test_plan_header_route_eligibility_and_capacity(probe):
    tb = (1, 1024, 4094, 4095, 8190, 8191, 16382, 16383, 16384)
    assert probe["tiles"] == [[BR.gate_tile(b, 1), BR.gate_tile(b, 2), BR.gate_tile(b, 9)] for b in tb]
    assert probe["tiles"][2] == [1, 2, 4] and probe["tiles"][3] == [1, 2, 2] and probe["tiles"][6] == [1, 1, 1] and probe["tiles"][7] == [0, 0, 0]
    # k 512 / 513; the largest n_bits whose histogram fits (16382) and the first that does not; k 0; the capacity's ceiling keeps the
    # sort's pair count below 2^32 - 16 whatever the call's size
    assert probe["eligible"] == [1, 0, 1, 0, 0, 1, 1]
    assert [bool(x) for x in probe["eligible"]] == [BR.gate_eligible(1024, 1, 512, 1000000), BR.gate_eligible(1024, 1, 513, 1000000), BR.gate_eligible(16382, 1, 10, 1000),
                                                    BR.gate_eligible(16383, 1, 10, 1000), BR.gate_eligible(1024, 1, 0, 1000), BR.gate_eligible(128, 1024, 10, 4294967000),
                                                    BR.gate_eligible(128, 8, 10, 4294967000)]
    want = [BR.gate_capacity(0, 1024, 10000000), BR.gate_capacity(0, 1, 200000), BR.gate_capacity(0, 4, 1000000), BR.gate_capacity(0, 64, 10000000), BR.gate_capacity(1024, 1, 200000),
            BR.gate_capacity(1024, 1, 100), BR.gate_capacity(0, 9, 0)]
    assert probe["caps"] == want == [1 << 27, 200000, 1 << 20, 80000000, 1024, 100, 0]  # the ceiling, every pair, the floor, an eighth, the option
    assert probe["take"] == [1, 0, 0, 1]
    assert probe["lds"] == [4 * 1026 * 4, 65544] and BR.gate_query_lds(16382) == 65536 == BR.GATE_LDS_BYTES


def test_plan_header_refusals(probe):
    names = ["SET_MULTI_GPU", "SET_BITS", "SET_BITS", "SET_LENGTH", "SET_NULL", "SET_PADDING", "OK", "SIGN_DIM", "OK", "Q_NO_QUERIES", "Q_TOO_MANY_QUERIES", "Q_MERGED",
             "Q_METRIC", "Q_MFMA", "Q_NULL", "OK", "Q_NO_ROWS", "Q_STALE", "Q_TIE_ORDER", "Q_TOO_MANY_ROWS", "OK", "Q_PADDING", "Q_CAP", "OK", "Q_TOO_MANY_PAIRS"]
    order = ["OK", "SET_MULTI_GPU", "SET_BITS", "SET_LENGTH", "SET_NULL", "SET_PADDING", "SIGN_MULTI_GPU", "SIGN_DIM", "Q_NO_QUERIES", "Q_TOO_MANY_QUERIES", "Q_MERGED",
             "Q_METRIC", "Q_MFMA", "Q_NULL", "Q_MULTI_GPU", "Q_NO_ROWS", "Q_STALE", "Q_TIE_ORDER", "Q_TOO_MANY_ROWS", "Q_PADDING", "Q_CAP", "Q_TOO_MANY_PAIRS", "READ_RANGE"]
    unsupported = {"SET_MULTI_GPU", "SIGN_MULTI_GPU", "Q_MFMA", "Q_MULTI_GPU", "Q_TIE_ORDER", "Q_TOO_MANY_ROWS", "Q_TOO_MANY_PAIRS"}
    assert [order[r] for r, _ in probe["refusals"]] == names
    assert [s for _, s in probe["refusals"]] == [0 if n == "OK" else -4 if n in unsupported else -1 for n in names]
    assert probe["texts"] == ["ott_store_set_binary: row 7 has a bit set at or above n_bits (65) in its last word; padding bits must be zero",
                              "ott_query_binary: the bit rows cover 4 rows, the store holds 5 (rows were appended since ott_store_set_binary: set them again)",
                              "ott_store_set_binary_sign: dim 16385 is above OTT_BINARY_MAX_BITS (16384)"]


def test_plan_header_hamming_and_sign_rule(probe):
    rows, q, x, nb = probe["_data"]
    assert probe["hamming"] == BR.distances(rows, q)[0].tolist()
    assert probe["sign"] == BR.sign_bits(x).astype(int).tolist() == [0, 0, 0, 1, 0, 1, 0, 1, 0]
    assert probe["bad_padding"] == rows.shape[0]  # none


def test_plan_header_run_bytes_a_slice_two_runs_share_counts_once(probe):
    """binary_run_bytes (what stats.bytes_scanned reports per pass) against the model's count of distinct slices, which knows no
    runs: single rows, several runs in one slice, a slice shared with the run before, runs that end on a slice's edge"""
    sets = probe["_run_sets"]
    want = [BR.run_bytes(r, u) for u, r in sets]
    assert probe["run_bytes"] == want
    assert want[:8] == [0, 3072, 3072, 6144, 2048, 4096, 4096, 5120] and want[8] == 3 * 5120 and want[9] == 6 * 1024
    shared = sum(1 for u, r in sets if r.shape[0] > 1 and ((r[1:, 0] // 64) == ((r[:-1, 0] + r[:-1, 1] - 1) // 64)).any())
    assert shared > 30 and max(r.shape[0] for _, r in sets) == 313
    # the model's three forms of `rows` agree
    u, r = sets[8]
    rows = np.concatenate([np.arange(s, s + c) for s, c in r])
    keep = np.zeros(200, bool)
    keep[rows] = True
    assert BR.run_bytes(rows, u) == BR.run_bytes(keep, u) == want[8]
    # ... and a range of whole slices is binary_range_bytes
    assert BR.run_bytes(np.array([[64, 640]]), 9) == BR.range_bytes(64, 704, 9)


# ---- the gated sweep, simulated ------------------------------------------------------------------------------------------------------------
def corpora(rng, n, n_bits):
    center = n_bits // 2
    iid = rng.binomial(n_bits, 0.5, n)
    return {"iid": iid, "equal": np.full(n, center), "descending": np.sort(iid)[::-1].copy(), "ascending": np.sort(iid),
            "tiny": rng.integers(0, 2, n), "best_last": np.concatenate([np.full(n - 7, center), np.arange(7)])}


@pytest.mark.parametrize("k", [1, 10, 512])
@pytest.mark.parametrize("n_groups", [1, 5, 64])
def test_simulated_gate_never_drops_a_row_of_the_top_k(k, n_groups):
    rng = np.random.default_rng(k * 100 + n_groups)
    n, n_bits = 6000, 128
    for name, levels in corpora(rng, n, n_bits).items():
        for recompute, share in ((1.0, 1.0), (0.5, 0.5), (0.1, 0.0), (0.0, 0.0)):
            em = BR.simulate_gate(levels, k, n_bits, n_groups, rng, recompute=recompute, share=share)
            assert np.unique(em).size == em.size <= n, name  # a row is emitted once at most
            need = BR.must_emit(levels, k)
            assert np.isin(need, em).all(), (name, recompute, share)
            # ... so the sort over the emitted pairs gives the model's hits
            S = levels.astype(np.float32)[None]
            keep = np.zeros(n, bool)
            keep[em] = True
            assert np.array_equal(BR.expected(S, M.TAKE_MIN, k, keep=keep)[0], BR.expected(S, M.TAKE_MIN, k)[0]), name


def test_simulated_gate_stays_inside_the_plans_capacity_on_the_gpu_tests_corpora():
    """The corpora of tests/test_gpu_binary.py's 200 000 x 128-bit store, for the capacity the plan chooses there: every row of
    one query — no gated case but the one that sets binary_gate_cap can overflow, whatever the interleaving."""
    n, n_bits, rng = 200000, 128, np.random.default_rng(3)
    cap = BR.gate_capacity(0, 1, n)
    assert cap == n
    for name, levels in corpora(rng, n, n_bits).items():
        em = BR.simulate_gate(levels, 10, n_bits, 256, rng, recompute=0.5, share=0.5)
        assert em.size <= cap, name
    # the overflow case's corpus: sorted so that every row is at most as far as all rows before it, and the last 3000 rows share the
    # best distance.  Rows tied at the k-th best level pass every gate, so whatever the interleaving more than 1024 pairs come out
    levels = sorted_with_floor(rng.binomial(n_bits, 0.5, n), 3000)
    assert (np.diff(levels) <= 0).all() and BR.must_emit(levels, 10).size >= 3000
    for seed, (recompute, share) in enumerate(((1.0, 1.0), (0.5, 0.5), (0.0, 0.0))):
        em = BR.simulate_gate(levels, 10, n_bits, 256, np.random.default_rng(seed), recompute=recompute, share=share)
        assert em.size >= 3000 > BR.gate_capacity(1024, 1, n) == 1024


def sorted_with_floor(levels, n_tied):
    """descending, the best n_tied rows (the last ones) raised to one common level"""
    d = np.sort(levels)[::-1].copy()
    return np.maximum(d, d[-n_tied])


def test_a_wave_that_recomputes_before_it_emits_keeps_only_its_tiles_best():
    """Visited in row order by one workgroup that recomputes after every tile, a descending corpus still loses rows: a tile's rows
    are counted first, the gate falls to the tile's k-th best, and only those at or inside it are appended.  What is never lost is
    must_emit — so the overflow case ties its best rows instead of relying on the order of arrival."""
    levels = np.sort(np.random.default_rng(4).binomial(128, 0.5, 5000))[::-1].copy()
    hist, T, em = np.zeros(129, np.int64), 128, []
    for t in range(0, levels.size, 64):
        rows = np.arange(t, min(t + 64, levels.size))
        inside = rows[levels[rows] <= T]
        np.add.at(hist, levels[inside], 1)
        T = min(T, BR.gate_scan(hist, T, 10))
        em.append(inside[levels[inside] <= T])
    em = np.concatenate(em)
    assert em.size < levels.size and np.isin(BR.must_emit(levels, 10), em).all()


# ---- what binary_query hands the native boundary ----------------------------------------------------------------------------------------------
QBITS = (np.arange(3 * 70).reshape(3, 70) % 3 == 0)


def bstore(native, n=N_ROWS):
    s = native.store(n)
    native.calls.clear()
    native.queries.clear()
    return s


@pytest.mark.parametrize("nq", [1, 3])
def test_binary_query_arguments_at_the_native_boundary(native, nq):
    s = bstore(native)
    mask = np.arange(N_ROWS) % 3 != 1
    plan = s.binary_query(QBITS[:nq]).filter(40.0, Cmp.Lt).with_row_mask(mask).take(5)
    assert isinstance(plan, BinaryQueryPlan)
    words_seen = []
    orig = native._snapshot

    def snap(args):  # the query words READ THROUGH THE POINTER DURING THE CALL
        words_seen.append(np.frombuffer(C.string_at(args[2].value if hasattr(args[2], "value") else args[2], 8 * nq * 2), dtype="<u8").copy())
        return orig(args)

    native._snapshot = snap
    hits, counts = plan.collect_arrays()
    assert hits.dtype == N.HIT_DTYPE and hits.size == 0 and counts == [0] * nq
    (name, args, d), = native.queries
    assert name == "ott_query_binary" and len(args) == 8 and args[0].value == HANDLE
    assert np.array_equal(words_seen[0].reshape(nq, 2), BR.pack(QBITS[:nq]))
    assert d["queries"] is None and d["nq"] == nq and d["metric"] == int(Metric.Manhattan) and d["take"] == M.TAKE_MIN
    assert d["filter_cmp"] == int(Cmp.Lt) and d["filter_thr"] == 40.0 and d["k"] == 5 and d["path"] == int(Path.Auto)
    assert d["mode"] == int(Mode.PerQuery if nq > 1 else Mode.Merged)
    assert d["row_mask"] == words_of(mask) and d["row_mask_bits"] == N_ROWS and d["chunk_mask"] is None
    assert args[4] == nq * 5  # cap = nq * min(k, rows)
    # take Max, a named path, no take: every row
    native.queries.clear()
    s.binary_query(QBITS[:nq]).with_path(Path.Exact).take_max(100).collect_arrays()
    d = native.queries[0][2]
    assert d["take"] == M.TAKE_MAX and d["k"] == 100 and d["path"] == int(Path.Exact) and native.queries[0][1][4] == nq * N_ROWS
    native.queries.clear()
    s.binary_query(QBITS[:nq]).collect_arrays()
    assert native.queries[0][2]["k"] == N_ROWS and native.queries[0][2]["take"] == M.TAKE_MIN


def test_binary_store_calls_at_the_native_boundary(native):
    s = bstore(native)
    bits = np.arange(N_ROWS * 70).reshape(N_ROWS, 70) % 5 == 0
    s.set_binary(bits)
    name, args = native.calls[-1]
    assert name == "ott_store_set_binary" and args[0].value == HANDLE and args[2:] == (N_ROWS, 70)
    s.set_binary(BR.pack(bits), 70)
    assert native.calls[-1][0] == "ott_store_set_binary" and native.calls[-1][1][2:] == (N_ROWS, 70)
    s.set_binary_sign()
    assert native.names()[-1] == "ott_store_set_binary_sign"
    s.clear_binary()
    assert native.names()[-1] == "ott_store_clear_binary"
    assert s.binary_info() is None and native.names()[-1] == "ott_store_binary_info"  # (the fake leaves n_bits at 0)
    assert s.binary_counters() == {"gated_calls": 0, "pairs_emitted": 0, "overflows": 0, "table_calls": 0}
    q = s.binary_query_sign(ROWS[:2])
    assert np.array_equal(q.resolve().words, BR.pack(BR.sign_bits(ROWS[:2]))) and q.resolve().n_bits == DIM
    n_before = len(native.calls)
    with pytest.raises(OttersError, match="holds only 0 and 1"):
        s.set_binary(np.full((N_ROWS, 4), 2))
    with pytest.raises(OttersError, match="3 words per row for n_bits = 70"):
        s.set_binary(np.zeros((N_ROWS, 3), np.uint64), 70)
    with pytest.raises(OttersError, match="^No queries provided$"):
        s.binary_query(np.zeros((0, 70), bool)).take(3).collect_arrays()
    with pytest.raises(OttersError, match="a batch needs OTT_MODE_PER_QUERY"):
        s.binary_query(QBITS).take(3).collect()
    assert len(native.calls) == n_before + 1  # only the batch's collect() reached the library


def test_meta_binary_query_prunes_chunks_and_sends_the_row_mask(native):
    cols = [Column("a", DataType.Int32).from_(list(range(N_ROWS)))]
    ms = MetaStore.from_columns(cols).with_vectors(ROWS[:N_ROWS]).with_chunk_size(CHUNK).build(_host_only=True)
    ms._store = bstore(native)
    hits, counts = ms.binary_query(QBITS[:2]).meta_filter(col("a").lt(20)).take(4).collect_arrays()
    assert hits.size == 0 and counts == [0, 0]
    (name, args, d), = native.queries
    assert name == "ott_query_binary" and d["nq"] == 2 and d["k"] == 4 and d["metric"] == int(Metric.Manhattan)
    assert d["chunk_mask"] == words_of([True, True, False])  # chunks of 16 rows: rows 0 .. 19 lie in the first two
    bare = MetaStore.from_columns(cols).with_vectors(ROWS[:N_ROWS]).with_chunk_size(CHUNK).build(_host_only=True)
    with pytest.raises(OttersError, match="^binary_query: the store holds no vectors$"):
        bare.binary_query(QBITS[:1]).take(3).collect_arrays()


# ---- the header, the bindings, the build -------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    for fn in ("ott_store_set_binary", "ott_store_set_binary_sign", "ott_store_clear_binary", "ott_store_binary_info", "ott_store_read_binary", "ott_query_binary",
               "ott_store_binary_counters"):
        assert ("int %s(" % fn) in src, fn
    assert "#define OTT_ABI_VERSION 4" in src and "#define OTT_BINARY_MAX_BITS 16384" in src and "#define OTT_BINARY_MAX_QUERIES 1024" in src
    assert N.BINARY_MAX_BITS == BR.MAX_BITS == 16384 and N.BINARY_MAX_QUERIES == BR.MAX_QUERIES == 1024
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ott_binary.hip" in mk
    for name in ("binary_gate", "binary_gate_cap"):
        assert ('"%s"' % name) in src and ('"%s"' % name) in open(os.path.join(CSRC, "ott_store.hip")).read()
