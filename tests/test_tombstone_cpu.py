"""CPU: deleting rows (include/otters_hip.h: ott_store_delete_rows and the four functions beside it) as far as it shows without
a GPU — the header declares the five functions (tests/test_abi_symbols.py then proves they are exported), the ctypes and Rust
bindings name them with the header's signatures, argument checks come before any device work, and the rule by which the live
mask joins a query's own row mask (and_live_kernel, otters_amd/csrc/ott_tomb.hip) holds in a numpy model over odd bit lengths."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = {
    "ott_store_delete_rows": "int ott_store_delete_rows(ott_store* s, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed);",
    "ott_store_restore_rows": "int ott_store_restore_rows(ott_store* s, const uint64_t* rows_host, uint64_t n, uint64_t* n_changed);",
    "ott_store_live_len": "uint64_t ott_store_live_len(const ott_store* s);",
    "ott_store_read_live_mask": "int ott_store_read_live_mask(const ott_store* s, uint64_t* out_host);",
    "ott_store_compact": "int ott_store_compact(ott_store* s, uint64_t* out_new_index);",
}


def test_header_declares_the_five_functions_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "otters_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for name, decl in FIVE.items():
        assert decl in flat, name
    assert "#define OTT_ABI_VERSION 4" in src
    # the library is one source list for the product and the audit build: the new file is in it
    mk = open(os.path.join(ROOT, "otters_amd", "csrc", "Makefile")).read()
    assert "ott_tomb.hip" in mk


def test_library_exports_them_and_checks_arguments_without_a_device():
    from otters_amd import _native as N
    N.build()
    L = N.lib()
    for name in FIVE:
        assert hasattr(L, name), name
    rows = np.array([0, 1], dtype=np.uint64)
    ch = C.c_uint64(99)
    for fn, who in ((L.ott_store_delete_rows, b"ott_store_delete_rows"), (L.ott_store_restore_rows, b"ott_store_restore_rows")):
        assert fn(None, N.ptr(rows), 2, C.byref(ch)) == -1
        msg = L.ott_last_error()
        assert who in msg and b"NULL" in msg, msg
        assert ch.value == 0  # nothing changed
        ch.value = 99
    assert L.ott_store_live_len(None) == 0
    out = np.zeros(1, dtype=np.uint64)
    assert L.ott_store_read_live_mask(None, N.ptr(out)) == -1 and b"ott_store_read_live_mask" in L.ott_last_error()
    assert L.ott_store_compact(None, None) == -1 and b"ott_store_compact" in L.ott_last_error()


def test_python_and_cpp_mirrors_have_the_methods():
    from otters_amd import MetaStore, VecStore
    for m in ("delete_rows", "restore_rows", "live_len", "live_mask", "compact"):
        assert callable(getattr(VecStore, m)), m
    for m in ("delete_rows", "restore_rows", "live_len"):
        assert callable(getattr(MetaStore, m)), m
    hpp = open(os.path.join(ROOT, "include", "otters.hpp")).read()
    meta = open(os.path.join(ROOT, "include", "otters_meta.hpp")).read()
    for m in ("delete_rows", "restore_rows", "live_len"):
        assert re.search(r"std::size_t " + m + r"\(", hpp), m
        assert re.search(r"std::size_t " + m + r"\(", meta), m


def test_rust_declarations_are_present():
    rs = open(os.path.join(ROOT, "bindings", "rust", "otters-hip-sys", "src", "lib.rs")).read()
    flat = re.sub(r"\s+", " ", rs)
    for decl in ("pub fn ott_store_delete_rows(s: *mut ott_store, rows_host: *const u64, n: u64, n_changed: *mut u64) -> c_int;",
                 "pub fn ott_store_restore_rows(s: *mut ott_store, rows_host: *const u64, n: u64, n_changed: *mut u64) -> c_int;",
                 "pub fn ott_store_live_len(s: *const ott_store) -> u64;",
                 "pub fn ott_store_read_live_mask(s: *const ott_store, out_host: *mut u64) -> c_int;",
                 "pub fn ott_store_compact(s: *mut ott_store, out_new_index: *mut u64) -> c_int;"):
        assert decl in flat, decl


# ---- the effective-mask rule ---------------------------------------------------------------------------------------------------
def effective_words(live_words, caller_words, caller_bits, n_bits):
    """and_live_kernel, word for word: out[w] = live[w] & caller[w], caller bits at and past caller_bits count as keep"""
    words = (n_bits + 63) // 64
    out = np.zeros(words, dtype=np.uint64)
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    for w in range(words):
        c = full
        if w * 64 < caller_bits:
            c = caller_words[w]
            rem = caller_bits - w * 64
            if rem < 64:
                c = c | np.uint64((0xFFFFFFFFFFFFFFFF << rem) & 0xFFFFFFFFFFFFFFFF)
        out[w] = live_words[w] & c
    return out


def kept_by_kernels(mask_words, mask_bits, n):
    """what the scoring kernels make of (row_mask, row_mask_bits): rows at and past mask_bits are kept (src/vec.rs:234)"""
    keep = np.ones(n, dtype=bool)
    m = min(mask_bits, n)
    bits = np.unpackbits(np.ascontiguousarray(mask_words).view(np.uint8), bitorder="little")[:m].astype(bool)
    keep[:m] = bits
    return keep


def test_effective_mask_rule_over_odd_bit_lengths():
    from otters_amd import _native as N
    rng = np.random.default_rng(7)
    for n in (1, 5, 63, 64, 65, 127, 128, 129, 1000, 4099):
        live = rng.random(n) < 0.8
        live_words = N.pack_bits(live).copy()
        if n & 63:  # the store's invariant: every bit at and past its length is 1
            live_words[-1] |= np.uint64((0xFFFFFFFFFFFFFFFF << (n & 63)) & 0xFFFFFFFFFFFFFFFF)
        for caller_bits in sorted({0, 1, n // 2, max(n - 1, 0), n, n + 1, n + 70, 63, 64, 65} - {-1}):
            caller = rng.random(caller_bits) < 0.5
            caller_words = N.pack_bits(caller)
            # rows the definition keeps: live AND (caller's bit, or keep where the caller's mask does not reach)
            want = live.copy()
            m = min(caller_bits, n)
            want[:m] &= caller[:m]
            if caller_bits == 0:  # an empty caller mask is no mask: the kernels get the live mask itself, n bits of it
                got = kept_by_kernels(live_words, n, n)
            else:
                if caller_words.size < (n + 63) // 64:  # the kernel never reads caller words at or past caller_bits
                    caller_words = np.concatenate([caller_words, rng.integers(0, 2**63, (n + 63) // 64 - caller_words.size, dtype=np.uint64)])
                got = kept_by_kernels(effective_words(live_words, caller_words, caller_bits, n), n, n)
            assert np.array_equal(got, want), (n, caller_bits)
