"""The sparse-constraints handle, host side (no GPU needed): the seven C ABI entries are declared, exported and bound; the
sequential reference of the canonical form (tests/sparse_handle_ref.py) agrees with ``csr_arrays`` and with SciPy;
``SparseConstraints`` rejects malformed shapes and dtypes before it needs a context; the host arithmetic of the device pass
(csrc/csr_canon.h: message precedence, radix bits, chunk counts, square root) as a g++-compiled program of its own."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_handle_ref as R
from conftest import ROOT

NEW_ENTRIES = {"sdpsr_sparse_create": 10, "sdpsr_sparse_destroy": 1, "sdpsr_sparse_info": 5, "sdpsr_sparse_export": 7,
               "sdpsr_admissible_setup_sparse": 13, "sdpsr_admissible_subspace_sparse": 11, "sdpsr_reduce_constraints_sparse": 6}


def test_entries_declared_exported_and_bound(pkg):
    L = pkg._lib
    declared = L.declared_symbols()
    lib = L.load_library()
    for name, nargs in NEW_ENTRIES.items():
        assert name in declared
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert lib.sdpsr_version() == 5
    hdr = (ROOT / "include" / "sdpsr.h").read_text()
    block = hdr[hdr.index("a device-resident sparse A"):hdr.index("int sdpsr_reduce_constraints_sparse")]
    for cite in ("src/partitions.jl:117-142", "src/utils.jl:58-66", "README.md:57-60", "docs/src/examples/ReduceAndSolveJuMP.jl:42-51"):
        assert cite in block
    assert "typedef struct sdpsr_sparse sdpsr_sparse;" in hdr
    assert hasattr(pkg, "SparseConstraints")


def test_reference_agrees_with_csr_arrays_and_scipy(pkg):
    for name, (len_, (rp, ci, va)) in R.canonical_cases().items():
        ref = R.canonical(len_, rp, ci, va)
        assert ref[0].size == rp.size and ref[0][-1] == ref[1].size == ref[2].size, name
        assert not np.any(ref[2] == 0.0), name
        assert R.bits_equal(R.canonical(len_, rp + 1, ci + 1, va, base=1), ref), name
        if R.max_run(rp, ci) < 8:  # (np.add.reduceat may sum longer runs pairwise)
            assert R.bits_equal(pkg.csr_arrays((rp, ci, va), len_), ref), name
            assert R.bits_equal(pkg.csr_arrays((rp + 1, ci + 1, va), len_, 1), ref), name
        if "sorted" in name or name in ("m0", "nnz0"):  # no duplicates: SciPy's canonical form is defined without an order
            m = rp.size - 1
            S = sp.csr_matrix((va, ci, rp), shape=(m, len_))
            S.sum_duplicates()
            S.eliminate_zeros()
            S.sort_indices()
            assert R.bits_equal((S.indptr, S.indices, S.data), ref), name
    # the canonical form is a fixed point
    len_, (rp, ci, va) = R.canonical_cases()["scan"]
    ref = R.canonical(len_, rp, ci, va)
    assert R.bits_equal(R.canonical(len_, *ref), ref)
    assert R.max_run(rp, ci) >= 2 and ref[1].size < ci.size
    # the order-sensitive sums: 1.0 survives at column 4, column 9 is dropped
    len_, (rp, ci, va) = R.canonical_cases()["order_sensitive"]
    ref = R.canonical(len_, rp, ci, va)
    assert list(ref[1]) == [4, 0] and list(ref[2]) == [1.0, 1.0]


def test_reference_messages_and_precedence():
    rp = np.array([0, 2, 3, 5], dtype=np.int64)
    ci = np.array([1, 5, 15, 2, 3], dtype=np.int64)
    va = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    R.canonical(16, rp, ci, va)

    def msg(*a, **k):
        with pytest.raises(ValueError) as e:
            R.canonical(16, *a, **k)
        return str(e.value)

    assert msg(rp + 1, ci, va) == "rowptr[0] != index_base"
    assert msg(np.array([0, 3, 2, 1]), ci, va) == "rowptr is not monotone at row 1"
    assert msg(rp, np.array([1, 16, 15, -1, 3]), va) == "column index out of [0, n^2) at entry 1"
    assert msg(rp, np.array([1, 5, 16, 2, 3]), np.array([1.0, np.nan, 3.0, 4.0, 5.0])) == "non-finite value at entry 1"
    assert msg(rp, np.array([1, 16, 15, 2, 3]), np.array([1.0, 2.0, np.inf, 4.0, 5.0])) == "column index out of [0, n^2) at entry 1"
    assert msg(rp, np.array([1, 16, 15, 2, 3]), np.array([1.0, np.nan, 3.0, 4.0, 5.0])) == "column index out of [0, n^2) at entry 1"
    assert msg(rp, np.array([1, 1, 15, 2, 3]), np.array([1e308, 1e308, 3.0, 4.0, 5.0])) == "duplicate entries sum to a non-finite value"
    assert msg(rp, ci, va, base=2) == "index_base must be 0 or 1"


def test_reference_symmetry_predicate():
    for name, (len_, (rp, ci, va), expect) in R.symmetry_cases().items():
        assert R.rows_symmetric(len_, *R.canonical(len_, rp, ci, va)) is expect, name


def test_sparse_constraints_rejects_malformed_input_before_any_context(pkg):
    rp = np.array([0, 2, 3], dtype=np.int64)
    ci = np.array([1, 5, 15], dtype=np.int64)
    va = np.array([1.0, 2.0, 3.0])

    class NoContext:  # any use of the context would raise AttributeError, not ValueError
        pass

    bad = [
        ((rp, ci), 0),                                       # not three arrays
        ((rp.astype(np.float64), ci, va), 0),                # rowptr not integer
        ((rp, ci.astype(np.float64), va), 0),                # colind not integer
        ((rp.reshape(1, -1), ci, va), 0),                    # rowptr not a vector
        ((np.zeros(0, dtype=np.int64), ci, va), 0),          # empty rowptr
        ((rp, ci.reshape(1, -1), va), 0),                    # colind not a vector
        ((rp, ci[:2], va), 0),                               # length mismatch
        ((rp, ci, va), 2),                                   # bad base
        (np.ones((2, 15)), 0),                               # dense, wrong width
        (np.ones(16), 0),                                    # dense, not 2-D
        (sp.csr_matrix((2, 15)), 0),                         # SciPy, wrong width
    ]
    for A, base in bad:
        with pytest.raises(ValueError):
            pkg.SparseConstraints(A, 16, ctx=NoContext(), index_base=base)


SRC = r'''
#include <cstdio>
#include "csr_canon.h"
using namespace sdpsr;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)
int main() {
    static_assert(sizeof(CanonVerdict) == 72, "nine 64-bit words");
    CanonVerdict v{};
    v.bad_row = v.bad_col = v.bad_val = CANON_NO_INDEX;
    CHECK(canon_validation_message(v).empty());
    // the flags that are no validation failure leave the message empty
    v.unsorted = v.asymmetric = v.dup_nonfinite = 1;
    v.total = 5;
    CHECK(canon_validation_message(v).empty());
    // precedence: rowptr[0], the monotone check, the length, then the lowest entry -- the column at equal p
    v.bad_col = 7;
    v.bad_val = 9;
    CHECK(canon_validation_message(v) == "column index out of [0, n^2) at entry 7");
    v.bad_val = 7;
    CHECK(canon_validation_message(v) == "column index out of [0, n^2) at entry 7");
    v.bad_val = 6;
    CHECK(canon_validation_message(v) == "non-finite value at entry 6");
    v.bad_col = CANON_NO_INDEX;
    CHECK(canon_validation_message(v) == "non-finite value at entry 6");
    v.bad_val = 0;
    v.bad_col = 0;
    CHECK(canon_validation_message(v) == "column index out of [0, n^2) at entry 0");
    v.nnz_mismatch = 1;
    CHECK(canon_validation_message(v) == "rowptr[m] - index_base != nnz");
    v.bad_row = 4294967296ull;
    CHECK(canon_validation_message(v) == "rowptr is not monotone at row 4294967296");
    v.bad_row = 0;
    CHECK(canon_validation_message(v) == "rowptr is not monotone at row 0");
    v.rowptr0_bad = 1;
    CHECK(canon_validation_message(v) == "rowptr[0] != index_base");
    // radix bits: keys 0 .. count - 1 fit, never zero passes
    CHECK(canon_sort_bits(0) == 1 && canon_sort_bits(1) == 1 && canon_sort_bits(2) == 1 && canon_sort_bits(3) == 2 && canon_sort_bits(4) == 2);
    CHECK(canon_sort_bits(16) == 4 && canon_sort_bits(17) == 5 && canon_sort_bits(2304) == 12 && canon_sort_bits(16777216) == 24);
    CHECK(canon_sort_bits(0xFFFFFFF0ull) == 32 && canon_sort_bits(0x7FFFFFFFull) == 31);
    for (uint64_t c = 1; c < 5000; ++c) CHECK(((uint64_t)1 << canon_sort_bits(c)) >= c && (canon_sort_bits(c) == 1 || ((uint64_t)1 << (canon_sort_bits(c) - 1)) < c));
    // chunks
    CHECK(canon_chunks(0) == 0 && canon_chunks(-3) == 0 && canon_chunks(1) == 1 && canon_chunks(2048) == 1 && canon_chunks(2049) == 2);
    CHECK(canon_chunks(3 * 2048 + 17) == 4 && canon_chunks(((int64_t)1 << 32) - 1) == (1 << 21));
    // perfect squares
    CHECK(canon_square_root(0) == 0 && canon_square_root(1) == 1 && canon_square_root(2) == 0 && canon_square_root(15) == 0 && canon_square_root(16) == 4);
    CHECK(canon_square_root(49) == 7 && canon_square_root(4096ll * 4096) == 4096 && canon_square_root(4096ll * 4096 - 1) == 0);
    CHECK(canon_square_root(65535ll * 65535) == 65535 && canon_square_root(65535ll * 65535 + 1) == 0 && canon_square_root(0xFFFFFFEFll) == 0);
    for (int64_t n = 1; n < 300; ++n) {
        CHECK(canon_square_root(n * n) == n);
        CHECK(canon_square_root(n * n + 1) == 0 || n * n + 1 == (n + 1) * (n + 1));
    }
    std::printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
'''


def test_csr_canon_header_as_a_program():
    inc = ROOT / "sdpsymmetryreduction.jl_amd" / "csrc"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "t.cpp"), os.path.join(tmp, "t")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-Wall", "-Werror", f"-I{inc}", src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
