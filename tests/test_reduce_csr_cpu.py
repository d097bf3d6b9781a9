"""A * PMat from a sparse A (sdpsr_reduce_constraints_csr), host side: the C ABI entry is declared, exported and bound, and
the Python mirror rejects malformed input before it touches the library (no GPU needed, no context created)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

ENTRY = "sdpsr_reduce_constraints_csr"


def test_entry_declared_exported_and_bound(pkg):
    L = pkg._lib
    assert ENTRY in L.declared_symbols()
    lib = L.load_library()
    fn = getattr(lib, ENTRY)
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert lib.sdpsr_version() == 5
    assert C.sizeof(L.Opts) == 64 and L.Opts.reserved.offset == 52  # the feature needs no option
    hdr = (ROOT / "include" / "sdpsr.h").read_text()
    block = hdr[hdr.index("The same product for a sparse A given as CSR"):hdr.index("int sdpsr_reduce_constraints_csr")]
    for cite in ("README.md:57-60", "test/sd_problems.jl:32-37,113-118", "docs/src/examples/ReduceAndSolveJuMP.jl:42-51"):
        assert cite in block, cite
    assert "label exceeds d" in block
    assert callable(pkg.reduce_constraints_csr)


def test_malformed_input_raises_before_any_library_call(pkg, monkeypatch):
    created = []
    monkeypatch.setattr(pkg.api, "_ctx", lambda ctx: created.append(ctx) or pytest.fail("a context was asked for"))
    P = pkg.Partition(3, np.array([[1, 2, 0, 3]] * 4, dtype=np.uint32))  # 4 x 4: len = 16
    rp = np.array([0, 2, 3], dtype=np.int64)
    ci = np.array([1, 5, 15], dtype=np.int64)
    va = np.array([1.0, 2.0, 3.0])
    bad = [
        np.ones((2, 15)),                                # wrong column count, dense
        sp.csr_matrix((2, 17)),                          # wrong column count, sparse
        np.ones(15),                                     # wrong length of a vector
        (rp, ci, np.array([1.0, np.nan, 3.0])),          # non-finite value
        sp.csr_matrix(np.full((1, 16), np.inf)),         # non-finite value, sparse
        (np.array([0, 3, 2]), ci, va),                   # non-monotone rowptr
        (rp + 1, ci, va),                                # rowptr[0] != index_base
        (rp, np.array([1, 5, 16]), va),                  # column index >= len
    ]
    for A in bad:
        with pytest.raises(ValueError):
            pkg.reduce_constraints_csr(P, A)
    with pytest.raises(ValueError):
        pkg.reduce_constraints_csr(P, (rp, ci, va), index_base=2)
    with pytest.raises(ValueError):
        pkg.reduce_constraints_csr(pkg.Partition(17, P.matrix), (rp, ci, va))  # dim(P) > len
    assert created == []
