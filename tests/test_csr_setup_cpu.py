"""Setup from a sparse A (CSR), host side: the C ABI entries and the Python converter (no GPU needed)."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

NEW_ENTRIES = ("sdpsr_admissible_setup_csr", "sdpsr_admissible_subspace_csr")


def test_entries_declared_exported_and_bound(pkg):
    L = pkg._lib
    declared = L.declared_symbols()
    lib = L.load_library()
    for name in NEW_ENTRIES:
        assert name in declared
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) in (15, 17)
    assert lib.sdpsr_version() == 5
    hdr = (ROOT / "include" / "sdpsr.h").read_text()
    block = hdr[hdr.index("setup from a sparse constraint matrix"):hdr.index("int sdpsr_admissible_subspace_csr")]
    assert "src/partitions.jl:117-142" in block and "src/utils.jl:58-66" in block
    assert re.search(r"SDPSR_SETUP_MGS\s*=\s*2", hdr) and L.SETUP_MGS == 2 and L.SETUP_CHOLESKY_QR2 == 1


def _qap_like(n=3, seed=0):
    """A few sparse rows over n^2 x n^2 entries, with repeated columns across rows."""
    rng = np.random.default_rng(seed)
    N2 = (n * n) ** 2
    A = sp.random(5, N2, density=0.05, random_state=rng, format="csr")
    A.data = np.round(A.data * 8) - 3  # integers, some zeros
    return A


def _canon(A, N2):
    A = sp.csr_matrix(A, copy=True)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data


def test_converter_canonical_for_every_input_form(pkg):
    A = _qap_like()
    N2 = A.shape[1]
    ref = _canon(A, N2)
    forms = [A, A.tocoo(), A.tocsc(), A.toarray(), sp.lil_matrix(A)]
    # explicit zeros, duplicates and unsorted columns in a raw COO
    coo = A.tocoo()
    r, c, v = list(coo.row), list(coo.col), list(coo.data)
    r += [0, 2, 2]
    c += [int(coo.col[0]), 7, 7]
    v += [0.0, 1.5, -1.5]  # a zero, and a duplicated pair that cancels
    perm = np.random.default_rng(3).permutation(len(r))
    forms.append(sp.coo_matrix((np.array(v)[perm], (np.array(r)[perm], np.array(c)[perm])), shape=A.shape))
    for f in forms:
        got = pkg.csr_arrays(f, N2)
        for g, e in zip(got, ref):
            assert np.array_equal(g, e), type(f)
        assert got[0].dtype == got[1].dtype == np.int64 and got[2].dtype == np.float64
    # raw CSR tuples: 0- and 1-based, unsorted columns, duplicated entries, explicit zeros
    rp, ci, va = ref
    assert all(np.array_equal(g, e) for g, e in zip(pkg.csr_arrays((rp, ci, va), N2, 0), ref))
    assert all(np.array_equal(g, e) for g, e in zip(pkg.csr_arrays((rp + 1, ci + 1, va), N2, 1), ref))
    rows = []
    for i in range(len(rp) - 1):
        cols, vals = list(ci[rp[i]:rp[i + 1]]), list(va[rp[i]:rp[i + 1]])
        if cols:  # split the first value into a duplicated pair, add an explicit zero, reverse the row
            cols = cols + [cols[0], int(cols[-1])]
            vals = [vals[0] / 2] + vals[1:] + [vals[0] / 2, 0.0]
            # (an explicit zero on a present column adds nothing)
        rows.append((cols[::-1], vals[::-1]))
    rp2 = np.concatenate([[0], np.cumsum([len(cc) for cc, _ in rows])]).astype(np.int64)
    ci2 = np.array([x for cc, _ in rows for x in cc], dtype=np.int64)
    va2 = np.array([x for _, vv in rows for x in vv])
    got = pkg.csr_arrays((rp2, ci2, va2), N2, 0)
    assert np.array_equal(got[0], rp) and np.array_equal(got[1], ci) and np.allclose(got[2], va, rtol=0, atol=0)


def test_converter_rejects_malformed_input(pkg):
    N2 = 16
    rp = np.array([0, 2, 3], dtype=np.int64)
    ci = np.array([1, 5, 15], dtype=np.int64)
    va = np.array([1.0, 2.0, 3.0])
    pkg.csr_arrays((rp, ci, va), N2)  # well-formed
    bad = [
        ((rp + 1, ci, va), 0),                              # rowptr[0] != base
        ((np.array([0, 3, 2]), ci, va), 0),                 # non-monotone
        ((rp, np.array([1, 5, 16]), va), 0),                # index out of range
        ((rp, np.array([1, -1, 3]), va), 0),                # negative index
        ((rp + 1, np.array([0, 5, 15]), va), 1),            # 1-based with a 0 index
        ((rp, ci, np.array([1.0, np.nan, 3.0])), 0),        # NaN
        ((rp, ci, np.array([1.0, np.inf, 3.0])), 0),        # inf
        ((rp, ci[:2], va), 0),                              # length mismatch
        ((rp, ci, va), 2),                                  # bad base
    ]
    for A, base in bad:
        with pytest.raises(ValueError):
            pkg.csr_arrays(A, N2, base)
    with pytest.raises(ValueError):
        pkg.csr_arrays(np.ones((2, 15)), N2)  # wrong width
    with pytest.raises(ValueError):
        pkg.csr_arrays(sp.csr_matrix(np.full((1, 16), np.nan)), N2)
    # the public entry rejects before any call into the library (no GPU here)
    with pytest.raises(ValueError):
        pkg.admissible_setup_csr(np.zeros(16), (rp, np.array([1, 5, 99]), va), np.zeros(2))
    with pytest.raises(ValueError):
        pkg.admissible_subspace(np.zeros(16), (rp, ci, va), np.zeros(3), csr_setup=True)  # len(b) != m
    with pytest.raises(ValueError):
        pkg.admissible_subspace(np.zeros(15), sp.csr_matrix((2, 15)), np.zeros(2), csr_setup=True)  # n^2 != len(C)
