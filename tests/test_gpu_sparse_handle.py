"""The sparse-constraints handle on the device (sdpsr_sparse_create / _info / _export, sdpsr_admissible_setup_sparse /
_subspace_sparse, sdpsr_reduce_constraints_sparse): the canonical arrays against the sequential reference of
tests/sparse_handle_ref.py and against ``csr_arrays``, the symmetry verdict, the messages of malformed input, and the
outputs of the setup stage and of the assembly through a handle against the existing _csr entries -- every equality on
the raw bits (``view(np.uint64)`` for doubles)."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_handle_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

ATOL = math.sqrt(np.finfo(np.float64).eps)
CASES = R.canonical_cases()
SYM_CASES = R.symmetry_cases()


def _p(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _create(ctx, len_, rp, ci, va, base=0, device=False, nnz=None):
    """(status, handle or None, message, kept) -- ``kept``: the arrays the call read (device: the three tensors)."""
    rp, ci, va = (np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int64), np.ascontiguousarray(va, dtype=np.float64))
    kept = (rp, ci, va)
    if device:
        import torch
        kept = tuple(torch.from_numpy(a).cuda() for a in kept)
        torch.cuda.synchronize()
    h = C.c_void_p()
    st = ctx._lib.sdpsr_sparse_create(ctx._h, len_, rp.size - 1, ci.size if nnz is None else nnz, _p(kept[0]), _p(kept[1]), _p(kept[2]), base,
                                      1 if device else 0, C.byref(h))
    return st, (h if h.value else None), ctx._lib.sdpsr_last_error(ctx._h).decode(), kept


def _info(ctx, h):
    ln, m, nz, sym = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
    assert ctx._lib.sdpsr_sparse_info(h, C.byref(ln), C.byref(m), C.byref(nz), C.byref(sym)) == 0
    return ln.value, m.value, nz.value, sym.value


def _export(ctx, h, base=0, device=False):
    _, m, nz, _ = _info(ctx, h)
    if device:
        import torch
        rp = torch.full((m + 1,), -7, dtype=torch.int64, device="cuda")
        ci = torch.full((nz,), -7, dtype=torch.int64, device="cuda")
        va = torch.full((nz,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    else:
        rp, ci, va = np.full(m + 1, -7, dtype=np.int64), np.full(nz, -7, dtype=np.int64), np.full(nz, np.nan)
    assert ctx._lib.sdpsr_sparse_export(ctx._h, h, base, _p(rp), _p(ci), _p(va), 1 if device else 0) == 0
    if device:
        rp, ci, va = (t.cpu().numpy() for t in (rp, ci, va))
    return rp, ci, va


def _destroy(ctx, h):
    assert ctx._lib.sdpsr_sparse_destroy(h) == 0


# ------------------------------------------------------------------ the canonical form
@pytest.fixture(scope="module")
def references():
    """The sequential reference of every case, computed once."""
    return {name: R.canonical(len_, *arrs) for name, (len_, arrs) in CASES.items()}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_canonical_form_equals_the_reference(pkg, gpu_ctx, references, name, device):
    len_, (rp, ci, va) = CASES[name]
    ref = references[name]
    short = R.max_run(rp, ci) < 8
    for base in (0, 1):
        st, h, msg, _ = _create(gpu_ctx, len_, rp + base, ci + base, va, base, device)
        assert st == 0 and h is not None, msg
        try:
            ln, m, nz, _ = _info(gpu_ctx, h)
            assert (ln, m, nz) == (len_, rp.size - 1, ref[1].size)
            got = _export(gpu_ctx, h, 0, device)
            assert R.bits_equal(got, ref), (name, base)
            if short:
                assert R.bits_equal(got, pkg.csr_arrays((rp + base, ci + base, va), len_, base)), (name, base)
        finally:
            _destroy(gpu_ctx, h)


def test_sort_route_and_no_sort_route_agree(gpu_ctx, references):
    """Rows already sorted take the route without a sort; one swapped pair forces the sort on the same matrix."""
    assert R.bits_equal(references["sorted"], references["one_swapped_pair"])
    got = []
    for name in ("sorted", "one_swapped_pair"):
        len_, (rp, ci, va) = CASES[name]
        st, h, msg, _ = _create(gpu_ctx, len_, rp, ci, va)
        assert st == 0, msg
        got.append(_export(gpu_ctx, h))
        _destroy(gpu_ctx, h)
    assert R.bits_equal(got[0], got[1]) and R.bits_equal(got[0], references["sorted"])


def test_order_sensitive_duplicates(gpu_ctx):
    len_, (rp, ci, va) = CASES["order_sensitive"]
    st, h, msg, _ = _create(gpu_ctx, len_, rp, ci, va)
    assert st == 0, msg
    rp2, ci2, va2 = _export(gpu_ctx, h)
    _destroy(gpu_ctx, h)
    assert list(rp2) == [0, 1, 2, 2] and list(ci2) == [4, 0] and list(va2) == [1.0, 1.0]


def test_device_arrays_are_read_only_and_not_aliased(gpu_ctx, references):
    import torch
    len_, (rp, ci, va) = CASES["scan"]
    st, h, msg, kept = _create(gpu_ctx, len_, rp, ci, va, 0, device=True)
    assert st == 0, msg
    try:
        for t, a in zip(kept, (rp, ci, va)):
            assert np.array_equal(t.cpu().numpy().view(np.uint64), a.view(np.uint64))  # unchanged by the pass
        for t in kept:
            t.zero_()
        torch.cuda.synchronize()
        assert R.bits_equal(_export(gpu_ctx, h), references["scan"])
    finally:
        _destroy(gpu_ctx, h)


def test_unaligned_device_arrays(gpu_ctx, references):
    """Caller's device pointers that are 8- but not 16-byte aligned take the one-by-one loads."""
    import torch
    len_, (rp, ci, va) = CASES["scan"]
    tci = torch.zeros(ci.size + 1, dtype=torch.int64, device="cuda")
    tva = torch.zeros(va.size + 1, dtype=torch.float64, device="cuda")
    tci[1:] = torch.from_numpy(ci).cuda()
    tva[1:] = torch.from_numpy(va).cuda()
    trp = torch.from_numpy(rp).cuda()
    torch.cuda.synchronize()
    assert tci[1:].data_ptr() % 16 == 8
    h = C.c_void_p()
    st = gpu_ctx._lib.sdpsr_sparse_create(gpu_ctx._h, len_, rp.size - 1, ci.size, _p(trp), _p(tci[1:]), _p(tva[1:]), 0, 1, C.byref(h))
    assert st == 0
    try:
        assert R.bits_equal(_export(gpu_ctx, h), references["scan"])
    finally:
        _destroy(gpu_ctx, h)


# ------------------------------------------------------------------ info and export
def test_info_export_and_reimport(gpu_ctx, references):
    len_, (rp, ci, va) = CASES["scan"]
    st, h, msg, _ = _create(gpu_ctx, len_, rp, ci, va)
    assert st == 0, msg
    e0, e1 = _export(gpu_ctx, h, 0), _export(gpu_ctx, h, 1)
    ln, m, nz, _ = _info(gpu_ctx, h)
    _destroy(gpu_ctx, h)
    assert e0[0].size == m + 1 and e0[1].size == e0[2].size == nz == e0[0][-1]
    assert np.array_equal(e1[0], e0[0] + 1) and np.array_equal(e1[1], e0[1] + 1) and np.array_equal(_bits(e1[2]), _bits(e0[2]))
    for base, arrs in ((0, e0), (1, e1)):  # the exported arrays reproduce themselves
        st, h2, msg, _ = _create(gpu_ctx, len_, *arrs, base)
        assert st == 0, msg
        assert R.bits_equal(_export(gpu_ctx, h2, 0), e0)
        assert _info(gpu_ctx, h2)[:3] == (ln, m, nz)
        _destroy(gpu_ctx, h2)


# ------------------------------------------------------------------ the symmetry verdict
@pytest.mark.parametrize("name", sorted(SYM_CASES))
def test_symmetry_verdict(gpu_ctx, name):
    len_, (rp, ci, va), expect = SYM_CASES[name]
    assert R.rows_symmetric(len_, *R.canonical(len_, rp, ci, va)) is expect
    for device in (False, True):
        st, h, msg, _ = _create(gpu_ctx, len_, rp, ci, va, 0, device)
        assert st == 0, msg
        sym = _info(gpu_ctx, h)[3]
        _destroy(gpu_ctx, h)
        assert sym == int(expect), (name, device)


# ------------------------------------------------------------------ malformed input
def _malformed():
    rp = np.array([0, 3, 5, 8], dtype=np.int64)
    ci = np.array([1, 5, 15, 2, 3, 0, 7, 9], dtype=np.int64)
    va = np.arange(1.0, 9.0)

    def mod(a, idx, x):
        a = a.copy()
        a[idx] = x
        return a

    nan_lo, col_hi = mod(va, 2, np.nan), mod(ci, 6, 16)
    col_lo, nan_hi = mod(ci, 2, -1), mod(va, 6, np.inf)
    return 16, (rp, ci, va), [
        ("bad rowptr[0]", (mod(rp, 0, 1), ci, va), 0, None, "rowptr[0] != index_base"),
        ("rowptr[0] against base 1", (rp, ci, va), 1, None, "rowptr[0] != index_base"),
        ("non-monotone at two rows", (np.array([0, 5, 3, 8, 6, 8]), ci, va), 0, None, "rowptr is not monotone at row 1"),
        ("two columns out of range", (rp, mod(mod(ci, 3, 16), 6, 99), va), 0, None, "column index out of [0, n^2) at entry 3"),
        ("negative column", (rp, mod(ci, 4, -1), va), 0, None, "column index out of [0, n^2) at entry 4"),
        ("NaN below a bad column", (rp, col_hi, nan_lo), 0, None, "non-finite value at entry 2"),
        ("bad column below an inf", (rp, col_lo, nan_hi), 0, None, "column index out of [0, n^2) at entry 2"),
        ("both at one entry", (rp, mod(ci, 5, 16), mod(va, 5, np.nan)), 0, None, "column index out of [0, n^2) at entry 5"),
        ("duplicates overflow", (rp, mod(ci, 1, 1), mod(mod(va, 0, 1e308), 1, 1e308)), 0, None, "duplicate entries sum to a non-finite value"),
        ("nnz too small", (rp, ci, va), 0, 7, "rowptr[m] - index_base != nnz"),
        ("index_base 2", (rp, ci, va), 2, None, "index_base must be 0 or 1"),
    ]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_malformed_input_messages_and_ctx_stays_usable(pkg, problems, device):
    len_, good, bad = _malformed()
    Cv, A, b = problems.theta_prime_problem(problems.petersen_adjacency())
    with pkg.Context(seed=1) as ctx:
        for what, arrs, base, nnz, message in bad:
            st, h, msg, _ = _create(ctx, len_, *arrs, base, device, nnz)
            assert st == 5 and h is None, what
            assert msg.endswith(message), (what, msg)
            with pytest.raises(ValueError):  # the reference refuses the same input (an explicit nnz is the handle's alone)
                R.canonical(len_, arrs[0], arrs[1][:nnz], arrs[2][:nnz], base)
        st, h, msg, _ = _create(ctx, len_, *good, 0, device)
        assert st == 0 and h is not None, msg
        assert R.bits_equal(_export(ctx, h), R.canonical(len_, *good))
        _destroy(ctx, h)
        with pkg.SparseConstraints(A, 100, ctx=ctx) as S:
            assert pkg.admissible_setup_csr(Cv, S, b, ctx=ctx).hint == 3
        with pytest.raises(ValueError, match="column index out of"):
            pkg.SparseConstraints((good[0], good[1] + 9, good[2]), 16, ctx=ctx)


# ------------------------------------------------------------------ the setup stage through a handle
def _problem(problems, name):
    if name == "petersen":
        return problems.theta_prime_problem(problems.petersen_adjacency())
    if name.startswith("er"):
        return problems.theta_prime_problem(problems.er_graph_adjacency(int(name[2:])))
    if name == "esc16j":
        fa, fb = problems.read_qapdata(ROOT / "tests" / "golden" / "esc16j.dat")
        return problems.qap_problem(fa, fb)
    raise KeyError(name)


def _vec(Cv):
    return np.ascontiguousarray(np.asarray(Cv, dtype=np.float64).reshape(-1))


def _raw(A):
    A = sp.csr_matrix(A)
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(A.data, dtype=np.float64)


def _shuffled_with_duplicates(rp, ci, va):
    """Every row reversed, its first value split into two halves (exact) and an explicit zero added."""
    rp2, ci2, va2 = [0], [], []
    for i in range(rp.size - 1):
        cols, vals = list(ci[rp[i]:rp[i + 1]]), list(va[rp[i]:rp[i + 1]])
        if cols:
            cols = cols + [cols[0], cols[-1]]
            vals = [vals[0] / 2] + vals[1:] + [vals[0] / 2, 0.0]
        ci2 += cols[::-1]
        va2 += vals[::-1]
        rp2.append(len(ci2))
    return np.array(rp2, dtype=np.int64), np.array(ci2, dtype=np.int64), np.array(va2, dtype=np.float64)


def _setup_case(problems, name):
    if name == "esc16j_rank_deficient":  # (MGS path)
        Cv, A, b = _problem(problems, "esc16j")
        A = sp.csr_matrix(A)
        return Cv, _raw(sp.vstack([A, A[0], A[1] + A[2]], format="csr")), np.concatenate([b, [b[0], b[1] + b[2]]])
    if name == "er5_non_symmetric":  # (hint 0)
        Cv, A, b = _problem(problems, "er5")
        n = math.isqrt(_vec(Cv).size)
        extra = sp.csr_matrix(([1.0], ([0], [1 + 4 * n])), shape=(1, n * n))  # entry (1, 4) without (4, 1)
        return Cv, _raw(sp.vstack([sp.csr_matrix(A), extra], format="csr")), np.concatenate([b, [0.0]])
    if name == "esc16j_shuffled":
        Cv, A, b = _problem(problems, "esc16j")
        return Cv, _shuffled_with_duplicates(*_raw(A)), b
    Cv, A, b = _problem(problems, name)
    return Cv, _raw(A), b


def _setup_outputs(ctx, n, m, b, c, call):
    ln = n * n
    CL, X0 = np.full(ln, np.nan), np.full(ln, np.nan)
    U = np.zeros((ln, max(m, 1)), order="F")
    r, hint, info = C.c_int64(-1), C.c_int(-1), C.c_int32(-1)
    st = call(_p(b), _p(c), ATOL, _p(CL), _p(X0), _p(U), C.byref(r), C.byref(hint), C.byref(info), 0)
    assert st == 0, ctx._lib.sdpsr_last_error(ctx._h).decode()
    return _bits(CL), _bits(X0), _bits(U[:, :r.value]), r.value, hint.value, info.value


SETUP_EXPECT = {"petersen": (1, 3), "er5": (1, 3), "esc16j": (1, 3), "esc16j_rank_deficient": (2, 3), "er5_non_symmetric": (None, 0),
                "esc16j_shuffled": (1, 3)}  # (sdpsr_setup_path or None = whichever, hint)


@pytest.mark.parametrize("name", sorted(SETUP_EXPECT))
def test_setup_through_the_handle_equals_the_csr_entry_bit_for_bit(pkg, problems, name):
    Cv, (rp, ci, va), b = _setup_case(problems, name)
    c = _vec(Cv)
    n = math.isqrt(c.size)
    m = rp.size - 1
    b = np.ascontiguousarray(b, dtype=np.float64)
    with pkg.Context(seed=1) as ctx:
        lib = ctx._lib
        ref = _setup_outputs(ctx, n, m, b, c, lambda *a: lib.sdpsr_admissible_setup_csr(ctx._h, n, m, _p(rp), _p(ci), _p(va), 0, *a))
        for device in (False, True):
            st, h, msg, _ = _create(ctx, n * n, rp, ci, va, 0, device)
            assert st == 0, msg
            got = _setup_outputs(ctx, n, m, b, c, lambda *a: lib.sdpsr_admissible_setup_sparse(ctx._h, n, h, *a))
            sym = _info(ctx, h)[3]
            _destroy(ctx, h)
            for g, e in zip(got[:3], ref[:3]):
                assert np.array_equal(g, e)
            assert got[3:] == ref[3:]
            assert got[4] == SETUP_EXPECT[name][1] == 3 * sym
            assert SETUP_EXPECT[name][0] in (None, got[5])


@pytest.mark.parametrize("name,width", [("petersen", 32), ("er3", 32), ("er5", 32), ("er7", 32), ("esc16j", 32), ("esc16j", 16)])
def test_golden_partitions_through_a_handle(pkg, problems, golden, name, width):
    Cv, A, b = _problem(problems, name)
    with pkg.Context(seed=1, label_width=width) as ctx:
        with pkg.SparseConstraints(A, _vec(Cv).size, ctx=ctx) as S:
            assert (S.m, S.len, S.rows_symmetric) == (A.shape[0], A.shape[1], True)
            P = pkg.admissible_subspace(Cv, S, b, ctx=ctx)
    assert P.matrix.dtype == np.dtype(f"uint{width}")
    assert P.nparts == int(golden[f"{name}_P"].max())
    assert np.array_equal(P.matrix, golden[f"{name}_P"])


# ------------------------------------------------------------------ the assembly through a handle
def _assembly_case(problems, golden, name):
    if name == "esc16j":
        _, A, _ = _problem(problems, "esc16j")
        L = golden["esc16j_P"]
        return _raw(A), np.ascontiguousarray(L.reshape(-1, order="F"), dtype=np.uint32), int(L.max())
    if name == "grid_qap_5x6":
        flow, dist = problems.grid_qap_instance(5, 6, seed=4, symmetric_flow=True)
        _, A, _ = problems.qap_problem(flow, dist)
        ln = A.shape[1]
        d = 1000
        return _raw(A), (np.random.default_rng(3).integers(0, d + 1, size=ln)).astype(np.uint32), d
    if name == "vector":  # C' * PMat: m = 1
        Cv, _, _ = _problem(problems, "esc16j")
        L = golden["esc16j_P"]
        rng = np.random.default_rng(5)
        c = _vec(Cv) + rng.standard_normal(L.size) * (rng.random(L.size) < 0.3)
        return _raw(sp.csr_matrix(c.reshape(1, -1))), np.ascontiguousarray(L.reshape(-1, order="F"), dtype=np.uint32), int(L.max())
    raise KeyError(name)


@pytest.mark.parametrize("name", ["esc16j", "grid_qap_5x6", "vector"])
def test_assembly_through_the_handle_equals_the_csr_entry_bit_for_bit(pkg, problems, golden, gpu_ctx, name):
    import torch
    (rp, ci, va), lab, d = _assembly_case(problems, golden, name)
    ctx, lib = gpu_ctx, gpu_ctx._lib
    ln, m = lab.size, rp.size - 1
    ref = np.full((m, d), np.nan, order="F")
    assert lib.sdpsr_reduce_constraints_csr(ctx._h, ln, _p(lab), d, m, _p(rp), _p(ci), _p(va), 0, _p(ref), 0) == 0
    st, h, msg, _ = _create(ctx, ln, rp, ci, va)
    assert st == 0, msg
    try:
        out = np.full((m, d), np.nan, order="F")
        assert lib.sdpsr_reduce_constraints_sparse(ctx._h, h, _p(lab), d, _p(out), 0) == 0
        assert np.array_equal(_bits(out), _bits(ref))
        tl = torch.from_numpy(lab.view(np.int32)).cuda()
        to = torch.full((m * d,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert lib.sdpsr_reduce_constraints_sparse(ctx._h, h, _p(tl), d, _p(to), 1) == 0
        assert np.array_equal(_bits(to.cpu().numpy()), _bits(ref.reshape(-1, order="F")))
        if d > 1:  # a label above d is refused, and named as before
            assert lib.sdpsr_reduce_constraints_sparse(ctx._h, h, _p(lab), d - 1, _p(out), 0) == 5
            assert "a label exceeds d" in lib.sdpsr_last_error(ctx._h).decode()
    finally:
        _destroy(ctx, h)


def test_python_dispatch(pkg, problems, golden, gpu_ctx):
    """``reduce_constraints_csr`` and ``admissible_setup_csr`` with a SparseConstraints equal the same calls with A itself."""
    Cv, A, b = _problem(problems, "esc16j")
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.eliminate_zeros()
    P = pkg.Partition(int(golden["esc16j_P"].max()), golden["esc16j_P"])
    ref = pkg.reduce_constraints_csr(P, A, ctx=gpu_ctx)
    Sref = pkg.admissible_setup_csr(Cv, A, b, ctx=gpu_ctx)
    import torch
    Ad = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int32)), torch.from_numpy(A.indices.astype(np.int32)),
                                 torch.from_numpy(A.data.astype(np.float64)), size=A.shape).cuda()
    forms = [A, _raw(A), Ad, (Ad.crow_indices(), Ad.col_indices(), Ad.values())]
    for form in forms:
        with pkg.SparseConstraints(form, A.shape[1], ctx=gpu_ctx) as S:
            assert S.nnz == A.nnz and S.m == A.shape[0] and S.rows_symmetric
            assert R.bits_equal(S.arrays(), pkg.csr_arrays(A, A.shape[1]))
            dev = S.arrays(index_base=1, device=True)
            assert R.bits_equal(tuple(t.cpu().numpy() - k for t, k in zip(dev, (1, 1, 0))), S.arrays())
            assert np.array_equal(_bits(pkg.reduce_constraints_csr(P, S)), _bits(ref))
            Sg = pkg.admissible_setup_csr(Cv, S, b)
            assert Sg.hint == Sref.hint and Sg.info == Sref.info
            for g, e in zip(Sg[1:], Sref[1:]):
                assert torch.equal(g.contiguous().view(torch.int64), e.contiguous().view(torch.int64))


# ------------------------------------------------------------------ one handle, two consumers, one upload
def test_one_upload_two_consumers_and_a_second_ctx(pkg, problems, golden):
    Cv, A, b = _problem(problems, "esc16j")
    rp, ci, va = _shuffled_with_duplicates(*_raw(A))
    c = _vec(Cv)
    n = math.isqrt(c.size)
    ln, m, nnz = c.size, rp.size - 1, ci.size
    b = np.ascontiguousarray(b, dtype=np.float64)
    L = golden["esc16j_P"]
    lab, d = np.ascontiguousarray(L.reshape(-1, order="F"), dtype=np.uint32), int(L.max())
    bytes_of_a = (m + 1) * 8 + nnz * 16
    with pkg.Context(seed=1) as ctx, pkg.Context(seed=99) as other:
        lib = ctx._lib
        up0 = ctx.transfer_bytes()[0]
        st, h, msg, _ = _create(ctx, ln, rp, ci, va)
        assert st == 0, msg
        up1 = ctx.transfer_bytes()[0]
        assert up1 - up0 == bytes_of_a
        outs = []
        for cx in (ctx, other):
            u0 = cx.transfer_bytes()[0]
            got = _setup_outputs(cx, n, m, b, c, lambda *a: lib.sdpsr_admissible_setup_sparse(cx._h, n, h, *a))
            u1 = cx.transfer_bytes()[0]
            # C, and the m x m factors and pivots of CholeskyQR2 (b is used on the host): not a byte of A
            assert ln * 8 <= u1 - u0 <= ln * 8 + 2 * m * m * 8 + m * 4 + m * 8
            out = np.full((m, d), np.nan, order="F")
            assert lib.sdpsr_reduce_constraints_sparse(cx._h, h, _p(lab), d, _p(out), 0) == 0
            assert cx.transfer_bytes()[0] - u1 == ln * 4  # its labels
            outs.append(got + (_bits(out),))
        _destroy(ctx, h)
        for g, e in zip(outs[0], outs[1]):
            assert np.array_equal(g, e)
        # device arrays: nothing goes up
        up2 = ctx.transfer_bytes()[0]
        st, h, msg, _ = _create(ctx, ln, rp, ci, va, 0, device=True)
        assert st == 0, msg
        assert ctx.transfer_bytes()[0] == up2
        _destroy(ctx, h)
