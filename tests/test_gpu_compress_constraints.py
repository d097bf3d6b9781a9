"""sdpsr_compress_constraints through the C ABI and its Python mirror (compress_constraints, reduced_sdp): the rows of
svd([A * PMat, b]').U[:, 1:rank]' (docs/src/examples/ReduceAndSolveJuMP.jl:44-50), compared with LAPACK on invariants
(compress_ref.py) -- repeated singular values leave a rotation free, so never entry by entry."""
import ctypes as C

import numpy as np
import pytest

import compress_ref as R

pytestmark = pytest.mark.gpu

NAMES = ["graded_6x37", "graded_7x4097", "integer_9x5", "duplicates_6x70", "esc16j"]
BAD_ARGUMENT = 5
SENTINEL = -12345.678


def _p(a):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _call(ctx, newA, b, rtol=0.0, droptol=0.0, out=None, m=None):
    """The C ABI on host arrays: (status, out m x ncols, rank, sv, nnz, passes)."""
    newA = np.asfortranarray(newA, dtype=np.float64)
    m, d = newA.shape if m is None else (m, newA.shape[1])
    ncols = d + (b is not None)
    if out is None:
        out = np.full((max(m, 0), ncols), SENTINEL, order="F")
    rank, nnz, passes = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    sv = np.full(max(m, 0), np.nan)
    st = ctx._lib.sdpsr_compress_constraints(ctx._h, m, d, _p(newA) if newA.size else None, _p(b), rtol, droptol,
                                             _p(out) if out.size else None, C.byref(rank), _p(sv), C.byref(nnz), C.byref(passes), 0)
    return st, out, rank.value, sv, nnz.value, passes.value


@pytest.fixture(scope="module")
def cases(problems, golden):
    return R.inputs(problems, golden)


@pytest.fixture(scope="module")
def refs(cases):
    """{name: (M, s, r, LAPACK's orth, LAPACK's resid)}, computed once."""
    out = {}
    for name, (newA, b, _) in cases.items():
        M = R.stack(newA, b)
        s, r, rows = R.reference(M)
        out[name] = (M, s, r, R.orth(rows), R.resid(M, rows))
    return out


@pytest.fixture(scope="module")
def plain(gpu_ctx, cases):
    """{name: the droptol = 0 call}, made once and left unchanged."""
    return {name: _call(gpu_ctx, newA, b) for name, (newA, b, _) in cases.items()}


@pytest.mark.parametrize("name", NAMES)
def test_rows_against_lapack_on_invariants(cases, refs, plain, name):
    """rank = the reference's; orth and resid <= max(8 x LAPACK's own figure on this input, ncols eps -- the bound of a
    length-ncols dot product); sverr <= ncols eps (absolute against sigma_1); rows r .. m-1 exactly zero; every row's
    largest-magnitude entry positive; sv descending.  Precondition (rank unambiguous for any correct method): no reference
    singular value in [1e-13, 1e-10] sigma_1."""
    M, s, r, orth_l, resid_l = refs[name]
    m, ncols = M.shape
    assert R.rank_is_unambiguous(s) and r == cases[name][2]
    st, out, rank, sv, nnz, passes = plain[name]
    assert st == 0
    rows = out[:rank]
    figures = (R.orth(rows), R.resid(M, rows) if rank else np.inf, R.sverr(sv, s, m))
    print(name, "rank", rank, "passes", passes, "orth %.3g resid %.3g sverr %.3g" % figures, "LAPACK orth %.3g resid %.3g" % (orth_l, resid_l))
    assert rank == r
    bound = ncols * R.EPS
    assert figures[0] <= max(8 * orth_l, bound)
    assert figures[1] <= max(8 * resid_l, bound)
    assert figures[2] <= bound
    assert np.array_equal(_bits(out[rank:]), np.zeros((m - rank, ncols), dtype=np.uint64))
    assert np.all(rows[np.arange(rank), np.abs(rows).argmax(axis=1)] > 0)
    assert np.all(np.diff(sv) <= 0) and np.all(sv >= 0)
    assert nnz == np.count_nonzero(rows) and 1 <= passes <= R.MAX_PASSES


@pytest.mark.parametrize("name", NAMES)
def test_drop_rule(gpu_ctx, cases, plain, name):
    """droptol = 1e-8: no kept entry has magnitude <= 1e-8, every other entry equals the droptol = 0 run bit for bit, nnz
    equals a NumPy count."""
    newA, b, _ = cases[name]
    _, out0, rank0, sv0, _, _ = plain[name]
    st, out, rank, sv, nnz, _ = _call(gpu_ctx, newA, b, droptol=1e-8)
    assert st == 0 and rank == rank0 and np.array_equal(_bits(sv), _bits(sv0))
    small = np.abs(out0) <= 1e-8
    assert not np.any((out != 0) & (np.abs(out) <= 1e-8))
    assert np.array_equal(_bits(out[small]), np.zeros(int(small.sum()), dtype=np.uint64))
    assert np.array_equal(_bits(out[~small]), _bits(out0[~small]))
    assert nnz == np.count_nonzero(out[:rank])


@pytest.mark.parametrize("name", NAMES)
def test_equal_inputs_give_equal_bytes(pkg, gpu_ctx, cases, plain, name):
    """Twice on one ctx and once on a second ctx: the same bytes; b = NULL on [newA | b] as one matrix: the same bytes again
    ((m, ncols) and the entries are the same), and the Python mirror hands out exactly these rows."""
    newA, b, _ = cases[name]
    _, out0, rank0, sv0, nnz0, passes0 = plain[name]
    with pkg.Context(device=0, seed=99) as other:
        for ctx in (gpu_ctx, other):
            st, out, rank, sv, nnz, passes = _call(ctx, newA, b)
            assert st == 0 and (rank, nnz, passes) == (rank0, nnz0, passes0)
            assert np.array_equal(_bits(out), _bits(out0)) and np.array_equal(_bits(sv), _bits(sv0))
    M = np.asfortranarray(R.stack(newA, b))
    st, out, rank, sv, _, _ = _call(gpu_ctx, M, None)
    assert st == 0 and rank == rank0 and np.array_equal(_bits(out), _bits(out0)) and np.array_equal(_bits(sv), _bits(sv0))
    alone = pkg.compress_constraints(M, droptol=0.0, ctx=gpu_ctx)
    assert alone.shape == (rank0, M.shape[1]) and np.array_equal(_bits(alone), _bits(out0[:rank0]))
    A2, B2, info = pkg.compress_constraints(newA, b, droptol=0.0, ctx=gpu_ctx, return_info=True)
    assert np.array_equal(_bits(A2), _bits(out0[:rank0, :-1])) and np.array_equal(_bits(B2), _bits(out0[:rank0, -1]))
    assert info["rank"] == rank0 and info["nnz"] == nnz0 and info["passes"] == passes0 and np.array_equal(_bits(info["sv"]), _bits(sv0))


def test_esc16j_from_a_device_tensor(pkg, gpu_ctx, cases, plain):
    """Device input in both accepted layouts (m x d with column-major strides, and the flat m * d buffer): read where it lies,
    device tensors back, the bytes of the host call."""
    import torch
    newA, b, _ = cases["esc16j"]
    _, out0, rank0, _, _, _ = plain["esc16j"]
    m, d = newA.shape
    flat = torch.from_numpy(np.ascontiguousarray(newA.reshape(-1, order="F"))).cuda()
    for arg in (flat.view(d, m).t(), flat):
        A2, B2 = pkg.compress_constraints(arg, b, droptol=0.0, ctx=gpu_ctx)
        assert A2.is_cuda and B2.is_cuda and tuple(A2.shape) == (rank0, d) and tuple(B2.shape) == (rank0,)
        assert np.array_equal(_bits(A2.cpu().numpy()), _bits(out0[:rank0, :-1]))
        assert np.array_equal(_bits(B2.cpu().numpy()), _bits(out0[:rank0, -1]))
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(newA.reshape(-1, order="F")))  # (the input is not written)


def test_reduced_sdp_on_esc16j(pkg, problems, golden, gpu_ctx, cases):
    """reduced_sdp with a SparseConstraints and device labels: newA2 x = newB2 has the solution set of newA x = b
    (rank [newA2 | newB2] == rank [newA | b; newA2 | newB2] == 9), newC = reduce_constraints_csr(P, C); the same rows from
    the SciPy route on host labels."""
    import scipy.sparse as sp
    import torch
    fa, fb = problems.read_qapdata(R.ROOT / "tests" / "golden" / "esc16j.dat")
    Cv, A, b = problems.qap_problem(fa, fb)
    L = np.asarray(golden["esc16j_P"])
    n, d = L.shape[0], int(L.max())
    newA, _, _ = cases["esc16j"]
    M = R.stack(newA, b)
    Ph = pkg.Partition(d, L)
    lab = torch.from_numpy(np.ascontiguousarray(L.reshape(-1, order="F")).astype(np.uint32).view(np.int32)).cuda()
    Pd = pkg.Partition(d, lab.view(n, n).t())
    c = np.asarray(Cv, dtype=np.float64).reshape(-1, order="F")
    newC_ref = pkg.reduce_constraints_csr(Ph, c, ctx=gpu_ctx)
    with pkg.SparseConstraints(A, n * n, ctx=gpu_ctx) as S:
        A2, B2, newC = pkg.reduced_sdp(Pd, S, b, Cv, droptol=0.0, ctx=gpu_ctx)
        plainA, plainB, _ = pkg.reduced_sdp(Pd, S, b, Cv, compress=False, ctx=gpu_ctx)
    assert A2.is_cuda and B2.is_cuda and plainA.is_cuda  # (A * PMat stays where the assembly wrote it)
    assert np.array_equal(_bits(plainA.cpu().numpy()), _bits(newA)) and np.array_equal(plainB, b)
    assert np.array_equal(_bits(newC), _bits(newC_ref))
    M2 = np.hstack([A2.cpu().numpy(), B2.cpu().numpy().reshape(-1, 1)])
    assert M2.shape == (9, 151)
    assert np.linalg.matrix_rank(M2) == 9 and np.linalg.matrix_rank(np.vstack([M, M2])) == 9
    H2, Hb, HC = pkg.reduced_sdp(Ph, sp.csr_matrix(A), b, Cv, droptol=0.0, ctx=gpu_ctx)
    assert np.array_equal(_bits(np.hstack([H2, Hb.reshape(-1, 1)])), _bits(M2)) and np.array_equal(_bits(HC), _bits(newC_ref))
    # the default drop leaves the solution set alone to 1e-8
    D2, Db, _ = pkg.reduced_sdp(Ph, sp.csr_matrix(A), b, Cv, ctx=gpu_ctx)
    assert np.abs(np.hstack([D2, Db.reshape(-1, 1)]) - M2).max() <= 1e-8


def test_explicit_rtol_and_the_small_shapes(gpu_ctx, cases):
    newA, b, _ = cases["graded_6x37"]
    st, out, rank, sv, _, _ = _call(gpu_ctx, newA, b, rtol=1e-5)
    assert st == 0 and rank == 2 and np.all(out[2:] == 0) and R.orth(out[:2]) <= 37 * R.EPS
    # m = 0
    st, _, rank, _, nnz, passes = _call(gpu_ctx, np.zeros((0, 5)), None)
    assert (st, rank, nnz, passes) == (0, 0, 0, 0)
    # an all-zero M (with a negative zero in it)
    Z = np.zeros((4, 6), order="F")
    Z[1, 2] = -0.0
    st, out, rank, sv, nnz, _ = _call(gpu_ctx, Z, np.zeros(4))
    assert (st, rank, nnz) == (0, 0, 0) and np.array_equal(_bits(out), np.zeros((4, 7), dtype=np.uint64)) and np.all(sv == 0)
    # m = 1
    row = np.array([[3.0, -4.0, 0.0]], order="F")
    st, out, rank, sv, nnz, _ = _call(gpu_ctx, row, np.array([12.0]))
    assert (st, rank, nnz) == (0, 1, 3)
    assert np.abs(out[0] - np.array([-3.0, 4.0, 0.0, -12.0]) / -13.0).max() <= 4 * R.EPS and abs(sv[0] - 13.0) <= 13 * 4 * R.EPS
    # m > ncols with b = NULL, and one column
    st, out, rank, sv, _, _ = _call(gpu_ctx, np.array([[2.0], [-1.0], [0.5]], order="F"), None)
    assert (st, rank) == (0, 1) and abs(out[0, 0] - 1.0) <= 2 * R.EPS and np.all(out[1:] == 0)


def test_bad_arguments_leave_out_and_ctx_alone(gpu_ctx, cases):
    """A NaN in newA and an Inf in b: SDPSR_BAD_ARGUMENT ("non-finite value"), out keeps its sentinel, and a good call
    follows; rtol = -1, rtol = NaN and m above the documented limit likewise."""
    newA, b, r = cases["duplicates_6x70"]
    lib = gpu_ctx._lib
    for bad_a, bad_b in ((True, False), (False, True)):
        A1, b1 = newA.copy(order="F"), b.copy()
        if bad_a:
            A1[4, 33] = np.nan
        if bad_b:
            b1[5] = -np.inf
        st, out, _, _, _, _ = _call(gpu_ctx, A1, b1)
        assert st == BAD_ARGUMENT and "non-finite value" in lib.sdpsr_last_error(gpu_ctx._h).decode()
        assert np.all(out == SENTINEL)
        st, _, rank, _, _, _ = _call(gpu_ctx, newA, b)
        assert st == 0 and rank == r
    for rtol in (-1.0, np.nan):
        st, out, _, _, _, _ = _call(gpu_ctx, newA, b, rtol=rtol)
        assert st == BAD_ARGUMENT and np.all(out == SENTINEL)
    # m above the limit: refused from the arguments alone (the arrays are never read)
    st, out, _, _, _, _ = _call(gpu_ctx, newA, None, out=np.full((6, 70), SENTINEL, order="F"), m=1025)
    assert st == BAD_ARGUMENT and np.all(out == SENTINEL)
    st, _, rank, _, _, _ = _call(gpu_ctx, newA, b)
    assert st == 0 and rank == r


def test_more_than_one_block_of_rows(gpu_ctx):
    """m = 70 > 64: three block pairs in the Gram kernel, J read through the caches in the rotation (it no longer fits the LDS
    beside the columns); rank 40 of 70 rows over 300 columns."""
    rng = np.random.default_rng(21)
    B = rng.integers(-2, 3, size=(40, 300)).astype(np.float64)
    M = np.asfortranarray(rng.integers(-1, 2, size=(70, 40)).astype(np.float64) @ B)
    s, r, rows = R.reference(M)
    assert r == 40 and R.rank_is_unambiguous(s)
    st, out, rank, sv, _, passes = _call(gpu_ctx, M, None)
    figures = (R.orth(out[:rank]), R.resid(M, out[:rank]), R.sverr(sv, s, 70))
    print("70x300 rank", rank, "passes", passes, "orth %.3g resid %.3g sverr %.3g" % figures)
    assert st == 0 and rank == 40
    bound = 300 * R.EPS
    assert figures[0] <= max(8 * R.orth(rows), bound) and figures[1] <= max(8 * R.resid(M, rows), bound) and figures[2] <= bound
    assert np.all(out[rank:] == 0)
