"""Setup stage from a sparse A given as CSR (sdpsr_admissible_setup_csr / sdpsr_admissible_subspace_csr,
src/partitions.jl:117-142, src/utils.jl:58-66): results against the golden partitions, the oracle, the NumPy setup and
the dense device entry; symmetry hint, rank decisions, input forms, malformed input, device setups downstream."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from csr_setup_helpers import _compare_with_host_setup

pytestmark = pytest.mark.gpu

ATOL = math.sqrt(np.finfo(np.float64).eps)


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


def _setup_ctypes(pkg, ctx, n, m, rowptr, colind, val, base, b, c, mem_out=0):
    """sdpsr_admissible_setup_csr with host outputs: (status, CL, X0L, U[:, :r], hint, info)."""
    ln = n * n
    CL, X0 = np.zeros(ln), np.zeros(ln)
    U = np.zeros((ln, max(m, 1)), order="F")
    r, hint, info = C.c_int64(-1), C.c_int(-1), C.c_int32(-1)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    st = ctx._lib.sdpsr_admissible_setup_csr(ctx._h, n, m, p(rowptr), p(colind), p(val), base, p(b), p(c), ATOL, p(CL), p(X0), p(U),
                                             C.byref(r), C.byref(hint), C.byref(info), mem_out)
    return st, CL, X0, U[:, :max(r.value, 0)], hint.value, info.value


# ------------------------------------------------------------------ results
@pytest.mark.parametrize("name", ["petersen", "er3", "er5", "er7", "esc16j"])
def test_golden_partitions_through_csr(pkg, problems, golden, name):
    Cv, A, b = _problem(problems, name)
    with pkg.Context(seed=1) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, csr_setup=True)
        Pd = pkg.admissible_subspace(Cv, A, b, ctx=ctx)  # the dense device entry
    assert P.nparts == int(golden[f"{name}_P"].max())
    assert np.array_equal(P.matrix, golden[f"{name}_P"])
    assert np.array_equal(P.matrix, Pd.matrix)


def test_config2_qap_grid30_against_oracle(pkg, problems, oracle):
    flow, dist = problems.grid_qap_instance(5, 6, seed=4, symmetric_flow=True)
    Cv, A, b = problems.qap_problem(flow, dist)
    assert A.shape == (61, 810000)
    n, CL, X0L, U = pkg.admissible_setup(Cv, A, b)
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0),
                                     setup=(n, U, CL.reshape(n, n, order="F"), X0L.reshape(n, n, order="F")))
    for mode in (pkg.SQUARE_I8, pkg.SQUARE_F64):
        with pkg.Context(seed=31, square_mode=mode) as ctx:
            h0 = ctx.transfer_bytes()[0]
            P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, csr_setup=True)
            h2d = ctx.transfer_bytes()[0] - h0
            assert P.nparts == ref.nparts
            assert np.array_equal(P.matrix, ref.matrix)
            assert h2d <= 25e6, h2d  # the CSR and C, not the 395 MB of a dense A


@pytest.mark.parametrize("name", ["er7", "esc16j"])
def test_setup_matches_numpy_setup(pkg, problems, name):
    Cv, A, b = _problem(problems, name)
    with pkg.Context(seed=3) as ctx:
        Sd = pkg.admissible_setup_csr(Cv, A, b, ctx=ctx)
        assert Sd.info == pkg._lib.SETUP_CHOLESKY_QR2
    _compare_with_host_setup(pkg, Sd, pkg.admissible_setup(Cv, A, b))


# ------------------------------------------------------------------ symmetry
@pytest.mark.parametrize("name", ["er5", "esc16j"])
def test_symmetric_rows_give_bitwise_symmetric_outputs_and_hint(pkg, problems, name):
    Cv, A, b = _problem(problems, name)
    with pkg.Context(seed=3) as ctx:
        n, CL, X0L, U = S = pkg.admissible_setup_csr(Cv, A, b, ctx=ctx)
    assert S.hint == 3
    Uh = U.cpu().numpy()
    for k in range(Uh.shape[1]):
        M = Uh[:, k].reshape(n, n, order="F")
        assert np.array_equal(M, M.T), k
    for v in (CL.cpu().numpy(), X0L.cpu().numpy()):
        M = v.reshape(n, n, order="F")
        assert np.array_equal(M, M.T)


def test_nonsymmetric_row_clears_hint(pkg, problems):
    Cv, A, b = _problem(problems, "er5")
    n = math.isqrt(len(_vec(Cv)))
    extra = sp.csr_matrix(([1.0], ([0], [1 + 4 * n])), shape=(1, n * n))  # entry (1, 4) without (4, 1)
    A2 = sp.vstack([sp.csr_matrix(A), extra], format="csr")
    b2 = np.concatenate([b, [0.0]])
    with pkg.Context(seed=5) as ctx:
        S = pkg.admissible_setup_csr(Cv, A2, b2, ctx=ctx)
        assert S.hint == 0
        P = pkg.admissible_subspace(Cv, A2, b2, ctx=ctx, csr_setup=True)
        Ph = pkg.admissible_subspace(Cv, A2, b2, ctx=ctx, host_setup=True)
    assert P.nparts == Ph.nparts and np.array_equal(P.matrix, Ph.matrix)
    _compare_with_host_setup(pkg, S, pkg.admissible_setup(Cv, A2, b2))


# ------------------------------------------------------------------ rank decisions
def test_rank_deficient_rows_take_the_mgs_path(pkg, problems):
    Cv, A, b = _problem(problems, "esc16j")
    A = sp.csr_matrix(A)
    A2 = sp.vstack([A, A[0], A[1] + A[2]], format="csr")
    b2 = np.concatenate([b, [b[0], b[1] + b[2]]])
    Sh = pkg.admissible_setup(Cv, A2, b2)
    with pkg.Context(seed=7) as ctx:
        S = pkg.admissible_setup_csr(Cv, A2, b2, ctx=ctx)
        assert S.info == pkg._lib.SETUP_MGS
        assert S[3].shape[1] == Sh[3].shape[1] == A.shape[0]
        P = pkg.admissible_subspace(Cv, A2, b2, ctx=ctx, csr_setup=True)
        Pd = pkg.admissible_subspace(Cv, A2, b2, ctx=ctx)
    assert np.array_equal(P.matrix, Pd.matrix)
    _compare_with_host_setup(pkg, S, Sh)


def test_nearly_dependent_row_is_kept(pkg, problems):
    Cv, A, b = _problem(problems, "er5")
    A = sp.csr_matrix(A)
    n = math.isqrt(len(_vec(Cv)))
    E = sp.csr_matrix(([1.0, 1.0], ([0, 0], [2 + 3 * n, 3 + 2 * n])), shape=(1, n * n))  # symmetric pair (2, 3)
    row = A[0] + 1e-9 * sp.linalg.norm(A[0]) / sp.linalg.norm(E) * E  # residual 1e-9 of its norm
    A2 = sp.vstack([A, row], format="csr")
    b2 = np.concatenate([b, [b[0]]])
    Sh = pkg.admissible_setup(Cv, A2, b2)
    with pkg.Context(seed=7) as ctx:
        S = pkg.admissible_setup_csr(Cv, A2, b2, ctx=ctx)
    assert S.info == pkg._lib.SETUP_MGS
    assert S[3].shape[1] == Sh[3].shape[1] == A.shape[0] + 1


def test_more_than_128_rows(pkg, problems):
    """m = 200 > 128 (the tiled Gram kernel), random sparse symmetric rows at n = 30."""
    n, m = 30, 200
    rng = np.random.default_rng(11)
    rows, cols, vals = [], [], []
    for i in range(m):
        for _ in range(5):
            p, q = rng.integers(0, n, size=2)
            v = float(rng.integers(1, 5))
            for (a, c_) in {(p, q), (q, p)}:
                rows.append(i)
                cols.append(a + c_ * n)
                vals.append(v)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(m, n * n))
    X = rng.standard_normal((n, n))
    X = X + X.T
    b = A @ X.reshape(-1, order="F")
    Cm = rng.integers(0, 3, size=(n, n)).astype(np.float64)
    Cv = (Cm + Cm.T).reshape(-1, order="F")
    with pkg.Context(seed=9) as ctx:
        S = pkg.admissible_setup_csr(Cv, A, b, ctx=ctx)
        assert S.info == pkg._lib.SETUP_CHOLESKY_QR2 and S.hint == 3
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, csr_setup=True)
        Ph = pkg.admissible_subspace(Cv, A, b, ctx=ctx, host_setup=True)
    assert np.array_equal(P.matrix, Ph.matrix)
    _compare_with_host_setup(pkg, S, pkg.admissible_setup(Cv, A, b))


# ------------------------------------------------------------------ the C entry's input contract
def test_input_forms_give_identical_outputs(pkg, problems):
    Cv, A, b = _problem(problems, "er5")
    c = _vec(Cv)
    n = math.isqrt(c.size)
    rp, ci, va = pkg.csr_arrays(A, n * n)
    m = rp.size - 1
    b = np.ascontiguousarray(b, dtype=np.float64)
    # unsorted + duplicated (each value split in halves, exact for these integers) + explicit zeros, 1-based
    rows = [(list(ci[rp[i]:rp[i + 1]]), list(va[rp[i]:rp[i + 1]])) for i in range(m)]
    rp2, ci2, va2 = [0], [], []
    for cols, vals in rows:
        cc = cols[::-1] + cols[:1] + cols[-1:]
        vv = [v / 2 if k == len(cols) - 1 else v for k, v in enumerate(vals[::-1])] + [vals[0] / 2, 0.0]
        ci2 += cc
        va2 += vv
        rp2.append(len(ci2))
    rp2, ci2, va2 = np.array(rp2, dtype=np.int64), np.array(ci2, dtype=np.int64), np.array(va2)
    with pkg.Context(seed=1) as ctx:
        ref = _setup_ctypes(pkg, ctx, n, m, rp, ci, va, 0, b, c)
        assert ref[0] == 0
        for arrs, base in (((rp + 1, ci + 1, va), 1), ((rp2, ci2, va2), 0), ((rp2 + 1, ci2 + 1, va2), 1)):
            got = _setup_ctypes(pkg, ctx, n, m, *[np.ascontiguousarray(a) for a in arrs], base, b, c)
            assert got[0] == 0
            for g, e in zip(got[1:4], ref[1:4]):
                assert np.array_equal(g, e)
            assert got[4:] == ref[4:]


def test_malformed_csr_returns_bad_argument_and_ctx_stays_usable(pkg, problems):
    Cv, A, b = _problem(problems, "petersen")
    c = _vec(Cv)
    n = math.isqrt(c.size)
    rp, ci, va = pkg.csr_arrays(A, n * n)
    m = rp.size - 1
    b = np.ascontiguousarray(b, dtype=np.float64)
    bad_ci = ci.copy()
    bad_ci[-1] = n * n
    bad_rp = rp.copy()
    bad_rp[1], bad_rp[2] = bad_rp[2], bad_rp[1]
    nan_va = va.copy()
    nan_va[0] = np.nan
    with pkg.Context(seed=1) as ctx:
        for arrs, base in (((rp, bad_ci, va), 0), ((bad_rp, ci, va), 0), ((rp, ci, nan_va), 0), ((rp, ci, va), 1), ((rp, ci, va), 2)):
            st = _setup_ctypes(pkg, ctx, n, m, *arrs, base, b, c)[0]
            assert st == 5, (base, st)
        st, CL, X0, U, hint, info = _setup_ctypes(pkg, ctx, n, m, rp, ci, va, 0, b, c)
        assert st == 0 and hint == 3 and U.shape[1] == m


def test_no_constraints_equals_oracle(pkg, problems, oracle):
    Cv, A, b = _problem(problems, "er5")
    n = math.isqrt(len(_vec(Cv)))
    A0 = sp.csr_matrix((0, n * n))
    b0 = np.zeros(0)
    nn, CL, X0L, U = pkg.admissible_setup(Cv, A0, b0)
    ref = oracle.admissible_subspace(Cv, A0, b0, rng=np.random.default_rng(0),
                                     setup=(nn, U, CL.reshape(n, n, order="F"), X0L.reshape(n, n, order="F")))
    with pkg.Context(seed=2) as ctx:
        S = pkg.admissible_setup_csr(Cv, A0, b0, ctx=ctx)
        assert S.info == pkg._lib.SETUP_NO_CONSTRAINTS and S[3].shape[1] == 0
        P = pkg.admissible_subspace(Cv, A0, b0, ctx=ctx, csr_setup=True)
    assert P.nparts == ref.nparts and np.array_equal(P.matrix, ref.matrix)


# ------------------------------------------------------------------ device setups downstream
def test_device_setup_into_problem_and_batch(pkg, problems, golden):
    Cv, A, b = _problem(problems, "esc16j")
    c = _vec(Cv)
    rp, ci, va = pkg.csr_arrays(A, c.size)
    with pkg.Context(seed=4) as ctx:
        h0 = ctx.transfer_bytes()[0]
        S = pkg.admissible_setup_csr(Cv, A, b, ctx=ctx)
        with pkg.Problem(setup=S, ctx=ctx) as prob:
            h2d = ctx.transfer_bytes()[0] - h0
            res = prob.reduce(seed=5)
        assert h2d <= rp.nbytes + ci.nbytes + va.nbytes + c.nbytes + 8 * len(b), h2d
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, csr_setup=True)
        assert np.array_equal(res["P"].matrix, P.matrix) and res["P"].nparts == P.nparts
        Ps = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=S)
        assert np.array_equal(np.asarray(Ps.matrix.cpu()), golden["esc16j_P"])
        out = pkg.jordan_reduce_batch(Cv, A, b, restarts=2, ctx=ctx, setup=S)
        assert any(o["status"] == 0 for o in out)
        for o in out:
            assert np.array_equal(o["P"].matrix, golden["esc16j_P"])


def test_qap_n64_completes(pkg, problems):
    """A QAP at the project's headline order: n = 64 facilities, N = 4096, A of 129 x 16.7M with ~17.2M nonzeros (17 GB
    dense) -- beyond the dense entry's 4 GiB and out of reach of the host QR."""
    import torch
    flow, dist = problems.grid_qap_instance(8, 8, seed=1, symmetric_flow=True)
    Cv, A, b = problems.qap_problem(flow, dist)
    assert A.shape == (129, 4096 ** 2)
    with pkg.Context(seed=6) as ctx:
        n, CL, X0L, U = S = pkg.admissible_setup_csr(Cv, A, b, ctx=ctx)
        assert n == 4096 and S.hint == 3
        r = U.shape[1]
        # U'U summed over row chunks: one dot product of 16.7M near-equal positive terms drifts by ~1e-9 on its own
        G = sum(U[k:k + (1 << 16)].t() @ U[k:k + (1 << 16)] for k in range(0, n * n, 1 << 16))
        assert (G - torch.eye(r, dtype=G.dtype, device=G.device)).abs().max().item() <= 1e-11
        x = torch.randn(n * n, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).to(U.device)
        res = (x - U @ (U.t() @ x)).cpu().numpy()
        Anorm = sp.linalg.norm(A)
        assert np.linalg.norm(A @ res) <= 1e-10 * Anorm * torch.linalg.norm(x).item()
        del G, res
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=S)
        lab = P.matrix.t().contiguous().view(-1).long()  # column-major labels on the device
        d = P.nparts
        hi = torch.full((d + 1,), -np.inf, dtype=torch.float64, device=lab.device).scatter_reduce(0, lab, CL, "amax")
        lo = torch.full((d + 1,), np.inf, dtype=torch.float64, device=lab.device).scatter_reduce(0, lab, CL, "amin")
        assert torch.equal(hi[1:], lo[1:])  # C_L is constant on every class
        # one more random square does not refine the result (randomize, square_f64, refine)
        Ph = pkg.Partition(d, np.ascontiguousarray(P.matrix.cpu().numpy()).view(np.uint32))
        Xr = np.asfortranarray(pkg.randomize(Ph, ctx=ctx))
        X2 = np.empty_like(Xr)
        ctx.check(ctx._lib.sdpsr_square_f64(ctx._h, n, C.c_void_p(Xr.ctypes.data), C.c_void_p(X2.ctypes.data), pkg.MEM_HOST))
        X2 = np.asfortranarray(X2)
        ctx.check(ctx._lib.sdpsr_clamp_round(ctx._h, n * n, C.c_void_p(X2.ctypes.data), ATOL, pkg.MEM_HOST))
        Q = pkg.Partition.from_matrix(X2, ctx=ctx)
        R = pkg.refine(pkg.Partition(d, Ph.matrix.copy()), Q, ctx=ctx)
        assert R.nparts == d
