"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the
golden fixtures.  Bit-exact for labels / integer products; stated tolerances for fp."""
import ctypes as C
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]


def _fl(a, dt):
    return np.ascontiguousarray(np.asarray(a, dtype=dt).ravel(order="F"))


# ------------------------------------------------------------------ primitives
def test_partition_from_values_matches_oracle(pkg, oracle, gpu_ctx):
    rng = np.random.default_rng(0)
    for shape in [(1, 1), (3, 3), (10, 10), (37, 37), (64, 64), (130, 130), (257, 255)]:
        M = rng.integers(0, 9, size=shape).astype(np.float64) * 0.125
        M[rng.random(shape) < 0.05] = -0.0  # isequal: -0.0 is its own class
        P = pkg.Partition.from_matrix(M, ctx=gpu_ctx)
        R = oracle.partition_from_values(M)
        assert P.nparts == R.nparts
        assert np.array_equal(P.matrix, R.matrix)


def test_partition_all_distinct_and_all_zero(pkg, oracle, gpu_ctx):
    M = np.arange(1, 300 * 300 + 1, dtype=np.float64).reshape(300, 300)
    P = pkg.Partition.from_matrix(M, ctx=gpu_ctx)
    assert P.nparts == 90000
    assert np.array_equal(P.matrix, oracle.partition_from_values(M).matrix)
    Z = np.zeros((17, 17))
    P = pkg.Partition.from_matrix(Z, ctx=gpu_ctx)
    assert P.nparts == 0 and not P.matrix.any()


def test_integer_ctor_and_counts(pkg, oracle, gpu_ctx):
    # test/runtests.jl:13-20
    rng = np.random.default_rng(5)
    M = rng.integers(1, 11, size=(10, 10))
    M[0, 0] = 0
    P = pkg.Partition.from_matrix(M, ctx=gpu_ctx)
    assert pkg.dim(P) == len(np.unique(M)) - 1
    assert np.array_equal(P.matrix, oracle.partition_from_labels(M).matrix)
    assert pkg.dim(pkg.Partition.from_matrix(M.astype(float), ctx=gpu_ctx)) == len(np.unique(M)) - 1


def test_refine_triple_and_random(pkg, oracle, gpu_ctx):
    # test/runtests.jl:22-25
    P1 = pkg.Partition.from_matrix(np.array([[1, 2, 2], [2, 3, 3], [2, 3, 3]]), ctx=gpu_ctx)
    P2 = pkg.Partition.from_matrix(np.array([[1, 1, 2], [1, 1, 2], [1, 1, 3]]), ctx=gpu_ctx)
    P3 = pkg.refine(P1, P2, ctx=gpu_ctx)
    assert P3.nparts == 6
    assert np.array_equal(P3.matrix, np.array([[1, 2, 4], [2, 3, 5], [2, 3, 6]]))
    rng = np.random.default_rng(7)
    for n, k1, k2 in [(50, 5, 7), (200, 40, 3), (333, 1000, 1000)]:
        A = rng.integers(0, k1, size=(n, n))
        B = rng.integers(0, k2, size=(n, n))
        Pa = pkg.Partition.from_matrix(A, ctx=gpu_ctx)
        Pb = pkg.Partition.from_matrix(B, ctx=gpu_ctx)
        ref = oracle.refine(oracle.partition_from_labels(A), oracle.partition_from_labels(B))
        got = pkg.refine(Pa, Pb, ctx=gpu_ctx)
        assert got.nparts == ref.nparts
        assert np.array_equal(got.matrix, ref.matrix)


def test_fill_and_randomize_roundtrip(pkg, oracle, gpu_ctx):
    rng = np.random.default_rng(2)
    A = rng.integers(0, 12, size=(40, 40))
    P = pkg.Partition.from_matrix(A, ctx=gpu_ctx)
    vals = rng.random(P.nparts)
    M = pkg.fill(P, vals, ctx=gpu_ctx)
    assert np.array_equal(M, oracle.fill(oracle.Partition(P.nparts, P.matrix.astype(np.int64)), vals))
    with pytest.raises(ValueError):
        pkg.fill(P, vals[:-1], ctx=gpu_ctx)
    # test/runtests.jl:27: part(rndPart(P1)) == P1
    R = pkg.randomize(P, ctx=gpu_ctx)
    assert ((R >= 0) & (R < 1)).all() and (R[P.matrix == 0] == 0).all()
    assert pkg.Partition.from_matrix(R, ctx=gpu_ctx) == P


def test_clamp_round_and_projection(pkg, oracle, gpu_ctx):
    lib = pkg.load_library()
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.standard_normal(5000) * 10.0 ** rng.integers(-12, 6, 5000), [0.0625, 1e-10, -1e-9, 0.0]])
    got = a.copy()
    gpu_ctx.check(lib.sdpsr_clamp_round(gpu_ctx._h, got.size, C.c_void_p(got.ctypes.data), 1.4901161193847656e-8, 0))
    ref = oracle.clamp_round(a)
    assert np.array_equal(got, ref)  # same arithmetic: bit-exact
    # x .-= projL(x): nothing left in the row space of A (test/runtests.jl:29-37 analogue)
    n2, r = 4096, 5
    A = rng.standard_normal((r, n2))
    U = oracle.rowspace_basis(A)
    x = rng.standard_normal(n2)
    y = x.copy()
    Uf = np.asfortranarray(U)
    gpu_ctx.check(lib.sdpsr_project_out(gpu_ctx._h, n2, C.c_void_p(y.ctypes.data), C.c_void_p(Uf.ctypes.data), r, 0))
    assert np.allclose(y, x - oracle.project_colspace(x, U), atol=1e-12)
    assert np.abs(A @ y).max() < 1e-10


# ------------------------------------------------------------------ the square
@pytest.mark.parametrize("n", [1, 10, 57, 128, 200, 384, 512, 1000])
def test_square_i8_exact(pkg, gpu_ctx, n):
    lib = pkg.load_library()
    rng = np.random.default_rng(n)
    X = rng.integers(-128, 128, size=(n, n)).astype(np.int8)
    X = np.triu(X) + np.triu(X, 1).T  # symmetric
    X = X.astype(np.int8)
    out = np.zeros(n * n, dtype=np.int32)
    Xf = _fl(X, np.int8)
    gpu_ctx.check(lib.sdpsr_square_i8(gpu_ctx._h, n, C.c_void_p(Xf.ctypes.data), C.c_void_p(out.ctypes.data), 0))
    ref = X.astype(np.int64) @ X.astype(np.int64)
    assert np.array_equal(out.reshape(n, n, order="F"), ref)


def _sym_i8(rng, n):
    X = rng.integers(-128, 128, size=(n, n))
    return (np.triu(X) + np.triu(X, 1).T).astype(np.int8)


@pytest.mark.parametrize("kernel", [64, 1, 0])
def test_square_i8_symmetric_batch_every_kernel(pkg, gpu_ctx, kernel):
    """mul!(X2, X, X) (src/partitions.jl:172) for the loop's symmetric channel matrices, batched as the loop launches
    them: the persistent 256 x 256 macro-tile launch forced at sizes with 1, 3 and 4 whole macro-tile rows, with and
    without a ragged last 128 rows (the quarter-tile jobs), odd and even numbers of diagonal tiles (the paired diagonal
    jobs incl. the one whose partner is missing); the 128 x 128 tiles; the default choice: bit-exact against integer
    matmul."""
    lib = pkg.load_library()
    with pkg.Context(seed=3, square_kernel=kernel) as ctx:
        for n, batch in ((200, 1), (256, 2), (300, 3), (700, 2), (1100, 3)):
            rng = np.random.default_rng(1000 * n + batch)
            Xs = [_sym_i8(rng, n) for _ in range(batch)]
            Xf = np.concatenate([_fl(X, np.int8) for X in Xs])
            out = np.zeros(batch * n * n, dtype=np.int32)
            ctx.check(lib.sdpsr_square_i8_symmetric(ctx._h, n, batch, C.c_void_p(Xf.ctypes.data), C.c_void_p(out.ctypes.data), 0))
            for b, X in enumerate(Xs):
                ref = (X.astype(np.float64) @ X.astype(np.float64)).astype(np.int64)  # |sums| < 2^53: exact in fp64
                got = out[b * n * n:(b + 1) * n * n].reshape(n, n, order="F")
                assert np.array_equal(got, ref), (kernel, n, batch, b)


def test_square_i8_symmetric_n4096_default_launch(pkg, gpu_ctx):
    """The product launch of the bench instances (N = 4096, 2 channels: 240 full + 16 paired diagonal jobs, one per CU)
    and the N = 4104 shape (padded to 4352: two rounds of jobs), default kernel choice."""
    lib = pkg.load_library()
    for n in (4096, 4104):
        rng = np.random.default_rng(n)
        Xs = [_sym_i8(rng, n) for _ in range(2)]
        Xf = np.concatenate([_fl(X, np.int8) for X in Xs])
        out = np.zeros(2 * n * n, dtype=np.int32)
        gpu_ctx.check(lib.sdpsr_square_i8_symmetric(gpu_ctx._h, n, 2, C.c_void_p(Xf.ctypes.data), C.c_void_p(out.ctypes.data), 0))
        for b, X in enumerate(Xs):
            Xd = X.astype(np.float64)
            ref = (Xd @ Xd).astype(np.int64)
            assert np.array_equal(out[b * n * n:(b + 1) * n * n].reshape(n, n, order="F"), ref), (n, b)


@pytest.mark.parametrize("n", [7, 130, 256])
def test_square_f32_exact_on_small_integers(pkg, gpu_ctx, n):
    lib = pkg.load_library()
    rng = np.random.default_rng(n)
    vmax = int(np.floor(np.sqrt(2 ** 24 / n)))
    vmax = min(vmax, 127)
    X = rng.integers(-vmax, vmax + 1, size=(n, n))
    X = np.triu(X) + np.triu(X, 1).T
    out = np.zeros(n * n, dtype=np.float32)
    Xf = _fl(X, np.float32)
    gpu_ctx.check(lib.sdpsr_square_f32(gpu_ctx._h, n, C.c_void_p(Xf.ctypes.data), C.c_void_p(out.ctypes.data), 0))
    assert np.array_equal(out.reshape(n, n, order="F").astype(np.int64), X @ X)


@pytest.mark.parametrize("n", [5, 129, 300])
def test_square_f64_and_gemm_tn(pkg, gpu_ctx, n):
    lib = pkg.load_library()
    rng = np.random.default_rng(n)
    X = rng.random((n, n))
    X = (X + X.T) / 2
    out = np.zeros(n * n)
    Xf = _fl(X, np.float64)
    gpu_ctx.check(lib.sdpsr_square_f64(gpu_ctx._h, n, C.c_void_p(Xf.ctypes.data), C.c_void_p(out.ctypes.data), 0))
    ref = X @ X
    # fp64 MFMA vs OpenBLAS: summation order differs; 1e-13 relative to |X||X|
    assert np.abs(out.reshape(n, n, order="F") - ref).max() <= 1e-13 * n
    # general C = A' B with an asymmetric B (catches a transposed C write)
    m, nn, k = n, max(1, n // 2 + 3), n + 11
    A = np.asfortranarray(rng.standard_normal((k, m)))
    B = np.asfortranarray(rng.standard_normal((k, nn)))
    Cc = np.zeros((m, nn), order="F")
    gpu_ctx.check(lib.sdpsr_gemm_tn_f64(gpu_ctx._h, m, nn, k, C.c_void_p(A.ctypes.data), k, C.c_void_p(B.ctypes.data), k,
                                        C.c_void_p(Cc.ctypes.data), m, 0))
    assert np.abs(Cc - A.T @ B).max() <= 1e-12 * k


def test_syev_matches_lapack(pkg, gpu_ctx):
    lib = pkg.load_library()
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 33, 64, 65, 129, 130, 191, 200, 257, 777, 1100):
        A = rng.standard_normal((n, n))
        A = np.asfortranarray((A + A.T) / 2)
        w = np.zeros(n)
        V = np.zeros((n, n), order="F")
        gpu_ctx.check(lib.sdpsr_syev_f64(gpu_ctx._h, n, C.c_void_p(A.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0))
        assert np.allclose(w, np.linalg.eigvalsh(A), rtol=1e-10, atol=1e-10)
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-10
        assert np.abs(A @ V - V * w).max() < 1e-9


def test_syev_row_form_panel_form_and_hybrid(pkg):
    """The tridiagonalisation has two forms: one launch per column with row-owning workgroups (n <= 2048, default) and
    Householder panels with trailing updates on the matrix cores (SDPSR_FLAG_SYTRD_PANELS, and the leading columns of
    larger orders, whose last 2048 columns are handed to the row form).  SDPSR_FLAG_SYTRD_ONE_LAUNCH: the panel columns of
    the larger orders with one launch per column (product with the unnormalised column, csrc/kernels_sytrd_look.hip).  All
    against LAPACK."""
    lib = pkg.load_library()
    rng = np.random.default_rng(7)
    for n, flags in ((777, 0), (777, pkg._lib.FLAG_SYTRD_PANELS), (1536, 0), (2304, 0), (2500, 0),
                     (2304, pkg._lib.FLAG_SYTRD_ONE_LAUNCH), (2500, pkg._lib.FLAG_SYTRD_ONE_LAUNCH)):
        A = rng.standard_normal((n, n))
        A = np.asfortranarray((A + A.T) / 2)
        A[np.triu_indices(n, 1)] = 1e300  # only the lower triangle is referenced (the row form mirrors it first)
        Asym = np.tril(A) + np.tril(A, -1).T
        w = np.zeros(n)
        V = np.zeros((n, n), order="F")
        with pkg.Context(seed=1, flags=flags) as ctx:
            ctx.check(lib.sdpsr_syev_f64(ctx._h, n, C.c_void_p(A.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0))
        assert np.allclose(w, np.linalg.eigvalsh(Asym), rtol=1e-10, atol=1e-10), (n, flags)
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-10, (n, flags)
        assert np.abs(Asym @ V - V * w).max() < 1e-9, (n, flags)


def test_tridiagonal_divide_and_conquer_hard_cases(pkg):
    """The tridiagonal eigensolver of the dense driver (csrc/kernels_stedc.hip: divide and conquer with the secular roots
    by bisection on the shift's bit pattern) on the matrices that break careless ones -- Wilkinson, glued Wilkinson,
    graded, decoupled blocks, a handful of eigenvalues with huge multiplicities, the identity -- through sdpsr_syev_f64
    (the tridiagonalisation of a tridiagonal matrix is the identity); orders with and without padding to 128.
    eig_driver = 5 (rocSOLVER's stedc behind the same tridiagonalisation) must agree."""
    import scipy.linalg as sl
    lib = pkg.load_library()

    def cases(n, rng):
        yield "random", rng.standard_normal(n), rng.standard_normal(n - 1)
        yield "1-2-1", 2 * np.ones(n), -np.ones(n - 1)
        yield "wilkinson", np.abs(np.arange(n) - n // 2).astype(float), np.ones(n - 1)
        yield "graded", 10.0 ** (-np.arange(n) * 12.0 / n), 10.0 ** (-np.arange(n - 1) * 12.0 / n)
        yield "decoupled blocks", rng.standard_normal(n), rng.standard_normal(n - 1) * (rng.random(n - 1) < 0.5)
        Q0, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Dg = np.repeat(rng.standard_normal(6) * 3, n // 6 + 1)[:n]
        A = (Q0 * Dg) @ Q0.T
        H = sl.hessenberg((A + A.T) / 2)
        yield "six eigenvalues", np.diag(H).copy(), np.diag(H, -1).copy()
        yield "glued wilkinson", np.tile(np.abs(np.arange(21) - 10.0), n // 21 + 1)[:n], np.where((np.arange(n - 1) + 1) % 21 == 0, 1e-8, 1.0)
        yield "identity", np.ones(n), np.zeros(n - 1)

    for drv, orders in ((0, (130, 200, 640, 1100)), (5, (200,))):
        with pkg.Context(seed=1, eig_driver=drv) as ctx:
            for n in orders:
                for name, d, e in cases(n, np.random.default_rng(n)):
                    T = np.asfortranarray(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
                    w = np.zeros(n)
                    V = np.zeros((n, n), order="F")
                    ctx.check(lib.sdpsr_syev_f64(ctx._h, n, C.c_void_p(T.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0))
                    wl = np.linalg.eigvalsh(T)
                    sc = np.abs(wl).max()
                    assert np.all(np.diff(w) >= 0), (drv, n, name)
                    assert np.abs(w - wl).max() <= 2e-13 * sc, (drv, n, name, np.abs(w - wl).max() / sc)
                    assert np.abs(T @ V - V * w).max() <= 1e-12 * sc, (drv, n, name)
                    assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12, (drv, n, name)


@pytest.mark.parametrize("n", [4096, 8192])
def test_tridiagonal_divide_and_conquer_hard_cases_large(pkg, n):
    """The same hard tridiagonal matrices at the orders where the deflation runs and the 64-terms-per-lane secular
    kernels of kernels_stedc.hip are at their limits (merges of 4096 poles; 8192 is the embedded order of the complex
    path at n = 4096): Wilkinson, glued Wilkinson, graded, and a spectrum of six eigenvalues with multiplicities of
    hundreds (at 8192: two such blocks of order 4096 glued by 1e-9).  Same bounds as at the small orders: eigenvalues to
    2e-13 |T| against LAPACK's tridiagonal solver, residual 1e-12 |T|, orthogonality 1e-12 (products on the device)."""
    import scipy.linalg as sl
    import torch
    lib = pkg.load_library()
    rng = np.random.default_rng(n)

    def six(m):
        Q0, _ = np.linalg.qr(rng.standard_normal((m, m)))
        Dg = np.repeat(rng.standard_normal(6) * 3, m // 6 + 1)[:m]
        A = (Q0 * Dg) @ Q0.T
        H = sl.hessenberg((A + A.T) / 2)
        return np.diag(H).copy(), np.diag(H, -1).copy()

    d6, e6 = six(4096)
    if n == 8192:
        d6, e6 = np.concatenate([d6, d6]), np.concatenate([e6, [1e-9], e6])
    cases = [("wilkinson", np.abs(np.arange(n) - n // 2).astype(float), np.ones(n - 1)),
             ("glued wilkinson", np.tile(np.abs(np.arange(21) - 10.0), n // 21 + 1)[:n], np.where((np.arange(n - 1) + 1) % 21 == 0, 1e-8, 1.0)),
             ("graded", 10.0 ** (-np.arange(n) * 12.0 / n), 10.0 ** (-np.arange(n - 1) * 12.0 / n)),
             ("six eigenvalues", d6, e6)]
    T = torch.zeros(n * n, dtype=torch.float64, device="cuda")
    w = torch.empty(n, dtype=torch.float64, device="cuda")
    V = torch.empty(n * n, dtype=torch.float64, device="cuda")
    with pkg.Context(seed=1) as ctx:
        for name, d, e in cases:
            T.zero_()
            Tm = T.view(n, n)  # symmetric: row- and column-major views coincide
            td, te = torch.from_numpy(d).cuda(), torch.from_numpy(e).cuda()
            idx = torch.arange(n, device="cuda")
            Tm[idx, idx] = td
            Tm[idx[:-1], idx[:-1] + 1] = te
            Tm[idx[:-1] + 1, idx[:-1]] = te
            ctx.check(lib.sdpsr_syev_f64(ctx._h, n, C.c_void_p(T.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(V.data_ptr()), 1))
            wl = sl.eigh_tridiagonal(d, e, eigvals_only=True)
            sc = np.abs(wl).max()
            wh = w.cpu().numpy()
            assert np.all(np.diff(wh) >= 0), (n, name)
            assert np.abs(wh - wl).max() <= 2e-13 * sc, (n, name, np.abs(wh - wl).max() / sc)
            Vm = V.view(n, n).t()  # column-major n x n
            R = td[:, None] * Vm
            R[:-1] += te[:, None] * Vm[1:]
            R[1:] += te[:, None] * Vm[:-1]
            R -= Vm * w[None, :]
            assert float(R.abs().max()) <= 1e-12 * sc, (n, name, float(R.abs().max()) / sc)
            G = Vm.t() @ Vm
            G -= torch.eye(n, dtype=torch.float64, device="cuda")
            assert float(G.abs().max()) < 1e-12, (n, name, float(G.abs().max()))
            del R, G


def test_syev_degenerate_spectrum_residual(pkg, problems, gpu_ctx):
    """Generic elements of symmetric algebras have a handful of eigenvalues with huge
    multiplicities: the tridiagonalisation deflates after ~dim columns and then works on
    rounding noise.  Residual must stay at eps*|A| level (the trailing matrix is kept bitwise
    symmetric for exactly this case)."""
    lib = pkg.load_library()
    n = 1024
    Ls, d = problems.synthetic_jordan_partition(n, seed=2)
    A = np.asfortranarray(np.concatenate([[0.0], np.random.default_rng(0).random(d)])[Ls])
    w = np.zeros(n)
    V = np.zeros((n, n), order="F")
    gpu_ctx.check(lib.sdpsr_syev_f64(gpu_ctx._h, n, C.c_void_p(A.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0))
    scale = np.abs(w).max()
    assert np.abs(A @ V - V * w).max() <= 1e-13 * scale * 8
    assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12
    assert np.allclose(w, np.linalg.eigvalsh(A), atol=1e-12 * scale)


def test_syev_n4096_degenerate_and_generic(pkg, problems, gpu_ctx):
    """The dense driver at the headline order: (i) the generic element of the 34-class scheme
    (34 distinct eigenvalues with multiplicities ~128: deflation after the first panels),
    (ii) a generic symmetric matrix.  Residual, orthogonality and eigenvalues against LAPACK."""
    lib = pkg.load_library()
    n = 4096
    Ls, d = problems.synthetic_jordan_partition(n, seed=2)
    A1 = np.asfortranarray(np.concatenate([[0.0], np.random.default_rng(0).random(d)])[Ls])
    G = np.random.default_rng(4).standard_normal((n, n))
    A2 = np.asfortranarray((G + G.T) / 2)
    for A in (A1, A2):
        w = np.zeros(n)
        V = np.zeros((n, n), order="F")
        gpu_ctx.check(lib.sdpsr_syev_f64(gpu_ctx._h, n, C.c_void_p(A.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0))
        scale = np.abs(w).max()
        assert np.abs(A @ V - V * w).max() <= 2e-12 * scale
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-11
        assert np.allclose(w, np.linalg.eigvalsh(A), atol=1e-11 * scale)


def test_syev_one_launch_panels_beyond_4096(pkg, problems):
    """SDPSR_FLAG_SYTRD_ONE_LAUNCH at an order whose leading dimension exceeds 4096 (the kernel instance with 64 slots of partial
    products per row) and is ragged (n = 4200, ld = 4224): the degenerate generic element of a 34-class scheme and a generic
    symmetric matrix; residual, orthogonality, trace and the two-launch form's eigenvalues."""
    lib = pkg.load_library()
    n = 4200
    Ls, d = problems.synthetic_jordan_partition(n, seed=2)
    A1 = np.asfortranarray(np.concatenate([[0.0], np.random.default_rng(0).random(d)])[Ls])
    G = np.random.default_rng(4).standard_normal((n, n))
    A2 = np.asfortranarray((G + G.T) / 2)
    for A in (A1, A2):
        ws = []
        for flags in (pkg._lib.FLAG_SYTRD_ONE_LAUNCH, 0):
            w = np.zeros(n)
            V = np.zeros((n, n), order="F")
            with pkg.Context(seed=1, flags=flags) as ctx:
                ctx.check(lib.sdpsr_syev_f64(ctx._h, n, C.c_void_p(A.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0))
            scale = np.abs(w).max()
            assert np.abs(A @ V - V * w).max() <= 2e-12 * scale, flags
            assert np.abs(V.T @ V - np.eye(n)).max() < 1e-11, flags
            assert abs(w.sum() - np.trace(A)) <= 1e-10 * scale * n ** 0.5, flags
            ws.append(w)
        assert np.allclose(ws[0], ws[1], atol=1e-11 * np.abs(ws[1]).max())


# ------------------------------------------------------------------ the whole path
def _problem(problems, name):
    if name == "petersen":
        return problems.theta_prime_problem(problems.petersen_adjacency())
    if name.startswith("er"):
        return problems.theta_prime_problem(problems.er_graph_adjacency(int(name[2:])))
    if name == "esc16j":
        fa, fb = problems.read_qapdata(ROOT / "tests" / "golden" / "esc16j.dat")
        return problems.qap_problem(fa, fb)
    raise KeyError(name)


@pytest.mark.parametrize("mode", ["i8", "f32", "f64"])
@pytest.mark.parametrize("name", ["petersen", "er3", "er5", "er7", "esc16j"])
def test_admissible_subspace_matches_golden(pkg, problems, golden, name, mode):
    sq = {"i8": pkg.SQUARE_I8, "f32": pkg.SQUARE_F32, "f64": pkg.SQUARE_F64}[mode]
    Cv, A, b = _problem(problems, name)
    setup = pkg.admissible_setup(Cv, A, b)
    for seed in (1, 2):
        with pkg.Context(seed=seed, square_mode=sq) as ctx:
            P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
            assert P.nparts == int(golden[f"{name}_P"].max())
            assert np.array_equal(P.matrix, golden[f"{name}_P"]), (name, mode, seed)


@pytest.mark.parametrize("name,eps", [("petersen", None), ("er3", None), ("er5", None), ("er7", None),
                                      ("esc16j", None), ("numerical_issues", 1e-7), ("circ64", None), ("circ256", None)])
def test_block_diagonalize_matches_pins(pkg, oracle, golden, gpu_ctx, name, eps):
    L = golden[f"{name}_P"]
    P = pkg.Partition(int(L.max()), L.copy())
    kw = {} if eps is None else {"epsilon": eps}
    bd = pkg.blockDiagonalize(P, ctx=gpu_ctx, **kw)
    assert sorted(bd.blkSizes) == list(golden[f"{name}_blk"])
    # spectrum invariant: block eigenvalues within 1e-6 rel
    x = np.random.default_rng(8).random(P.nparts)
    Po = oracle.Partition(P.nparts, L.astype(np.int64))
    full, blk = oracle.spectrum_invariant(Po, bd.blks, x)
    assert len(full) == len(blk)
    assert np.allclose(full, blk, rtol=1e-6, atol=1e-8)
    # blks are exactly Q_k' 1[P==i] Q_k of the returned Q_hat
    ref = oracle.basis_image([np.asarray(q) for q in bd.Q_hat], Po)
    for i in range(P.nparts):
        for k in range(len(bd.blkSizes)):
            assert np.allclose(bd.blks[i][k], ref[i][k], atol=1e-10)


def test_desymmetrize_triple_and_oracle(pkg, oracle, golden, gpu_ctx):
    # test/runtests.jl:40: unSymmetrize(P1) == Partition(4, [1 3 3; 2 4 4; 2 4 4])
    P1 = pkg.Partition.from_matrix(np.array([[1, 2, 2], [2, 3, 3], [2, 3, 3]]), ctx=gpu_ctx)
    out = pkg.unSymmetrize(P1, ctx=gpu_ctx)
    assert out.nparts == 4
    assert np.array_equal(out.matrix, np.array([[1, 3, 3], [2, 4, 4], [2, 4, 4]]))
    # the canonical result does not depend on the draws: compare with the oracle on real algebras
    for name in ("petersen", "er3", "er5", "er7"):
        L = golden[f"{name}_P"].astype(np.int64)
        ref = oracle.desymmetrize(oracle.Partition(int(L.max()), L), rng=np.random.default_rng(1))
        got = pkg.desymmetrize(pkg.Partition(int(L.max()), L.astype(np.uint32)), ctx=gpu_ctx)
        assert got.nparts == ref.nparts, name
        assert np.array_equal(got.matrix, ref.matrix), name
    # a symmetric association scheme is already a coherent configuration: nothing to split
    Lc = golden["circ256_P"].astype(np.int64)
    got = pkg.desymmetrize(pkg.Partition(int(Lc.max()), Lc.astype(np.uint32)), ctx=gpu_ctx)
    assert got.nparts == int(Lc.max()) and np.array_equal(got.matrix, Lc)


def test_reduce_constraints_matches_pmat_product(pkg, problems, golden, gpu_ctx):
    # README.md:57-60 / test/sd_problems.jl:32-37: newA = A * PMat, newC = C' * PMat
    for name in ("er5", "esc16j"):
        Cv, A, b = _problem(problems, name)
        L = golden[f"{name}_P"]
        P = pkg.Partition(int(L.max()), L.copy())
        flat = L.ravel(order="F")
        PMat = np.zeros((flat.size, P.nparts))
        PMat[np.nonzero(flat)[0], flat[flat > 0] - 1] = 1.0
        Ad = np.asarray(A.todense()) if hasattr(A, "todense") else A
        got = pkg.reduce_constraints(P, Ad, ctx=gpu_ctx)
        assert np.allclose(got, Ad @ PMat, rtol=1e-13, atol=1e-12)
        gc = pkg.reduce_constraints(P, np.asarray(Cv), ctx=gpu_ctx)
        assert np.allclose(gc, np.asarray(Cv) @ PMat, rtol=1e-13, atol=1e-12)


def test_cyclic_c3_raises_invalid_field(pkg, gpu_ctx):
    # test/runtests.jl:50-56
    C3 = np.array([[1, 3, 2], [2, 1, 3], [3, 2, 1]])
    P = pkg.Partition.from_matrix(C3, ctx=gpu_ctx)
    with pytest.raises(pkg.InvalidDecompositionField):
        pkg.blockDiagonalize(P, ctx=gpu_ctx)


def test_numerical_issues_never_throws(pkg, golden, gpu_ctx):
    # test/numerical_issues.jl:91-94 through the single-problem entry point (300 launches)
    L = golden["numerical_issues_P"]
    P = pkg.Partition(1312, L.copy())
    for _ in range(300):
        ne, nc = pkg.eigen_decomposition(P, atol=1e-7, ctx=gpu_ctx)
        assert nc == 2


def test_numerical_issues_full_pin_batched(pkg, golden, gpu_ctx):
    """The reference's full robustness pin, test/numerical_issues.jl:85-94: 10 000 runs of
    eigen_decomposition(part, A, atol=1e-7) on the 64 x 64 / 1312-class partition, none may throw.
    Batched entry point: one workgroup per run on all CUs; must finish in < 5 s."""
    import time
    L = golden["numerical_issues_P"]
    P = pkg.Partition(1312, L.copy())
    pkg.eigen_decomposition_batched(P, 16, atol=1e-7, ctx=gpu_ctx)  # warm-up (buffers)
    t0 = time.perf_counter()
    st, ne, nc = pkg.eigen_decomposition_batched(P, 10000, atol=1e-7, ctx=gpu_ctx)
    dt = time.perf_counter() - t0
    assert not st.any()                      # no NumericalInconsistency, no non-convergence
    # 64 simple eigenvalues, classes of 16 and 48.  Two of the 64 random eigenvalues fall within atol = 1e-7
    # of each other once in ~1e5 runs (one two-dimensional eigenspace, ne = 63: a legitimate outcome, the
    # reference only demands that nothing throws), so ne is pinned statistically
    # (the merged eigenspace then stands alone: one more class)
    assert (ne >= 62).all() and (ne == 64).mean() > 0.999 and (nc[ne == 64] == 2).all() and (nc <= 4).all()
    assert dt < 5.0, dt


@pytest.mark.parametrize("name,atol", [("er3", None), ("er5", None), ("er7", None), ("numerical_issues", 1e-7),
                                       ("circ64", None), ("petersen", None)])
def test_batched_eigen_decomposition_matches_oracle_steps(pkg, oracle, golden, gpu_ctx, name, atol):
    """Same generic elements on both sides (explicit class values): the device's clustering
    (EigenDecomposition ctor, src/eigen_decomposition.jl:19-40), block norms + Otsu threshold
    (:83-139,177-193), union-find merges (:205-217) and __isconsistent (:163-167) must give the
    oracle's number of eigenspaces, number of isomorphism classes and verdict, run by run."""
    L = golden[f"{name}_P"].astype(np.int64)
    d = int(L.max())
    n = L.shape[0]
    atol = 1e-12 * n if atol is None else atol
    Po = oracle.Partition(d, L)
    rng = np.random.default_rng(17)
    count = 40
    vals = rng.random((count, 2, d))
    st, ne, nc = pkg.eigen_decomposition_batched(pkg.Partition(d, L.astype(np.uint32)), count, atol=atol, values=vals,
                                                 ctx=gpu_ctx, raise_on_failure=False)
    for r in range(count):
        A1 = oracle.fill(Po, vals[r, 0])
        w, Q = oracle._eigen(A1)
        ed = oracle.make_eigen_decomposition(w, Q, atol)
        K = oracle.isomorphism_partition(ed, oracle.fill(Po, vals[r, 1]), atol)
        roots = {K.find_root(i) for i in range(len(K))}
        assert ne[r] == len(ed), (name, r)
        assert nc[r] == len(roots), (name, r)
        assert (st[r] == 0) == oracle.is_consistent(K), (name, r)


def test_device_setup_equals_host_setup(pkg, problems, golden):
    """Setup stage on the device (sdpsr_admissible_subspace_dense) vs the NumPy setup: same
    canonical partition, including the sparse-A QAP with a 33 x 65536 constraint matrix."""
    for name in ("petersen", "er7", "esc16j"):
        Cv, A, b = _problem(problems, name)
        with pkg.Context(seed=11) as ctx:
            Pd = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
            Ph = pkg.admissible_subspace(Cv, A, b, ctx=ctx, host_setup=True)
        assert Pd.nparts == Ph.nparts == int(golden[f"{name}_P"].max())
        assert np.array_equal(Pd.matrix, golden[f"{name}_P"])
        assert np.array_equal(Ph.matrix, golden[f"{name}_P"])


def test_generic_graph_reaches_maximal_dimension(pkg, problems, oracle):
    # BASELINE.json configs[1] at a size the oracle finishes in seconds: trivial symmetry
    n = 96
    Cv, A, b = problems.theta_prime_problem(problems.gnp_adjacency(n, 0.5, seed=3))
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0))
    with pkg.Context(seed=5) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
    assert ref.nparts == (n * n + n) // 2 == P.nparts
    assert np.array_equal(P.matrix, ref.matrix)


def test_synthetic_scheme_fixed_point_and_idempotence(pkg, problems):
    n = 512
    Ls, d = problems.synthetic_jordan_partition(n, seed=1)
    Cv, A, b = problems.partition_as_sdp(Ls, seed=1)
    with pkg.Context(seed=9) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
        assert P.nparts == d and np.array_equal(P.matrix, Ls)
        # idempotence: feeding the result back changes nothing
        Cv2, A2, b2 = problems.partition_as_sdp(P.matrix.astype(np.int64), seed=2)
        P2 = pkg.admissible_subspace(Cv2, A2, b2, ctx=ctx)
        assert np.array_equal(P2.matrix, P.matrix)
        bd = pkg.blockDiagonalize(P, ctx=ctx)
        assert sorted(bd.blkSizes) == [1] * d


def test_dense_convenience_entry(pkg, problems, golden, gpu_ctx):
    lib = pkg.load_library()
    Cv, A, b = _problem(problems, "er5")
    n = 31
    m = A.shape[0]
    Af = np.asfortranarray(A)
    P = np.zeros(n * n, dtype=np.uint32)
    d = C.c_int64(0)
    it = C.c_int32(0)
    gpu_ctx.check(lib.sdpsr_admissible_subspace_dense(gpu_ctx._h, n, m, C.c_void_p(Cv.ctypes.data), C.c_void_p(Af.ctypes.data),
                                                      C.c_void_p(b.ctypes.data), 1.4901161193847656e-8, C.c_void_p(P.ctypes.data),
                                                      C.byref(d), C.byref(it), None, 0))
    assert d.value == 15
    assert np.array_equal(P.reshape(n, n, order="F"), golden["er5_P"])


# ------------------------------------------------------------------ edge cases
def test_tiny_and_degenerate_inputs(pkg, oracle, gpu_ctx):
    # 1 x 1
    P = pkg.Partition.from_matrix(np.array([[1]]), ctx=gpu_ctx)
    bd = pkg.blockDiagonalize(P, ctx=gpu_ctx)
    assert bd.blkSizes == [1] and abs(bd.blks[0][0][0, 0] - 1.0) < 1e-12
    # 2 x 2 full symmetric algebra: one block of size 2.  The Otsu threshold of the reference
    # (src/eigen_decomposition.jl:112-139) needs a gap between zero and non-zero couplings, which a
    # full matrix algebra does not have: the oracle itself ends in DimensionMismatch on ~60 % of the
    # draws here, so retry like the error text asks ("try again").
    P = pkg.Partition.from_matrix(np.array([[1, 2], [2, 3]]), ctx=gpu_ctx)
    bd = pkg.blockDiagonalize(P, ctx=gpu_ctx, retries=200)
    assert bd.blkSizes == [2]
    # identity-only partition (diagonal class, zeros elsewhere): n blocks?  dim = 1, generic
    # element = x*I has ONE eigenspace -> one block of size 1: 1*2/2 == dim(P)
    P = pkg.Partition.from_matrix(np.eye(5), ctx=gpu_ctx)
    assert P.nparts == 1
    bd = pkg.blockDiagonalize(P, ctx=gpu_ctx)
    assert bd.blkSizes == [1]
    # all-zero partition: dim 0, the decomposition cannot match -> DimensionMismatch, no crash
    Z = pkg.Partition(0, np.zeros((4, 4), dtype=np.uint32))
    with pytest.raises(pkg.DimensionMismatch):
        pkg.blockDiagonalize(Z, ctx=gpu_ctx)


def test_admissible_without_constraints_and_bad_arguments(pkg, problems, oracle, gpu_ctx):
    # m = 0 constraints: L is the whole space, x0 = 0, the loop only squares
    n = 12
    rng = np.random.default_rng(0)
    M = rng.integers(1, 4, size=(n, n))
    M = np.triu(M) + np.triu(M, 1).T
    Cv = M.astype(np.float64).ravel(order="F")
    A = np.zeros((0, n * n))
    b = np.zeros(0)
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(1))
    P = pkg.admissible_subspace(Cv, A, b, ctx=gpu_ctx, host_setup=True)
    assert P.nparts == ref.nparts and np.array_equal(P.matrix, ref.matrix)
    Pd = pkg.admissible_subspace(Cv, A, b, ctx=gpu_ctx)  # device setup with m = 0
    assert np.array_equal(Pd.matrix, ref.matrix)
    # @assert n^2 == length(C) (src/partitions.jl:118)
    with pytest.raises(ValueError):
        pkg.admissible_subspace(np.ones(10), np.zeros((1, 10)), np.zeros(1), ctx=gpu_ctx)
    # null pointers / bad sizes come back as BAD_ARGUMENT, never as a fault
    lib = pkg.load_library()
    d = C.c_int64(0)
    assert lib.sdpsr_partition_from_f64(gpu_ctx._h, 0, None, None, C.byref(d), 0) == 5
    assert lib.sdpsr_block_diagonalize(gpu_ctx._h, 0, None, 0, 1e-8, None, None, None, None, 0) == 5


@pytest.mark.gpu
def test_admissible_nonsymmetric_labels_square_literally(pkg, oracle, gpu_ctx):
    """Non-symmetric C through admissible_subspace: the setup symmetrises it (src/partitions.jl:129-134),
    so the loop's labels are symmetric here.  The loop on non-symmetric labels (X*X literally, the left
    operand gathered from the transposed labels) is covered by test_gpu_squares.py, which hands it a
    non-symmetric C_L directly."""
    rng = np.random.default_rng(5)
    for n in (9, 16):
        M = rng.integers(0, 3, size=(n, n))
        assert not np.array_equal(M, M.T)
        Cv = M.astype(np.float64).ravel(order="F")
        A = np.zeros((0, n * n))
        b = np.zeros(0)
        ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(2))
        P = pkg.admissible_subspace(Cv, A, b, ctx=gpu_ctx)
        assert P.nparts == ref.nparts
        assert np.array_equal(P.matrix, ref.matrix)
        with pkg.Context(seed=3, square_mode=pkg.SQUARE_F32) as ctx32:
            P32 = pkg.admissible_subspace(Cv, A, b, ctx=ctx32)
            assert np.array_equal(P32.matrix, ref.matrix)


@pytest.mark.gpu
def test_partition_checksum_matches_restatement(pkg, gpu_ctx):
    """sdpsr_partition_checksum (the probabilistic == of src/partitions.jl:16-17 used to agree
    restarts across GPUs) against its formula in NumPy and against the torch stand-in."""
    import torch
    rng = np.random.default_rng(3)
    for n in (1, 7, 300):
        lab = rng.integers(0, 50, size=n * n).astype(np.uint32)
        e = np.arange(n * n, dtype=np.uint64)
        l = lab.astype(np.uint64) + np.uint64(1)
        with np.errstate(over="ignore"):
            h1 = int((l * (e * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1342543DE82EF95))).sum(dtype=np.uint64))
            h2 = int(((l * l + np.uint64(0x27D4EB2F165667C5)) *
                      ((e ^ (e >> np.uint64(13))) * np.uint64(0xBF58476D1CE4E5B9) + np.uint64(0x94D049BB133111EB))).sum(dtype=np.uint64))
        got = pkg.partition_checksum(lab, ctx=gpu_ctx)
        assert got == (h1, h2)
        dev = pkg.partition_checksum(torch.from_numpy(lab.astype(np.int32)).cuda(), ctx=gpu_ctx)
        assert dev == (h1, h2)
        tw = pkg.parallel.torch_checksum(torch.from_numpy(lab.astype(np.int64)))
        assert (tw[0] % 2**64, tw[1] % 2**64) == (h1, h2)
        lab2 = lab.copy()
        lab2[n * n // 2] += 1
        assert pkg.partition_checksum(lab2, ctx=gpu_ctx) != (h1, h2)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["two_stage", "outer", "chunk"])
@pytest.mark.parametrize("name", ["er7", "esc16j", "numerical_issues"])
def test_basis_image_kernel_variants(pkg, oracle, golden, name, variant):
    """The three basis_image kernels (class sums + contraction; outer products per class for many
    small classes; sorted chunks with partial sums) against Q_k' 1[P==i] Q_k (src/diagonalize.jl:64-89).
    The automatic choice only reaches the last two for shapes far beyond these sizes."""
    L = golden[f"{name}_P"]
    P = pkg.Partition(int(L.max()), L.copy())
    kw = {"epsilon": 1e-7} if name == "numerical_issues" else {}
    with pkg.Context(seed=4, basis_image_kernel=variant) as ctx:  # sdpsr_opts.basis_image_kernel
        bd = pkg.blockDiagonalize(P, ctx=ctx, **kw)
    assert sorted(bd.blkSizes) == list(golden[f"{name}_blk"])
    Po = oracle.Partition(P.nparts, L.astype(np.int64))
    ref = oracle.basis_image([np.asarray(q) for q in bd.Q_hat], Po)
    for i in range(P.nparts):
        for k in range(len(bd.blkSizes)):
            assert np.allclose(bd.blks[i][k], ref[i][k], atol=1e-10), (variant, i, k)


@pytest.mark.gpu
def test_nonsymmetric_partition_rejected_by_both_drivers(pkg, gpu_ctx):
    """A non-symmetric partition has a generic element with a complex spectrum
    (src/eigen_decomposition.jl:247-253): InvalidDecompositionField from the dense driver (small n)
    and from the module-compression driver (n >= 512, verdict read with the first Gram matrix)."""
    rng = np.random.default_rng(11)
    for n in (24, 640):
        M = rng.integers(1, 4, size=(n, n)).astype(np.uint32)
        assert not np.array_equal(M, M.T)
        P = pkg.Partition(3, M)
        with pytest.raises(pkg.InvalidDecompositionField):
            pkg.blockDiagonalize(P, ctx=gpu_ctx)
    # the ctx stays usable afterwards
    Ls = np.array([[1, 2], [2, 1]], dtype=np.uint32)
    bd = pkg.blockDiagonalize(pkg.Partition(2, Ls), ctx=gpu_ctx, retries=50)
    assert sorted(bd.blkSizes) == [1, 1]


@pytest.mark.gpu
def test_device_resident_labels_copy_and_symmetry_check(pkg, gpu_ctx, golden):
    """blockDiagonalize on device-resident labels copies them and checks their symmetry in one tile
    pass (16-byte accesses when n % 4 == 0, scalar otherwise); the label pass of refine! does the
    same for the projection step.  Non-symmetric labels -> InvalidDecompositionField from both
    drivers, a mismatch in the last row/column included; symmetric ones go through unchanged."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(12)
    for n in (24, 57, 640, 642):
        M = rng.integers(1, 4, size=(n, n)).astype(np.uint32)
        M = np.triu(M) + np.triu(M, 1).T  # symmetric ...
        M[n - 1, 0] = 1 + (M[0, n - 1] % 3)  # ... but for one entry in the last row
        assert not np.array_equal(M, M.T)
        t = torch.from_numpy(np.asfortranarray(M).ravel(order="F").view(np.int32).copy()).to(dev)
        lib = gpu_ctx._lib
        nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        st = lib.sdpsr_block_diagonalize(gpu_ctx._h, n, C.c_void_p(t.data_ptr()), 3, 1e-8, C.byref(nb), C.byref(ssq),
                                         C.byref(ss), None, pkg.MEM_DEVICE)
        assert st == 1, (n, st)  # SDPSR_INVALID_DECOMPOSITION_FIELD
        assert "not symmetric" in lib.sdpsr_last_error(gpu_ctx._h).decode(), n
    for name in ("er5", "er7"):  # symmetric, n = 31 (scalar tiles) and 57
        Lm = golden[f"{name}_P"]
        n = Lm.shape[0]
        t = torch.from_numpy(np.asfortranarray(Lm).ravel(order="F").astype(np.int32)).to(dev)
        for attempt in range(20):
            nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
            st = lib.sdpsr_block_diagonalize(gpu_ctx._h, n, C.c_void_p(t.data_ptr()), int(Lm.max()), 1e-8, C.byref(nb),
                                             C.byref(ssq), C.byref(ss), None, pkg.MEM_DEVICE)
            if st == 0:
                break
        assert st == 0, lib.sdpsr_last_error(gpu_ctx._h)
        sizes = np.zeros(nb.value, dtype=np.int32)
        gpu_ctx.check(lib.sdpsr_block_sizes(gpu_ctx._h, sizes.ctypes.data_as(C.c_void_p)))
        assert sorted(int(x) for x in sizes) == list(golden[f"{name}_blk"])


@pytest.mark.gpu
def test_seed_and_external_stream(pkg, problems, golden):
    """sdpsr_set_seed reproduces / changes the draws; sdpsr_set_stream runs everything (including
    the compression driver with its side stream) on a caller-owned HIP stream."""
    import torch
    L = golden["er5_P"]
    P = pkg.Partition(int(L.max()), L.copy())
    with pkg.Context(seed=1) as ctx:
        ctx.set_seed(123)
        a = pkg.randomize(P, ctx=ctx)
        ctx.set_seed(123)
        b = pkg.randomize(P, ctx=ctx)
        ctx.set_seed(124)
        c = pkg.randomize(P, ctx=ctx)
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        # same class -> same value, zero class -> 0.0 (src/abstract_part.jl:107-110)
        for lbl in range(1, P.nparts + 1):
            assert np.unique(a[L == lbl]).size == 1
    stream = torch.cuda.Stream()
    with pkg.Context(seed=5) as ctx:
        ctx.set_stream(stream.cuda_stream)
        Cv, A, bb = problems.theta_prime_problem(problems.er_graph_adjacency(5))
        Pe = pkg.admissible_subspace(Cv, A, bb, ctx=ctx)
        assert np.array_equal(Pe.matrix, golden["er5_P"])
        Ls, d = problems.synthetic_jordan_partition(1024, seed=2)
        bd = pkg.blockDiagonalize(pkg.Partition(d, Ls.astype(np.uint32)), ctx=ctx)
        assert len(bd.blkSizes) == d and set(bd.blkSizes) == {1}
        ctx.synchronize()
        ctx.set_stream(0)  # back to the ctx's own stream
        bd2 = pkg.blockDiagonalize(pkg.Partition(int(L.max()), L.copy()), ctx=ctx)
        assert sorted(bd2.blkSizes) == list(golden["er5_blk"])


@pytest.mark.gpu
def test_error_paths(pkg, problems, golden):
    """Status codes that mirror the reference's exceptions / guards: NOT_CONVERGED when the
    iteration cap is hit, BAD_STATE for block_images without a decomposition, a library exception
    (DimensionMismatch / NumericalInconsistency, src/diagonalize.jl:4-9,
    src/eigen_decomposition.jl:264-270) for a symmetric partition that is not an algebra --
    and the ctx stays usable after each of them."""
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(7))
    with pkg.Context(seed=3, max_iters=1) as ctx:
        with pytest.raises(pkg.NotConverged):
            pkg.admissible_subspace(Cv, A, b, ctx=ctx)  # ER(7) needs 5 iterations
    with pkg.Context(seed=3) as ctx:
        lib = ctx._lib
        buf = np.zeros(4)
        st = lib.sdpsr_block_images(ctx._h, C.c_void_p(buf.ctypes.data), None, None, pkg.MEM_HOST)
        assert st == 10 and b"sdpsr_block_diagonalize" in lib.sdpsr_last_error(ctx._h)
        rng = np.random.default_rng(2)
        n = 40
        M = rng.integers(1, 4, size=(n, n))
        M = np.triu(M) + np.triu(M, 1).T  # symmetric, 3 classes, not closed under products
        with pytest.raises((pkg.DimensionMismatch, pkg.NumericalInconsistency)):
            pkg.blockDiagonalize(pkg.Partition(3, M.astype(np.uint32)), ctx=ctx)
        L = golden["er3_P"]
        bd = pkg.blockDiagonalize(pkg.Partition(int(L.max()), L.copy()), ctx=ctx)
        assert sorted(bd.blkSizes) == list(golden["er3_blk"])


@pytest.mark.parametrize("name", ["petersen", "er3", "er5", "er7", "esc16j"])
def test_projection_skipped_once_the_basis_is_class_constant(pkg, problems, golden, name):
    """Once every U_k is constant on the classes of S the projection half of the loop cannot refine S (x - U U'x stays in
    span(S)); the loop checks that on the device and then iterates on the square alone.  Same canonical partition, same
    iteration count and same dimension trajectory as with SDPSR_FLAG_ALWAYS_PROJECT (the projection in every iteration,
    src/partitions.jl:159-164), over several seeds; both against the golden matrix."""
    Cv, A, b = _problem(problems, name)
    Lg = golden[f"{name}_P"].astype(np.int64)
    setup = pkg.admissible_setup(Cv, A, b)
    outs = {}
    for flags in (0, pkg._lib.FLAG_ALWAYS_PROJECT):
        outs[flags] = []
        for seed in (1, 2, 3, 4):
            with pkg.Context(seed=seed, flags=flags) as ctx:
                P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
                assert np.array_equal(P.matrix, Lg), (name, flags, seed)
                outs[flags].append((P.iterations, tuple(P.dims)))
    assert outs[0] == outs[pkg._lib.FLAG_ALWAYS_PROJECT], outs


def test_batch_error_paths(pkg, problems):
    """sdpsr_jordan_reduce_batch: bad restart counts are BAD_ARGUMENT; a restart that fails reports ITS status (here
    NOT_CONVERGED under an iteration cap of 1 on ER(7), which needs 5 iterations) in status[i] and as the call's return
    value (or, as sdpsr_jordan_reduce does, the failure of blockDiagonalize on the unconverged partition), and the ctx (and the restarts' ctxs inside it) stay usable:
    the same call without the cap succeeds afterwards on a fresh ctx sharing nothing; sdpsr_square_i8_symmetric rejects
    null pointers and batch sizes outside 1..8."""
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(7))
    setup = pkg.admissible_setup(Cv, A, b)
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    with pkg.Context(seed=3) as ctx:
        lib = ctx._lib
        dd, st = (C.c_int64 * 2)(), (C.c_int32 * 2)()
        args = (C.c_void_p(CL.ctypes.data), C.c_void_p(X0L.ctypes.data), C.c_void_p(Uf.ctypes.data), U.shape[1], 1.5e-8, 1.5e-8)
        for R in (0, 65):
            assert lib.sdpsr_jordan_reduce_batch(ctx._h, R, None, n, *args, None, dd, None, None, None, None, None, None, st, 0) == 5
        assert lib.sdpsr_jordan_reduce_batch(ctx._h, 2, None, n, *args, None, None, None, None, None, None, None, None, st, 0) == 5
        x = np.zeros(16, dtype=np.int8)
        o = np.zeros(16, dtype=np.int32)
        assert lib.sdpsr_square_i8_symmetric(ctx._h, 4, 0, C.c_void_p(x.ctypes.data), C.c_void_p(o.ctypes.data), 0) == 5
        assert lib.sdpsr_square_i8_symmetric(ctx._h, 4, 9, C.c_void_p(x.ctypes.data), C.c_void_p(o.ctypes.data), 0) == 5
        assert lib.sdpsr_square_i8_symmetric(ctx._h, 4, 1, None, C.c_void_p(o.ctypes.data), 0) == 5
    with pkg.Context(seed=3, max_iters=1) as ctx:
        res = pkg.jordan_reduce_batch(Cv, A, b, restarts=2, seeds=[1, 2], ctx=ctx, setup=setup)
        # the loop stops unconverged; blockDiagonalize then runs on a partition that is not an algebra: its own failure
        # (DimensionMismatch / NumericalInconsistency) or, had it passed, NOT_CONVERGED -- per restart, never OK
        assert all(x["status"] in (2, 3, 9) for x in res), [x["status"] for x in res]
    with pkg.Context(seed=3) as ctx:
        res = pkg.jordan_reduce_batch(Cv, A, b, restarts=2, seeds=[1, 2], ctx=ctx, setup=setup)
        assert [x["status"] for x in res] == [0, 0] and all(x["P"].nparts == 18 for x in res)


# ------------------------------------------------ ctx contract (include/sdpsr.h:20-25)
def test_two_contexts_from_two_threads(pkg, golden):
    """Distinct ctxs may be driven from distinct host threads (no process-global state: kernel
    attributes per device in sdpsr_create, graph cache inside the ctx)."""
    import threading
    res, errs = {}, []

    def work(tag, name, seed):
        try:
            L = golden[f"{name}_P"]
            with pkg.Context(seed=seed) as ctx:
                for _ in range(3):
                    bd = pkg.blockDiagonalize(pkg.Partition(int(L.max()), L.copy()), ctx=ctx)
                    assert sorted(bd.blkSizes) == list(golden[f"{name}_blk"])
                x = np.random.default_rng(seed).random((200, 200))
                x = x + x.T
                w = np.empty(200)
                v = np.empty(200 * 200)
                xf = _fl(x, np.float64)  # kept alive across the call: the library reads it through a raw pointer
                ctx.check(ctx._lib.sdpsr_syev_f64(ctx._h, 200, C.c_void_p(xf.ctypes.data),
                                                  C.c_void_p(w.ctypes.data), C.c_void_p(v.ctypes.data), pkg.MEM_HOST))
                res[tag] = float(np.abs(w - np.linalg.eigvalsh(x)).max())
        except Exception as e:  # noqa: BLE001
            errs.append((tag, repr(e)))

    ts = [threading.Thread(target=work, args=(i, nm, 10 + i)) for i, nm in enumerate(["er5", "er7", "esc16j", "er3"])]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errs == []
    assert all(res[i] < 1e-10 for i in range(4)), res


def test_device_inputs_from_an_async_torch_kernel(pkg, problems, golden):
    """MEM_DEVICE arguments produced by torch kernels that may still be running when the call is
    made: the wrapper orders ctx's stream behind torch's current stream (sdpsr_wait_stream), and
    every entry point returns with its outputs complete."""
    import torch
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(7))
    n, CL, X0L, U = pkg.admissible_setup(Cv, A, b)
    dev = torch.device("cuda:0")
    big = torch.randn(4096, 4096, device=dev)
    with pkg.Context(seed=5) as ctx:
        for rep in range(3):
            junk = big @ big  # keeps torch's stream busy for a while
            tCL = torch.from_numpy(CL).to(dev) + junk[0, 0] * 0.0  # queued behind the GEMM
            tX0 = torch.from_numpy(X0L).to(dev) * 1.0
            tU = torch.from_numpy(np.asfortranarray(U).ravel(order="F").copy()).to(dev).view(U.shape[1], -1).t()
            P = pkg.admissible_subspace(None, None, None, ctx=ctx, setup=(n, tCL, tX0, tU))
            assert P.nparts == 18
            assert np.array_equal(P.matrix.cpu().numpy().astype(np.uint32), golden["er7_P"])
            del junk


def test_batch_device_inputs_from_an_async_torch_kernel(pkg, problems, golden):
    """The same ordering rule for sdpsr_jordan_reduce_batch: the inputs are produced by torch kernels queued behind a long
    GEMM; ctx's stream is ordered behind torch's (sdpsr_wait_stream) and EVERY restart's stream must inherit that -- a
    restart that started early would read unfinished inputs and end on another partition."""
    import torch
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(7))
    n, CL, X0L, U = pkg.admissible_setup(Cv, A, b)
    dev = torch.device("cuda:0")
    big = torch.randn(6144, 6144, device=dev)
    R = 3
    gold = torch.from_numpy(np.ascontiguousarray(golden["er7_P"].ravel(order="F")).astype(np.int32)).to(dev)
    with pkg.Context(seed=5) as ctx:
        lib = ctx._lib
        for rep in range(3):
            junk = big @ big
            tCL = torch.from_numpy(CL).to(dev) + junk[0, 0] * 0.0  # queued behind the GEMM
            tX0 = torch.from_numpy(X0L).to(dev) * 1.0
            tU = (torch.from_numpy(np.ascontiguousarray(U.T)).to(dev) + junk[1, 1] * 0.0).contiguous()
            tPs = [torch.zeros(n * n, dtype=torch.int32, device=dev) for _ in range(R)]
            ctx.check(lib.sdpsr_wait_stream(ctx._h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            pP = (C.c_void_p * R)(*[t.data_ptr() for t in tPs])
            dd, st = (C.c_int64 * R)(), (C.c_int32 * R)()
            lib.sdpsr_jordan_reduce_batch(ctx._h, R, None, n, C.c_void_p(tCL.data_ptr()), C.c_void_p(tX0.data_ptr()), C.c_void_p(tU.data_ptr()), U.shape[1],
                                          1.5e-8, 1.5e-8, C.cast(pP, C.c_void_p), dd, None, None, None, None, None, None, st, 1)
            for i in range(R):
                assert st[i] in (0, 2, 3), st[i]  # blockDiagonalize may fail at random; the partition must be right
                assert dd[i] == 18 and bool((tPs[i] == gold).all()), (rep, i)
            del junk


def test_sort_based_refine_matches_oracle(pkg, oracle):
    """The relabels of the many-classes regime -- the hand-written bucketed grouping (kernels_refine_bucket.hip, the
    default there) and hipCUB's radix sort (kernels_refine_sort.hip, comparison) -- against the oracle's canonical
    labels: forced on inputs with few, many and all-distinct classes, a zero class, skewed class sizes (one class
    holding half of the entries: a bucket far beyond the resolver's table), and through refine! (pairs of labels)."""
    rng = np.random.default_rng(21)
    n = 640  # n^2 >= 2^18: the relabel path is eligible
    cases = {
        "few": rng.integers(0, 7, size=(n, n)).astype(np.float64) * 0.25,
        "many": rng.integers(0, 150000, size=(n, n)).astype(np.float64),
        "distinct": rng.permutation(n * n).reshape(n, n).astype(np.float64) + 1.0,
        "skewed": np.where(rng.random((n, n)) < 0.5, 7.0, rng.integers(1, 200000, size=(n, n)).astype(np.float64)),
    }
    cases["many"][rng.random((n, n)) < 0.1] = 0.0
    # classes of ~64 and ~500 entries: bucket and sub-pass sizes vary by sqrt(entries per class * mean) -- sub-pass lists
    # walked in batches, buckets beyond the register file (round 5: such inputs fell back to the radix sort)
    cases["mult64"] = rng.integers(1, n * n // 64, size=(n, n)).astype(np.float64)
    cases["mult500"] = rng.integers(1, n * n // 500, size=(n, n)).astype(np.float64)
    for path in ("bucket", "sort", "auto"):
        with pkg.Context(seed=2, refine_path=path) as ctx:  # sdpsr_opts.refine_path
            for name, M in cases.items():
                P = pkg.Partition.from_matrix(M, ctx=ctx)
                R = oracle.partition_from_values(M)
                assert P.nparts == R.nparts, (name, path)
                assert np.array_equal(P.matrix, R.matrix), (name, path)
            A = rng.integers(0, 900, size=(n, n))
            B = rng.integers(0, 900, size=(n, n))
            P1 = pkg.Partition.from_matrix(A, ctx=ctx)
            P2 = pkg.Partition.from_matrix(B, ctx=ctx)
            R = oracle.refine(oracle.partition_from_labels(A), oracle.partition_from_labels(B))
            P3 = pkg.refine(P1, P2, ctx=ctx)
            assert P3.nparts == R.nparts and np.array_equal(P3.matrix, R.matrix), path


def test_lds_table_insert_kernel_matches_oracle(pkg, oracle):
    """refine_insert_mid_kernel (array sources of >= 2^20 entries, tables of <= 2^16 slots): one workgroup per CU with every
    signature in LDS, preloaded from the workgroups that go first.  Canonical labels against the oracle at 3 ... 7000 classes
    (7000: more than the 8192-slot LDS table takes -- the overflow goes to the global table entry by entry), with a zero class,
    a class that first appears in the very last entry, classes absent from the first 16 384 entries (not preloaded) and a
    ragged length; every input twice in one ctx (first call: the table size is a guess; second: predicted) and through the
    comparison paths (no such kernel / no first workgroups)."""
    rng = np.random.default_rng(55)
    n = 1100  # 1.21 M entries, not a multiple of the 8192-entry chunk
    cases = {}
    for d in (3, 40, 600, 3000, 7000):
        M = rng.integers(1, d + 1, size=(n, n)).astype(np.float64)
        M[rng.random((n, n)) < 0.05] = 0.0
        cases["d%d" % d] = M
    late = rng.integers(1, 200, size=(n, n)).astype(np.float64)
    late[:, :20] = rng.integers(1, 20, size=(n, 20))  # the first 22 000 entries (column-major) hold 19 of the classes
    late[n - 1, n - 1] = 1e6                        # a class of one entry, the last
    cases["late"] = late
    refs = {k: oracle.partition_from_values(M) for k, M in cases.items()}
    for path in ("auto", "no_mid", "mid_no_first"):
        with pkg.Context(seed=6, refine_path=path) as ctx:
            for name in ("d3000", "d3", "d7000", "d40", "late", "d600"):  # class counts up and down: the prediction is wrong every time ...
                for rep in range(2):                                      # ... and right the second time
                    P = pkg.Partition.from_matrix(cases[name], ctx=ctx)
                    assert P.nparts == refs[name].nparts, (name, path, rep)
                    assert np.array_equal(P.matrix, refs[name].matrix), (name, path, rep)


@pytest.mark.parametrize("n", [37, 300, 1500])
def test_bucketed_refine_small_and_ragged_sizes(pkg, oracle, n):
    """The bucketed grouping forced at sizes below its regime (one chunk, 16 buckets) and at a ragged size whose last
    chunk and last rank block are partial; all-zero and all-equal inputs."""
    rng = np.random.default_rng(n)
    with pkg.Context(seed=4, refine_path="bucket") as ctx:
        for M in (rng.integers(0, 5, size=(n, n)).astype(np.float64), rng.integers(0, n * n // 3, size=(n, n)).astype(np.float64),
                  np.zeros((n, n)), np.full((n, n), 3.5)):
            P = pkg.Partition.from_matrix(M, ctx=ctx)
            R = oracle.partition_from_values(M)
            assert P.nparts == R.nparts and np.array_equal(P.matrix, R.matrix), n


def test_bucketed_refine_beyond_the_one_level_front_end(pkg, oracle):
    """len > 22.7 M entries: the grouping keeps the two-level scatter + one-workgroup-per-bucket resolver of round 4 in front of the
    round-5 back end (rank records, ballot label pass).  n = 4800 (23.04 M entries), ~len / 2 classes and a zero class."""
    n = 4800
    rng = np.random.default_rng(99)
    M = rng.integers(0, n * n // 2, size=(n, n)).astype(np.float64)
    with pkg.Context(seed=4, refine_path="bucket") as ctx:
        P = pkg.Partition.from_matrix(M, ctx=ctx)
    R = oracle.partition_from_values(M)
    assert P.nparts == R.nparts and np.array_equal(P.matrix, R.matrix)


def test_syev_alternating_orders_replay_their_graphs(pkg):
    """A caller that alternates between a few orders (the dense driver on problems of different size) must pay the
    construction of the tridiagonalisation's hipGraph once per order (twice where the ctx's grow-only buffers were still
    growing): from the third round on every call is a replay (hit / miss counters of the ctx's cache), and no
    device-resident call takes more than twice the median of its order.  (The 75-95 ms calls of
    profiles/r03_stedc_check.txt are not graph rebuilds -- that run built 3 graphs in 24 calls, 4 ms each; they come and go
    with the host's BLAS thread pool, which tools/stedc_check.py used for its LAPACK comparison between the calls with
    128 threads on the box's 16-core share.)"""
    import time
    import torch
    lib = pkg.load_library()
    prof = pkg._lib.load_prof_library()
    orders = (640, 900, 1152)
    rng = np.random.default_rng(5)
    with pkg.Context(seed=1) as ctx:
        mats = {}
        for n in orders:
            A = rng.standard_normal((n, n))
            mats[n] = torch.from_numpy(np.asfortranarray((A + A.T) / 2).ravel(order="F").copy()).cuda()
        w = {n: torch.empty(n, dtype=torch.float64, device="cuda") for n in orders}
        V = {n: torch.empty(n * n, dtype=torch.float64, device="cuda") for n in orders}
        times = {n: [] for n in orders}
        st = (C.c_double * 3)()
        for rnd in range(6):
            for n in orders:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.check(lib.sdpsr_syev_f64(ctx._h, n, C.c_void_p(mats[n].data_ptr()), C.c_void_p(w[n].data_ptr()), C.c_void_p(V[n].data_ptr()), 1))
                times[n].append((time.perf_counter() - t0) * 1e3)
            if rnd == 1:
                ctx.check(prof.sdpsr_profile_sytrd_graphs(ctx._h, st))
                misses_settled = st[1]
        ctx.check(prof.sdpsr_profile_sytrd_graphs(ctx._h, st))
        # one build per order, plus one more for every order whose graph was built before the ctx's grow-only padded
        # buffers reached their final size (the first round visits the orders in increasing size): settled after round 2
        assert st[1] == misses_settled <= 2 * len(orders), (st[0], st[1], misses_settled)
        assert st[0] >= 4 * len(orders)
        for n in orders:
            rest = sorted(times[n][2:])
            med = rest[len(rest) // 2]
            assert max(rest) <= 2.0 * med + 0.5, (n, times[n])
        # spectrum still right after the replays
        for n in orders:
            ref = np.linalg.eigvalsh(mats[n].cpu().numpy().reshape(n, n, order="F"))
            assert np.abs(w[n].cpu().numpy() - ref).max() <= 1e-12 * n


def test_syev_nonfinite_input_is_reported(pkg):
    """NaN / Inf in the matrix: the own divide and conquer must not return garbage eigenpairs with a clean status
    (rocSOLVER's drivers report SOLVER_ERROR there; so does the own path now, through its eigenvalue check)."""
    lib = pkg.load_library()
    n = 300
    A = np.random.default_rng(1).standard_normal((n, n))
    A = (A + A.T) / 2
    for bad in (np.nan, np.inf):
        B = A.copy()
        B[17, 17] = bad
        Bf = np.asfortranarray(B)
        w = np.zeros(n)
        V = np.zeros((n, n), order="F")
        with pkg.Context(seed=1) as ctx:
            st = lib.sdpsr_syev_f64(ctx._h, n, C.c_void_p(Bf.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0)
        assert st == 7, st  # SDPSR_SOLVER_ERROR


# ------------------------------------------------ complex path (src/compat.jl:26-32,54-57)
def _s3_cayley_labels():
    import itertools
    perms = list(itertools.permutations(range(3)))
    idx = {p: i for i, p in enumerate(perms)}

    def mul(a, b):
        return tuple(a[b[i]] for i in range(3))

    def inv(a):
        r = [0] * 3
        for i, x in enumerate(a):
            r[x] = i
        return tuple(r)

    return np.array([[idx[mul(inv(g), h)] + 1 for h in perms] for g in perms])


def test_complex_block_diagonalize_pins_and_images(pkg, oracle, gpu_ctx):
    """test/runtests.jl:43-57 on the device: [1,1,1] for the 4 x 4 partition and for C3 (real
    request: InvalidDecompositionField); plus the group algebra of S3 (non-symmetric partition,
    C + C + M_2(C): blocks [1,1,2]).  Checked beyond the sizes: blks == Q_k^H 1[P==i] Q_k with
    the returned Q_hat, orthonormal columns, and the complex spectrum invariant (block spectra of
    sum_i x_i blks[i][k] = distinct eigenvalues of sum_i x_i 1[P==i], 1e-6 rel)."""
    P4 = np.array([[1, 2, 3, 2], [2, 1, 2, 3], [3, 2, 1, 2], [2, 3, 2, 1]])
    C3 = np.array([[1, 3, 2], [2, 1, 3], [3, 2, 1]])
    cases = [(P4, [1, 1, 1]), (C3, [1, 1, 1]), (_s3_cayley_labels(), [1, 1, 2])]
    with pytest.raises(pkg.InvalidDecompositionField):
        pkg.blockDiagonalize(pkg.Partition.from_matrix(C3, ctx=gpu_ctx), ctx=gpu_ctx)
    for Lm, expect in cases:
        P = pkg.Partition.from_matrix(Lm, ctx=gpu_ctx)
        for rep in range(5):
            bd = pkg.blockDiagonalize(P, complex=True, ctx=gpu_ctx, retries=2)
            assert sorted(bd.blkSizes) == expect
            Pd = bd.partition
            ref_pd = oracle.desymmetrize(oracle.partition_from_labels(Lm), rng=np.random.default_rng(rep))
            assert Pd.nparts == ref_pd.nparts and np.array_equal(Pd.matrix, ref_pd.matrix)
            assert sum(s * s for s in bd.blkSizes) == Pd.nparts
            for k, q in enumerate(bd.Q_hat):
                assert np.allclose(q.conj().T @ q, np.eye(q.shape[1]), atol=1e-10)
                for i in range(Pd.nparts):
                    M = (np.asarray(Pd.matrix) == i + 1).astype(np.float64)
                    assert np.allclose(bd.blks[i][k], q.conj().T @ M @ q, atol=1e-10)
            x = np.random.default_rng(7 + rep).random(Pd.nparts)
            full, blk = oracle.spectrum_invariant_complex(oracle.Partition(Pd.nparts, np.asarray(Pd.matrix).astype(np.int64)), bd.blks, x)
            assert len(full) == len(blk)
            assert np.allclose(full, blk, rtol=1e-6, atol=1e-9)


def test_complex_heev_against_lapack_through_block_images(pkg, gpu_ctx):
    """A commutative non-symmetric scheme of order 63 (cyclic group Z_63: 63 classes, 63 blocks of
    size 1): exercises the Hermitian Jacobi eigensolver near its size limit."""
    n = 63
    i = np.arange(n)
    Lm = (i[None, :] - i[:, None]) % n + 1
    P = pkg.Partition.from_matrix(Lm, ctx=gpu_ctx)
    bd = pkg.blockDiagonalize(P, complex=True, ctx=gpu_ctx, retries=2)
    assert bd.blkSizes == [1] * n
    x = np.random.default_rng(3).random(n)
    A = np.concatenate([[0.0], x])[np.asarray(bd.partition.matrix)]
    ev = np.array([sum(x[c] * bd.blks[c][k][0, 0] for c in range(n)) for k in range(n)])
    ref = np.linalg.eigvals(A)
    assert np.allclose(np.sort_complex(np.round(ev, 8)), np.sort_complex(np.round(ref, 8)), atol=1e-7)


@pytest.mark.gpu
def test_complex_path_beyond_one_workgroup(pkg, problems, oracle, gpu_ctx):
    """Orders n > 64 of blockDiagonalize(P; complex=true): the Hermitian eigensolver runs through the
    real symmetric embedding (2n x 2n, the real dense solver), eigenspaces are extracted per cluster
    by a pivoted Cholesky of the Gram matrix, Q'AQ goes through fp64 MFMA GEMMs.  Z_100 (100 blocks of
    size 1, simple spectrum) and C[S3] (x) {I, J - I}_12 (n = 72, non-commutative, eigenspaces of
    dimension up to 22): block sizes against the oracle's, orthonormal Q_hat, blks == Q_k^H 1[P==i] Q_k,
    complex spectrum invariant."""
    n = 100
    i = np.arange(n)
    cases = [((i[None, :] - i[:, None]) % n + 1, [1] * n)]
    Ls3, _ = problems.kron_with_complete(_s3_cayley_labels(), 12, seed=3)
    ref = oracle.block_diagonalize_complex(oracle.partition_from_labels(Ls3), rng=np.random.default_rng(1))
    cases.append((Ls3, sorted(int(b) for b in ref[0])))
    assert cases[1][1] == [1, 1, 1, 1, 2, 2]
    Lbig, _ = problems.kron_with_complete(_s3_cayley_labels(), 64, seed=4)  # n = 384: embedded order 768, eigenspaces up to 126
    cases.append((Lbig, [1, 1, 1, 1, 2, 2]))
    for Lm, expect in cases:
        P = pkg.Partition.from_matrix(Lm, ctx=gpu_ctx)
        for rep in range(2):
            bd = pkg.blockDiagonalize(P, complex=True, ctx=gpu_ctx, retries=3)
            assert sorted(bd.blkSizes) == expect
            Pd = bd.partition
            assert sum(s * s for s in bd.blkSizes) == Pd.nparts
            for k, q in enumerate(bd.Q_hat):
                assert np.allclose(q.conj().T @ q, np.eye(q.shape[1]), atol=1e-9)
                for c in range(0, Pd.nparts, max(1, Pd.nparts // 12)):
                    M = (np.asarray(Pd.matrix) == c + 1).astype(np.float64)
                    assert np.allclose(bd.blks[c][k], q.conj().T @ M @ q, atol=1e-9)
            x = np.random.default_rng(17 + rep).random(Pd.nparts)
            full, blk = oracle.spectrum_invariant_complex(oracle.Partition(Pd.nparts, np.asarray(Pd.matrix).astype(np.int64)), bd.blks, x)
            assert len(full) == len(blk)
            assert np.allclose(full, blk, rtol=1e-6, atol=1e-8)


@pytest.mark.gpu
def test_projection_on_the_lower_triangle(pkg, problems, golden):
    """With symmetric labels and symmetric basis matrices the projection step runs on the lower
    triangle: vouched for by the caller (sdpsr_hint_symmetric_basis, set by the wrapper from the
    host setup), or found by the randomized probe of the first iteration (plain tuple: no hint).
    Both must give the golden partition, as must a basis that is NOT symmetric (probe says no)."""
    for name, q in (("er5", 5), ("er7", 7)):
        Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(q))
        setup = pkg.admissible_setup(Cv, A, b)
        assert setup.basis_symmetric and setup.inputs_symmetric and setup.hint == 3
        for seed in (1, 2, 3):
            with pkg.Context(seed=seed) as ctx:
                P1 = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)            # hint
                P2 = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=tuple(setup))     # probe
                assert np.array_equal(P1.matrix, golden[f"{name}_P"]) and np.array_equal(P2.matrix, golden[f"{name}_P"])
    # a non-symmetric constraint matrix: U has a non-symmetric column, the projected element is not
    # symmetric, the probe must keep the full pass (result: the oracle's partition, checked by dim here
    # through the device-setup path, which never hints)
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(5))
    n = int(round(np.sqrt(A.shape[1])))
    extra = np.zeros((n, n))
    extra[0, 1] = 1.0  # E_01 alone: not symmetric
    A2 = np.vstack([A, extra.ravel(order="F")[None, :]])
    b2 = np.concatenate([b, [0.0]])
    s2 = pkg.admissible_setup(Cv, A2, b2)
    assert not s2.basis_symmetric
    with pkg.Context(seed=4) as ctx:
        Pa = pkg.admissible_subspace(Cv, A2, b2, ctx=ctx, setup=s2)
        Pb = pkg.admissible_subspace(Cv, A2, b2, ctx=ctx)  # device setup, probe
        assert Pa.nparts == Pb.nparts and np.array_equal(Pa.matrix, Pb.matrix)


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,G,d", [(4096, 34, 1, 34), (4104, 36, 1, 36), (4104, 20, 2, 36), (777, 7, 4, 11),
                                     (100, 64, 1, 5), (1000, 48, 1, 3000), (65, 1, 1, 2), (1030, 16, 4, 200),
                                     (513, 17, 2, 1)])
def test_label_product_on_the_matrix_cores(pkg, gpu_ctx, n, w, G, d):
    """Y = A(v) W straight from the labels (randomize!, src/abstract_part.jl:107-110, fused into the products of
    the module-compression driver) on v_mfma_f64_16x16x4_f64: sampled rows against a host evaluation in
    extended precision, all tile counts (w <= 16 ... 64), 1 / 2 / 4 elements per pass, ragged n, label 0 = 0."""
    import ctypes as C
    v = C.c_double(0)
    aux = w | (G << 8) | (d << 12) | (1 << 30)
    prof = pkg._lib.load_prof_library()  # measurement entry points live in libsdpsr_prof.so
    gpu_ctx.check(prof.sdpsr_profile_kernel(gpu_ctx._h, 9, n, aux, 1, C.byref(v)))
    assert v.value < 1e-11 * n, v.value   # |A| <= 1, |W| <= 1: sums of n products


# ------------------------------------------------ ABI 0.3: sdpsr_opts switches (round mode, label width, flags), trajectory
def test_clamp_round_trunc_mode_is_the_reference_rule(pkg, oracle):
    """sdpsr_opts.round_mode = SDPSR_ROUND_TRUNC: unsafe_round as written (unsafe_trunc(Int, scale * x) / scale,
    src/utils.jl:49-53), bit for bit against the oracle's literal restatement; the default stays round-to-nearest."""
    lib = pkg.load_library()
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-12, 6, 20000), [0.0625, 0.0625 * (1 - 2e-16), 1e-10, -1e-9, 0.0, -0.0]])
    with pkg.Context(seed=1, round_mode="trunc") as ctx:
        got = a.copy()
        ctx.check(lib.sdpsr_clamp_round(ctx._h, got.size, C.c_void_p(got.ctypes.data), 1.4901161193847656e-8, 0))
    ref = oracle.clamp_round(a, round_mode="trunc")
    assert np.array_equal(got, ref) and np.array_equal(np.signbit(got), np.signbit(ref))
    near = oracle.clamp_round(a, round_mode="nearest")
    assert 0.3 < np.mean(got != near) < 0.7  # the two rules differ in the 7th digit of about every second input
    with pytest.raises(pkg.SdpsrError):
        pkg.Context(round_mode=7)


@pytest.mark.parametrize("name,q", [("er3", 3), ("er5", 5), ("er7", 7)])
def test_reference_literal_loop_with_truncation(pkg, problems, oracle, golden, name, q):
    """The whole loop in the reference's own arithmetic: fp64 square, two refinements per iteration, TRUNCATED 7-digit
    mantissas in the setup stage (device), the projection step and the square (src/partitions.jl:117-185,
    src/utils.jl:34-53).  Golden partition, and the dimension after every iteration equal to the oracle's trace in
    the same mode."""
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(q))
    trace = []
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0), round_mode="trunc", trace=trace)
    assert np.array_equal(ref.matrix, golden[f"{name}_P"])
    for seed in (1, 2, 3):
        with pkg.Context(seed=seed, square_mode=pkg.SQUARE_F64, round_mode="trunc", flags=pkg._lib.FLAG_SEPARATE_REFINEMENTS) as ctx:
            P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)  # device setup: rounds with the ctx's rule
            assert P.nparts == ref.nparts and np.array_equal(P.matrix, golden[f"{name}_P"]), (name, seed)
            assert P.dims[1:] == trace and P.iterations == ref.iterations, (P.dims, trace)
            assert ctx.dimension_trajectory() == P.dims


@pytest.mark.parametrize("name", ["petersen", "er3", "er5", "er7", "esc16j"])
def test_dimension_trajectory_default_mode(pkg, problems, oracle, golden, name):
    """sdpsr_dimension_trajectory (src/partitions.jl:150,156,187-188 under verbose): the default loop (int8 squares,
    2 channels + confirm round, one joint refinement per iteration) walks through the same dimensions as the oracle."""
    Cv, A, b = _problem(problems, name)
    setup = pkg.admissible_setup(Cv, A, b)
    n, CL, X0L, U = setup
    trace = []
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0), trace=trace,
                                     setup=(n, U, CL.reshape(n, n, order="F"), X0L.reshape(n, n, order="F")))
    with pkg.Context(seed=11) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
        dims = ctx.dimension_trajectory()
    assert np.array_equal(P.matrix, golden[f"{name}_P"])
    assert len(dims) == P.iterations + 1 and dims[-1] == P.nparts
    assert all(x <= y for x, y in zip(dims, dims[1:]))
    assert dims[1:] == trace, (name, dims, trace)
    cnt = C.c_int32(0)  # capacity smaller than the trajectory: count still reported, no overrun
    two = np.full(3, -1, dtype=np.int64)
    ctx2 = pkg.Context(seed=12)
    pkg.admissible_subspace(Cv, A, b, ctx=ctx2, setup=setup)
    ctx2.check(ctx2._lib.sdpsr_dimension_trajectory(ctx2._h, two.ctypes.data_as(C.c_void_p), 2, C.byref(cnt)))
    assert cnt.value == len(dims) and list(two[:2]) == dims[:2] and two[2] == -1
    ctx2.close()


@pytest.mark.parametrize("channels,confirm", [(0, 0), (2, 1), (4, 0), (1, 3), (8, 0)])
def test_channel_counts_and_confirm_rounds(pkg, problems, golden, channels, confirm):
    """channels = 0 is the default pair (2 channels + 1 confirm round); every explicit choice must end on the same
    canonical matrix with the same iteration count (a confirm round is not an iteration)."""
    for name, iters in (("er5", 4), ("esc16j", 3)):
        Cv, A, b = _problem(problems, name)
        setup = pkg.admissible_setup(Cv, A, b)
        for seed in (5, 6):
            with pkg.Context(seed=seed, channels=channels, confirm_rounds=confirm) as ctx:
                P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
            assert np.array_equal(P.matrix, golden[f"{name}_P"]), (name, channels, confirm, seed)
            assert P.iterations == iters


def test_label_overflow_like_the_reference(pkg, oracle, problems):
    """sdpsr_opts.label_bits: InexactError of Partition{T} (src/partitions.jl:29,63) as SDPSR_LABEL_OVERFLOW.  refine!
    decides on the largest pair code l1 + l2 (dim(P1) + 1), exactly like the reference (and the oracle's label_bits)."""
    rng = np.random.default_rng(4)
    n = 40
    A = rng.integers(0, 400, size=(n, n))
    B = rng.integers(0, 300, size=(n, n))  # pair codes up to ~300 * 401: beyond UInt16, within UInt32
    for bits, expect in ((8, True), (16, True), (32, False), (0, False)):
        with pkg.Context(seed=1, label_bits=bits) as ctx:
            if bits == 8:  # <= 199 classes fit UInt8, ~299 do not: the ctor itself throws (T(l + 1), :29)
                pkg.Partition.from_matrix(rng.integers(0, 200, size=(n, n)), ctx=ctx)
                with pytest.raises(pkg.LabelOverflow):
                    pkg.Partition.from_matrix(B, ctx=ctx)
                with pytest.raises(pkg.LabelOverflow):
                    pkg.Partition.from_matrix(B.astype(np.float64), ctx=ctx)
                continue
            Pa = pkg.Partition.from_matrix(A, ctx=ctx)
            Pb = pkg.Partition.from_matrix(B, ctx=ctx)
            if expect:
                with pytest.raises(pkg.LabelOverflow):
                    pkg.refine(Pa, Pb, ctx=ctx)
                with pytest.raises(oracle.LabelOverflow):
                    oracle.refine(oracle.partition_from_labels(A), oracle.partition_from_labels(B), bits)
            else:
                got = pkg.refine(Pa, Pb, ctx=ctx)
                ref = oracle.refine(oracle.partition_from_labels(A), oracle.partition_from_labels(B), bits or None)
                assert got.nparts == ref.nparts and np.array_equal(got.matrix, ref.matrix)
    # the edge, exactly: max pair code 255 fits UInt8, 256 does not
    P1 = np.array([[1, 2], [3, 4]])  # dim 4
    P2ok = np.array([[1, 2], [3, 50]])  # canonical labels 1..4: max code = 4 + 4 * 5 = 24
    with pkg.Context(seed=1, label_bits=8) as ctx:
        assert pkg.refine(pkg.Partition.from_matrix(P1, ctx=ctx), pkg.Partition.from_matrix(P2ok, ctx=ctx), ctx=ctx).nparts == 4
        big1 = np.arange(1, 51).reshape(5, 10)  # dim 50
        big2 = np.arange(1, 51).reshape(5, 10)  # last entry: 50 + 50 * 51 = 2600 > 255
        with pytest.raises(pkg.LabelOverflow):
            pkg.refine(pkg.Partition.from_matrix(big1, ctx=ctx), pkg.Partition.from_matrix(big2, ctx=ctx), ctx=ctx)
        lab15 = np.arange(1, 16).reshape(3, 5)  # dim 15: max code 15 + 15 * 16 = 255 = typemax(UInt8): still fits
        assert pkg.refine(pkg.Partition.from_matrix(lab15, ctx=ctx), pkg.Partition.from_matrix(lab15, ctx=ctx), ctx=ctx).nparts == 15
    # the loop: G(n, 1/2) theta' ends at dim (n^2 + n) / 2 -- beyond UInt16 for n = 400, as in the reference's default
    # admissible_subspace(Partition{UInt16}, ...) (src/partitions.jl:84)
    Cv, Am, b = problems.theta_prime_problem(problems.gnp_adjacency(400, 0.5, seed=2))
    with pkg.Context(seed=3, label_bits=16) as ctx:
        with pytest.raises(pkg.LabelOverflow):
            pkg.admissible_subspace(Cv, Am, b, ctx=ctx)
    with pkg.Context(seed=3, label_bits=32) as ctx:
        assert pkg.admissible_subspace(Cv, Am, b, ctx=ctx).nparts == (400 * 400 + 400) // 2
    with pytest.raises(pkg.SdpsrError):
        pkg.Context(label_bits=12)


def test_int64_keys_ctor(pkg, oracle, gpu_ctx):
    """sdpsr_partition_from_u64: integer entries beyond 2^32 (and the relabel of hash-combined labels in the multi-GPU
    agreement) -- canonical first-occurrence numbering, 0 preserved."""
    import torch
    rng = np.random.default_rng(9)
    base = rng.integers(0, 40, size=(70, 70)).astype(np.int64)
    M = base * (2 ** 40 + 12345)
    P = pkg.Partition.from_matrix(M, ctx=gpu_ctx)
    R = oracle.partition_from_labels(base)
    assert P.nparts == R.nparts and np.array_equal(P.matrix, R.matrix)
    keys = torch.from_numpy(M.ravel(order="F").copy()).cuda() * -7  # negative int64 = large uint64: keys, not values
    lab, d = pkg.relabel_keys(keys, ctx=gpu_ctx)
    assert d == R.nparts and np.array_equal(lab.cpu().numpy().reshape(70, 70, order="F"), R.matrix)


def test_symmetry_verdict_is_not_reused_for_other_labels(pkg, gpu_ctx, golden):
    """a device-resident symmetric blockDiagonalize caches its symmetry verdict in the ctx; a later
    eigen_decomposition of a NON-symmetric host partition on the same ctx must still raise
    InvalidDecompositionField (and the other order must not raise spuriously)."""
    import torch
    L = golden["er5_P"]
    n = L.shape[0]
    tP = torch.from_numpy(np.ascontiguousarray(L.ravel(order="F")).astype(np.int32)).cuda()
    Pd = pkg.Partition(int(L.max()), tP.view(n, n).t())
    bd = pkg.blockDiagonalize(Pd, ctx=gpu_ctx)
    assert sorted(bd.blkSizes) == [2, 2, 2, 3]
    c3 = np.zeros((n, n), dtype=np.uint32)  # directed cycle: not symmetric
    for i in range(n):
        c3[i, (i + 1) % n] = 1
        c3[i, i] = 2
    with pytest.raises(pkg.InvalidDecompositionField):
        pkg.eigen_decomposition(pkg.Partition(2, c3), ctx=gpu_ctx)
    ne, nc = pkg.eigen_decomposition(pkg.Partition(int(L.max()), L.copy()), ctx=gpu_ctx)  # symmetric host labels after it
    assert ne >= nc >= 1
    bd = pkg.blockDiagonalize(Pd, ctx=gpu_ctx)
    assert sorted(bd.blkSizes) == [2, 2, 2, 3]


def test_symmetry_hint_does_not_survive_a_failed_call(pkg, problems, golden):
    """sdpsr_hint_symmetric_basis applies to ONE call, also when that call fails early."""
    Cv, A, b = problems.theta_prime_problem(problems.er_graph_adjacency(3))
    setup = pkg.admissible_setup(Cv, A, b)
    n, CL, X0L, U = setup
    rng = np.random.default_rng(1)
    with pkg.Context(seed=2) as ctx:
        lib = ctx._lib
        lib.sdpsr_hint_symmetric_basis(ctx._h, 3)
        d, it = C.c_int64(0), C.c_int32(0)
        P = np.zeros(n * n, dtype=np.uint32)
        st = lib.sdpsr_admissible_subspace(ctx._h, n, C.c_void_p(CL.ctypes.data), C.c_void_p(X0L.ctypes.data), None, 2, 1e-8,
                                           C.c_void_p(P.ctypes.data), C.byref(d), C.byref(it), None, 0)  # r > 0 without U
        assert st == 5
        # a NON-symmetric problem next: with a stale hint (bit 1) its initial partition would be the mirrored lower triangle
        M1 = rng.integers(0, 4, size=(n, n)).astype(np.float64)
        M2 = rng.integers(0, 3, size=(n, n)).astype(np.float64)
        f1, f2 = np.ascontiguousarray(M1.ravel(order="F")), np.ascontiguousarray(M2.ravel(order="F"))
        ctx.check(lib.sdpsr_admissible_subspace(ctx._h, n, C.c_void_p(f1.ctypes.data), C.c_void_p(f2.ctypes.data), None, 0, 1e-8,
                                                C.c_void_p(P.ctypes.data), C.byref(d), C.byref(it), None, 0))
        got = P.reshape(n, n, order="F")
        assert not np.array_equal(got, got.T)  # the labels refine the (non-symmetric) pair partition


@pytest.mark.parametrize("name", ["circ1024", "er7xK16", "er5xK20"])
def test_small_compressed_problem_host_and_device_paths(pkg, problems, oracle, golden, name):
    """Module-compression driver, compressed order w <= 64: Murota's steps on the host (default: host tridiagonal-QL
    eigensolver inside the read-back the driver makes anyway) against the one-workgroup device kernels
    (SDPSR_FLAG_SMALL_EIGEN_ON_DEVICE) -- same block sizes, orthonormal Q_hat, blks == Q_k' 1[P==i] Q_k and the
    spectrum invariant on both; also with the reference-literal switches of the irreducible / coupling steps."""
    if name == "circ1024":
        L, d = problems.synthetic_jordan_partition(1024, seed=4)
        expect = [1] * d
    elif name == "er7xK16":
        L, d = problems.kron_with_complete(golden["er7_P"].astype(np.int64), 16, seed=5)
        expect = sorted([2, 2, 2, 2, 3] * 2)
    else:
        L, d = problems.kron_with_complete(golden["er5_P"].astype(np.int64), 20, seed=6)
        expect = sorted([2, 2, 2, 3] * 2)
    P = pkg.Partition(d, L.astype(np.uint32))
    Po = oracle.Partition(d, L)
    x = np.random.default_rng(8).random(d)
    F = pkg._lib
    for flags in (0, F.FLAG_SMALL_EIGEN_ON_DEVICE, F.FLAG_FRESH_IRREDUCIBLE_ELEMENT, F.FLAG_SINGLE_COUPLING_ELEMENT | F.FLAG_ALWAYS_REORTHOGONALIZE,
                  F.FLAG_SPMM_ONE_BY_ONE):
        for seed in (3, 4, 5):
            with pkg.Context(seed=seed, eig_driver=6, flags=flags) as ctx:
                bd = pkg.blockDiagonalize(P, ctx=ctx, retries=3)
            assert sorted(bd.blkSizes) == expect, (name, flags, seed)
            full, blk = oracle.spectrum_invariant(Po, bd.blks, x)
            assert len(full) == len(blk) and np.allclose(full, blk, rtol=1e-6, atol=1e-8), (name, flags, seed)
            for q in bd.Q_hat:
                q = np.asarray(q)
                assert np.abs(q.T @ q - np.eye(q.shape[1])).max() < 1e-7
            ref = oracle.basis_image_fast([np.asarray(q) for q in bd.Q_hat], Po)
            for i in range(0, d, max(1, d // 5)):
                for k in range(len(bd.blkSizes)):
                    assert np.allclose(bd.blks[i][k], ref[i][k], atol=1e-9)


@pytest.mark.parametrize("name", ["petersen", "er5", "er7", "esc16j", "circ256"])
def test_verify_shortcut_agrees_with_full_refinement(pkg, problems, golden, name):
    """Rounds expected not to refine (confirm rounds, the first iteration) compare every entry with its class
    representative before running a refinement; with SDPSR_FLAG_NO_VERIFY_SHORTCUT every round refines.  Same
    canonical matrix, same iteration count, same dimension trajectory -- on inputs whose first iteration splits
    (theta' problems: the shortcut says "differs" and the refinement runs) and on an already closed one (circ256:
    neither the first iteration nor the confirm round relabels anything)."""
    if name == "circ256":
        Lg = golden["circ256_P"].astype(np.int64)
        Cv, A, b = problems.partition_as_sdp(Lg, seed=1)
    else:
        Lg = golden[f"{name}_P"]
        Cv, A, b = _problem(problems, name)
    setup = pkg.admissible_setup(Cv, A, b)
    outs = []
    for flags in (0, pkg._lib.FLAG_NO_VERIFY_SHORTCUT):
        for seed in (1, 2, 3):
            with pkg.Context(seed=seed, flags=flags) as ctx:
                P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
                outs.append((P.iterations, tuple(P.dims)))
                assert np.array_equal(P.matrix, Lg), (name, flags, seed)
    assert len(set(outs)) == 1, outs


@pytest.mark.parametrize("name", ["er7", "esc16j", "circ256"])
def test_jordan_reduce_equals_the_three_calls(pkg, problems, oracle, golden, name):
    """sdpsr_jordan_reduce = admissible_subspace + blockDiagonalize + basis_image in one stream-ordered call:
    same canonical partition, pinned block sizes, blks == Q_k' 1[P==i] Q_k for the Q_hat it returns; the capacity
    protocol (sizes only -> sdpsr_block_images afterwards) and host / device memory spaces."""
    import torch
    if name == "circ256":
        Lg = golden["circ256_P"].astype(np.int64)
        Cv, A, b = problems.partition_as_sdp(Lg, seed=1)
    else:
        Lg = golden[f"{name}_P"].astype(np.int64)
        Cv, A, b = _problem(problems, name)
    expect = list(golden[f"{name}_blk"])
    setup = pkg.admissible_setup(Cv, A, b)
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    r = U.shape[1]
    d = int(Lg.max())
    Po = oracle.Partition(d, Lg)
    L = pkg._lib
    for mem in (L.MEM_HOST, L.MEM_DEVICE):
        with pkg.Context(seed=5) as ctx:
            lib = ctx._lib
            if mem == L.MEM_DEVICE:
                tCL, tX0 = torch.from_numpy(CL).cuda(), torch.from_numpy(X0L).cuda()
                tU = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
                tP = torch.empty(n * n, dtype=torch.int32, device="cuda")
                args = [C.c_void_p(t.data_ptr()) for t in (tCL, tX0, tU)]
                pP = C.c_void_p(tP.data_ptr())
            else:
                P = np.zeros(n * n, dtype=np.uint32)
                args = [C.c_void_p(a.ctypes.data) for a in (CL, X0L, Uf)]
                pP = C.c_void_p(P.ctypes.data)
            dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
            ms = (C.c_double * L.T_COUNT)()
            if setup.hint:
                lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
            # sizes only
            ctx.check(lib.sdpsr_jordan_reduce(ctx._h, n, *args, r, pkg.api.RTOL_DEFAULT, pkg.api.RTOL_DEFAULT, pP, C.byref(dd), C.byref(it), C.byref(nb),
                                              C.byref(ssq), C.byref(ss), None, 0, None, 0, C.cast(ms, C.c_void_p), mem))
            assert dd.value == d and ms[L.T_TOTAL] > 0
            sizes = np.zeros(nb.value, dtype=np.int32)
            ctx.check(lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
            assert sorted(int(x) for x in sizes) == expect
            S, S1 = ssq.value, ss.value
            got = (tP.cpu().numpy().view(np.uint32) if mem == L.MEM_DEVICE else P).reshape(n, n, order="F")
            assert np.array_equal(got, Lg)
            # images in the same call (capacity given), again with fresh generic elements
            if mem == L.MEM_DEVICE:
                tb = torch.empty(d * S, dtype=torch.float64, device="cuda")
                tq = torch.empty(n * S1, dtype=torch.float64, device="cuda")
                pb, pq = C.c_void_p(tb.data_ptr()), C.c_void_p(tq.data_ptr())
            else:
                hb, hq = np.zeros(d * S), np.zeros(n * S1)
                pb, pq = C.c_void_p(hb.ctypes.data), C.c_void_p(hq.ctypes.data)
            if setup.hint:
                lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
            for attempt in range(4):
                st = lib.sdpsr_jordan_reduce(ctx._h, n, *args, r, pkg.api.RTOL_DEFAULT, pkg.api.RTOL_DEFAULT, None, C.byref(dd), C.byref(it), C.byref(nb),
                                             C.byref(ssq), C.byref(ss), pb, d * S, pq, n * S1, None, mem)
                if st not in (2, 3):
                    break
            ctx.check(st)
            assert (ssq.value, ss.value) == (S, S1)
            ctx.check(lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
            blks = (tb.cpu().numpy() if mem == L.MEM_DEVICE else hb).reshape(d, S)
            Q = (tq.cpu().numpy() if mem == L.MEM_DEVICE else hq).reshape(n, S1, order="F")
            cols = np.concatenate([[0], np.cumsum(sizes)])
            offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64) ** 2)])
            Qs = [Q[:, cols[k]:cols[k + 1]] for k in range(len(sizes))]
            ref = oracle.basis_image_fast(Qs, Po)
            for i in range(d):
                for k in range(len(sizes)):
                    assert np.allclose(blks[i, offs[k]:offs[k + 1]].reshape(sizes[k], sizes[k], order="F"), ref[i][k], atol=1e-9)


@pytest.mark.parametrize("name", ["er7", "circ256"])
def test_jordan_reduce_batch_equals_single_calls(pkg, problems, golden, name):
    """sdpsr_jordan_reduce_batch (R restarts on fibers of one host thread, one ctx): every restart returns what a single
    sdpsr_jordan_reduce returns -- the golden partition bit for bit, the pinned block sizes, the same iteration count --
    and, restart by restart with the same seed, the same block images as a single call on a fresh ctx with that seed
    (columns compared as a set: the order of the blocks follows the random generic element)."""
    if name == "circ256":
        Lg = golden["circ256_P"].astype(np.int64)
        Cv, A, b = problems.partition_as_sdp(Lg, seed=1)
    else:
        Lg = golden[f"{name}_P"].astype(np.int64)
        Cv, A, b = _problem(problems, name)
    expect = list(golden[f"{name}_blk"])
    setup = pkg.admissible_setup(Cv, A, b)
    d = int(Lg.max())
    S = sum(int(x) ** 2 for x in expect)

    def colset(M):
        M = np.round(np.asarray(M), 7)
        return M[:, np.lexsort(M[::-1])]

    with pkg.Context(seed=5) as ctx:
        for R in (1, 2, 3):
            for attempt in range(4):  # blockDiagonalize is randomized ("try again"): fresh seeds per attempt
                seeds = [1000 * R + 10 * attempt + i for i in range(R)]
                res = pkg.jordan_reduce_batch(Cv, A, b, restarts=R, seeds=seeds, ctx=ctx, setup=setup)
                if all(x["status"] == 0 for x in res):
                    break
            assert all(x["status"] == 0 for x in res), [x["status"] for x in res]
            its = set()
            for x in res:
                assert x["P"].nparts == d and np.array_equal(x["P"].matrix, Lg)
                assert x["sum_sq"] == S and x["nblocks"] == len(expect)
                its.add(x["iterations"])
            assert len(its) == 1
            if name == "circ256":  # 1 x 1 blocks: the images are the characters of the scheme, a set of d columns
                ref = colset(res[0]["blks"])
                for x in res[1:]:
                    assert np.allclose(colset(x["blks"]), ref, atol=1e-6)
        # the same seed on a fresh ctx, one restart at a time
        single = []
        for sd in seeds:
            with pkg.Context(seed=sd) as c1:
                y = pkg.jordan_reduce_batch(Cv, A, b, restarts=1, seeds=[sd], ctx=c1, setup=setup)[0]
            single.append(y)
        for x, y in zip(res, single):
            assert x["status"] == y["status"] == 0
            assert np.array_equal(x["P"].matrix, y["P"].matrix) and x["iterations"] == y["iterations"]
            assert np.allclose(colset(x["blks"]), colset(y["blks"]), atol=1e-6)


@pytest.mark.parametrize("name", ["circ64", "circ256", "circ1024"])
def test_commutative_basis_image_shortcut_equals_projection_formula(pkg, problems, oracle, golden, name):
    """Every block 1 x 1: blks[i][k] = q_k'(1[P==i] x), x = sum_k q_k (one vector's class sums, randomized self-check)
    against the projection formula Q_k' 1[P==i] Q_k (SDPSR_FLAG_FULL_BASIS_IMAGE, and the host products of the
    oracle): same numbers to 1e-9, same clamping of |x| < 1e-12 n."""
    if name == "circ1024":
        L, d = problems.synthetic_jordan_partition(1024, seed=4)
    else:
        L = golden[f"{name}_P"].astype(np.int64)
        d = int(L.max())
    P = pkg.Partition(d, L.astype(np.uint32))
    Po = oracle.Partition(d, L)
    for flags in (0, pkg._lib.FLAG_FULL_BASIS_IMAGE):
        for seed in (1, 2):
            with pkg.Context(seed=seed, flags=flags) as ctx:
                bd = pkg.blockDiagonalize(P, ctx=ctx, retries=3)
            assert bd.blkSizes == [1] * d
            ref = oracle.basis_image_fast([np.asarray(q) for q in bd.Q_hat], Po)
            got = np.array([[bd.blks[i][k][0, 0] for k in range(d)] for i in range(d)])
            want = np.array([[ref[i][k][0, 0] for k in range(d)] for i in range(d)])
            assert np.allclose(got, want, atol=1e-9), (name, flags, seed, np.abs(got - want).max())


@pytest.mark.gpu
def test_complex_path_largest_orders(pkg, problems):
    """blockDiagonalize(P; complex=true) beyond n = 3072 (the limit of rounds 1-2; now 4096: the embedded real problem of
    order 2 n <= 8192 goes through the row / panel tridiagonalisation and the tridiagonal divide and conquer): C[S3] (x)
    {I, J - I} on 560 points, n = 3360, non-commutative, blocks [1, 1, 1, 1, 2, 2] known by construction; orthonormal
    Q_hat, blks == Q_k^H 1[P==i] Q_k on every class, sum s^2 == dim(P)."""
    Lm, _ = problems.kron_with_complete(_s3_cayley_labels(), 560, seed=6)
    n = Lm.shape[0]
    assert n == 3360
    with pkg.Context(seed=11) as ctx:
        P = pkg.Partition.from_matrix(Lm, ctx=ctx)
        bd = pkg.blockDiagonalize(P, complex=True, ctx=ctx, retries=3)
    assert sorted(bd.blkSizes) == [1, 1, 1, 1, 2, 2]
    Pd = bd.partition
    assert sum(s * s for s in bd.blkSizes) == Pd.nparts
    Mlab = np.asarray(Pd.matrix)
    for k, q in enumerate(bd.Q_hat):
        assert np.allclose(q.conj().T @ q, np.eye(q.shape[1]), atol=1e-9)
        for c in range(Pd.nparts):
            M = (Mlab == c + 1).astype(np.float64)
            assert np.allclose(bd.blks[c][k], q.conj().T @ (M @ q), atol=1e-7), (k, c)


def test_deferred_verdicts_of_a_wrong_guess_repeat_the_reduction(pkg, problems, golden, capfd, monkeypatch):
    """sdpsr_jordan_reduce on a ctx whose previous input of this order was closed leaves the verdicts of the first verify pass
    and of the speculative confirm round unread, goes on into blockDiagonalize in stream order and reads them behind its later
    host waits (one host wait less per reduction).  (a) closed input again: same partition, same block sizes, fewer host
    waits than the ctx's first reduction; (b) an input of the SAME order that is not closed (theta' of C_16 [] K_16, N = 256, after
    circ256: the loop starts from {diagonal, edges, non-edges} on the packed lower triangle, the shape the guess applies to): the
    guess is wrong, the verdicts say so, everything is discarded and the reduction repeated -- the generator's closure, block
    sizes and iteration count as on a fresh ctx."""
    L = pkg._lib
    prof = L.load_prof_library()
    Lc = golden["circ256_P"].astype(np.int64)
    closed = pkg.admissible_setup(*problems.partition_as_sdp(Lc, seed=1))
    Cv, A, b, Le, dopen = problems.theta_prime_product_problem(problems.cycle_adjacency(16), problems.symmetric_circulant_labels(16), 16, seed=1)
    open_ = pkg.admissible_setup(Cv, A, b)
    assert closed[0] == open_[0] == 256

    def reduce(ctx, setup):
        n, CL, X0L, U = setup
        Uf = np.asfortranarray(U)
        P = np.zeros(n * n, dtype=np.uint32)
        dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        w0, w1 = C.c_uint64(0), C.c_uint64(0)
        if setup.hint:
            ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
        ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w0)))
        ctx.check(ctx._lib.sdpsr_jordan_reduce(ctx._h, n, C.c_void_p(CL.ctypes.data), C.c_void_p(X0L.ctypes.data), C.c_void_p(Uf.ctypes.data), U.shape[1],
                                               pkg.api.RTOL_DEFAULT, pkg.api.RTOL_DEFAULT, C.c_void_p(P.ctypes.data), C.byref(dd), C.byref(it), C.byref(nb),
                                               C.byref(ssq), C.byref(ss), None, 0, None, 0, None, L.MEM_HOST))
        ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w1)))
        sizes = np.zeros(nb.value, dtype=np.int32)
        ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
        return P.reshape(n, n, order="F"), dd.value, it.value, sorted(int(x) for x in sizes), w1.value - w0.value

    with pkg.Context(seed=11) as fresh:
        Pe, de, ite, blke, _ = reduce(fresh, open_)
    assert np.array_equal(Pe, Le) and de == dopen and ite > 1
    with pkg.Context(seed=12) as ctx:
        P1, d1, it1, blk1, waits1 = reduce(ctx, closed)   # no guess yet
        P2, d2, it2, blk2, waits2 = reduce(ctx, closed)   # guessed closed, verdicts deferred
        assert np.array_equal(P1, Lc) and np.array_equal(P2, Lc) and d1 == d2 and it1 == it2 == 1
        assert blk1 == blk2 == sorted(int(x) for x in golden["circ256_blk"])
        assert waits2 < waits1, (waits1, waits2)
        monkeypatch.setenv("SDPSR_DEBUG", "1")             # (read by the library at every trace point)
        capfd.readouterr()
        P3, d3, it3, blk3, _ = reduce(ctx, open_)          # same order, NOT closed: the guess is wrong
        monkeypatch.delenv("SDPSR_DEBUG")
        assert "not closed after all" in capfd.readouterr().err  # the repeated reduction is what ran
        assert np.array_equal(P3, Le) and d3 == de and it3 == ite and blk3 == blke
        P4, d4, it4, blk4, _ = reduce(ctx, closed)          # and the ctx has unlearnt the guess
        assert np.array_equal(P4, Lc) and blk4 == blk1
    # A/B (SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT: the control flow of rounds 1-4): same matrices, iterations, dimensions; more host waits
    with pkg.Context(seed=12, flags=L.FLAG_WAIT_FOR_EVERY_VERDICT) as ctx:
        Q1, e1, jt1, bl1, _ = reduce(ctx, closed)
        Q2, e2, jt2, bl2, waits_ab = reduce(ctx, closed)
        assert np.array_equal(Q2, Lc) and e2 == d2 and jt2 == it2 and bl2 == blk2 and waits_ab > waits2, (waits_ab, waits2)
        Q3, e3, jt3, bl3, _ = reduce(ctx, open_)
        assert np.array_equal(Q3, Le) and e3 == de and jt3 == ite and bl3 == blke


def test_problem_handle_uploads_once(pkg, problems, golden):
    """Upload once, restart many: the PCIe bytes of a 4-restart batch from HOST arrays are those of
    one call -- through the problem handle (sdpsr_problem_create + sdpsr_problem_reduce_batch: nothing but small words
    travel after the creation) and through sdpsr_jordan_reduce_batch itself with SDPSR_MEM_HOST (one upload into the
    ctx's input buffers, not one per restart) -- counted by sdpsr_transfer_bytes; four single host-array calls move four
    times as much.  Every restart still returns the golden partition and the pinned block sizes."""
    Lg, d = problems.kron_with_complete(golden["er7_P"].astype(np.int64), 8, seed=3)  # N = 456, blocks [2,2,2,2,3] twice
    n = Lg.shape[0]
    Cv, A, b = problems.partition_as_sdp(Lg, seed=2)
    setup = pkg.admissible_setup(Cv, A, b)
    _, CL, X0L, U = setup
    r = U.shape[1]
    Uf = np.asfortranarray(U)
    inputs = 8 * n * n * (2 + r)
    outputs = 4 * n * n
    expect = sorted([2, 2, 2, 2, 3] * 2)
    R = 4
    with pkg.Context(seed=9) as ctx:
        lib = ctx._lib
        h0, _ = ctx.transfer_bytes()
        with pkg.Problem(setup=setup, ctx=ctx) as prob:
            h1, d1 = ctx.transfer_bytes()
            assert h1 - h0 == inputs
            for attempt in range(4):
                res = prob.reduce_batch(R, seeds=[50 + 10 * attempt + i for i in range(R)])
                if all(x["status"] == 0 for x in res):
                    break
            h2, d2 = ctx.transfer_bytes()
            assert h2 - h1 < inputs // 4, (h2 - h1, inputs)  # descriptors and class values only: no second copy of C_L, X0, U
            for x in res:
                assert x["status"] in (0, 2, 3)
                assert x["P"].nparts == d and np.array_equal(x["P"].matrix, Lg)
                if x["status"] == 0:
                    assert x["sum_sq"] == sum(s * s for s in expect) and x["nblocks"] == len(expect)
            one = prob.reduce(seed=77) if True else None
            assert one["P"].nparts == d
        # the host-array batch entry point: one upload for R restarts
        Ps = [np.zeros(n * n, dtype=np.uint32) for _ in range(R)]
        pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
        dd, st = (C.c_int64 * R)(), (C.c_int32 * R)()
        h3, _ = ctx.transfer_bytes()
        lib.sdpsr_jordan_reduce_batch(ctx._h, R, None, n, CL.ctypes.data_as(C.c_void_p), X0L.ctypes.data_as(C.c_void_p), Uf.ctypes.data_as(C.c_void_p), r,
                                      1.5e-8, 1.5e-8, C.cast(pP, C.c_void_p), dd, None, None, None, None, None, None, st, 0)
        h4, _ = ctx.transfer_bytes()
        assert inputs <= h4 - h3 < inputs + inputs // 4, (h4 - h3, inputs)
        for i in range(R):
            assert st[i] in (0, 2, 3) and dd[i] == d and np.array_equal(Ps[i].reshape(n, n, order="F"), Lg)
        # four single calls from host arrays: four uploads
        dim, it = C.c_int64(0), C.c_int32(0)
        h5, _ = ctx.transfer_bytes()
        for i in range(R):
            rc = lib.sdpsr_jordan_reduce(ctx._h, n, CL.ctypes.data_as(C.c_void_p), X0L.ctypes.data_as(C.c_void_p), Uf.ctypes.data_as(C.c_void_p), r, 1.5e-8, 1.5e-8,
                                         Ps[0].ctypes.data_as(C.c_void_p), C.byref(dim), C.byref(it), None, None, None, None, 0, None, 0, None, 0)
            assert rc in (0, 2, 3) and dim.value == d
        h6, _ = ctx.transfer_bytes()
        assert h6 - h5 >= R * inputs
    # bad arguments before the restarts start: every status word says so
    with pkg.Context(seed=1) as ctx:
        st = (C.c_int32 * 2)(0, 0)
        dd = (C.c_int64 * 2)()
        rc = ctx._lib.sdpsr_jordan_reduce_batch(ctx._h, 2, None, 0, None, None, None, 0, 1.5e-8, 1.5e-8, None, dd, None, None, None, None, None, None, st, 0)
        assert rc != 0 and all(s != 0 for s in st)
        with pytest.raises(ValueError):
            pkg.Problem(setup=setup, ctx=ctx).reduce_batch(2, seeds=[1, 2, 3])


# ------------------------------------------------ signature sources: the array path against the fused path
SIG_INSTANCES = ["petersen", "er7", "esc16j", "closed256", "er7_as_sdp", "open256"]


@pytest.fixture(scope="module")
def sig_instances(pkg, problems, golden):
    """name -> (setup, expected partition).  The golden problems (esc16j: r > 4, the projection keeps the full matrix and goes
    through proj_apply_kernel, then the channel source) and the three instances of test_gpu_loop_contract.py: circ256 and er7
    wrapped as SDPs (closed, everything symmetric: the joint iteration on packed labels; N = 57 is ragged) and theta' of
    C_16 [] K_16 (open: dimension trajectory 6, 10, 18, 18)."""
    out = {}
    for name in ("petersen", "er7", "esc16j"):
        out[name] = (pkg.admissible_setup(*_problem(problems, name)), golden[f"{name}_P"])
    out["closed256"] = (pkg.admissible_setup(*problems.partition_as_sdp(golden["circ256_P"].astype(np.int64), seed=1)), golden["circ256_P"])
    out["er7_as_sdp"] = (pkg.admissible_setup(*problems.partition_as_sdp(golden["er7_P"].astype(np.int64), seed=1)), golden["er7_P"])
    Cv, A, b, Le, dopen = problems.theta_prime_product_problem(problems.cycle_adjacency(16), problems.symmetric_circulant_labels(16), 16, seed=1)
    out["open256"] = (pkg.admissible_setup(Cv, A, b), Le)
    assert out["closed256"][0][0] == out["open256"][0][0] == 256 and out["er7_as_sdp"][0][0] == 57
    return out


def _loop_run(pkg, setup, channels, flags=0, refine_path="auto"):
    # int8 squares; one confirm round, as the default pair has: a stop is believed after two squares that split nothing
    with pkg.Context(seed=7, square_mode=pkg.SQUARE_I8, channels=channels, confirm_rounds=1, flags=flags, refine_path=refine_path) as ctx:
        P = pkg.admissible_subspace(None, None, None, ctx=ctx, setup=setup)
    return np.array(P.matrix), list(P.dims), P.iterations


@pytest.mark.parametrize("channels", [2, 3, 4])
@pytest.mark.parametrize("name", SIG_INSTANCES)
def test_signature_array_path_equals_fused_path(pkg, sig_instances, name, channels):
    """A computed signature source (pair, projection, channels, joint) is defined once, by its functor in
    sig_sources.h; the insert pass evaluates it entry by entry, and SDPSR_FLAG_REFINE_NO_FUSE writes it out as an array
    first (the materialise kernel, or the stand-alone kernel of a run-time shape: 3 channels, r > 4) and refines that.  Same
    seed and same control flow, so the same keys and the same signatures either way: labels BIT-IDENTICAL, and the same
    dimension after every iteration and the same iteration count -- in the default loop (joint iteration on packed labels), with
    the labels unpacked after every step, and with the reference's two refinements per iteration.  Every result is the golden /
    generating partition."""
    setup, expect = sig_instances[name]
    F = pkg._lib
    for flags in (0, F.FLAG_UNPACK_EVERY_STEP, F.FLAG_SEPARATE_REFINEMENTS):
        fused = _loop_run(pkg, setup, channels, flags)
        array = _loop_run(pkg, setup, channels, flags | F.FLAG_REFINE_NO_FUSE)
        assert np.array_equal(fused[0], expect), (name, channels, flags)
        assert np.array_equal(array[0], fused[0]), (name, channels, flags)
        assert array[1] == fused[1], (name, channels, flags, array[1], fused[1])
        assert array[2] == fused[2], (name, channels, flags, array[2], fused[2])
        assert fused[1][-1] == int(expect.max())


@pytest.mark.parametrize("channels", [2, 3, 4])
@pytest.mark.parametrize("name", SIG_INSTANCES)
def test_forced_relabel_paths_read_the_same_signatures(pkg, sig_instances, name, channels):
    """refine_path = "sort" / "bucket" (forced at any size) always go through the written-out signatures of the loop's sources:
    labels bit-identical to refine_path = "auto" and the same final dimension.  (Their control flow differs -- the radix sort
    leaves no class representatives, so no compare shortcut -- and the trajectory is not compared.)"""
    setup, expect = sig_instances[name]
    auto = _loop_run(pkg, setup, channels)
    assert np.array_equal(auto[0], expect), (name, channels)
    for path in ("sort", "bucket"):
        got = _loop_run(pkg, setup, channels, refine_path=path)
        assert np.array_equal(got[0], auto[0]), (name, channels, path)
        assert got[1][-1] == auto[1][-1] == int(expect.max()), (name, channels, path, got[1], auto[1])
