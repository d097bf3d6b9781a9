"""Every launch shape of the matrix-core squares and products (csrc/kernels_gemm.hip, csrc/kernels_gemm_sym.hip)
against a host reference: exact integer products (int8, fp32 on exact integers, fp64 on integers), a rounding bound
for fp64 on real data, and closed-form partitions for the loop in its fp32 / fp64 / non-symmetric modes.

Branches, from launch_gemm() and launch_i8_symsquare().  Every ABI entry pads its operands (K to 128 int8, 32 floats
or 16 doubles per K-tile of 128 bytes, 16-byte aligned rows), so the LDS-DMA kernels always run:
  * int8 / fp32 with m, n multiples of 256 and >= 1024 workgroups of 256 x 256 (full: (m/256)(n/256) per channel;
    lower triangle: t2 (t2 + 1) / 2 with t2 = m/256) -> gemm_tn_dma_kernel<KIND, 0, 256>, otherwise
    gemm_tn_dma_kernel<KIND, CMODE, 128> ("dma128" below);
  * full grids are XCD-swizzled when gm % 8 == 0 and gm gn % 8 == 0 (gm = m / tile, gn = n / tile); lower-triangle
    grids deal the ntri = gm (gm + 1) / 2 tiles in 8 runs of ntri / 8, the last ntri % 8 keep their own number;
  * sdpsr_square_i8_symmetric with square_kernel != 1 takes the persistent i8_symsquare_kernel when
    i8_symsquare_pays() (rounds of one macro-tile job per CU well filled; 256 CUs).

  entry point                       shape                      ld / grid                    branch
  sdpsr_square_i8 / _f32            n = 1100                   1152, 9 x 9                  dma128, unswizzled
                                    n = 8192, 8100             8192, 32 x 32 (256-tiles)    gemm_tn_dma_kernel<I8/F32, 0, 256> full, swizzled
                                    n = 8200                   8320, 65 x 65                dma128, unswizzled, 4225 wgs
  sdpsr_square_f32                  n = 4096, +-vmax constant  4096, 32 x 32                dma128, swizzled, sums 2^24
  sdpsr_square_f64                  n = 1024 / 1100 / 8192     8 x 8 / 9 x 9 / 64 x 64      dma128 swz / unswz / swz large
  sdpsr_gemm_tn_f64                 (1024, 640, 777)           8 x 5, K 777 -> 784          dma128 swizzled, gm != gn
                                    (1000, 1500, 300)          8 x 12, K 300 -> 304         dma128 swizzled, gm != gn
                                    (1000, 1016, 333), lda 345, ldb 340, ldc 1009  8 x 8   leading dimensions
  sdpsr_square_i8_symmetric, sk 1   (4096, 8), (8192, 2)       136 x 8, 528 x 2 triangles   gemm_tn_dma_kernel<I8, 0, 256> lower
                           , sk 1   (4096, 2)                  gm 32: 528 = 8 x 66 tiles    dma128 lower, all renumbered
                           , sk 1   (4104, 3)                  4224, gm 33: 561 = 8 x 70 + 1  dma128 lower, 1 keeps its number
                           , sk 0   (8192, 2), (4096, 8)       1024 jobs on 256 CUs         persistent i8_symsquare_kernel
  loop fp32, closed_scheme N 4096   channels 0 (2) / 8         272 / 1088 lower tiles       dma128 lower / gemm_tn_dma_kernel<F32, 0, 256> lower
  loop fp32, theta_er7xk72 N 4104   channels 0 / 8             4224: not a multiple of 256  dma128 lower
  loop fp64, both                   4096 / 4224                32 x 32 / 33 x 33            dma128<F64> swizzled / unswizzled
  loop non-symmetric (int8, fp32)   n = 300, 1100              384 / 1152: 3 x 3 / 9 x 9    dma128 full, batch stride
                                    n = 4096, channels 0 (2)   32 x 32 x 2                  dma128 full, swizzled
                                    n = 4096, channels 4       16 x 16 x 4 = 1024 256-tiles gemm_tn_dma_kernel<I8/F32, 0, 256> full, batch stride

Checking cost: a full fp64 host product up to about 0.3 TFLOP in all; beyond that (n >= 8100, batches of 8, the
ragged 4104 x 3) an exact O(n^2) check: Freivalds with 3 random integer vectors plus every row and column at a
128-tile boundary (128 t, 128 t + 127) and the last one of the unpadded n.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _fl(a, dt):
    return np.ascontiguousarray(np.asarray(a, dtype=dt).ravel(order="F"))


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _sym_int(rng, n, vmax, dtype):
    """Symmetric n x n matrix of integers in [-vmax, vmax] (int8: [-128, 127] for vmax = 128)."""
    hi = 127 if vmax == 128 else vmax
    X = rng.integers(-vmax, hi + 1, size=(n, n), dtype=np.int8 if vmax <= 128 else np.int64)
    return (np.triu(X) + np.triu(X, 1).T).astype(dtype)


def _boundary_indices(n):
    """Rows / columns where a tile index, swizzle or padding error shows first: 128 t and 128 t + 127 below n, n - 1."""
    t = np.arange(0, n, 128)
    return np.unique(np.concatenate([t, t + 127, [n - 1]]).clip(max=n - 1))


def _assert_exact_square(got, X, bound, full, seed=0):
    """got == X X exactly, X symmetric with integer entries, |(X X)_ij| <= bound.

    full: one fp64 BLAS product (every partial sum is an integer below 2^53: exact in any order).
    Otherwise, O(n^2):
      * Freivalds: got r == X (X r) for 3 integer vectors r in [-1000, 1000]^n.  With |got| <= bound (asserted first)
        every partial sum on either side is an integer of magnitude <= n * bound * 1000 < 2^53 for the shapes here, so
        both sides are exact.  A wrong got has a row d != 0 of got - X X, and d . r = 0 for at most one value of the
        coordinate of r at a nonzero of d: each vector misses with probability <= 1/2001, all three <= 1.3e-10.
      * every row and column at a 128-tile boundary and the last one, against X[idx] X (= (X X[:, idx])' as X is
        symmetric)."""
    n = X.shape[0]
    Xd = X.astype(np.float64)
    G = got.astype(np.float64)
    if full:
        np.testing.assert_array_equal(G, Xd @ Xd)
        return
    assert np.abs(G).max() <= bound
    assert n * bound * 1000 < 2.0 ** 53
    rng = np.random.default_rng(seed)
    for _ in range(3):
        r = rng.integers(-1000, 1001, size=n).astype(np.float64)
        np.testing.assert_array_equal(G @ r, Xd @ (Xd @ r))
    idx = _boundary_indices(n)
    ref = Xd[idx] @ Xd
    np.testing.assert_array_equal(G[idx, :], ref)
    np.testing.assert_array_equal(G[:, idx], ref.T)


def _square(lib, ctx, fn, X, in_dt, out_dt):
    n = X.shape[0]
    out = np.zeros(n * n, dtype=out_dt)
    Xf = _fl(X, in_dt)
    ctx.check(fn(ctx._h, n, _ptr(Xf), _ptr(out), 0))
    return out.reshape(n, n, order="F")


# ------------------------------------------------------------------ int8 and fp32 full squares
@pytest.mark.parametrize("n", [1100, 8192, 8100, 8200])
def test_square_i8_every_launch(pkg, gpu_ctx, n):
    """sdpsr_square_i8: n = 1100 dma128 unswizzled (gm 9); 8192 / 8100 gemm_tn_dma_kernel<I8, 0, 256> full, swizzled, 8100
    with a zero-padded border; 8200 dma128 gm 65 unswizzled, large grid.  Full int8 range; at 8192 also the all -128
    matrix (every sum n * 16384 = 2^27, the largest magnitude)."""
    lib = pkg.load_library()
    X = _sym_int(np.random.default_rng(n), n, 128, np.int8)
    got = _square(lib, gpu_ctx, lib.sdpsr_square_i8, X, np.int8, np.int32)
    _assert_exact_square(got, X, n * 16384, full=n <= 2048, seed=n)
    if n == 8192:
        X = np.full((n, n), -128, dtype=np.int8)
        got = _square(lib, gpu_ctx, lib.sdpsr_square_i8, X, np.int8, np.int32)
        assert (got == n * 16384).all()


@pytest.mark.parametrize("n", [1100, 8192, 8100, 8200])
def test_square_f32_every_launch(pkg, gpu_ctx, n):
    """sdpsr_square_f32 on integers in [-vmax, vmax], vmax = floor(sqrt(2^24 / n)) (the loop's rule, loop.cpp): every
    sum is an integer <= 2^24, exact in fp32.  n = 1100 dma128 unswizzled (gm 9); 8192 / 8100
    gemm_tn_dma_kernel<F32, 0, 256> full, swizzled (8100 padded); 8200 dma128 gm 65 unswizzled."""
    lib = pkg.load_library()
    vmax = int(np.floor(np.sqrt(2 ** 24 / n)))
    X = _sym_int(np.random.default_rng(n), n, vmax, np.float32)
    got = _square(lib, gpu_ctx, lib.sdpsr_square_f32, X, np.float32, np.float32)
    _assert_exact_square(got, X, n * vmax * vmax, full=n <= 2048, seed=n)


def test_square_f32_exactness_edge_n4096(pkg, gpu_ctx):
    """sdpsr_square_f32 at n = 4096 (dma128, gm 32, swizzled) on X = vmax s s', s in {-1, 1}^n, vmax = 64: every entry
    of X X = n vmax^2 s s' is +-2^24 exactly, the edge of the loop's exact fp32 range."""
    lib = pkg.load_library()
    n = 4096
    vmax = int(np.floor(np.sqrt(2 ** 24 / n)))
    assert n * vmax * vmax == 2 ** 24
    s = np.where(np.random.default_rng(4).random(n) < 0.5, -1.0, 1.0)
    X = vmax * np.outer(s, s)
    got = _square(lib, gpu_ctx, lib.sdpsr_square_f32, X, np.float32, np.float32)
    assert np.array_equal(got, (2.0 ** 24) * np.outer(s, s))


# ------------------------------------------------------------------ fp64
@pytest.mark.parametrize("n", [1024, 1100])
def test_square_f64_tile_orders(pkg, gpu_ctx, n):
    """sdpsr_square_f64 on signed real data: n = 1024 dma128 swizzled (gm 8), 1100 unswizzled (gm 9).  Elementwise
    |got - X X| <= 4 n eps (|X| |X|): the sum of the worst-case rounding bounds of the two dot products."""
    lib = pkg.load_library()
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, n))
    X = (X + X.T) / 2
    got = _square(lib, gpu_ctx, lib.sdpsr_square_f64, X, np.float64, np.float64)
    A = np.abs(X)
    assert (np.abs(got - X @ X) <= 4 * n * EPS * (A @ A)).all()


def test_square_f64_large_grid_exact(pkg, gpu_ctx):
    """sdpsr_square_f64 at n = 8192 (dma128, 64 x 64 tiles, swizzled) on integers in [-100, 100]: every sum is an
    integer below 2^53, so the product is exact and checked exactly (Freivalds + tile-boundary rows and columns)."""
    lib = pkg.load_library()
    n = 8192
    X = _sym_int(np.random.default_rng(8), n, 100, np.float64)
    got = _square(lib, gpu_ctx, lib.sdpsr_square_f64, X, np.float64, np.float64)
    _assert_exact_square(got, X, n * 100 * 100, full=False, seed=8)


@pytest.mark.parametrize("m, n, k, lda, ldb, ldc", [
    (1024, 640, 777, 777, 777, 1024),
    (1000, 1500, 300, 300, 300, 1000),
    (1000, 1016, 333, 345, 340, 1009),
])
def test_gemm_tn_f64_shapes(pkg, gpu_ctx, m, n, k, lda, ldb, ldc):
    """sdpsr_gemm_tn_f64, C = A'B: (1024, 640, 777) swizzled 8 x 5 grid with gm != gn and K 777 padded to 784;
    (1000, 1500, 300) swizzled 8 x 12, K 304; (1000, 1016, 333) with lda > k, ldb > k, ldc > m: the entries between
    the leading dimension and the matrix are neither read into the product nor written.  Elementwise bound
    4 k eps (|A|' |B|)."""
    lib = pkg.load_library()
    rng = np.random.default_rng(m + n + k)
    Ab = np.asfortranarray(rng.standard_normal((lda, m)))
    Bb = np.asfortranarray(rng.standard_normal((ldb, n)))
    Ab[k:] = np.nan  # padding rows: reading one of them into the product would poison it
    Bb[k:] = np.nan
    Cb = np.full((ldc, n), -7.0, order="F")
    gpu_ctx.check(lib.sdpsr_gemm_tn_f64(gpu_ctx._h, m, n, k, _ptr(Ab), lda, _ptr(Bb), ldb, _ptr(Cb), ldc, 0))
    A, B = Ab[:k], Bb[:k]
    assert (np.abs(Cb[:m] - A.T @ B) <= 4 * k * EPS * (np.abs(A).T @ np.abs(B))).all()
    assert (Cb[m:] == -7.0).all()


# ------------------------------------------------------------------ the loop's batched symmetric int8 square
@pytest.mark.parametrize("kernel, n, batch", [
    (1, 4096, 8),
    (1, 8192, 2),
    (1, 4096, 2),
    (1, 4104, 3),
    (0, 8192, 2),
    (0, 4096, 8),
])
def test_square_i8_symmetric_every_launch(pkg, kernel, n, batch):
    """sdpsr_square_i8_symmetric (lower-triangle tiles, upper mirrored).  square_kernel 1: (4096, 8) and (8192, 2)
    gemm_tn_dma_kernel<I8, 0, 256> lower-triangle mapping; (4096, 2) dma128 lower, 528 tiles all renumbered; (4104, 3)
    dma128 lower, gm 33, the last of 561 tiles keeps its number.  Default kernel: (8192, 2) (the bench's N = 8192
    shape) and (4096, 8) persistent i8_symsquare_kernel, 1024 jobs.  Batches of 8 carry one all -128 matrix."""
    lib = pkg.load_library()
    rng = np.random.default_rng(10 * n + batch + kernel)
    Xs = [_sym_int(rng, n, 128, np.int8) for _ in range(batch)]
    if batch == 8:
        Xs[5] = np.full((n, n), -128, dtype=np.int8)
    Xf = np.concatenate([_fl(X, np.int8) for X in Xs])
    out = np.zeros(batch * n * n, dtype=np.int32)
    with pkg.Context(seed=3, square_kernel=kernel) as ctx:
        ctx.check(lib.sdpsr_square_i8_symmetric(ctx._h, n, batch, _ptr(Xf), _ptr(out), 0))
    full = n * n * batch <= 2 * 4096 * 4096  # the (4096, 2) case: 0.27 TFLOP of host products
    for b, X in enumerate(Xs):
        got = out[b * n * n:(b + 1) * n * n].reshape(n, n, order="F")
        _assert_exact_square(got, X, n * 16384, full=full, seed=b)


# ------------------------------------------------------------------ the loop at scale, every square mode
@pytest.fixture(scope="module", params=["closed_scheme", "theta_er7xk72"])
def bench_case(request, pkg, problems, golden):
    """(name, setup, labels, dim, iterations): the host setup stage once per instance."""
    Cv, A, b, L, d, _, iters = problems.bench_instance(request.param, golden["er7_P"])
    return request.param, pkg.admissible_setup(Cv, A, b), L, d, iters


@pytest.mark.parametrize("mode, channels", [("f32", 0), ("f32", 8), ("f64", 0)])
def test_bench_instances_every_square_mode(pkg, bench_case, mode, channels):
    """The bench instances in the fp32 and fp64 square modes must reach the generator's partition bit for bit
    (README: P.matrix is the same in all three modes).  closed_scheme, N = 4096: fp32 with 2 channels squares in
    dma128 lower tiles, with 8 channels in gemm_tn_dma_kernel<F32, 0, 256> lower tiles (vmax = 64: sums up to 2^24);
    fp64 in dma128 swizzled.  theta_er7xk72, N = 4104 (ld 4224): dma128 lower / unswizzled fp64.  closed_scheme is
    closed: one iteration in every mode."""
    name, setup, L, d, iters = bench_case
    sq = {"f32": pkg.SQUARE_F32, "f64": pkg.SQUARE_F64}[mode]
    with pkg.Context(seed=11, square_mode=sq, channels=channels) as ctx:
        P = pkg.admissible_subspace(None, None, None, ctx=ctx, setup=setup)
    assert P.nparts == d, (name, mode, channels)
    assert np.array_equal(P.matrix, L), (name, mode, channels)
    if name == "closed_scheme":
        assert P.iterations == iters, (mode, channels)


# ------------------------------------------------------------------ the non-symmetric loop
@pytest.mark.parametrize("mode", ["i8", "f32"])
@pytest.mark.parametrize("n, channels", [(300, 0), (1100, 0), (4096, 0), (4096, 4)])
def test_nonsymmetric_loop_closes_the_directed_cycle(pkg, problems, mode, n, channels):
    """C_L = the directed n-cycle S handed to the loop as it is (X0_L = 0, no constraints): the labels stay
    non-symmetric, so every square is X X literally (left operand from the transposed labels, full -- not
    lower-triangle -- batched squares), and the closure is all n circulant classes, label ((i - j) mod n) + 1
    (pinned against the oracle in test_oracle_golden.py).  n = 300 / 1100: dma128 3 x 3 / 9 x 9; n = 4096,
    2 channels: dma128 32 x 32 swizzled; 4 channels: gemm_tn_dma_kernel<I8/F32, 0, 256> full with batch stride."""
    S = problems.directed_cycle_adjacency(n)
    setup = (n, S.ravel(order="F"), np.zeros(n * n), np.zeros((n * n, 0), order="F"))
    sq = {"i8": pkg.SQUARE_I8, "f32": pkg.SQUARE_F32}[mode]
    with pkg.Context(seed=5, square_mode=sq, channels=channels) as ctx:
        P = pkg.admissible_subspace(None, None, None, ctx=ctx, setup=setup)
    i, j = np.indices((n, n))
    assert P.nparts == n
    assert np.array_equal(P.matrix, (i - j) % n + 1)
