"""The references of tests/eigen_stages_ref.py judged without a GPU: the evaluator on LAPACK's own tridiagonalisation of every
input family, the exact reflector families of the back-transformation against the float64 restatement of the library's block
algorithm, and LAPACK's eigenvalues on the scaled inputs of the range test."""
import numpy as np
import pytest

import eigen_stages_ref as R


@pytest.mark.parametrize("n", [129, 257, 640])
def test_evaluator_on_lapack_dsytrd(n):
    """If LAPACK's dsytrd alone broke 2e-15 under the evaluator, the evaluator would be wrong (measured: at most 5.8e-16 / 9.4e-16)."""
    for name in R.FAMILIES:
        bwd, orth = R.lapack_values(name, n)
        assert bwd <= 2e-15 and orth <= 2e-15, (n, name, bwd, orth)
        if name in ("diag", "zero", "tridiag"):
            assert bwd == 0 and orth == 0, (n, name)


def test_evaluator_sees_a_wrong_tridiagonalisation():
    """One stale reflector entry, one wrong tau, one wrong e: each shows far above the 16 x LAPACK margin of the GPU test."""
    n = 129
    A = R.family("gauss", n)
    d, e, tau, S = R.lapack_sytrd(A)
    ref = R.lapack_values("gauss", n)
    S2 = S.copy()
    S2[n - 1, 64] += 1e-8
    assert R.evaluate(A, d, e, tau, S2)[0] > 1e3 * ref[0]
    tau2 = tau.copy()
    tau2[100] *= 1 + 1e-8
    assert R.evaluate(A, d, e, tau2, S)[1] > 1e3 * ref[1]
    e2 = e.copy()
    e2[5] = -e2[5]
    assert R.evaluate(A, d, e2, tau, S)[0] > 1e-3


def test_families_have_the_structure_the_gpu_test_relies_on():
    for n in (100, 129, 300):
        A = R.family("sum", n)
        assert sum(R.sum_blocks(n)) == n
        for j in R.sum_boundaries(n):
            assert not A[j + 1:, :j + 1].any(), (n, j)  # exactly zero below the boundary
        P = R.family("sum_perm", n)
        assert np.array_equal(np.sort(np.linalg.eigvalsh(P)), np.sort(np.linalg.eigvalsh(P)))
        assert np.count_nonzero(P) == np.count_nonzero(A)
        assert np.abs(np.linalg.eigvalsh(A) - np.linalg.eigvalsh(P)).max() <= 1e-12 * np.abs(A).sum(axis=0).max()
        w = np.linalg.eigvalsh(R.family("two", n))
        assert np.abs(w[:-1] - 0.5).max() <= 1e-13 * n and abs(w[-1] - (0.5 + n / 4)) <= 1e-13 * n
        C = R.family("scheme", n)
        assert np.array_equal(C, np.roll(np.roll(C, 1, 0), 1, 1))  # circulant
    assert R.sum_blocks(300) == [1, 40, 1, 60, 198] and R.sum_boundaries(300) == [0, 40, 41, 101]
    assert R.sum_blocks(100) == [1, 40, 1, 58]


def test_column0_is_dlarfg():
    """The longdouble column-0 reference against LAPACK's dsytrd (which calls dlarfg on the untouched first column)."""
    for n in (129, 300):
        for name in R.FAMILIES:
            A = R.family(name, n)
            d, e, tau, S = R.lapack_sytrd(A)
            e0, tau0, v0 = R.column0(A)
            assert R.ulp_distance(e[0], e0) <= 4 and R.ulp_distance(tau[0], tau0) <= 4 and R.ulp_distance(S[2:, 0], v0) <= 4, (n, name)


@pytest.mark.parametrize("n", [129, 130, 257, 300])
def test_exact_reflector_families(n):
    """signs / swaps: the reflector-by-reflector product is exact in fp64 (integers), Q is a signed permutation, and the float64
    restatement of the block algorithm gives the same VALUES, with integer T of magnitude <= 2 and |W| <= 18."""
    Z = R.integer_z(n)
    for make in (R.reflectors_signs, R.reflectors_swaps):
        S, tau = make(n)
        exact = R.apply_reflectors(S, tau, Z)
        assert np.array_equal(exact, np.asarray(R.apply_reflectors(S, tau, Z, R.LD), dtype=np.float64))
        Q = R.apply_reflectors(S, tau, np.eye(n))
        assert np.array_equal(np.abs(Q).sum(axis=0), np.ones(n)) and np.array_equal(np.abs(Q).sum(axis=1), np.ones(n))
        assert set(np.unique(Q)) <= {-1.0, 0.0, 1.0}
        assert np.array_equal(np.sort(np.abs(exact), axis=0), np.sort(np.abs(Z), axis=0))
        trace = []
        got = R.block_wy(S, tau, Z, trace)
        assert (got == exact).all(), make.__name__
        for T, W in trace:
            assert np.array_equal(T, np.round(T)) and np.abs(T).max() <= 2 and np.abs(W).max() <= 18
    # swaps: a cycle really crosses the first block boundary (rows 128, 129 move together with rows below 128)
    S, tau = R.reflectors_swaps(n)
    Q = R.apply_reflectors(S, tau, np.eye(n))
    src = np.abs(Q).argmax(axis=1)
    assert (src[:128] >= 128).any() or (src[128:] < 128).any()


@pytest.mark.parametrize("n", [129, 300])
def test_general_reflector_family_block_form(n):
    """For any tau the compact-WY blocks equal the product of the factors: the float64 restatement stays within 16 x the error of
    the float64 reflector-by-reflector application, both against longdouble -- the bound the GPU test holds the kernels to."""
    S, tau = R.reflectors_general(n)
    assert (tau == 0).any() and ((tau >= 0.5) | (tau == 0)).all() and tau.max() <= 2
    Z = R.integer_z(n)
    ref = R.apply_reflectors(S, tau, Z, R.LD)
    assert np.isfinite(np.asarray(ref, dtype=np.float64)).all()
    e_seq = float(np.abs(R.apply_reflectors(S, tau, Z) - ref).max())
    e_blk = float(np.abs(R.block_wy(S, tau, Z) - ref).max())
    assert e_seq > 0 and e_blk <= 16 * e_seq, (n, e_blk, e_seq)


def test_lapack_is_right_at_every_scale():
    """numpy.linalg.eigvalsh on 2^k A is finite and equals 2^k eigvalsh(A) to the range test's own bound, for every k it uses."""
    for name in ("gauss", "scheme"):
        for n in (100, 130, 300):
            A = R.family(name, n)
            w0 = np.linalg.eigvalsh(A)
            for k in R.SCALE_EXPONENTS:
                wk = np.linalg.eigvalsh(np.ldexp(A, k))
                assert np.isfinite(wk).all(), (name, n, k)
                assert np.abs(np.ldexp(wk, -k) - w0).max() <= 1e-12 * np.abs(w0).max(), (name, n, k)
