"""sdpsr_syev_f64 on every route, with the hard spectra of syev_families.py: the one-workgroup Jacobi kernels of the small
orders (ping-pong form up to 64, small_syev_jacobi_kernel up to 128) and the dense driver (tridiagonalisation in row form,
panel form and one-launch form, divide and conquer, back-transformation).  The existing tests reach these with full-rank
Gaussian matrices, and the tridiagonal hard cases never exercise the tridiagonalisation; here the matrices have exact low
rank, huge multiplicities, decoupled blocks, grading and extreme scales.  Bounds of
test_tridiagonal_divide_and_conquer_hard_cases: w ascending, |w - w_lapack| <= 2e-13 |A|, |A V - V diag(w)| <= 1e-12 |A|,
|V'V - I| < 1e-12, with |A| = max |eigenvalue| (1 for the zero matrix)."""
import ctypes as C

import numpy as np
import pytest

import syev_families as fam

pytestmark = pytest.mark.gpu

BOUNDS = (2e-13, 1e-12, 1e-12)  # eigenvalues / |A|, residual / |A|, orthogonality


def figures(lib, ctx, A, wl, sc):
    """(status, |w - w_lapack| / |A|, |A V - V diag(w)| / |A|, |V'V - I|, ascending) of one solve from host arrays; the upper
    triangle holds 1e300 (only the lower one is referenced)."""
    n = A.shape[0]
    B = np.array(A, order="F")
    B[np.triu_indices(n, 1)] = 1e300
    w = np.full(n, np.nan)
    V = np.full((n, n), np.nan, order="F")
    st = lib.sdpsr_syev_f64(ctx._h, n, C.c_void_p(B.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(V.ctypes.data), 0)
    if st != 0 or not (np.all(np.isfinite(w)) and np.all(np.isfinite(V))):
        return st, np.inf, np.inf, np.inf, False
    return (st, float(np.abs(w - wl).max() / sc), float(np.abs(A @ V - V * w).max() / sc), float(np.abs(V.T @ V - np.eye(n)).max()),
            bool(np.all(np.diff(w) >= 0)))


def run_cases(lib, ctx, route, cases, reference=fam.reference):
    """Solves every (family, n), prints the worst figures per family, and returns the cases out of bounds."""
    worst, bad = {}, []
    for name, n in cases:
        st, dw, res, orth, asc = figures(lib, ctx, *reference(name, n))
        cur = worst.setdefault(name, [0.0, 0.0, 0.0])
        worst[name] = [max(a, b) for a, b in zip(cur, (dw, res, orth))]
        if st != 0 or not asc or dw > BOUNDS[0] or res > BOUNDS[1] or not orth < BOUNDS[2]:
            bad.append((route, name, n, st, asc, dw, res, orth))
    for name, (dw, res, orth) in worst.items():
        print("%-28s %-20s eigenvalues %.2e  residual %.2e  orthogonality %.2e" % (route, name, dw, res, orth))
    return bad


def test_syev_families_ping_pong_jacobi(pkg, gpu_ctx):
    """n <= 64, small_syev_jacobi64_kernel: a random matrix at every order, every family (the extreme scales take the
    IEEE branch of jacobi_angle) at orders around the even padding and the wave boundaries of the (n/2)^2 threads."""
    lib = pkg.load_library()
    cases = [("random symmetric", n) for n in range(1, 65)]
    cases += [(name, n) for n in (1, 2, 3, 4, 5, 7, 8, 16, 17, 33, 34, 63, 64) for name in fam.names(n) if (name, n) not in cases]
    bad = run_cases(lib, gpu_ctx, "ping-pong jacobi", cases)
    assert not bad, bad


def test_syev_families_one_workgroup_jacobi(pkg, gpu_ctx):
    """65 <= n <= 128, small_syev_jacobi_kernel: a random matrix at every order, every family with the extreme scales at
    orders on both sides of 96 (eigenvectors in LDS / in global memory), odd and even."""
    lib = pkg.load_library()
    cases = [("random symmetric", n) for n in range(65, 129)]
    cases += [(name, n) for n in (65, 66, 72, 100, 127, 128) for name in fam.names(n) if (name, n) not in cases]
    bad = run_cases(lib, gpu_ctx, "one-workgroup jacobi", cases)
    assert not bad, bad


def test_syev_families_dense_driver(pkg, gpu_ctx):
    """n >= 129: every family but the extreme scales (the driver's norms are unscaled by design) in the default row form;
    the low-rank families, whose trailing blocks are rounding noise of low rank, in the panel form at 640 and at 2304 --
    the smallest order with panel columns in front of the row form -- in the two-launch and the one-launch panel forms."""
    lib = pkg.load_library()
    bad = run_cases(lib, gpu_ctx, "dense, row form", [(name, n) for n in (129, 130, 200, 256, 384, 640) for name in fam.names(n, extreme=False)])
    large = {name: fam.reference.__wrapped__(name, 2304) for name in fam.LOW_RANK}  # 42 MB each: not kept beyond this test
    for route, n, flags in (("dense, panels 640", 640, pkg._lib.FLAG_SYTRD_PANELS), ("dense, hybrid 2304", 2304, 0),
                            ("dense, one-launch 2304", 2304, pkg._lib.FLAG_SYTRD_ONE_LAUNCH)):
        with pkg.Context(seed=1, flags=flags) as ctx:
            bad += run_cases(lib, ctx, route, [(name, n) for name in fam.LOW_RANK], fam.reference if n == 640 else lambda name, n: large[name])
    assert not bad, bad
