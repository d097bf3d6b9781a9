"""The steps of blockDiagonalize(P; complex = true) (csrc/kernels_complex.hip, csrc/complex.cpp), one by one, on made-up inputs
through the test entry points of libsdpsr_prof.so, against the references of tests/complex_steps_ref.py: the Hermitian gather, the
Hermitian eigensolver on both routes (route 0: the one-workgroup Jacobi kernel of n <= 64; route 1: the real symmetric embedding
with cx_embed, the real solver, cx_zero_pad, cx_rot, cx_stack, cx_combine and the host's pivoted Cholesky), the block norms and the
irreducible columns on both routes.

No tolerance here is measured on a kernel.  The eigensolver figures are those of the real twin (tests/test_gpu_small_syev.py), the
other bounds are the running error bounds written out in complex_steps_ref.py and judged there on a float64 evaluation
(tests/test_complex_steps_ref_cpu.py).  Every in/out array carries one NaN bit pattern (SENT) and is compared as BITS: outside the
documented region nothing may change, inside it everything must be written.

What these tests found, fixed in the same change ("The complex path's steps, tested one by one"): route 0 returned
eigenvalues wrong by 0.9 |H| at |H| ~ 1e-145 from order 3 on (a phase from a subnormal sum of squares); route 1 ended in
SDPSR_NUMERICAL_INCONSISTENCY on Wilkinson and graded matrices and lost orthogonality between clusters in proportion to rounding
error / eigenvalue gap (5.7e-5 on a graded matrix of order 96, 2e-11 on the driver's own element of Z_96); the general irreducible
kernel asked for more LDS than a workgroup has from n = 3371 on.

Excluded: the two extreme-scale families ("scale 1e145", "scale 1e-145", phased and real) on route 1 only -- the route runs the
dense real driver, whose norms are unscaled by design (test_syev_families_dense_driver excludes them for the same reason).
Route 0 runs every family."""
import ctypes as C

import numpy as np
import pytest

import complex_steps_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF85A5ADEADBEEF
GUARD = 300
BAD_ARGUMENT = 5


def _vp(a):
    """(the pointer alone: the caller keeps the array alive in a variable of its own until the call has returned)"""
    return C.c_void_p(a.ctypes.data)


def _fill(count):
    return np.full(int(count), SENT, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((_bits(a) == np.uint64(SENT)).all())


def _written(a):
    return not bool((_bits(a) == np.uint64(SENT)).any())


def _planes(Z):
    """column-major real and imaginary planes of a complex matrix"""
    return np.asfortranarray(Z.real).ravel(order="F").copy(), np.asfortranarray(Z.imag).ravel(order="F").copy()


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


# ---------------------------------------------------------------------------------------------------------------------------
# The gather
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GATHER_ORDERS)
def test_gather_herm_bit_exact(prof, gpu_ctx, n):
    """cx_gather_herm_kernel on non-symmetric labels with zeros: both planes bit for bit, the guard as it was."""
    L, _ = R.gather_labels(n)
    for key in R.GATHER_KEYS:
        Hr, Hi = _fill(n * n + GUARD), _fill(n * n + GUARD)
        gpu_ctx.check(prof.sdpsr_profile_cx_gather_herm(gpu_ctx._h, n, _vp(L), key, _vp(Hr), _vp(Hi), GUARD))
        wr, wi = R.gather_herm(n, L, key)
        assert np.array_equal(_bits(Hr[:n * n]), _bits(wr.ravel(order="F"))), (n, hex(key))
        assert np.array_equal(_bits(Hi[:n * n]), _bits(wi.ravel(order="F"))), (n, hex(key))
        assert _untouched(Hr[n * n:]) and _untouched(Hi[n * n:])


# ---------------------------------------------------------------------------------------------------------------------------
# The Hermitian eigensolver
# ---------------------------------------------------------------------------------------------------------------------------
def heev(prof, ctx, route, H, atol=0.0):
    """(status, w, V complex n x n, info, sentinel verdict) of one solve"""
    n = H.shape[0]
    hr, hi = _planes(H)
    w, Vr, Vi = _fill(n + GUARD), _fill(n * n + GUARD), _fill(n * n + GUARD)
    info = (C.c_int32 * 2)(-1, -1)
    st = prof.sdpsr_profile_cx_heev(ctx._h, route, n, _vp(hr), _vp(hi), float(atol), _vp(w), _vp(Vr), _vp(Vi), GUARD, info)
    clean = (_untouched(w[n:]) and _untouched(Vr[n * n:]) and _untouched(Vi[n * n:]) and _written(w[:n]) and _written(Vr[:n * n]) and
             _written(Vi[:n * n]))
    V = (Vr[:n * n] + 1j * Vi[:n * n]).reshape(n, n, order="F")
    return st, w[:n].copy(), V, (info[0], info[1]), clean


def heev_figures(st, w, V, info, clean, H, wl, sc):
    """(ok, |w - w_lapack| / |H|, |H V - V diag(w)| / |H|, |V^H V - I|): ok = status 0, info[0] == 0, the sentinels in order,
    everything finite, w ascending"""
    n = H.shape[0]
    if st != 0 or not (np.all(np.isfinite(w)) and np.all(np.isfinite(V))):
        return False, np.inf, np.inf, np.inf
    ok = info[0] == 0 and clean and bool(np.all(np.diff(w) >= 0))
    return (ok, float(np.abs(w - wl).max() / sc), float(np.abs(H @ V - V * w).max() / sc), float(np.abs(V.conj().T @ V - np.eye(n)).max()))


def run_heev_cases(prof, ctx, route, cases, keep=None, report=True):
    """Solves every (family, n), prints the worst figures per family, and returns the cases out of bounds."""
    worst, bad = {}, []
    for name, n in cases:
        H, wl, sc = R.hermitian(name, n)
        st, w, V, info, clean = heev(prof, ctx, route, H, R.heev1_atol(sc) if route == 1 else 0.0)
        ok, dw, res, orth = heev_figures(st, w, V, info, clean, H, wl, sc)
        cur = worst.setdefault(name, [0.0, 0.0, 0.0])
        worst[name] = [max(a, b) for a, b in zip(cur, (dw, res, orth))]
        if not ok or dw > R.HEEV_BOUNDS[0] or res > R.HEEV_BOUNDS[1] or not orth < R.HEEV_BOUNDS[2]:
            bad.append((route, name, n, st, info, clean, dw, res, orth))
        if keep is not None:
            keep[(name, n)] = (w, V)
    for name, (dw, res, orth) in worst.items() if report else ():
        print("cx_heev route %d  %-36s eigenvalues %.2e  residual %.2e  orthogonality %.2e" % (route, name, dw, res, orth))
    return bad


def test_heev_route0_families(prof, gpu_ctx):
    """cx_heev_jacobi64_kernel: a random Hermitian matrix at every n = 1..64, every family at the orders around the even padding and
    the wave boundaries of the (n/2)^2 threads."""
    bad = run_heev_cases(prof, gpu_ctx, 0, R.heev0_cases())
    assert not bad, bad


@pytest.fixture(scope="module")
def route0_solutions(prof, gpu_ctx):
    """route 0 on the cases both routes take, solved once"""
    keep = {}
    run_heev_cases(prof, gpu_ctx, 0, [c for n in R.HEEV1_ORDERS if n <= 64 for c in R.heev1_cases(n)], keep, report=False)
    return keep


@pytest.mark.parametrize("n", R.HEEV1_ORDERS)
def test_heev_route1_families(prof, gpu_ctx, route0_solutions, n):
    """cx_heev_general at 2n = 128 and 256 (no padding), 130 (a whole tile of padding) and around them, on every family but the
    extreme scales: real H (M(H) = diag(H, H)), imaginary H, clusters of multiplicity up to n.  Where route 0 applies too, the
    routes agree on w to the eigenvalue bound, and on the low-multiplicity families on the spectral projector of every eigenvalue
    to (residual bound) / (smallest gap of LAPACK's spectrum).  The route's cluster tolerance is complex_steps_ref.heev1_atol: the
    vectors of a cluster of distinct eigenvalues chained within it (the bottom of a graded spectrum) keep a residual of its order,
    7e-13 |H| at the worst."""
    keep = {}
    bad = run_heev_cases(prof, gpu_ctx, 1, R.heev1_cases(n), keep)
    if n <= 64:
        for (name, _), (w1, V1) in keep.items():
            w0, V0 = route0_solutions[(name, n)]
            sc = R.hermitian(name, n)[2]
            dw = float(np.abs(w1 - w0).max() / sc)
            if not dw <= R.HEEV_BOUNDS[0]:
                bad.append(("routes, eigenvalues", name, n, dw))
            if (name, n) in R.projector_cases():
                q = R.HEEV_BOUNDS[1] * sc / R.smallest_gap(name, n)
                assert q < R.PROJECTOR_QUOTIENT
                dp = max(float(np.abs(np.outer(V0[:, k], V0[:, k].conj()) - np.outer(V1[:, k], V1[:, k].conj())).max()) for k in range(n))
                print("cx_heev routes   %-36s n %3d  projectors %.2e  (bound %.2e)" % (name, n, dp, q))
                if not dp <= q:
                    bad.append(("routes, projectors", name, n, dp, q))
    assert not bad, bad


def test_heev_refusals(prof, gpu_ctx):
    H = R.hermitian("phased random symmetric", 65)[0]
    hr, hi = _planes(H)
    w, Vr, Vi = _fill(65 + GUARD), _fill(65 * 65 + GUARD), _fill(65 * 65 + GUARD)
    info = (C.c_int32 * 2)(-1, -1)
    for route, n, hrp in ((0, 65, _vp(hr)), (2, 8, _vp(hr)), (1, 0, _vp(hr)), (1, 4097, _vp(hr)), (1, 8, None)):
        assert prof.sdpsr_profile_cx_heev(gpu_ctx._h, route, n, hrp, _vp(hi), 0.0, _vp(w), _vp(Vr), _vp(Vi), GUARD, info) == BAD_ARGUMENT
    assert _untouched(w) and _untouched(Vr) and _untouched(Vi)


# ---------------------------------------------------------------------------------------------------------------------------
# Block norms
# ---------------------------------------------------------------------------------------------------------------------------
def block_norms(prof, ctx, route, H, V, space_of, neig):
    n = H.shape[0]
    hr, hi = _planes(H)
    vr, vi = _planes(V)
    out = _fill(neig * neig + GUARD)
    sp = np.ascontiguousarray(space_of, dtype=np.int32)
    ctx.check(prof.sdpsr_profile_cx_block_norms(ctx._h, route, n, _vp(hr), _vp(hi), _vp(vr), _vp(vi), _vp(sp), neig, _vp(out), GUARD))
    assert _untouched(out[neig * neig:]) and _written(out[:neig * neig])
    return out[:neig * neig].reshape(neig, neig)  # [sa, sb] = norms[sa * neig + sb]


def _two_ulp(got, sq):
    want = np.sqrt(sq.astype(np.float64))  # the correctly rounded root of an exact integer < 2^53
    return bool((np.abs(got - want) <= 2 * np.spacing(want)).all())


@pytest.mark.parametrize("route,n", [(r, n) for r in (0, 1) for n in R.NORM_ORDERS[r]])
def test_block_norms(prof, gpu_ctx, route, n):
    """cx_block_norms_kernel (route 0) and cx_block_norms_general (route 1: cx_embed, cx_stack, cx_rot, three MFMA GEMMs, the
    maximum kernel) with one space, n spaces and spaces of sizes 1 / 2 / rest: Gaussian integers, where every entry of V^H H V is an
    exact integer pair, to 2 ulp of the exact root; random complex inputs within the derived bound."""
    Hi_, Vi_ = R.gaussian_integers(n, 3)
    Hr_, Vr_ = R.random_complex(n, 3)
    for pname, space_of in R.partitions(n).items():
        neig = int(space_of.max()) + 1
        got = block_norms(prof, gpu_ctx, route, Hi_, Vi_, space_of, neig)
        assert _two_ulp(got, R.block_norms_exact(Hi_, Vi_, space_of, neig)), (route, n, pname)
        got = block_norms(prof, gpu_ctx, route, Hr_, Vr_, space_of, neig)
        ref, bound = R.block_norms(Hr_, Vr_, space_of, neig)
        assert (np.abs(got.astype(np.longdouble) - ref) <= bound).all(), (route, n, pname, float(np.abs(got - ref.astype(np.float64)).max()))


@pytest.mark.parametrize("n", (2, 5, 33, 64))
def test_block_norms_layout_on_a_general_matrix(prof, gpu_ctx, n):
    """route 0 multiplies by H as it is given, so a non-Hermitian H -- |G[a, b]| != |G[b, a]| -- pins the [sa * neig + sb] layout
    against its transpose (the embedding route needs M(H) symmetric, and a Hermitian H cannot tell the two apart)."""
    H, V = R.gaussian_integers(n, 9)
    H = np.triu(H) + 2 * np.tril(H, -1)
    for pname, space_of in R.partitions(n).items():
        neig = int(space_of.max()) + 1
        sq = R.block_norms_exact(H, V, space_of, neig)
        assert neig == 1 or not np.array_equal(sq, sq.T)
        assert _two_ulp(block_norms(prof, gpu_ctx, 0, H, V, space_of, neig), sq), (n, pname)


def test_block_norms_refusals(prof, gpu_ctx):
    H, V = R.gaussian_integers(5, 3)
    hr, hi = _planes(H)
    vr, vi = _planes(V)
    out = _fill(25 + GUARD)
    for route, n, neig, sp in ((0, 5, 3, [0, 1, 2, 3, 0]), (1, 5, 3, [0, -1, 2, 1, 0]), (1, 5, 6, [0] * 5), (1, 5, 0, [0] * 5), (3, 5, 1, [0] * 5)):
        sp = np.array(sp, dtype=np.int32)
        st = prof.sdpsr_profile_cx_block_norms(gpu_ctx._h, route, n, _vp(hr), _vp(hi), _vp(vr), _vp(vi), _vp(sp), neig, _vp(out), GUARD)
        assert st == BAD_ARGUMENT, (route, n, neig)
    assert _untouched(out)


# ---------------------------------------------------------------------------------------------------------------------------
# Irreducible columns
# ---------------------------------------------------------------------------------------------------------------------------
def irreducible(prof, ctx, route, H, V, desc, atol):
    n, vcols, ncols = H.shape[0], V.shape[1], desc.shape[0]
    hr, hi = _planes(H)
    vr, vi = _planes(V)
    out = _fill(2 * n * ncols + GUARD)
    d = np.ascontiguousarray(desc, dtype=np.int32)
    ctx.check(prof.sdpsr_profile_cx_irreducible(ctx._h, route, n, vcols, _vp(hr), _vp(hi), _vp(vr), _vp(vi), _vp(d), ncols, float(atol), _vp(out), GUARD))
    assert _untouched(out[2 * n * ncols:]) and _written(out[:2 * n * ncols])
    return out[:2 * n * ncols].view(np.complex128).reshape(n, ncols, order="F")  # column col at 2 n col, (re, im) interleaved


def _check_irreducible(got, case, where, factor=1):
    H, V, desc, atol, ref, bound, mask = case
    assert not _bits(got[mask]).any(), where  # clamped entries: +0.0 + 0.0i, bit for bit
    assert (np.abs(got[~mask]) > 0).all(), where
    assert (np.abs(got.real - ref.real) <= factor * bound).all() and (np.abs(got.imag - ref.imag) <= factor * bound).all(), \
        (where, float(np.abs(got - ref).max()), float(bound.max()))
    for kind, i0, _, _, _, col in desc:
        if kind == 0:  # the clamped eigenvector itself
            assert np.array_equal(_bits(got[:, col]), _bits(ref[:, col])), where


@pytest.mark.parametrize("n", R.IRREDUCIBLE_BOTH)
def test_irreducible_both_routes(prof, gpu_ctx, n):
    """cx_irreducible_kernel and cx_irreducible_general_kernel on the same inputs: a kind-0 column (bitwise the clamped eigenvector)
    and kind-1 columns with (mi, mj) in {(1, 1), (2, 3), (3, 2), (n/2, n/2)} as far as n goes, a root in front of and behind its
    member; within the bound, clamped entries +0.0, the routes within twice the bound of each other."""
    case = R.irreducible_case(n)
    H, V, desc, atol, ref, bound, mask = case
    got = [irreducible(prof, gpu_ctx, route, H, V, desc, atol) for route in (0, 1)]
    for route in (0, 1):
        _check_irreducible(got[route], case, (n, route))
    assert (np.abs(got[0].real - got[1].real) <= 2 * bound).all() and (np.abs(got[0].imag - got[1].imag) <= 2 * bound).all()


@pytest.mark.parametrize("n", R.IRREDUCIBLE_GENERAL)
def test_irreducible_general_route(prof, gpu_ctx, n):
    """cx_irreducible_general_kernel at n = 65; at n = 600 with (mi, mj) = (257, 300) and (300, 257): both strided loops and all 256
    slots of the norm's reduction; at 3370 (the last order the former 6 n doubles of LDS could hold), 3371 and 4096 (the largest
    order the complex path documents) with three columns of small mi, mj on made-up columns."""
    case = R.irreducible_case(n)
    H, V, desc, atol = case[:4]
    _check_irreducible(irreducible(prof, gpu_ctx, 1, H, V, desc, atol), case, n)


def test_irreducible_refusals(prof, gpu_ctx):
    H, V, desc, atol = R.irreducible_case(7)[:4]
    hr, hi = _planes(H)
    vr, vi = _planes(V)
    out = _fill(2 * 7 * len(desc) + GUARD)

    def call(route, n, vcols, d, ncols):
        d = np.ascontiguousarray(d, dtype=np.int32)
        return prof.sdpsr_profile_cx_irreducible(gpu_ctx._h, route, n, vcols, _vp(hr), _vp(hi), _vp(vr), _vp(vi), _vp(d), ncols, atol, _vp(out), GUARD)
    vcols, ncols = V.shape[1], len(desc)
    assert call(0, 65, vcols, desc, ncols) == BAD_ARGUMENT and call(1, 4097, vcols, desc, ncols) == BAD_ARGUMENT
    for row in ((1, 0, 2, vcols - 1, 2, 0), (1, vcols - 1, 2, 0, 1, 0), (0, vcols, 1, 0, 1, 0), (1, 0, 1, 1, 1, ncols), (1, 0, 0, 1, 1, 0),
                (1, 0, 1, 1, 8, 0), (2, 0, 1, 1, 1, 0), (1, -1, 1, 1, 1, 0)):
        d = np.array(desc)
        d[1] = row
        for route in (0, 1):
            assert call(route, 7, vcols, d, ncols) == BAD_ARGUMENT, row
    assert _untouched(out)
