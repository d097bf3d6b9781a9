"""The steps of the real dense blockDiagonalize (csrc/eigdec.cpp; the kernels at the head of csrc/kernels_blockdiag.hip), one by one,
on made-up inputs through the test entry points of libsdpsr_prof.so, against the references of tests/dense_steps_ref.py: the coupling
matrix on its three routes (the one-workgroup kernel, EigDec::couple(), launch_block_norms alone), the one-read-back cluster kernel,
isomorphism_classes_device (coupling_symmetrize_minmax, coupling_count, coupling_bits and the host chain between them), the
irreducible columns by the pair kernel and one by one (gemv_t, inv_norm, gemv_n_scaled), copy_cols and clamptol.

No tolerance here is measured on a kernel.  The integer families are exact in fp64 in every order of summation and are compared as
BITS; the Otsu chain is an exact function of the entries and is compared as bits; the real-data bounds are the running error bounds
written out in dense_steps_ref.py and judged there on a float64 evaluation (tests/test_dense_steps_ref_cpu.py).  Every in/out array
carries one NaN bit pattern (SENT) and is compared as bits: outside the documented region nothing may change, inside it everything
must be written."""
import ctypes as C

import numpy as np
import pytest

import dense_steps_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF85A5ADEADBEEF
GUARD = 300
POISON = 12345.0  # padding rows of an input: finite, so that a kernel that reads them shows in the result


def _vp(a):
    """(the pointer alone: the caller keeps the array alive in a variable of its own until the call has returned)"""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _fill(count):
    return np.full(int(count), SENT, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((_bits(a) == np.uint64(SENT)).all())


def _written(a):
    return not bool((_bits(a) == np.uint64(SENT)).any())


def _same(a, b):
    return np.array_equal(_bits(np.asarray(a, dtype=np.float64)), _bits(np.asarray(b, dtype=np.float64)))


def _colmajor(X, ld, cols, pad):
    """X (r x c) in a column-major ld x cols array, everything else `pad`"""
    buf = np.full(ld * cols, pad, dtype=np.float64)
    buf.reshape(cols, ld)[:X.shape[1], :X.shape[0]] = X.T
    return buf


def _matrix(buf, ld, cols):
    """the ld x cols matrix a column-major array holds (a view)"""
    return buf[:ld * cols].reshape(cols, ld).T


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


# ---------------------------------------------------------------------------------------------------------------------------
# Block norms
# ---------------------------------------------------------------------------------------------------------------------------
def block_norms(prof, ctx, route, n, ld, A, Q, space_of, neig, start, with_m=True, with_t=True, m_given=None):
    """(norms neig x neig, M n x n or None, T n x n or None) of one call, after the sentinel checks.  route 2: m_given is M."""
    cols = ld if route == 1 else n
    pad = 0.0 if route == 1 else POISON
    a = _colmajor(A, ld, cols, pad) if route != 2 else None
    q = _colmajor(Q, ld, cols, pad) if route != 2 else None
    sp = np.ascontiguousarray(space_of, dtype=np.int32)
    norms = _fill(neig * neig + GUARD)
    norms[:neig * neig] = np.asarray(start, dtype=np.float64).ravel()
    m = t = None
    if route == 2:
        m = _fill(ld * n + GUARD)
        _matrix(m, ld, n)[:n] = m_given
        m_before = m.copy()
    elif with_m:
        m = _fill(ld * cols + GUARD)
    if with_t and route != 2:
        t = _fill(ld * cols + GUARD)
    ctx.check(prof.sdpsr_profile_dense_block_norms(ctx._h, route, n, ld, _vp(a), _vp(q), _vp(sp), neig, _vp(norms), _vp(m), _vp(t), GUARD))
    assert _untouched(norms[neig * neig:])
    out = [norms[:neig * neig].reshape(neig, neig).copy(), None, None]
    if route == 2:
        assert np.array_equal(_bits(m), _bits(m_before))  # read only
    for k, x in ((1, m), (2, t)):
        if x is None or route == 2:
            continue
        X = _matrix(x, ld, cols)
        assert _untouched(x[ld * cols:])
        if route == 0:
            assert _written(X[:n]) and _untouched(X[n:])
        else:
            assert _written(X) and not X[n:].any() and not X[:, n:].any()  # the products of the zero padding
        out[k] = X[:n, :n].copy()
    return out


def _integer_expectation(n):
    A, Q = R.integer_family(n)
    R.assert_exact_qtaq(A, Q)
    T, M = R.qtaq_exact(A, Q)
    return A, Q, T.astype(np.float64), M.astype(np.float64)


def _starts(neig, new):
    return {name: R.start_values(name, neig, new) for name in ("zeros", "raise")}


@pytest.mark.parametrize("n", R.SMALL_ORDERS)
def test_block_norms_small_kernel(prof, gpu_ctx, n):
    """small_qtaq_block_norms_kernel with ld = n and ld = 128, M and T each null and non-null, every layout, norms from zeros and from
    values above and below the new maxima: the integer family bit for bit (norms, M, T); the real family within the bound."""
    A, Q, T, M = _integer_expectation(n)
    absr, boundr = R.real_qtaq(n)
    Ar, Qr = R.real_family(n)
    worst = 0.0
    for ld in (n, 128):
        for lname, sp in R.layouts(n, False).items():
            neig = int(sp.max()) + 1
            new = R.block_max(np.abs(M), sp, neig)
            for sname, start in _starts(neig, new).items():
                for with_m, with_t in ((True, True), (False, True), (True, False), (False, False)):
                    got, gm, gt = block_norms(prof, gpu_ctx, 0, n, ld, A, Q, sp, neig, start, with_m, with_t)
                    where = (n, ld, lname, sname, with_m, with_t)
                    assert _same(got, np.maximum(start, new)), where
                    assert (gm is None) == (not with_m) and (gt is None) == (not with_t)
                    assert gm is None or _same(gm, M), where
                    assert gt is None or _same(gt, T), where
            ref, bound = R.block_max(absr, sp, neig), R.block_max(boundr, sp, neig)
            got = block_norms(prof, gpu_ctx, 0, n, ld, Ar, Qr, sp, neig, np.zeros((neig, neig)))[0]
            err = np.abs(got.astype(R.LD) - ref)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (n, ld, lname, float(err.max()), float(bound.max()))
    print("block norms route 0  n %4d  real family: largest error / bound %.3f" % (n, worst))


@pytest.mark.parametrize("n", R.LARGE_ORDERS)
def test_block_norms_couple_and_kernel_alone(prof, gpu_ctx, n):
    """EigDec::couple() (route 1: two MFMA products on the padded squares, then block_norms_kernel) and launch_block_norms alone
    (route 2, with ld = n and ld > n), every layout and the non-monotone one, norms from zeros and from a raise.  n = 65, 127, 129,
    200: waves that straddle columns; 730: the second trip of the grid-stride loop."""
    A, Q, T, M = _integer_expectation(n)
    absr, boundr = R.real_qtaq(n)
    Ar, Qr = R.real_family(n)
    Mr = np.asarray(absr, dtype=np.float64)  # route 2 gets the rounded reference as its matrix: its maxima are then exact
    ld1 = R.round_up(n, 128)
    worst = 0.0
    for lname, sp in R.layouts(n, True).items():
        neig = int(sp.max()) + 1
        new = R.block_max(np.abs(M), sp, neig)
        for sname, start in _starts(neig, new).items():
            got, gm, gt = block_norms(prof, gpu_ctx, 1, n, ld1, A, Q, sp, neig, start)
            assert _same(got, np.maximum(start, new)) and _same(gm, M) and _same(gt, T), (n, 1, lname, sname)
            for ld in (n, n + 3, ld1):
                got = block_norms(prof, gpu_ctx, 2, n, ld, None, None, sp, neig, start, m_given=-M)[0]  # (|.| of negated entries)
                assert _same(got, np.maximum(start, new)), (n, 2, ld, lname, sname)
        ref, bound = R.block_max(absr, sp, neig), R.block_max(boundr, sp, neig)
        got = block_norms(prof, gpu_ctx, 1, n, ld1, Ar, Qr, sp, neig, np.zeros((neig, neig)))[0]
        err = np.abs(got.astype(R.LD) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (n, lname, float(err.max()), float(bound.max()))
        start = R.start_values("raise", neig, ref.astype(np.float64))
        got = block_norms(prof, gpu_ctx, 1, n, ld1, Ar, Qr, sp, neig, start)[0]
        up = start > ref.astype(np.float64)
        assert _same(got[up], start[up]) and (np.abs(got.astype(R.LD) - ref)[~up] <= bound[~up]).all(), (n, lname)
        got = block_norms(prof, gpu_ctx, 2, n, n + 3, None, None, sp, neig, np.zeros((neig, neig)), m_given=Mr)[0]
        assert _same(got, R.block_max(Mr, sp, neig)), (n, lname)
    print("block norms route 1  n %4d  real family: largest error / bound %.3f" % (n, worst))


@pytest.mark.parametrize("n", (3, 64, 65, 200))
def test_block_norms_zero_entries_do_not_write(prof, gpu_ctx, n):
    """-0.0 and +0.0 entries of M write nothing: norms keeps its zero bits (the bit pattern of -0.0 would win every maximum) and its
    start values, on the block_norms_kernel; the zero row and column the integer family gives M do the same on routes 0 and 1."""
    sp = (np.arange(n) % 3).astype(np.int32)
    M = np.arange(1.0, n * n + 1).reshape(n, n)
    M[np.ix_(sp == 1, sp == 2)] = -0.0
    M[np.ix_(sp == 2, sp == 2)] = 0.0
    M[0, 0] = -0.0
    for start in (np.zeros((3, 3)), np.full((3, 3), 0.25)):
        got = block_norms(prof, gpu_ctx, 2, n, n + 1, None, None, sp, 3, start, m_given=M)[0]
        want = np.maximum(start, R.block_max(np.abs(M), sp, 3))
        assert _same(got, want) and _same(got[1:, 2], start[1:, 2]), n
    A, Q, _, Mi = _integer_expectation(n)
    assert not Mi[n - 1].any() and not Mi[:, n - 1].any()
    spn = np.arange(n, dtype=np.int32)
    for route in (0, 1) if n <= 64 else (1,):
        got = block_norms(prof, gpu_ctx, route, n, 128 * ((n + 127) // 128), A, Q, spn, n, np.zeros((n, n)))[0]
        assert not _bits(got[n - 1]).any() and not _bits(got[:, n - 1]).any() and _same(got, np.abs(Mi)), (n, route)


@pytest.mark.parametrize("n", R.SMALL_ORDERS)
def test_block_norms_routes_agree(prof, gpu_ctx, n):
    """routes 0 and 1 bit for bit on the integer family at n <= 64: norms, M and T"""
    A, Q = R.integer_family(n)
    for sp in R.layouts(n, False).values():
        neig = int(sp.max()) + 1
        r0 = block_norms(prof, gpu_ctx, 0, n, 128, A, Q, sp, neig, np.zeros((neig, neig)))
        r1 = block_norms(prof, gpu_ctx, 1, n, 128, A, Q, sp, neig, np.zeros((neig, neig)))
        assert all(_same(x, y) for x, y in zip(r0, r1)), n


@pytest.mark.parametrize("n", (2, 5, 33, 64, 65, 200))
def test_block_norms_layout_on_a_general_matrix(prof, gpu_ctx, n):
    """A non-symmetric element makes M = Q' A' Q non-symmetric: norms[sa * neig + sb] has the ROW space first, on routes 0 and 1 and
    in the cluster kernel (a symmetric element cannot tell the layout from its transpose)."""
    A, Q = R.general_integer_family(n)
    R.assert_exact_qtaq(A, Q, symmetric=False)
    T, M = (x.astype(np.float64) for x in R.qtaq_exact(A, Q))
    for lname, sp in R.layouts(n, True).items():
        neig = int(sp.max()) + 1
        want = R.block_max(np.abs(M), sp, neig)
        assert neig == 1 or not np.array_equal(want, want.T)
        for route in (0, 1) if n <= 64 else (1,):
            if route == 0 and lname == "non-monotone":
                continue
            got, gm, gt = block_norms(prof, gpu_ctx, route, n, R.round_up(n, 128), A, Q, sp, neig, np.zeros((neig, neig)))
            assert _same(got, want) and _same(gm, M) and _same(gt, T), (n, route, lname)
    if n <= 64:
        ev = np.ascontiguousarray(R.eigenvalue_lists(n, R.CLUSTER_ATOL)["all apart"])
        o_norms = R.pack_layout(n)[2]
        a, q, einfo, pack = _colmajor(A, n, n, POISON), _colmajor(Q, n, n, POISON), np.zeros(2, dtype=np.int32), _fill(R.pack_layout(n)[3] // 8 + GUARD)
        gpu_ctx.check(prof.sdpsr_profile_dense_cluster_norms(gpu_ctx._h, n, n, _vp(a), _vp(q), _vp(ev), R.CLUSTER_ATOL, _vp(einfo), _vp(pack), None, GUARD))
        assert _same(pack[o_norms // 8:o_norms // 8 + n * n].reshape(n, n), np.abs(M)), n


def test_block_norms_refusals(prof, gpu_ctx):
    A, Q = R.integer_family(5)
    a, q = _colmajor(A, 128, 128, 0.0), _colmajor(Q, 128, 128, 0.0)
    norms, m, t = _fill(25 + GUARD), _fill(128 * 128 + GUARD), _fill(128 * 128 + GUARD)
    ok = np.zeros(65, dtype=np.int32)

    def call(route, n, ld, ap, qp, sp, neig, np_, mp, tp, guard=GUARD):
        return prof.sdpsr_profile_dense_block_norms(gpu_ctx._h, route, n, ld, ap, qp, _vp(sp) if sp is not None else None, neig, np_, mp, tp, guard)
    V = _vp
    cases = [(3, 5, 128, V(a), V(q), ok, 1, V(norms), V(m), V(t)), (-1, 5, 128, V(a), V(q), ok, 1, V(norms), V(m), V(t)),
             (0, 65, 128, V(a), V(q), ok, 1, V(norms), V(m), V(t)), (0, 0, 128, V(a), V(q), ok, 1, V(norms), V(m), V(t)),
             (1, 4097, 4224, V(a), V(q), ok, 1, V(norms), V(m), V(t)), (0, 5, 4, V(a), V(q), ok, 1, V(norms), V(m), V(t)),
             (1, 5, 127, V(a), V(q), ok, 1, V(norms), V(m), V(t)), (1, 5, 128, V(a), V(q), ok, 1, V(norms), None, V(t)),
             (1, 5, 128, V(a), V(q), ok, 1, V(norms), V(m), None), (2, 5, 128, None, None, ok, 1, V(norms), None, None),
             (0, 5, 128, None, V(q), ok, 1, V(norms), V(m), V(t)), (0, 5, 128, V(a), None, ok, 1, V(norms), V(m), V(t)),
             (0, 5, 128, V(a), V(q), None, 1, V(norms), V(m), V(t)), (0, 5, 128, V(a), V(q), ok, 1, None, V(m), V(t)),
             (0, 5, 128, V(a), V(q), ok, 0, V(norms), V(m), V(t)), (0, 5, 128, V(a), V(q), ok, 6, V(norms), V(m), V(t)),
             (0, 5, 128, V(a), V(q), np.array([0, 1, 2, 3, 0], dtype=np.int32), 3, V(norms), V(m), V(t)),
             (2, 5, 128, None, None, np.array([0, -1, 2, 1, 0], dtype=np.int32), 3, V(norms), V(m), None)]
    for case in cases:
        assert call(*case) == R.BAD_ARGUMENT, case[:3]
    assert call(0, 5, 128, V(a), V(q), ok, 1, V(norms), V(m), V(t), guard=-1) == R.BAD_ARGUMENT
    assert call(0, 5, 128, V(a), V(q), ok, 1, V(norms), V(m), V(t), guard=(1 << 20) + 1) == R.BAD_ARGUMENT
    assert _untouched(norms) and _untouched(m) and _untouched(t)


# ---------------------------------------------------------------------------------------------------------------------------
# The cluster kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 33, 64))
def test_cluster_kernel(prof, gpu_ctx, n):
    """small_cluster_qtaq_block_norms_kernel: the whole pack -- einfo in words 0, 1, words 2, 3 and the padding untouched, the number
    of eigenspaces, space_of, the values and the norms as bits --, T, and the norms equal to route 0's given the same space_of."""
    A, Q, T, M = _integer_expectation(n)
    o_space, o_vals, o_norms, total = R.pack_layout(n)
    for ld in (n, 128):
        a, q = _colmajor(A, ld, n, POISON), _colmajor(Q, ld, n, POISON)
        for name, ev in R.eigenvalue_lists(n, R.CLUSTER_ATOL).items():
            ev = np.ascontiguousarray(ev, dtype=np.float64)
            sp = R.cluster(ev, R.CLUSTER_ATOL)
            neig = int(sp.max()) + 1
            einfo = np.array([0, 7], dtype=np.int32)
            pack = _fill(total // 8 + GUARD)
            t = _fill(ld * n + GUARD)
            gpu_ctx.check(prof.sdpsr_profile_dense_cluster_norms(gpu_ctx._h, n, ld, _vp(a), _vp(q), _vp(ev), R.CLUSTER_ATOL, _vp(einfo), _vp(pack),
                                                                  _vp(t), GUARD))
            where = (n, ld, name)
            words = pack.view(np.int32)
            sent32 = np.array([SENT], dtype=np.uint64).view(np.int32)
            assert list(words[:2]) == [0, 7] and words[4] == neig, where
            assert np.array_equal(words[2:4], sent32) and _untouched(pack[3:8]) and np.array_equal(words[5:6], sent32[1:]), where
            assert np.array_equal(words[o_space // 4:o_space // 4 + n], sp), where
            tail = words[o_space // 4 + n:o_vals // 4]  # the padding of space_of: halves of the sentinel
            assert np.array_equal(tail, np.resize(sent32[n % 2:].tolist() + sent32[:n % 2].tolist(), tail.size)), where
            assert np.array_equal(_bits(pack[o_vals // 8:o_vals // 8 + n]), _bits(ev)), where
            got = pack[o_norms // 8:o_norms // 8 + neig * neig].reshape(neig, neig)
            assert _same(got, R.block_max(np.abs(M), sp, neig)), where
            assert _untouched(pack[o_norms // 8 + neig * neig:]), where  # the rest of the n x n room and the guard
            assert _same(_matrix(t, ld, n)[:n], T) and _untouched(_matrix(t, ld, n)[n:]) and _untouched(t[ld * n:]), where
            r0 = block_norms(prof, gpu_ctx, 0, n, ld, A, Q, sp, neig, np.zeros((neig, neig)))[0]
            assert _same(got, r0), where


def test_cluster_kernel_refusals(prof, gpu_ctx):
    A, Q = R.integer_family(5)
    a, q = _colmajor(A, 8, 5, POISON), _colmajor(Q, 8, 5, POISON)
    ev, einfo = np.zeros(5), np.zeros(2, dtype=np.int32)
    pack, t = _fill(R.pack_layout(5)[3] // 8 + GUARD), _fill(8 * 5 + GUARD)
    V = _vp
    for n, ld, ap, qp, evp, ip, pp, guard in ((0, 8, V(a), V(q), V(ev), V(einfo), V(pack), GUARD), (65, 128, V(a), V(q), V(ev), V(einfo), V(pack), GUARD),
                                               (5, 4, V(a), V(q), V(ev), V(einfo), V(pack), GUARD), (5, 8, None, V(q), V(ev), V(einfo), V(pack), GUARD),
                                               (5, 8, V(a), None, V(ev), V(einfo), V(pack), GUARD), (5, 8, V(a), V(q), None, V(einfo), V(pack), GUARD),
                                               (5, 8, V(a), V(q), V(ev), None, V(pack), GUARD), (5, 8, V(a), V(q), V(ev), V(einfo), None, GUARD),
                                               (5, 8, V(a), V(q), V(ev), V(einfo), V(pack), -1)):
        assert prof.sdpsr_profile_dense_cluster_norms(gpu_ctx._h, n, ld, ap, qp, evp, 1e-9, ip, pp, V(t), guard) == R.BAD_ARGUMENT, (n, ld)
    assert _untouched(pack) and _untouched(t)


# ---------------------------------------------------------------------------------------------------------------------------
# The classes
# ---------------------------------------------------------------------------------------------------------------------------
def classes(prof, ctx, raw, dims, atol):
    ne = len(dims)
    W = (ne + 63) // 64
    norms = _fill(ne * ne + GUARD)
    norms[:ne * ne] = np.asarray(raw, dtype=np.float64).ravel()
    d = np.ascontiguousarray(dims, dtype=np.int32)
    stat, edges, thr = np.full(20, SENT, dtype=np.uint64), _fill(17), _fill(1)
    bits = np.full(ne * W + GUARD, SENT, dtype=np.uint64)
    kpart = np.full(ne, -1, dtype=np.int32)
    st = prof.sdpsr_profile_dense_classes(ctx._h, ne, _vp(norms), _vp(d), float(atol), _vp(stat), _vp(edges), _vp(thr), _vp(bits), _vp(kpart), GUARD)
    assert _untouched(norms[ne * ne:]) and (bits[ne * W:] == np.uint64(SENT)).all()
    return st, norms[:ne * ne].reshape(ne, ne), stat, edges, thr[0], bits[:ne * W].reshape(ne, W), kpart


def _check_classes(got, want, where):
    st, sym, stat, edges, thr, bits, kpart = got
    assert np.array_equal(_bits(sym), _bits(want["sym"])), where
    assert np.array_equal(stat, want["stat"]), (where, stat, want["stat"])
    assert np.array_equal(_bits(edges), _bits(want["edges"])), (where, edges, want["edges"])
    assert _bits(np.array([thr]))[0] == _bits(np.array([want["thr"]]))[0], (where, thr, want["thr"])
    assert np.array_equal(bits, want["bits"]), where  # every word whole: the bits j <= i and j >= neig are zero
    assert list(kpart) == want["kpart"] and st == want["status"], (where, st)


@pytest.mark.parametrize("ne", R.CLASS_ORDERS)
def test_classes(prof, gpu_ctx, ne):
    """isomorphism_classes_device at every neig (the driver takes it from 256 on): the symmetrised matrix, the 20 stat words, the
    edges, the threshold, every pair-bit word, kpart and the status, all as bits"""
    for name, dims, raw in R.class_cases(ne):
        _check_classes(classes(prof, gpu_ctx, raw, dims, R.ATOL), R.classes_expected(raw, dims, R.ATOL), (ne, name))


def test_classes_of_the_host_chain_cases(prof, gpu_ctx):
    """the matrices of tests/test_iso_classes_cpu.py: the status and kpart are those of the oracle's chain (_expected_classes), the
    inconsistent chain included"""
    verdicts = {}
    for name, dims, raw in R._matrix_cases():
        got = classes(prof, gpu_ctx, raw, dims, R.ATOL)
        _check_classes(got, R.classes_expected(raw, dims, R.ATOL), name)
        K = R._oracle_chain(dims, raw)[5]
        want = R._expected_classes(K, 0)
        assert list(got[6]) == want["kpart"] and got[0] == (R.OK if want["verdict"][0] else R.NUMERICAL_INCONSISTENCY), name
        verdicts[name] = got[0]
    assert verdicts.pop("chain") == R.NUMERICAL_INCONSISTENCY and not any(verdicts.values())


def test_classes_refusals(prof, gpu_ctx):
    norms, bits = _fill(9 + GUARD), np.full(3 + GUARD, SENT, dtype=np.uint64)
    dims, stat, edges, thr, kpart = np.ones(3, dtype=np.int32), np.zeros(20, dtype=np.uint64), np.zeros(17), np.zeros(1), np.zeros(3, dtype=np.int32)
    V = _vp
    good = [3, V(norms), V(dims), 1e-9, V(stat), V(edges), V(thr), V(bits), V(kpart), GUARD]
    dims0 = np.array([1, 0, 1], dtype=np.int32)
    bad = [(0, 0), (0, 4097), (3, 0.0), (3, -1.0), (9, -1), (2, V(dims0))] + [(k, None) for k in (1, 2, 4, 5, 6, 7, 8)]
    for k, v in bad:
        args = list(good)
        args[k] = v
        assert prof.sdpsr_profile_dense_classes(gpu_ctx._h, *args) == R.BAD_ARGUMENT, (k, v)
    assert _untouched(norms) and (bits == np.uint64(SENT)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# Irreducible columns
# ---------------------------------------------------------------------------------------------------------------------------
def irreducible(prof, ctx, route, n, Q, B, desc, ncols, status=None):
    """(columns n x npairs in desc order, the route that ran) after the sentinel checks: named columns written, the others and the
    guard untouched"""
    ldq, vcols, nf = Q.shape[0], Q.shape[1], B.shape[1]
    q, b = np.ascontiguousarray(Q.T).ravel(), np.ascontiguousarray(B.T).ravel()
    d = np.ascontiguousarray(desc, dtype=np.int32)
    out = _fill(n * ncols + GUARD)
    report = (C.c_int32 * 1)(-7)
    st = prof.sdpsr_profile_dense_irreducible(ctx._h, route, n, ldq, vcols, _vp(q), _vp(b), nf, _vp(d), len(d), _vp(out), ncols, GUARD, report)
    if status is not None:
        assert st == status and _untouched(out)
        return None, None
    ctx.check(st)
    X = out[:n * ncols].reshape(ncols, n).T
    named = np.zeros(ncols, dtype=bool)
    named[d[:, 6]] = True
    assert _written(X[:, named]) and _untouched(X[:, ~named]) and _untouched(out[n * ncols:])
    return X[:, d[:, 6]].copy(), report[0]


@pytest.mark.parametrize("n", R.IRREDUCIBLE_ORDERS)
def test_irreducible_routes(prof, gpu_ctx, n):
    """irreducible_pairs_kernel (route 0) and the four launches per pair (route 1) with 1, 2 and 300 pairs in one call, every
    (m_i, m_j) that fits, output columns shuffled.  The integer family to 4 ulp of the exact column; the real family within the
    written bound; the routes within twice the bound of each other."""
    Qi, Bi = R.irreducible_integer_inputs(n)
    Qr, Br = R.irreducible_real_inputs(n)
    worst = [0.0, 0.0]
    for npairs in (1, 2, 300):
        desc, _, _, ncols = R.pair_descriptors(n, npairs)
        ref, ulp4 = R.irreducible_exact_columns(n, Qi, Bi, desc)
        got = []
        for route in (0, 1):
            x, ran = irreducible(prof, gpu_ctx, route, n, Qi, Bi, desc, ncols)
            err = np.abs(x.astype(R.LD) - ref)
            worst[0] = max(worst[0], float((err / np.maximum(ulp4 / 4, 1e-300)).max()))
            assert ran == route and (err <= ulp4).all(), (n, npairs, route, float((err / np.maximum(ulp4, 1e-300)).max()))
            got.append(x)
        assert (np.abs(got[0] - got[1]) <= 2 * ulp4).all()
        ref, bound = R.irreducible_real(n, Qr, Br, desc)
        got = []
        for route in (0, 1):
            x, ran = irreducible(prof, gpu_ctx, route, n, Qr, Br, desc, ncols)
            err = np.abs(x.astype(R.LD) - ref)
            worst[1] = max(worst[1], float((err / bound).max()))
            assert ran == route and (err <= bound).all(), (n, npairs, route, float((err / bound).max()))
            got.append(x)
        assert (np.abs(got[0] - got[1]) <= 2 * bound).all()
    assert irreducible(prof, gpu_ctx, -1, n, Qi, Bi, desc, ncols)[1] == 0  # the driver's rule: the pair kernel
    print("irreducible  n %4d  integer family: largest error %.2f ulp (allowed 4);  real family: largest error / bound %.3f" % (n, *worst))


def test_irreducible_lds_rule_boundary(prof, gpu_ctx):
    """n = 3840 with overlapping windows c_i = c_j = 0: m_i + m_j = 7678 is the last sum the driver's rule gives to the pair kernel
    (61440 bytes of LDS), 7679 the first it takes one by one; both within the real-data bound.  Asking for the pair kernel at 7679
    is refused."""
    n = 3840
    Q, B = R.irreducible_real_inputs(n)
    desc = np.array([[0, R.LDS_RULE_M2 - n, 0, n, 0, 1, 1], [0, R.LDS_RULE_M2 + 1 - n, 0, n, 0, 1, 1]], dtype=np.int32)
    ref, bound = R.irreducible_real(n, Q, B, desc)
    for k, want_route in ((0, 0), (1, 1)):
        x, ran = irreducible(prof, gpu_ctx, -1, n, Q, B, desc[k:k + 1], 3)
        err = np.abs(x[:, 0].astype(R.LD) - ref[:, k])
        print("irreducible  n 3840  m_i + m_j = %d: route %d, largest error / bound %.3f" % (desc[k, 1] + desc[k, 3], ran, float((err / bound[:, k]).max())))
        assert ran == want_route and (err <= bound[:, k]).all(), (k, ran, float((err / bound[:, k]).max()))
    irreducible(prof, gpu_ctx, 0, n, Q, B, desc[1:2], 3, status=R.BAD_ARGUMENT)


def test_irreducible_refusals(prof, gpu_ctx):
    n = 7
    Q, B = R.irreducible_integer_inputs(n)
    good = (1, 2, 3, 2, 0, 1, 0)
    for k, v in ((0, -1), (0, 6), (1, 0), (2, 6), (3, 0), (2, -1), (4, 5), (4, -1), (5, 5), (6, 4), (6, -1)):
        row = list(good)
        row[k] = v
        for route in (-1, 0, 1):
            irreducible(prof, gpu_ctx, route, n, Q, B, np.array([good, row]), 4, status=R.BAD_ARGUMENT)
    wide = np.hstack([Q, Q])  # 14 columns of 7 rows: a window of 8 columns fits in Q but is no eigenspace of order 7
    irreducible(prof, gpu_ctx, 1, n, wide, B, np.array([(0, 8, 3, 2, 0, 1, 0)]), 4, status=R.BAD_ARGUMENT)
    irreducible(prof, gpu_ctx, 0, n, wide, B, np.array([(0, 2, 3, 8, 0, 1, 0)]), 4, status=R.BAD_ARGUMENT)
    irreducible(prof, gpu_ctx, 2, n, Q, B, np.array([good]), 4, status=R.BAD_ARGUMENT)
    irreducible(prof, gpu_ctx, -2, n, Q, B, np.array([good]), 4, status=R.BAD_ARGUMENT)
    irreducible(prof, gpu_ctx, 0, 129, Q, B, np.array([good]), 4, status=R.BAD_ARGUMENT)  # ldq = 128 < n
    irreducible(prof, gpu_ctx, 0, 0, Q, B, np.array([good]), 4, status=R.BAD_ARGUMENT)
    irreducible(prof, gpu_ctx, 0, n, Q, B, np.array([good]), 0, status=R.BAD_ARGUMENT)
    q, b, d, out, rep = Q.T.ravel().copy(), B.T.ravel().copy(), np.array([good], dtype=np.int32), _fill(28 + GUARD), (C.c_int32 * 1)(0)
    V = _vp
    base = [0, n, 128, n, V(q), V(b), 5, V(d), 1, V(out), 4, GUARD, rep]
    for k in (4, 5, 7, 9, 12):
        args = list(base)
        args[k] = None
        assert prof.sdpsr_profile_dense_irreducible(gpu_ctx._h, *args) == R.BAD_ARGUMENT, k
    for k, v in ((3, 0), (3, 4097), (6, 0), (8, 0), (8, 4097), (10, 4097), (11, -1)):
        args = list(base)
        args[k] = v
        assert prof.sdpsr_profile_dense_irreducible(gpu_ctx._h, *args) == R.BAD_ARGUMENT, (k, v)
    assert _untouched(out)


# ---------------------------------------------------------------------------------------------------------------------------
# copy_cols and clamptol
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", R.COPY_COUNTS)
def test_copy_cols(prof, gpu_ctx, count):
    """copy_cols_kernel in launches of 128 columns: different leading dimensions on the two sides, repeated sources, shuffled
    destinations, rows >= n and unnamed columns untouched; n = 70 and 300 (a second block of rows)"""
    for n in (70, 300):
        rng = np.random.default_rng([n, count])
        ld_src, ld_dst, scols, dcols = n + 3, n + 5, 40, count + 2
        src = rng.standard_normal((ld_src, scols))
        sc = rng.integers(0, scols, count).astype(np.int32)
        dc = rng.permutation(dcols)[:count].astype(np.int32)
        s = np.ascontiguousarray(src.T).ravel()
        dst = _fill(ld_dst * dcols + GUARD)
        gpu_ctx.check(prof.sdpsr_profile_copy_cols(gpu_ctx._h, n, count, _vp(sc), _vp(dc), _vp(s), ld_src, scols, _vp(dst), ld_dst, dcols, GUARD))
        want = R.copy_cols(n, src, _matrix(_fill(ld_dst * dcols), ld_dst, dcols), sc, dc)
        assert np.array_equal(_bits(_matrix(dst, ld_dst, dcols)), _bits(want)) and _untouched(dst[ld_dst * dcols:]), (n, count)


def test_clamptol(prof, gpu_ctx):
    """clamptol_kernel across the grid cap: -|x| < atol becomes +0.0 (so does -0.0), |x| == atol stays with its sign, a NaN stays"""
    atol = 1e-7
    rng = np.random.default_rng(3)
    for length in (1, 255, R.GRID_CAP + 1000):
        a = _fill(length + GUARD)
        a[:length] = rng.standard_normal(length) * 3e-7
        special = np.array([-0.5e-7, 0.5e-7, -atol, atol, np.nan, -0.0, 0.0, -np.nextafter(atol, 0.0), np.nextafter(atol, 1.0), -np.inf])
        k = min(length, special.size)
        a[length - k:length] = special[:k]  # (behind the grid cap in the long array)
        a[0] = special[0]
        want = R.clamptol(a[:length], atol)
        assert length < special.size or (_bits(want[length - k:length]) == _bits(np.array([0.0, 0.0, -atol, atol, np.nan, 0.0, 0.0, 0.0, special[8], -np.inf]))).all()
        gpu_ctx.check(prof.sdpsr_profile_clamptol(gpu_ctx._h, length, _vp(a), atol, GUARD))
        assert np.array_equal(_bits(a[:length]), _bits(want)) and _untouched(a[length:]), length


def test_copy_cols_and_clamptol_refusals(prof, gpu_ctx):
    src, dst = np.zeros(8 * 4), _fill(8 * 4 + GUARD)
    sc, dc = np.array([0, 3], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    V = _vp
    base = [5, 2, V(sc), V(dc), V(src), 8, 4, V(dst), 8, 4, GUARD]
    c04, cm1, c14 = np.array([0, 4], dtype=np.int32), np.array([-1, 0], dtype=np.int32), np.array([1, 4], dtype=np.int32)
    bad = [(0, 0), (0, 4097), (1, 0), (1, 4097), (5, 4), (8, 4), (6, 0), (9, 0), (10, -1), (2, None), (3, None), (4, None), (7, None),
           (2, V(c04)), (2, V(cm1)), (3, V(c14))]
    for k, v in bad:
        args = list(base)
        args[k] = v
        assert prof.sdpsr_profile_copy_cols(gpu_ctx._h, *args) == R.BAD_ARGUMENT, (k, v)
    assert _untouched(dst)
    for length, ap, atol, guard in ((0, V(dst), 1e-9, GUARD), (4096 * 4096 + 1, V(dst), 1e-9, GUARD), (5, None, 1e-9, GUARD), (5, V(dst), -1.0, GUARD),
                                    (5, V(dst), float("nan"), GUARD), (5, V(dst), 1e-9, -1)):
        assert prof.sdpsr_profile_clamptol(gpu_ctx._h, length, ap, atol, guard) == R.BAD_ARGUMENT, (length, atol, guard)
    assert _untouched(dst)
