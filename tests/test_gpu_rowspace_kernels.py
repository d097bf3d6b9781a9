"""The row-space kernels of sdpsr_compress_constraints (csrc/kernels_rowspace.hip), one by one, on made-up inputs through the test
entry points of libsdpsr_prof.so, against the references of tests/rowspace_kernels_ref.py -- and the driver where the invariants of
tests/test_gpu_compress_constraints.py cannot see: the driver forms G afresh in every pass, so a wrong product or rotation is
absorbed by a later pass; here each kernel answers for its own result.

No tolerance is measured.  Integer-valued inputs (times a power of two) make every partial sum exact in any order: the result must
equal the int64 reference bit for bit.  Real inputs: an fp64 dot product of n terms, in any order, with or without FMA, lies within
gamma_n sum |a_i b_i| of the exact value, gamma_n = n u / (1 - n u), u = 2^-53; the Gram test adds the long-double reference's own
n 2^-64 sum |a_i b_i|.  The scale copy, the lead signs and the write-out are IEEE operations on single numbers: bit for bit.

Every in/out array ends in GUARD doubles of one NaN pattern, which must come back unchanged; preconditions of the inputs (exactness,
what the planted rows hold, rank unambiguity) are checked without a GPU in tests/test_rowspace_kernels_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import compress_ref as CR
import rowspace_kernels_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF85A5ADEADBEEF
GUARD = 64
BAD_ARGUMENT = 5


def _vp(a):
    """(the pointer alone: the caller keeps the array alive in a variable of its own until the call has returned)"""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _fill(count):
    return np.full(int(count), SENT, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((_bits(a) == np.uint64(SENT)).all())


def _cm(M, guard=False):
    """M (m x ncols) as the column-major array of the ABI, with the guard behind it"""
    flat = np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).ravel()
    return np.concatenate([flat, _fill(GUARD)]) if guard else flat


def _mat(flat, m, ncols):
    return flat[:m * ncols].reshape(ncols, m).T


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


def _report(count):
    return (C.c_int32 * count)(*([-1] * count))


# ---------------------------------------------------------------------------------------------------------------------------
# Gram product
# ---------------------------------------------------------------------------------------------------------------------------
def _gram(prof, ctx, W):
    m, ncols = W.shape
    Wh, G, rep = _cm(W), _fill(m * m + GUARD), _report(3)
    ctx.check(prof.sdpsr_profile_rowspace_gram(ctx._h, m, ncols, _vp(Wh), _vp(G), GUARD, rep))
    assert _untouched(G[m * m:])
    return _mat(G, m, m), tuple(rep)


@pytest.mark.parametrize("m,ncols", R.GRAM_SHAPES)
def test_gram_exact(prof, gpu_ctx, m, ncols):
    """Integers in [-8, 8] times 2^-4, and the same with all-zero rows and columns: G equals the exact product bit for bit in both
    triangles; (npairs, Z, cps) are the table's."""
    want = R.GRAM_TABLE[(m, ncols)]
    for zero_lines in (False, True):
        Wi, W = R.gram_int_input(m, ncols, zero_lines)
        G, rep = _gram(prof, gpu_ctx, W)
        assert rep == R.gram_shape(m, ncols) and rep[0] == want[0] and (want[1] is None or rep[1:] == want[1:])
        ref = R.gram_int_ref(Wi)
        bad = np.argwhere(_bits(G) != _bits(ref))
        assert bad.size == 0, (zero_lines, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("m,ncols", R.GRAM_SHAPES)
def test_gram_real(prof, gpu_ctx, m, ncols):
    """A standard-normal W and one whose row norms fall from 1 to 1e-12: |G - ref| <= gamma_ncols (|W||W|')[p, q] plus the
    reference's own ncols 2^-64 (|W||W|')[p, q]; G[p, q] and G[q, p] are one value; two calls give equal bytes."""
    for name, W in R.gram_real_inputs(m, ncols).items():
        G, _ = _gram(prof, gpu_ctx, W)
        G2, _ = _gram(prof, gpu_ctx, W)
        ref, ab = R.gram_real_ref(W)
        err, bound = np.abs(G.astype(np.longdouble) - ref), R.gram_bound(ab, ncols)
        print("gram %dx%d %s: largest error / bound %.3g" % (m, ncols, name, float((err / bound).max())))
        assert _same(G, G.T) and _same(G, G2), name
        assert np.all(err <= bound), (name, np.argwhere(err > bound)[:5].tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# rotation
# ---------------------------------------------------------------------------------------------------------------------------
def _rotate(prof, ctx, J, W):
    m, ncols = W.shape
    Jh, Wh, rep = _cm(J), _cm(W, guard=True), _report(2)
    ctx.check(prof.sdpsr_profile_rowspace_rotate(ctx._h, m, ncols, _vp(Jh), _vp(Wh), GUARD, rep))
    assert _untouched(Wh[m * ncols:])
    return _mat(Wh, m, ncols), tuple(rep)


@pytest.mark.parametrize("m", R.ROTATE_M)
def test_rotate_exact(prof, gpu_ctx, m):
    """J = a signed permutation plus integers in [-3, 3], W integers times 2^-4, in place: bit for bit, for a ragged last chunk of
    every size mod 4 and a matrix narrower than four columns; (cc, j_lds) are the rule's."""
    for ncols in R.rotate_ncols(m):
        Ji, Wi, W = R.rotate_int_input(m, ncols)
        got, rep = _rotate(prof, gpu_ctx, Ji.astype(np.float64), W)
        assert rep == R.chunk(m), ncols
        ref = R.rotate_int_ref(Ji, Wi)
        bad = np.argwhere(_bits(got) != _bits(ref))
        assert bad.size == 0, (ncols, len(bad), bad[:5].tolist())
    assert R.chunk(m)[1] == (1 if m <= 62 else 0) and (m != 200 or R.chunk(m)[0] == 40) and (m != 1024 or R.chunk(m)[0] == 7)


@pytest.mark.parametrize("m", R.ROTATE_M)
def test_rotate_real(prof, gpu_ctx, m):
    """J = a product of true plane rotations, W standard normal: |got - ref| <= gamma_m sum_k |J_ik| |W_kc| against the
    long-double product; two calls give equal bytes."""
    J = R.plane_rotations(m, 500 + m)
    worst = 0.0
    for ncols in R.rotate_ncols(m):
        W = np.random.default_rng(17000 * m + ncols).standard_normal((m, ncols))
        got, _ = _rotate(prof, gpu_ctx, J, W)
        again, _ = _rotate(prof, gpu_ctx, J, W)
        ref, ab = R.rotate_real_ref(J, W)
        err, bound = np.abs(got.astype(np.longdouble) - ref), np.longdouble(R.gamma(m)) * ab
        worst = max(worst, float((err / bound).max()))
        assert _same(got, again), ncols
        assert np.all(err <= bound), (ncols, np.argwhere(err > bound)[:5].tolist())
    print("rotate m=%d: largest error / bound %.3g" % (m, worst))


# ---------------------------------------------------------------------------------------------------------------------------
# scale copy
# ---------------------------------------------------------------------------------------------------------------------------
def _scale(prof, ctx, A, b):
    """(status, W_inout whole, info) of one call on M = [A | b]"""
    m, d = A.shape
    ncols = d + (b is not None)
    Ah = _cm(A) if d else None
    bh = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    Wh, info = _fill(m * ncols + GUARD), np.full(2, np.nan)
    st = prof.sdpsr_profile_rowspace_scale(ctx._h, m, d, _vp(Ah), _vp(bh), _vp(Wh), _vp(info), GUARD)
    return st, Wh, info


@pytest.fixture(scope="module")
def scale_cases():
    return R.scale_cases()


@pytest.mark.parametrize("name", ["order_one", "up_900", "down_900", "denormal", "dbl_max", "zeros", "many_blocks"])
def test_scale_copy(prof, gpu_ctx, scale_cases, name):
    """W = M * scale bit for bit (NumPy's IEEE product, denormals included), info = (max |M|, 0); b = NULL on the same matrix gives
    the same bytes."""
    M = scale_cases[name]
    m, ncols = M.shape
    ref, mx, _ = R.scale_ref(M)
    want = _cm(ref)
    st, Wh, info = _scale(prof, gpu_ctx, M[:, :-1], M[:, -1])
    st2, Wh2, info2 = _scale(prof, gpu_ctx, M, None)
    assert st == 0 and st2 == 0
    assert _same(Wh[:m * ncols], want) and _untouched(Wh[m * ncols:])
    assert _same(info, np.array([mx, 0.0])) and _same(Wh2, Wh) and _same(info2, info)
    if name == "zeros":
        assert np.signbit(_mat(Wh, m, ncols)[1, 2]) and not _bits(np.abs(Wh[:m * ncols])).any()
    if name in ("up_900", "down_900"):
        assert _same(Wh, _scale(prof, gpu_ctx, scale_cases["order_one"][:, :-1], scale_cases["order_one"][:, -1])[1])


def test_scale_copy_of_one_entry(prof, gpu_ctx):
    """total = 1, as A alone and as b alone (d = 0, A = NULL)."""
    st, Wh, info = _scale(prof, gpu_ctx, np.array([[-3.5]]), None)
    assert st == 0 and _same(Wh[:1], np.array([-0.875])) and _untouched(Wh[1:]) and _same(info, np.array([3.5, 0.0]))
    st, Wh, info = _scale(prof, gpu_ctx, np.zeros((1, 0)), np.array([2.0 ** -1074]))
    assert st == 0 and _same(Wh[:1], np.array([2.0 ** -74])) and _untouched(Wh[1:]) and _same(info, np.array([2.0 ** -1074, 0.0]))


def test_scale_copy_refuses_non_finite_input(prof, gpu_ctx, scale_cases):
    """A NaN as the last entry of A, an Inf in b only, a NaN that another block than block 0 reads, one that block 0 reads in its
    second stride: info[1] = 1 and NO element of W is written; info[0] is the largest finite magnitude."""
    base = scale_cases["order_one"]
    wide = np.random.default_rng(32).standard_normal((40, 200))  # 8000 entries: four blocks of the absmax grid
    assert R.absmax_blocks(wide.size) == 4
    many = scale_cases["many_blocks"]
    plants = []
    M = base.copy()
    M[-1, -2] = np.nan
    plants.append(M)
    M = base.copy()
    M[3, -1] = -np.inf
    plants.append(M)
    M = wide.copy()
    e = 256 * 2 + 17
    M[e % 40, e // 40] = np.nan
    plants.append(M)
    M = many.copy()
    e = 1024 * 256 * 5 + 3
    assert e < many.size - many.shape[0]
    M[e % 5, e // 5] = np.inf
    plants.append(M)
    for M in plants:
        st, Wh, info = _scale(prof, gpu_ctx, M[:, :-1], M[:, -1])
        assert st == 0 and _untouched(Wh), M.shape
        assert _same(info, np.array([R.scale_ref(M)[1], 1.0])), M.shape
    # and the flag is zeroed for the next call
    st, Wh, info = _scale(prof, gpu_ctx, base[:, :-1], base[:, -1])
    assert st == 0 and info[1] == 0.0 and _same(Wh[:base.size], _cm(R.scale_ref(base)[0]))


# ---------------------------------------------------------------------------------------------------------------------------
# lead signs and write-out
# ---------------------------------------------------------------------------------------------------------------------------
def _finish(prof, ctx, W, perm, sigma, r, droptol, in_place):
    """(out m x ncols, W as it came back, sig_inout whole, nnz)"""
    m, ncols = W.shape
    Wh, sig, nnz = _cm(W, guard=True), _fill(m + GUARD), C.c_int64(-1)
    out = None if in_place else _fill(m * ncols + GUARD)
    ph, sh = np.ascontiguousarray(perm, dtype=np.int32), np.ascontiguousarray(sigma, dtype=np.float64)
    ctx.check(prof.sdpsr_profile_rowspace_finish(ctx._h, m, ncols, r, _vp(ph), _vp(sh), droptol, in_place, _vp(Wh), _vp(out), _vp(sig),
                                                  C.byref(nnz), GUARD))
    res = Wh if in_place else out
    assert _untouched(res[m * ncols:]) and _untouched(Wh[m * ncols:])
    return _mat(res, m, ncols), _mat(Wh, m, ncols), sig, nnz.value


@pytest.mark.parametrize("m", R.FINISH_M)
def test_finish(prof, gpu_ctx, m):
    """sig[k] = +-sigma[k] by the first entry of largest magnitude of row perm[k] -- with ties of opposite signs planted across two
    threads' strides, a lead entry in the last column, an all-zero kept row --; out = the permuted rows over sig, bit for bit, with
    entries planted at droptol and one ulp to either side of it; rows >= r are +0.0; nnz is the count; sig beyond r is not written;
    in place and apart give equal bytes."""
    onlys = range(len(R.FINISH_PATTERNS)) if m == 1 else (None,)
    t0, up, down = R.drop_targets()
    for only in onlys:
        W, perm, sigma, planted = R.finish_input(m, only)
        ncols = W.shape[1]
        for r in sorted({0, 1, m - 1, m}):
            for droptol in ((R.DROPTOL, 0.0) if r == m else (R.DROPTOL,)):
                sig_ref = R.lead_ref(W, perm, sigma, r)
                ref, nnz_ref = R.write_ref(W, perm, sig_ref, r, droptol)
                results = []
                for in_place in (0, 1):
                    out, Wback, sig, nnz = _finish(prof, gpu_ctx, W, perm, sigma, r, droptol, in_place)
                    where = (only, r, droptol, in_place)
                    assert _same(sig[:r], sig_ref) and _untouched(sig[r:]), where
                    bad = np.argwhere(_bits(out) != _bits(ref))
                    assert bad.size == 0, (where, len(bad), bad[:5].tolist())
                    assert not _bits(out[r:]).any() and nnz == nnz_ref == np.count_nonzero(out), where
                    assert in_place or _same(Wback, W), where
                    results.append(out)
                assert _same(results[0], results[1])
                out = results[0]
                for name, k in planted.items():
                    if k >= r:
                        continue
                    if name.startswith("tie"):
                        a, b = dict(R.FINISH_PATTERNS)[name]
                        first = min(a[0] % ncols, b[0] % ncols)
                        assert out[k, first] == R.TIE / sigma[k] and sig_ref[k] == np.copysign(sigma[k], W[perm[k], first])
                    elif name == "last_column":
                        assert out[k, -1] == 0.9 / sigma[k] and out[k, -1] == np.abs(out[k]).max()
                    elif name == "droptol" and droptol > 0:
                        c0, c1, c2 = (c % ncols for c in R.DROP_COLS)
                        assert _bits(out[k, [c0, c2]]).tolist() == [0, 0] and out[k, c1] == -up  # at and below: +0.0; above: kept
                    elif name == "droptol":
                        c0, c1, c2 = (c % ncols for c in R.DROP_COLS)
                        assert out[k, [c0, c1, c2]].tolist() == [t0, -up, down]


# ---------------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_upload(prof, gpu_ctx):
    h = gpu_ctx._h
    a, w, g, s = np.ones(64), _fill(64 + GUARD), _fill(64 + GUARD), _fill(8 + GUARD)
    info, rep, nnz = np.full(2, np.nan), _report(3), C.c_int64(-1)
    perm, bad_perm = np.arange(8, dtype=np.int32), np.array([0, 1, 2, 8, 4, 5, 6, 7], dtype=np.int32)
    big = (1 << 20) + 1
    calls = []
    for m, d, A, W, I, guard in ((0, 8, a, w, info, GUARD), (1025, 8, a, w, info, GUARD), (8, 0, a, w, info, GUARD), (8, -1, a, w, info, GUARD),
                                 (8, 8, None, w, info, GUARD), (8, 8, a, None, info, GUARD), (8, 8, a, w, None, GUARD), (8, 8, a, w, info, -1),
                                 (8, 8, a, w, info, big)):
        calls.append(prof.sdpsr_profile_rowspace_scale(h, m, d, _vp(A), None, _vp(W), _vp(I), guard))
    for m, ncols, W, G, guard, rp in ((0, 8, a, g, GUARD, rep), (1025, 8, a, g, GUARD, rep), (8, 0, a, g, GUARD, rep), (8, 8, None, g, GUARD, rep),
                                      (8, 8, a, None, GUARD, rep), (8, 8, a, g, -1, rep), (8, 8, a, g, big, rep), (8, 8, a, g, GUARD, None),
                                      (1024, (1 << 16) + 1, a, g, GUARD, rep)):
        calls.append(prof.sdpsr_profile_rowspace_gram(h, m, ncols, _vp(W), _vp(G), guard, rp))
        calls.append(prof.sdpsr_profile_rowspace_rotate(h, m, ncols, _vp(W), _vp(G), guard, rp))
    for m, ncols, r, P, S, tol, W, O, Sg, guard in ((0, 8, 0, perm, a, 0.0, w, g, s, GUARD), (1025, 8, 0, perm, a, 0.0, w, g, s, GUARD),
                                                     (8, 0, 0, perm, a, 0.0, w, g, s, GUARD), (8, 8, -1, perm, a, 0.0, w, g, s, GUARD),
                                                     (8, 8, 9, perm, a, 0.0, w, g, s, GUARD), (8, 8, 8, bad_perm, a, 0.0, w, g, s, GUARD),
                                                     (8, 8, 8, None, a, 0.0, w, g, s, GUARD), (8, 8, 8, perm, None, 0.0, w, g, s, GUARD),
                                                     (8, 8, 8, perm, a, -1.0, w, g, s, GUARD), (8, 8, 8, perm, a, np.nan, w, g, s, GUARD),
                                                     (8, 8, 8, perm, a, 0.0, None, g, s, GUARD), (8, 8, 8, perm, a, 0.0, w, g, None, GUARD),
                                                     (8, 8, 8, perm, a, 0.0, w, g, s, -1), (8, 8, 8, perm, a, 0.0, w, g, s, big)):
        calls.append(prof.sdpsr_profile_rowspace_finish(h, m, ncols, r, _vp(P), _vp(S), tol, 0, _vp(W), _vp(O), _vp(Sg), C.byref(nnz), guard))
    calls.append(prof.sdpsr_profile_rowspace_finish(h, 8, 8, 8, _vp(perm), _vp(a), 0.0, 0, _vp(w), None, _vp(s), C.byref(nnz), GUARD))  # apart, no out
    assert calls == [BAD_ARGUMENT] * len(calls)
    assert _untouched(w) and _untouched(g) and _untouched(s) and np.isnan(info).all() and tuple(rep) == (-1, -1, -1) and nnz.value == -1
    # and a good call follows
    G, got = _gram(prof, gpu_ctx, np.eye(3))
    assert np.array_equal(G, np.eye(3)) and got == (1, 1, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the driver, where the invariants are blind
# ---------------------------------------------------------------------------------------------------------------------------
def _call(ctx, M):
    """sdpsr_compress_constraints on M with b = NULL, rtol = droptol = 0: (status, out, rank, sv, nnz, passes)"""
    M = np.asfortranarray(M, dtype=np.float64)
    m, ncols = M.shape
    out = np.full((m, ncols), -12345.678, order="F")
    rank, nnz, passes = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    sv = np.full(m, np.nan)
    st = ctx._lib.sdpsr_compress_constraints(ctx._h, m, ncols, _vp(M), None, 0.0, 0.0, _vp(out), C.byref(rank), _vp(sv), C.byref(nnz),
                                             C.byref(passes), 0)
    return st, out, rank.value, sv, nnz.value, passes.value


@pytest.fixture(scope="module")
def driver_inputs(problems, golden):
    cases = CR.inputs(problems, golden)
    mats = {name: CR.stack(*cases[name][:2]) for name in ("graded_6x37", "duplicates_6x70", "integer_9x5")}
    mats["rows_70x300"] = R.rows_70x300()
    return mats


@pytest.mark.parametrize("name", ["graded_6x37", "duplicates_6x70", "rows_70x300"])
def test_driver_is_invariant_under_powers_of_two(gpu_ctx, driver_inputs, name):
    """M 2^900 and M 2^-900 scale to the W of M itself, and everything after the scale copy sees only W: the bytes of out, and rank,
    nnz and passes, are those of the plain run; sv is the plain sv times 2^+-900 exactly."""
    M = driver_inputs[name]
    st0, out0, rank0, sv0, nnz0, passes0 = _call(gpu_ctx, M)
    assert st0 == 0
    for k in (900, -900):
        st, out, rank, sv, nnz, passes = _call(gpu_ctx, np.ldexp(M, k))
        assert st == 0 and (rank, nnz, passes) == (rank0, nnz0, passes0), k
        assert _same(out, out0), k
        assert _same(sv, np.ldexp(sv0, k)), k


def test_driver_on_denormal_input(gpu_ctx, driver_inputs):
    """The integer 9 x 5 matrix times 2^-1070 (every entry denormal; the scale stops at 2^1000): status 0, the integer matrix's
    rank, orth and resid within the bounds of the order-one inputs, |sv 2^1070 - s| <= ncols eps sigma_1 + 2^-4 (one denormal
    quantum, 2^-1074 2^1070: sv itself is a denormal number)."""
    Mi = driver_inputs["integer_9x5"]
    m, ncols = Mi.shape
    s, r, rows_l = CR.reference(Mi)
    st, out, rank, sv, nnz, passes = _call(gpu_ctx, np.ldexp(Mi, -1070))
    assert st == 0 and rank == r == 5
    rows = out[:rank]
    full = np.zeros(m)
    full[:s.size] = s
    figures = (CR.orth(rows), CR.resid(Mi, rows), float(np.abs(np.ldexp(sv, 1070) - full).max()))
    print("denormal 9x5: passes", passes, "orth %.3g resid %.3g |sv 2^1070 - s| %.3g" % figures)
    bound = ncols * CR.EPS
    assert figures[0] <= max(8 * CR.orth(rows_l), bound) and figures[1] <= max(8 * CR.resid(Mi, rows_l), bound)
    assert figures[2] <= bound * s[0] + 2.0 ** -4
    assert not _bits(out[rank:]).any() and nnz == np.count_nonzero(rows)


@pytest.mark.parametrize("m,ncols,r,seed", R.MORE_ROWS)
def test_driver_on_more_rows(gpu_ctx, m, ncols, r, seed):
    """129 x 70 (rank 70: six block pairs, more rows than columns) and 200 x 517 (rank 90: ten block pairs, chunks of 40 columns),
    products of small-integer matrices: the figures and bounds of test_rows_against_lapack_on_invariants."""
    M = R.more_rows(m, ncols, r, seed)
    s, r_ref, rows_l = CR.reference(M)
    assert r_ref == r and CR.rank_is_unambiguous(s)
    orth_l, resid_l = CR.orth(rows_l), CR.resid(M, rows_l)
    st, out, rank, sv, nnz, passes = _call(gpu_ctx, M)
    assert st == 0
    rows = out[:rank]
    figures = (CR.orth(rows), CR.resid(M, rows) if rank else np.inf, CR.sverr(sv, s, m))
    print("%dx%d rank" % (m, ncols), rank, "passes", passes, "orth %.3g resid %.3g sverr %.3g" % figures, "LAPACK orth %.3g resid %.3g" % (orth_l, resid_l))
    assert rank == r
    bound = ncols * CR.EPS
    assert figures[0] <= max(8 * orth_l, bound)
    assert figures[1] <= max(8 * resid_l, bound)
    assert figures[2] <= bound
    assert not _bits(out[rank:]).any()
    assert np.all(rows[np.arange(rank), np.abs(rows).argmax(axis=1)] > 0)
    assert np.all(np.diff(sv) <= 0) and np.all(sv >= 0)
    assert nnz == np.count_nonzero(rows) and 1 <= passes <= CR.MAX_PASSES

