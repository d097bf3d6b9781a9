"""The kernels of the module-compression driver (csrc/kernels_module.hip, the class sums of csrc/kernels_blockdiag.hip), one by one,
on made-up inputs through the test entry points of libsdpsr_prof.so, against the references of tests/module_kernels_ref.py.

No tolerance here is measured.  An fp64 dot product of k terms, in any order, with or without FMA, is within gamma_k sum |a_i b_i|
of the exact value (gamma_k ~ k 2^-53); the tests assert entrywise |got - ref| <= 2 k 2^-53 (|A|'|B|)_ij against a long-double
reference, and array_equal against an exact int64 reference where the inputs are small integers (every partial sum is then an
exactly representable integer: any dropped, doubled or misplaced term shows).

Every in/out array is pre-filled with one NaN bit pattern (SENT) and compared as BITS: outside the documented output region nothing
may change, inside it everything must be written.  The parts of the inputs a kernel must not read hold NaN."""
import ctypes as C

import numpy as np
import pytest

import module_kernels_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF85A5ADEADBEEF    # the fill of every in/out array
POISON = 0x7FF80BAD0BAD0BAD  # the fill of input regions nobody may read
U = 2.0 ** -53
BAD_ARGUMENT = 5


def _vp(a):
    """(the pointer alone: the caller keeps the array alive in a variable of its own until the call has returned)"""
    return C.c_void_p(a.ctypes.data)


def _fill(count, pattern=SENT):
    return np.full(int(count), pattern, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((_bits(a) == np.uint64(SENT)).all())


def _zero_bits(a):
    return not _bits(a).any()  # +0.0, bit for bit


def _round_up(x, m):
    return -(-x // m) * m


def _colmajor(M, ld, cols, pattern=POISON):
    """M (rows x c) in the leading part of a column-major ld x cols array whose other entries hold `pattern`."""
    buf = _fill(ld * cols, pattern)
    buf.reshape(cols, ld)[:M.shape[1], :M.shape[0]] = M.T
    return buf


def _within(got, ref, ab, k):
    return bool((np.abs(got.astype(np.longdouble) - ref) <= np.longdouble(2 * k * U) * ab.astype(np.longdouble)).all())


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


def _report(count=4):
    return (C.c_int32 * count)(*([-1] * count))


# ---------------------------------------------------------------------------------------------------------------------------
# Gram products
# ---------------------------------------------------------------------------------------------------------------------------
GRAM_K = (1, 31, 32, 33, 1000, 1025, 4224)  # 32 rows per workgroup: 1025 -> 33 partial sums (odd, both accumulators of the reduction)
GRAM_SKINNY = ((1, 1), (2, 1), (17, 16), (64, 64), (65, 63), (100, 37), (128, 1), (1, 128), (112, 128), (128, 112))
GRAM_SPLITK = ((128, 113), (128, 128), (129, 5), (200, 130))
GUARD = 300


def _gram(prof, ctx, mode, k, ma, nb, lda, ldb, mp, np_, A, B, pinned=True, a_pad=POISON):
    """One call: A (k x ma), B (k x nb) in lda x mp, ldb x np_ arrays (rows >= k: NaN; columns >= ma / nb: a_pad).
    Returns (C as np_ x mp rows = columns of the result, guard tail, pinned copy or None, route, host_filled)."""
    Ah, Bh = _colmajor(A, lda, mp), _colmajor(B, ldb, np_)
    if a_pad != POISON:
        Ah.reshape(mp, lda)[ma:, :] = a_pad
        Bh.reshape(np_, ldb)[nb:, :] = a_pad
    Cc = _fill(mp * np_ + GUARD)
    P = _fill(mp * np_ + GUARD) if pinned else None
    rep = _report(2)
    ctx.check(prof.sdpsr_profile_gram(ctx._h, mode, k, ma, nb, lda, ldb, mp, np_, _vp(Ah), _vp(Bh), _vp(Cc), _vp(P) if pinned else None, GUARD, rep))
    return Cc[:mp * np_].reshape(np_, mp), Cc[mp * np_:], P, rep[0], rep[1]


def _check_gram_result(Cm, tail, ma, nb, check):
    """the ma x nb result, +0.0 on the rest of the padded result, the guard tail as it was"""
    assert check(Cm[:nb, :ma].T)
    assert _zero_bits(Cm[nb:, :]) and _zero_bits(Cm[:, ma:])
    assert _untouched(tail)


@pytest.mark.parametrize("ma,nb", GRAM_SKINNY)
def test_gram_skinny_route(prof, gpu_ctx, ma, nb):
    """gram_partial_kernel / gram_reduce_kernel through gram_tn (padded result, mp = np = 128) and through launch_gram_small with the
    exact-shape result (ldc = mp = ma, np = nb), with lda = ldb = k and with larger leading dimensions; integers exactly, reals
    within the bound; the pinned copy equals the device result bit for bit.  The operands' rows >= k and columns >= ma / nb are NaN."""
    rng = np.random.default_rng(1000 * ma + nb)
    for k in GRAM_K:
        Ai, Bi = rng.integers(-8, 9, (k, ma)).astype(np.float64), rng.integers(-8, 9, (k, nb)).astype(np.float64)
        ref_i = R.tn_product_int(Ai, Bi)
        Ar, Br = rng.standard_normal((k, ma)), rng.standard_normal((k, nb))
        ref_r, ab = R.tn_product(Ar, Br)
        for lda, ldb in ((k, k), (k + 3, k + 8)):
            for mode, mp, np_ in ((0, _round_up(ma, 128), 128), (1, ma, nb)):
                for A, B, check in ((Ai, Bi, lambda X: np.array_equal(X, ref_i)), (Ar, Br, lambda X: _within(X, ref_r, ab, k))):
                    Cm, tail, P, route, host_filled = _gram(prof, gpu_ctx, mode, k, ma, nb, lda, ldb, mp, np_, A, B)
                    where = (k, lda, ldb, mode)
                    assert route == 1 and host_filled == 1, where
                    _check_gram_result(Cm, tail, ma, nb, check)
                    assert np.array_equal(_bits(P[:mp * np_]), _bits(Cm).ravel()), where  # the second store, into pinned host memory
                    assert _untouched(P[mp * np_:]), where


def test_gram_skinny_padding_is_zero_whatever_the_operands_padding_holds(prof, gpu_ctx):
    """The skinny route WRITES the zeros of the padded result: NaN in the operands' columns ma..mp / nb..np does not reach it
    (on the split-K route those columns are multiplied: the caller keeps them zero, see gram_tn)."""
    rng = np.random.default_rng(3)
    k, ma, nb = 256, 37, 21
    A, B = rng.integers(-8, 9, (k, ma)).astype(np.float64), rng.integers(-8, 9, (k, nb)).astype(np.float64)
    Cm, tail, P, route, host_filled = _gram(prof, gpu_ctx, 0, k, ma, nb, k, k, 128, 128, A, B, pinned=False)
    assert route == 1 and host_filled == 0  # (no pinned copy asked for)
    ref = R.tn_product_int(A, B)
    _check_gram_result(Cm, tail, ma, nb, lambda X: np.array_equal(X, ref))


@pytest.mark.parametrize("ma,nb", GRAM_SPLITK)
def test_gram_split_k_route(prof, gpu_ctx, ma, nb):
    """(128, 113) is the first shape whose LDS stage does not fit 64 KiB: gram_tn hands over to the split-K MFMA product over all
    mp x np columns, K in tiles (the driver passes k = ld, a multiple of 128), the operands zero in their padding columns."""
    rng = np.random.default_rng(2000 * ma + nb)
    mp, np_ = _round_up(ma, 128), _round_up(nb, 128)
    for k in (128, 256, 1024, 4224):
        Ai, Bi = rng.integers(-8, 9, (k, ma)).astype(np.float64), rng.integers(-8, 9, (k, nb)).astype(np.float64)
        ref_i = R.tn_product_int(Ai, Bi)
        Ar, Br = rng.standard_normal((k, ma)), rng.standard_normal((k, nb))
        ref_r, ab = R.tn_product(Ar, Br)
        for A, B, check in ((Ai, Bi, lambda X: np.array_equal(X, ref_i)), (Ar, Br, lambda X: _within(X, ref_r, ab, k))):
            Cm, tail, P, route, host_filled = _gram(prof, gpu_ctx, 0, k, ma, nb, k, k, mp, np_, A, B, a_pad=0)
            assert route == 0 and host_filled == 0, k
            _check_gram_result(Cm, tail, ma, nb, check)
            assert _untouched(P), k  # the split-K route leaves the pinned copy alone (host_filled says so)


def test_gram_entry_refuses_what_could_index_outside(prof, gpu_ctx):
    h = gpu_ctx._h
    a = np.zeros(256 * 256)
    rep = _report(2)
    ok = dict(mode=0, k=128, ma=4, nb=4, lda=128, ldb=128, mp=128, np=128)
    for change in (dict(k=0), dict(k=8193), dict(ma=0), dict(nb=0), dict(lda=127), dict(ldb=127), dict(mp=3), dict(np=3), dict(mp=384), dict(mode=2),
                   dict(mode=1, ma=128, nb=128, mp=128, np=128),  # no exact-shape kernel for this shape
                   dict(ma=128, nb=128, k=100, lda=100, ldb=100)):  # split-K route with K not in tiles
        q = dict(ok, **change)
        st = prof.sdpsr_profile_gram(h, q["mode"], q["k"], q["ma"], q["nb"], q["lda"], q["ldb"], q["mp"], q["np"], _vp(a), _vp(a), _vp(a), None, 0, rep)
        assert st == BAD_ARGUMENT, change
    assert prof.sdpsr_profile_gram(h, 0, 128, 4, 4, 128, 128, 128, 128, None, _vp(a), _vp(a), None, 0, rep) == BAD_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------
# tall times small
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_tall_times_small(prof, gpu_ctx, n):
    """out = beta out + alpha In S: 64 rows x 8 columns per wave, eight coefficient rows per round -- kk in {7, 8, 9}, ncols in {7, 8, 9}
    and n in {63, 64, 65} are the ragged tails on every side (n = 65, kk = 9, ncols = 9 all at once).  Integer inputs make every
    (alpha, beta) exact.  lds > kk, ldi > n; ldo = ldi and ldo = n (the layout of the final lift Q_hat = W Q_small).  With beta == 0
    the output region holds NaN before the call and must come back finite."""
    rng = np.random.default_rng(n)
    ldi = n + 5
    for kk in (1, 7, 8, 9, 16, 75):
        lds = kk + 3
        In = rng.integers(-8, 9, (n, kk)).astype(np.float64)
        Inh = _colmajor(In, ldi, kk)
        for ncols in (1, 7, 8, 9, 20):
            S = rng.integers(-8, 9, (kk, ncols)).astype(np.float64)
            Sh = _colmajor(S, lds, ncols)
            ref = R.nn_product_int(In, S).astype(np.float64)
            old = rng.integers(-8, 9, (n, ncols)).astype(np.float64)
            for ldo in (ldi, n):
                guard = 2 * ldo + 7  # two more columns' worth behind the ncols the kernel owns
                for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, 2.0)):
                    out = _fill(ldo * ncols + guard)
                    if beta != 0.0:
                        out[:ldo * ncols].reshape(ncols, ldo)[:, :n] = old.T
                    gpu_ctx.check(prof.sdpsr_profile_tall_times_small(gpu_ctx._h, n, ldi, kk, lds, ncols, alpha, beta, ldo, _vp(Inh), _vp(Sh),
                                                                      _vp(out), guard))
                    where = (kk, ncols, ldo, alpha, beta)
                    O = out[:ldo * ncols].reshape(ncols, ldo)
                    want = alpha * ref + (beta * old if beta != 0.0 else 0.0)  # exact: integers and halves
                    assert np.isfinite(O[:, :n]).all(), where
                    assert np.array_equal(O[:, :n].T, want), where
                    assert _untouched(O[:, n:]) and _untouched(out[ldo * ncols:]), where


def test_tall_times_small_real_values_within_the_bound(prof, gpu_ctx):
    rng = np.random.default_rng(11)
    n, kk, ncols, ldi, lds, ldo = 65, 75, 9, 128, 80, 65
    In, S = rng.standard_normal((n, kk)), rng.standard_normal((kk, ncols))
    ref, ab = R.nn_product(In, S)
    out = _fill(ldo * ncols + 64)
    Inh, Sh = _colmajor(In, ldi, kk), _colmajor(S, lds, ncols)
    gpu_ctx.check(prof.sdpsr_profile_tall_times_small(gpu_ctx._h, n, ldi, kk, lds, ncols, 1.0, 0.0, ldo, _vp(Inh), _vp(Sh), _vp(out), 64))
    assert _within(out[:ldo * ncols].reshape(ncols, ldo)[:, :n].T, ref, ab, kk)
    assert _untouched(out[ldo * ncols:])


def test_tall_times_small_entry_refuses_what_could_index_outside(prof, gpu_ctx):
    a = np.zeros(4096)
    ok = dict(n=8, ldi=8, kk=4, lds=4, ncols=4, ldo=8)
    for change in (dict(n=0), dict(n=8193), dict(ldi=7), dict(ldo=7), dict(kk=0), dict(lds=3), dict(ncols=0), dict(ncols=513)):
        q = dict(ok, **change)
        st = prof.sdpsr_profile_tall_times_small(gpu_ctx._h, q["n"], q["ldi"], q["kk"], q["lds"], q["ncols"], 1.0, 0.0, q["ldo"], _vp(a), _vp(a), _vp(a), 0)
        assert st == BAD_ARGUMENT, change


# ---------------------------------------------------------------------------------------------------------------------------
# label product
# ---------------------------------------------------------------------------------------------------------------------------
def _label_product(prof, ctx, n, w, G, d, L, W, keys):
    """Y (G w columns of ldy, as rows), guard tail, the reported form"""
    ld = _round_up(n, 128)
    if ld == n:
        ld += 128  # ldw, ldy != n
    Wh = _colmajor(W, ld, 64)  # rows n..ld and columns >= w: NaN
    guard = 2 * ld + 5
    Y = _fill(ld * G * w + guard)
    rep = _report(4)
    kk = np.array(keys, dtype=np.uint64)
    ctx.check(prof.sdpsr_profile_label_product(ctx._h, n, d, G, w, ld, ld, _vp(kk), _vp(L), _vp(Wh), _vp(Y), guard, rep))
    return Y[:ld * G * w].reshape(G * w, ld), Y[ld * G * w:], tuple(rep)


@pytest.fixture(scope="module")
def label_cases():
    """inputs and long-double references of the rows, made once and left alone"""
    cache = {}

    def get(n, w, d, keys):
        key = (n, w, d, keys)
        if key not in cache:
            L = R.hashed_labels(n, d)
            W = np.random.default_rng(n * 100 + w).standard_normal((n, w))
            cache[key] = (L, W) + R.label_product(n, L, keys, W)
        return cache[key]
    return get


@pytest.mark.parametrize("row,form", R.LABEL_ROWS, ids=lambda v: "-".join(map(str, v)))
def test_label_product(prof, gpu_ctx, label_cases, row, form):
    """Y = A(v) W, every row of the result, against the long-double reference with k = n; the form that ran, as reported by the function
    the launcher asked, is the one this row is in the table for.  Non-symmetric hashed labels with 0 and d, ldw = ldy != n, NaN in the
    rows n..ldw and the columns >= w of W, G distinct keys."""
    n, w, G, d = row
    keys = R.KEYS[:G]
    L, W, ref, ab = label_cases(n, w, d, keys)
    assert L.max() == d and (L.min() == 0 or n == 1)
    Y, tail, rep = _label_product(prof, gpu_ctx, n, w, G, d, L, W, keys)
    assert rep[:2] == form, rep
    assert rep == R.label_form(n, d, G, w), rep  # the CPU test's restatement of the rule is the rule
    if row in R.LABEL_ROW_SPLIT:
        assert rep[2:] == R.LABEL_ROW_SPLIT[row]
    assert _within(Y[:, :n].T, ref, ab, n)
    assert _untouched(Y[:, n:]) and _untouched(tail)
    if G > 1:
        # block g of the batched result = the one-element result with key g.  Both sum in fixed order; the order is the same -- bit for
        # bit -- when both take the same form with the same column split (an output's sum does not depend on the tile width or on the
        # other elements).  Where the one-element call takes another form or split, the two are two summation orders of the same n
        # terms: each is within the bound of the reference.
        for g in range(G):
            Y1, tail1, rep1 = _label_product(prof, gpu_ctx, n, w, 1, d, L, W, (keys[g],))
            assert rep1 == R.label_form(n, d, 1, w)
            if (rep1[0], rep1[2], rep1[3]) == (rep[0], rep[2], rep[3]):
                assert np.array_equal(_bits(Y[g * w:(g + 1) * w, :n]), _bits(Y1[:, :n])), (g, rep, rep1)
            else:
                assert _within(Y1[:, :n].T, ref[:, g * w:(g + 1) * w], ab[:, g * w:(g + 1) * w], n), (g, rep1)
            assert _untouched(Y1[:, n:]) and _untouched(tail1)


def test_label_product_entry_refuses(prof, gpu_ctx):
    """what the launcher refuses (G = 3, G w > 64, d > 4000, four class tables beyond 64 KiB) and what could index outside a buffer"""
    n = 63
    L = R.hashed_labels(n, 7)
    Wh = np.zeros(128 * 64)
    Y = np.zeros(128 * 64 + 8)
    keys = np.array(R.KEYS, dtype=np.uint64)
    rep = _report(4)

    def call(n=n, d=7, G=1, w=8, ldw=128, ldy=128, L=L):
        return prof.sdpsr_profile_label_product(gpu_ctx._h, n, d, G, w, ldw, ldy, _vp(keys), _vp(L), _vp(Wh), _vp(Y), 8, rep)
    assert call() == 0
    assert call(G=3) == BAD_ARGUMENT and call(G=2, w=33) == BAD_ARGUMENT and call(d=4001) == BAD_ARGUMENT and call(G=4, w=17) == BAD_ARGUMENT
    assert call(G=4, d=2047) == BAD_ARGUMENT and call(w=65) == BAD_ARGUMENT and call(w=0) == BAD_ARGUMENT and call(G=0) == BAD_ARGUMENT
    assert call(n=0) == BAD_ARGUMENT and call(ldw=62) == BAD_ARGUMENT and call(ldy=62) == BAD_ARGUMENT
    assert call(d=6) == BAD_ARGUMENT  # a label exceeds d: found on the host copy, nothing uploaded
    assert b"exceeds d" in gpu_ctx._lib.sdpsr_last_error(gpu_ctx._h)


# ---------------------------------------------------------------------------------------------------------------------------
# class sums
# ---------------------------------------------------------------------------------------------------------------------------
def _class_labels(n, d):
    """non-symmetric labels 0..d with a label 0 and, from d = 2 on, a class without any entry (class 2)"""
    L = R.hashed_labels(n, d, salt=23)
    if d >= 2:
        L[L == 2] = 1
    return L


def _table_fits(n, d):
    """the per-lane tables of class_sums_small_d_kernel in LDS: x (n doubles) + 4 waves x 64 lanes x (d + 1, made odd) doubles"""
    return (n + 4 * 64 * ((d + 1) | 1)) * 8 <= 150 * 1024


@pytest.mark.parametrize("n", [1, 3, 4, 5, 511, 512, 513, 1030])
def test_class_sums(prof, gpu_ctx, n):
    """out[(i - 1) ldo + r] = sum over c with L[c + r n] == i of x[c] (COLUMN r of the labels): batches of 512 columns, 4 rows per
    workgroup; ldo = n and ldo = n rounded up to 128 (the driver's layout); an integer x, exact.  At n = 1030, d = 70 the tables no
    longer fit LDS: class_sums_supports says no for ldo != n and the row-sort fallback runs for ldo == n."""
    rng = np.random.default_rng(n)
    x = rng.integers(-8, 9, n).astype(np.float64)
    for d in (1, 2, 34, 70):
        L = _class_labels(n, d)
        ref = R.class_sums_int(n, d, L, x)
        if d >= 2 and n > 1:
            assert (L == 0).any() and not ref[1].any() and not (L == 2).any()
        for ldo in (n, _round_up(n, 128) if n % 128 else n + 128):
            out = _fill(ldo * d + 77)
            rep = _report(2)
            gpu_ctx.check(prof.sdpsr_profile_class_sums(gpu_ctx._h, n, d, ldo, _vp(L), _vp(x), _vp(out), 77, rep))
            table = _table_fits(n, d)
            assert rep[1] == int(table) and rep[0] == int(table or ldo == n), (d, ldo, tuple(rep))
            assert table or (n, d) == (1030, 70)
            if not rep[0]:
                assert _untouched(out)  # nothing ran
                continue
            O = out[:ldo * d].reshape(d, ldo)
            assert np.array_equal(O[:, :n], ref), (d, ldo)
            assert _untouched(O[:, n:]) and _untouched(out[ldo * d:]), (d, ldo)


def test_class_sums_fallback_route(prof, gpu_ctx):
    """d = 200 at n = 513: no room for the tables -- not supported with ldo != n, basis_image_rows_kernel<1> with ldo == n."""
    n, d = 513, 200
    x = np.random.default_rng(8).integers(-8, 9, n).astype(np.float64)
    L = _class_labels(n, d)
    ref = R.class_sums_int(n, d, L, x)
    assert not _table_fits(n, d)
    out = _fill(640 * d + 77)
    rep = _report(2)
    gpu_ctx.check(prof.sdpsr_profile_class_sums(gpu_ctx._h, n, d, 640, _vp(L), _vp(x), _vp(out), 77, rep))
    assert tuple(rep) == (0, 0) and _untouched(out)
    out = _fill(n * d + 77)
    gpu_ctx.check(prof.sdpsr_profile_class_sums(gpu_ctx._h, n, d, n, _vp(L), _vp(x), _vp(out), 77, rep))
    assert tuple(rep) == (1, 0)
    assert np.array_equal(out[:n * d].reshape(d, n), ref)
    assert _untouched(out[n * d:])
    assert prof.sdpsr_profile_class_sums(gpu_ctx._h, n, 199, n, _vp(L), _vp(x), _vp(out), 77, rep) == BAD_ARGUMENT  # a label exceeds d
    assert prof.sdpsr_profile_class_sums(gpu_ctx._h, n, d, n - 1, _vp(L), _vp(x), _vp(out), 77, rep) == BAD_ARGUMENT
    assert prof.sdpsr_profile_class_sums(gpu_ctx._h, n, 0, n, _vp(L), _vp(x), _vp(out), 77, rep) == BAD_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------
# glue
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7, 33, 72])
def test_symmetrize_and_extract_symmetric(prof, gpu_ctx, m):
    """0.5 (B + B') is one rounding per entry, the same in NumPy: bit equality, and a bitwise symmetric result.  symmetrize touches
    the leading m x m alone; extract_symmetric writes zeros on all of mp x mp outside m x m."""
    rng = np.random.default_rng(m)
    mp = _round_up(m, 128)
    B = rng.standard_normal((m, m))
    want = 0.5 * (B + B.T)
    buf = _colmajor(B, mp, m, SENT)
    buf = np.concatenate([buf, _fill(50)])
    gpu_ctx.check(prof.sdpsr_profile_symmetrize(gpu_ctx._h, m, mp, _vp(buf), 50))
    G = buf[:mp * m].reshape(m, mp)
    assert np.array_equal(_bits(G[:, :m].T), _bits(want)) and np.array_equal(_bits(G[:, :m]), _bits(G[:, :m].T))
    assert _untouched(G[:, m:]) and _untouched(buf[mp * m:])
    lds = m + 5
    dst = _fill(mp * mp + 50)
    src = _colmajor(B, lds, m)
    gpu_ctx.check(prof.sdpsr_profile_extract_symmetric(gpu_ctx._h, m, mp, lds, _vp(src), _vp(dst), 50))
    D = dst[:mp * mp].reshape(mp, mp)
    assert np.array_equal(_bits(D[:m, :m].T), _bits(want)) and np.array_equal(_bits(D[:m, :m]), _bits(D[:m, :m].T))
    assert _zero_bits(D[m:, :]) and _zero_bits(D[:, m:])
    assert _untouched(dst[mp * mp:])
    assert prof.sdpsr_profile_symmetrize(gpu_ctx._h, m, m - 1, _vp(buf), 0) == BAD_ARGUMENT
    assert prof.sdpsr_profile_extract_symmetric(gpu_ctx._h, m, m - 1, lds, _vp(buf), _vp(dst), 0) == BAD_ARGUMENT
    assert prof.sdpsr_profile_extract_symmetric(gpu_ctx._h, m, mp, m - 1, _vp(buf), _vp(dst), 0) == BAD_ARGUMENT


@pytest.mark.parametrize("n", [1, 1023, 1025])
def test_normalize_columns(prof, gpu_ctx, n):
    """One workgroup of 1024 threads per run: n = 1023, 1025 straddle one pass.  The norm is a sum of n squares and a square root:
    within 2 n 2^-53 relative (n 2^-53 for the sum, halved by the root, + the root's own rounding).  H = X (1 / norm): two roundings on
    top of the norm the kernel itself reports, 3 2^-53 relative.  A zero column gives a zero column and norm 0."""
    rng = np.random.default_rng(n)
    nruns, ldx, hstride = 4, n + 3, n + 5
    X = rng.standard_normal((n, nruns))
    X[:, 2] = 0.0
    H = _fill(hstride * (nruns - 1) + n + 40)
    nrm = _fill(nruns + 40)
    Xh = _colmajor(X, ldx, nruns)
    gpu_ctx.check(prof.sdpsr_profile_normalize_columns(gpu_ctx._h, n, ldx, hstride, nruns, _vp(Xh), _vp(H), _vp(nrm), 40))
    Xl = X.astype(np.longdouble)
    ref = np.sqrt((Xl * Xl).sum(axis=0))
    assert (np.abs(nrm[:nruns].astype(np.longdouble) - ref) <= np.longdouble(2 * n * U) * ref).all()
    assert _bits(nrm[2:3])[0] == 0 and _untouched(nrm[nruns:])
    for r in range(nruns):
        h = H[r * hstride:r * hstride + n]
        if r == 2:
            assert _zero_bits(h)
        else:
            q = Xl[:, r] / np.longdouble(nrm[r])
            assert (np.abs(h.astype(np.longdouble) - q) <= np.longdouble(3 * U) * np.abs(q)).all()
        assert _untouched(H[r * hstride + n:(r + 1) * hstride if r + 1 < nruns else None])
    assert prof.sdpsr_profile_normalize_columns(gpu_ctx._h, n, n - 1, hstride, nruns, _vp(X), _vp(H), _vp(nrm), 0) == BAD_ARGUMENT
    assert prof.sdpsr_profile_normalize_columns(gpu_ctx._h, n, ldx, n - 1, nruns, _vp(X), _vp(H), _vp(nrm), 0) == BAD_ARGUMENT


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4000])
def test_random_vector(prof, gpu_ctx, n):
    """x[i] = 2 v(key, i + 1) - 1: v is a multiple of 2^-53 below 1, so 2 v - 1 is exactly representable and an FMA changes nothing."""
    for key in R.RANDOM_VECTOR_KEYS:
        x = _fill(n + 300)
        gpu_ctx.check(prof.sdpsr_profile_random_vector(gpu_ctx._h, n, key, _vp(x), 300))
        want = 2.0 * R.class_uniform(key, np.arange(1, n + 1, dtype=np.uint64)) - 1.0
        assert np.array_equal(_bits(x[:n]), _bits(want))
        assert ((x[:n] >= -1) & (x[:n] < 1)).all() and _untouched(x[n:])
    assert prof.sdpsr_profile_random_vector(gpu_ctx._h, 0, 1, _vp(x), 0) == BAD_ARGUMENT
