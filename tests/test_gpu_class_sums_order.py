"""The class-sum kernels with per-lane tables (class_sums_small_d_kernel, class_sums2_kernel of csrc/kernels_blockdiag.hip) keep
their documented summation order, bit for bit: per lane its columns ascending from +0.0, then the lanes 0 .. 63 in order
(tests/class_sums_order_ref.py).  A lane's entries arrive in batches of eight, and two entries of a batch may carry the same label:
any form of the update that does not finish one entry before it starts the next (queued LDS adds today; reads issued together with
the earlier entry's sum forwarded in registers was tried, profiles/r16_bd_label_passes.txt) must still give the left-to-right sum.
So the shapes are those where that can go wrong: one and two classes (every batch is all duplicates), many classes, label 0, a last
batch of one column, ragged rows per round.  x has mixed signs and magnitudes 1e-8 .. 1e8: a sum formed in another order differs
in its bits."""
import ctypes as C

import numpy as np
import pytest

import class_sums_order_ref as O
import module_kernels_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF85A5ADEADBEEF  # the fill of every in/out array
GUARD = 77
BAD_ARGUMENT = 5
NS = (5, 511, 513, 1030)  # 513: a last batch of ONE column; 5, 511, 1030: rows that do not fill the rounds of a workgroup


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _fill(count):
    return np.full(int(count), SENT, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((_bits(a) == np.uint64(SENT)).all())


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


def _labels(n, dmax, salt):
    """non-symmetric hashed labels 0 .. dmax, with 0 and dmax present"""
    return R.hashed_labels(n, dmax, salt=salt)


@pytest.mark.parametrize("n", NS)
def test_class_sums_one_vector_order(prof, gpu_ctx, n):
    """class_sums_small_d_kernel through launch_class_sums, ldo = n: d = 1, 2 (all duplicates), 34; labels with 0."""
    x = O.mixed_magnitudes(np.random.default_rng(100 + n), n)
    for d in (1, 2, 34):
        L = _labels(n, d, salt=31 + d)
        assert (L == 0).any() and L.max() == d
        ref = O.class_sums_in_order(n, d, L, x)[:, :, 0]
        out = _fill(n * d + GUARD)
        rep = (C.c_int32 * 2)(-1, -1)
        gpu_ctx.check(prof.sdpsr_profile_class_sums(gpu_ctx._h, n, d, n, _vp(L), _vp(x), _vp(out), GUARD, rep))
        assert tuple(rep) == (1, 1), (d, tuple(rep))  # the kernel with per-lane tables ran
        assert np.array_equal(_bits(out[:n * d].reshape(d, n)), _bits(ref)), (n, d)
        assert _untouched(out[n * d:]), (n, d)


def _class_sums2(prof, ctx, n, d, first, plain, L, X):
    Y = _fill(2 * n * d + GUARD)
    rep = (C.c_int32 * 1)(-1)
    Xh = np.ascontiguousarray(X, dtype=np.float64)  # n pairs, interleaved
    ctx.check(prof.sdpsr_profile_class_sums2(ctx._h, n, d, first, int(plain), _vp(L), _vp(Xh), _vp(Y), GUARD, rep))
    return Y[:2 * n * d].reshape(d, n, 2), Y[2 * n * d:], rep[0]


@pytest.mark.parametrize("d,waves", [(1, 4), (2, 4), (34, 4), (70, 2), (140, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("n", NS)
def test_class_sums_pair_order(prof, gpu_ctx, n, d, waves):
    """class_sums2_kernel<W, WIN>: the labels as they are (plain, WIN = false) and a window of d classes that starts at class 3 of
    d + 4 (WIN = true: labels below, inside and above the window, and 0); W = 4 / 2 / 1 waves per workgroup by d."""
    X = O.mixed_magnitudes(np.random.default_rng(7 * n + d), (n, 2))
    L = _labels(n, d, salt=41 + d)
    assert (L == 0).any() and L.max() == d
    got, tail, W = _class_sums2(prof, gpu_ctx, n, d, 1, True, L, X)
    assert W == waves
    assert np.array_equal(_bits(got), _bits(O.class_sums_in_order(n, d, L, X))), (n, d, "plain")
    assert _untouched(tail)
    first = 3
    Lw = _labels(n, d + 4, salt=43 + d)
    assert (Lw == 0).any() and (Lw < first).any() and Lw.max() == d + 4 >= first + d
    got, tail, W = _class_sums2(prof, gpu_ctx, n, d, first, False, Lw, X)
    assert W == waves
    assert np.array_equal(_bits(got), _bits(O.class_sums_in_order(n, d, Lw, X, first=first))), (n, d, "window")
    assert _untouched(tail)


def test_class_sums_pair_all_label_zero_and_refusals(prof, gpu_ctx):
    """every label 0: nothing belongs to a class, every sum is +0.0; and what the entry refuses"""
    n, d = 513, 2
    X = O.mixed_magnitudes(np.random.default_rng(5), (n, 2))
    L = np.zeros(n * n, dtype=np.uint32)
    for plain in (True, False):
        got, tail, _ = _class_sums2(prof, gpu_ctx, n, d, 1, plain, L, X)
        assert not _bits(got).any() and _untouched(tail)
    Y = _fill(2 * n * 149 + GUARD)
    rep = (C.c_int32 * 1)(-1)
    L[7] = 3
    h = gpu_ctx._h
    assert prof.sdpsr_profile_class_sums2(h, n, d, 1, 1, _vp(L), _vp(X), _vp(Y), GUARD, rep) == BAD_ARGUMENT  # plain: a label exceeds d
    assert prof.sdpsr_profile_class_sums2(h, n, d, 2, 1, _vp(L), _vp(X), _vp(Y), GUARD, rep) == BAD_ARGUMENT  # plain means first = 1
    assert prof.sdpsr_profile_class_sums2(h, n, 0, 1, 0, _vp(L), _vp(X), _vp(Y), GUARD, rep) == BAD_ARGUMENT
    assert prof.sdpsr_profile_class_sums2(h, n, 149, 1, 0, _vp(L), _vp(X), _vp(Y), GUARD, rep) == BAD_ARGUMENT  # one wave's tables beyond LDS
    assert _untouched(Y)
