"""launch_label_spmm_pair (csrc/kernels_module.hip): two label products on one W in one pass over the labels -- the invariance round
of the module growth and its rider -- through sdpsr_profile_label_product_pair.  The pair runs the one-element matrix-core form of
its shape with two class tables, so each block must equal, BIT FOR BIT, what the existing one-element entry
(sdpsr_profile_label_product, G = 1) gives with that key: same form, same column split, same partial sums in the same order."""
import ctypes as C

import numpy as np
import pytest

import module_kernels_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF85A5ADEADBEEF    # the fill of every in/out array
POISON = 0x7FF80BAD0BAD0BAD  # the fill of input regions nobody may read
BAD_ARGUMENT = 5
KEYS = (R.KEYS[2], R.KEYS[1])


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _fill(count, pattern=SENT):
    return np.full(int(count), pattern, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((_bits(a) == np.uint64(SENT)).all())


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


def _ld(n):
    ld = -(-n // 128) * 128
    return ld + 128 if ld == n else ld  # ldw = ldy != n


def _w_host(n, w, ld):
    """W (n x w) in ld x 64 whose rows n .. ld and columns >= w hold NaN"""
    W = np.random.default_rng(n * 100 + w).standard_normal((n, w))
    buf = _fill(ld * 64, POISON)
    buf.reshape(64, ld)[:w, :n] = W.T
    return buf


def _single(prof, ctx, n, w, d, ld, key, L, Wh, guard):
    Y = _fill(ld * w + guard)
    rep = (C.c_int32 * 4)(-1, -1, -1, -1)
    kk = np.array([key], dtype=np.uint64)
    ctx.check(prof.sdpsr_profile_label_product(ctx._h, n, d, 1, w, ld, ld, _vp(kk), _vp(L), _vp(Wh), _vp(Y), guard, rep))
    return Y, tuple(rep)


@pytest.mark.parametrize("w", [33, 34, 48, 49, 64])  # JT = 3 and 4, full and ragged last tile
@pytest.mark.parametrize("n", [64, 130, 513])
def test_pair_equals_two_single_products(prof, gpu_ctx, n, w):
    ld = _ld(n)
    guard = 2 * ld + 5
    Wh = _w_host(n, w, ld)
    kk = np.array(KEYS, dtype=np.uint64)
    for d in (1, 34, 200):
        L = R.hashed_labels(n, d)  # non-symmetric, 0 and d present
        assert L.max() == d and L.min() == 0
        Y0, Y1 = _fill(ld * w + guard), _fill(ld * w + guard)
        rep = (C.c_int32 * 4)(-1, -1, -1, -1)
        gpu_ctx.check(prof.sdpsr_profile_label_product_pair(gpu_ctx._h, n, d, w, ld, ld, _vp(kk), _vp(L), _vp(Wh), _vp(Y0), _vp(Y1), guard, rep))
        assert tuple(rep) == R.label_form(n, d, 1, w) and rep[0] == 1 and rep[1] == (w + 15) // 16, tuple(rep)
        for g, Y in enumerate((Y0, Y1)):
            S, rep1 = _single(prof, gpu_ctx, n, w, d, ld, KEYS[g], L, Wh, guard)
            assert rep1 == tuple(rep)  # the same form and split, by construction
            got, ref = Y[:ld * w].reshape(w, ld), S[:ld * w].reshape(w, ld)
            assert not np.isnan(ref[:, :n]).any()
            assert np.array_equal(_bits(got[:, :n]), _bits(ref[:, :n])), (n, w, d, g)
            assert _untouched(got[:, n:]) and _untouched(Y[ld * w:]), (n, w, d, g)
        assert not np.array_equal(_bits(Y0[:ld * w]), _bits(Y1[:ld * w]))  # two keys, two results


def test_pair_entry_refuses(prof, gpu_ctx):
    """what the pair launch cannot run: w > 64, n < 64 (no matrix-core form), class tables that do not fit"""
    n, ld = 130, 256
    L = R.hashed_labels(n, 7)
    Wh = np.zeros(ld * 64)
    Y0, Y1 = _fill(ld * 64 + 8), _fill(ld * 64 + 8)
    kk = np.array(KEYS, dtype=np.uint64)
    rep = (C.c_int32 * 4)(-1, -1, -1, -1)

    def call(n=n, d=7, w=34, ldw=ld, ldy=ld, L=L):
        return prof.sdpsr_profile_label_product_pair(gpu_ctx._h, n, d, w, ldw, ldy, _vp(kk), _vp(L), _vp(Wh), _vp(Y0), _vp(Y1), 8, rep)
    assert call() == 0
    Y0[:], Y1[:] = _fill(Y0.size), _fill(Y1.size)
    assert call(w=65) == BAD_ARGUMENT and call(w=0) == BAD_ARGUMENT
    assert call(n=63, L=R.hashed_labels(63, 7)) == BAD_ARGUMENT
    assert R.label_form(n, 3000, 1, 34)[0] == 0  # the one-element form of this shape is the VALU one: its table is beyond 64 KiB with the slabs
    assert call(d=3000) == BAD_ARGUMENT and call(d=4001) == BAD_ARGUMENT
    assert call(ldw=129) == BAD_ARGUMENT and call(ldy=129) == BAD_ARGUMENT
    assert call(d=6) == BAD_ARGUMENT  # a label exceeds d
    assert _untouched(Y0) and _untouched(Y1)
