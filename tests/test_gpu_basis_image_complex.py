"""sdpsr_basis_image_complex: basis_image(Q, P; atol) over ComplexF64 (src/diagonalize.jl:64-89, called with the
desymmetrized partition by src/compat.jl:54-57) of a caller's Q_hat for a window of classes.
The reference is the formula blks[i][k] = Q_k^H 1[P == i] Q_k in np.clongdouble over the entries of each class
(tests/basis_image_complex_helpers.py).  The bound is the project's 2e-12 n in complex magnitude: both sides zero entries
below atol = 1e-12 n, so an entry may differ by atol; fp64 rounding is orders of magnitude below
(tests/test_basis_image_complex_cpu.py checks the complex128 evaluation against a tenth of the bound, and that the Gaussian
instances have no non-zero image anywhere near atol).

The instances, all but N1 / P4 non-symmetric, and the kernel boundary each one hits:
  Z3K70   directed(3) (x) K_70, n = 210, d = 6, classes of 210 and 14 490 entries: 14 490 = 3 full chunks of 4096 and a ragged
          fourth, summed in chunk order by the reduce kernel; blocks (1, 2, 5, 17), S = 319 = 39 output tiles of 8 and a
          ragged fortieth; `auto` is chunk (average class 7350 entries); on `outer` the 14 490 entries are 1811 batches of 8
          and a ragged one of 2
  M4K17   full(4) (x) K_17, n = 68, d = 32, classes of 17 and 272 entries; blocks (40, 3): s = 40 gives G = 6 column groups,
          240 of 256 threads active, columns g + 6 j ragged against 40; s = 3 leaves most of the workgroup idle; `auto` is
          outer (average class 144 entries) -- where a choice by the window's count would switch to chunk for one class
  M4K17W  the same labels, blocks (65, 3): s = 65 gives G = 3 and 48 columns per pass of the outer kernel's 16 accumulators,
          so the 65 columns take two passes over the class
  Z16K5   directed(16) (x) K_5, n = 80, d = 32, eighteen 1 x 1 blocks: S = 18, two full output tiles and a ragged third
  DSF     a direct sum of M_s (x) I_k, n = 76, d = 319, label 0 on most entries (skipped), classes of 1 .. 7 entries: a batch
          of the outer kernel is never full, every chunk is a few entries
  N1      n = 1
  C3, P4  the reference's own C_3 matrix and its 4 x 4 Partition(3, ...) (test/runtests.jl:43-57)"""
import ctypes as C
import functools

import numpy as np
import pytest

import basis_image_complex_helpers as H
from basis_image_helpers import gaussian_unit_columns

pytestmark = pytest.mark.gpu

OK, BAD_ARGUMENT = 0, 5
HOST, DEVICE = 0, 1
OUTER, CHUNK = 4, 5
ROUTES = ["outer", "chunk", "auto"]
FULL = 1 << 10  # SDPSR_FLAG_FULL_BASIS_IMAGE: no effect on this entry
GUARD = 5       # complex numbers on either side of the output
AUTO_ROUTE = {"Z3K70": CHUNK, "M4K17": OUTER, "M4K17W": OUTER, "Z16K5": OUTER, "DSF": OUTER, "N1": OUTER, "C3": OUTER, "P4": OUTER}


def _kw(route):
    return {} if route == "auto" else {"basis_image_kernel": route}


def _want_route(route, name):
    return {"outer": OUTER, "chunk": CHUNK}.get(route, AUTO_ROUTE[name])


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _flat(L, dtype=np.uint32):
    return np.ascontiguousarray(np.asarray(L).ravel(order="F").astype(dtype))


def _qflat(Q):
    return np.ascontiguousarray(np.asarray(Q, dtype=np.complex128).ravel(order="F"))


def _call(ctx, lab, n, d, sizes, Q, first, count, atol=-1.0):
    """The C entry on host arrays; the output sits between GUARD NaNs on either side.
    Returns (status, window as count x S complex or None, route, whole buffer)."""
    sz = np.asarray(sizes, dtype=np.int32)
    S = int(sum(int(s) * int(s) for s in sizes))
    q = _qflat(Q)
    buf = np.full(2 * GUARD + max(count, 0) * S, np.nan + 1j * np.nan, dtype=np.complex128)
    route = C.c_int32(-1)
    st = ctx._lib.sdpsr_basis_image_complex(ctx._h, n, _vp(lab), d, len(sz), _vp(sz), _vp(q), first, count, atol,
                                            C.c_void_p(buf.ctypes.data + 16 * GUARD), C.byref(route), None, HOST)
    win = buf[GUARD:GUARD + count * S].reshape(count, S) if st == OK and count >= 0 else None
    return st, win, route.value, buf


def _guards_intact(buf):
    g = np.concatenate([buf[:GUARD], buf[len(buf) - GUARD:]])
    return bool(np.isnan(g.real).all() and np.isnan(g.imag).all())


def _err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.clongdouble) - ref).max()) if got.size else 0.0


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _rows(blks):
    return np.array([np.concatenate([np.asarray(b).ravel(order="F") for b in row]) for row in blks])


# ------------------------------------------------------------------ 1. the closed form
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("m", [1, 3, 63, 64, 65])
def test_closed_form_on_the_cyclic_group(pkg, m, route):
    """directed(m), Fourier Q_hat, all blocks 1 x 1: blks[1 + t][k] = omega^(t k).  m = 64 / 65: S on either side of the
    output tiles, m workgroups per block row on `outer`."""
    F, want = H.fourier_columns(m), H.fourier_closed_form(m)
    with pkg.Context(seed=21, **_kw(route)) as ctx:
        st, win, rt, buf = _call(ctx, _flat(H.directed(m)), m, m, (1,) * m, F, 1, m, atol=0.0)
        assert st == OK and _guards_intact(buf), ctx._lib.sdpsr_last_error(ctx._h)
        err = _err(win, want.astype(np.clongdouble))
        print(f"basis_image_complex closed form m={m} {route} route={rt} err={err:.3e} bound={2e-12 * m:.3e}")
        assert rt == _want_route(route, "C3")  # m classes of m entries: `auto` is outer
        assert err <= 2e-12 * m
        if m == 3:  # C_3 exactly as the reference writes it: the transpose, omega^(-t k)
            st, win, rt, buf = _call(ctx, _flat(H.C3), 3, 3, (1, 1, 1), F, 1, 3)
            assert st == OK and _guards_intact(buf)
            assert _err(win, H.fourier_closed_form(3, -1).astype(np.clongdouble)) <= 2e-12 * 3


# ------------------------------------------------------------------ 2. Gaussian Q against the reference
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["Z3K70", "M4K17", "M4K17W", "Z16K5", "DSF", "N1", "C3", "P4"])
def test_gaussian_q_against_the_reference(pkg, name, route):
    L, d = H.instance(name)
    n = L.shape[0]
    sizes, Q, ref = H.gaussian_case(name)
    with pkg.Context(seed=22, flags=FULL if name == "Z16K5" else 0, **_kw(route)) as ctx:
        st, win, rt, buf = _call(ctx, _flat(L), n, d, sizes, Q, 1, d)
    assert st == OK and _guards_intact(buf)
    err = _err(win, ref)
    print(f"basis_image_complex gaussian {name} {route} route={rt} err={err:.3e} bound={2e-12 * n:.3e}")
    assert rt == _want_route(route, name), (name, route, rt)
    assert not (np.isnan(win.real).any() or np.isnan(win.imag).any())
    assert err <= 2e-12 * n


# ------------------------------------------------------------------ 3. windows
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["Z3K70", "M4K17", "Z16K5", "DSF", "C3"])
def test_windows_equal_the_slice_of_the_full_call_bit_for_bit(pkg, name, route):
    L, d = H.instance(name)
    n = L.shape[0]
    sizes, Q, ref = H.gaussian_case(name)
    lab = _flat(L)
    with pkg.Context(seed=23, **_kw(route)) as ctx:
        st, full, rt_full, buf = _call(ctx, lab, n, d, sizes, Q, 1, d)
        assert st == OK and _guards_intact(buf) and rt_full == _want_route(route, name)
        assert _err(full, ref) <= 2e-12 * n
        empty = 0
        for parts in (2, 3, d, d + 3):
            for j in range(parts):
                first, count = H.class_window(d, parts, j)
                assert (first, count) == pkg.class_window(d, parts, j)
                st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
                assert st == OK, (first, count, ctx._lib.sdpsr_last_error(ctx._h))
                assert _guards_intact(buf), (name, route, first, count)
                if count == 0:
                    empty += 1
                    assert rt == 0 and win.size == 0
                    continue
                assert rt == rt_full, (name, route, first, count, rt)  # the route never depends on the window
                assert _same_bits(win, full[first - 1:first - 1 + count]), (name, route, first, count)
        assert empty == 3  # parts = d + 3


# ------------------------------------------------------------------ 4. the clamp is by magnitude
@pytest.mark.parametrize("route", ROUTES)
def test_clamp_is_by_magnitude(pkg, route):
    """Fourier instance m = 8: every image has |z| = 1; for odd t k both components of omega^(t k) are 0.707 < 0.9, so a
    clamp per component at atol = 0.9 would zero them."""
    m = 8
    F, want = H.fourier_columns(m), H.fourier_closed_form(m)
    assert (np.maximum(np.abs(want.real), np.abs(want.imag)) < 0.9).any()
    lab = _flat(H.directed(m))
    with pkg.Context(seed=24, **_kw(route)) as ctx:
        res = {}
        for atol in (0.9, 1.1, 0.0, -1.0):
            st, win, rt, buf = _call(ctx, lab, m, m, (1,) * m, F, 1, m, atol=atol)
            assert st == OK and _guards_intact(buf)
            res[atol] = win
    assert _same_bits(res[0.9], res[0.0]) and _same_bits(res[-1.0], res[0.0])  # nothing is below 0.9, or below 8e-12
    assert np.all(np.abs(np.abs(res[0.9]) - 1.0) <= 1e-14)
    assert _err(res[0.9], want.astype(np.clongdouble)) <= 2e-12 * m
    assert np.all(res[1.1] == 0) and not np.signbit(res[1.1].real).any() and not np.signbit(res[1.1].imag).any()  # 0 + 0i


@pytest.mark.parametrize("route", ROUTES)
def test_default_atol_clamps_and_zero_does_not(pkg, route):
    """One entry of Q is 1e-7 in the row of a single-entry class of DSF: that class's image of the 1 x 1 block is
    |1e-7|^2 = 1e-14 < 1e-12 n.  atol = 0 must leave it, atol < 0 must clamp it."""
    L, d = H.instance("DSF")
    n = L.shape[0]
    sizes, Q0, _ = H.gaussian_case("DSF")
    counts = np.bincount(L.ravel(), minlength=d + 1)
    cls = int(np.flatnonzero(counts[1:] == 1)[0]) + 1
    r, c = (int(v) for v in np.argwhere(L == cls)[0])
    assert r == c  # the 1 x 1 diagonal block of the direct sum
    k = sizes.index(1)
    col, off = sum(sizes[:k]), sum(s * s for s in sizes[:k])
    Q = Q0.copy()
    Q[r, col] = 6e-8 + 8e-8j
    ref = H.reference_images_complex(L, d, Q, sizes)
    assert abs(complex(ref[cls - 1, off]) - 1e-14) < 1e-20
    with pkg.Context(seed=25, **_kw(route)) as ctx:
        st, raw, _, buf = _call(ctx, _flat(L), n, d, sizes, Q, 1, d, atol=0.0)
        assert st == OK and _guards_intact(buf)
        st, clamped, _, buf = _call(ctx, _flat(L), n, d, sizes, Q, 1, d, atol=-1.0)
        assert st == OK and _guards_intact(buf)
    assert _err(raw, ref) <= 2e-12 * n and _err(clamped, ref) <= 2e-12 * n
    assert abs(raw[cls - 1, off] - 1e-14) < 1e-20
    assert clamped[cls - 1, off] == 0
    assert not np.any((clamped != 0) & (np.abs(clamped) < 1e-12 * n))


# ------------------------------------------------------------------ 5. a real Q_hat
@pytest.mark.parametrize("route", ROUTES)
def test_real_q_hat_gives_zero_imaginary_parts_and_the_real_entry(pkg, problems, route):
    L, d, _ = problems.known_blocks_instance("DS")  # symmetric
    L = np.asarray(L, dtype=np.int64)
    n = L.shape[0]
    sizes = (3, 1, 5)
    Q = gaussian_unit_columns(n, sum(sizes), 41)
    S = sum(s * s for s in sizes)
    with pkg.Context(seed=26, **_kw(route)) as ctx:
        st, win, rt, buf = _call(ctx, _flat(L), n, d, sizes, Q.astype(np.complex128), 1, d)
        assert st == OK and _guards_intact(buf)
    with pkg.Context(seed=26, basis_image_kernel="chunk") as ctx:
        real = np.full(d * S, np.nan)
        sz, q = np.asarray(sizes, dtype=np.int32), np.ascontiguousarray(Q.ravel(order="F"))
        lab, rr = _flat(L), C.c_int32(-1)
        assert ctx._lib.sdpsr_basis_image(ctx._h, n, _vp(lab), d, len(sz), _vp(sz), _vp(q), 1, d, -1.0, _vp(real), C.byref(rr), None, HOST) == OK
        assert rr.value == CHUNK
    assert np.all(win.imag == 0)
    err = float(np.abs(win.real - real.reshape(d, S)).max())
    print(f"basis_image_complex real Q {route} route={rt} err against sdpsr_basis_image(chunk)={err:.3e} bound={2e-12 * n:.3e}")
    assert err <= 2e-12 * n


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_output_and_the_ctx_alone(pkg):
    L, d = H.instance("Z16K5")
    n = L.shape[0]
    sizes, Q, ref = H.gaussian_case("Z16K5")
    lab = _flat(L)
    S = sum(s * s for s in sizes)

    def beyond(v):
        b = lab.copy()
        b[(n - 1) + 2 * n] = v  # one entry; its mirror is left alone
        return b

    cases = [("class_first = 0", dict(first=0), "window"),
             ("window end d + 1", dict(first=d, count=2), "window"),
             ("class_first = d + 1", dict(first=d + 1, count=1), "window"),
             ("class_count = -1", dict(count=-1), "class_count"),
             ("s_k = 0", dict(sizes=(3, 0, 5)), "block size"),
             ("sum s_k = n + 1", dict(sizes=(n - 3, 4), Q=np.zeros((n, n + 1))), "more than n"),
             ("nblocks = 0", dict(nblocks=0), "nblocks"),
             ("n = 0", dict(n=0), "n < 1"),
             ("d = -1", dict(d=-1), "d < 0"),
             ("NULL Q_hat", dict(null="Q"), "null pointer"),
             ("NULL P", dict(null="P"), "null pointer"),
             ("NULL blks", dict(null="blks"), "null pointer"),
             ("NULL blk_sizes", dict(null="sizes"), "null pointer"),
             ("label d + 1", dict(lab=beyond(d + 1)), "a label exceeds d"),
             ("label 2^32 - 1", dict(lab=beyond(0xFFFFFFFF)), "a label exceeds d")]
    for route in ROUTES:
        with pkg.Context(seed=27, **_kw(route)) as ctx:
            for what, kw, msg in cases:
                if route != "outer" and "label" not in what:
                    continue  # the argument checks run before any route is chosen: once is enough
                szs = np.asarray(kw.get("sizes", sizes), dtype=np.int32)
                q = _qflat(kw.get("Q", Q))
                la = kw.get("lab", lab)
                first, count = kw.get("first", 1), kw.get("count", d)
                buf = np.full(2 * GUARD + d * S, -7.25 + 3.5j, dtype=np.complex128)
                null = kw.get("null")
                st = ctx._lib.sdpsr_basis_image_complex(ctx._h, kw.get("n", n), None if null == "P" else _vp(la), kw.get("d", d), kw.get("nblocks", len(szs)),
                                                        None if null == "sizes" else _vp(szs), None if null == "Q" else _vp(q), first, count, -1.0,
                                                        None if null == "blks" else C.c_void_p(buf.ctypes.data + 16 * GUARD), None, None, HOST)
                err = ctx._lib.sdpsr_last_error(ctx._h).decode()
                assert st == BAD_ARGUMENT and msg in err, (route, what, st, err)
                assert np.all(buf == -7.25 + 3.5j), (route, what)
                st, win, rt, b2 = _call(ctx, lab, n, d, sizes, Q, 3, 4)  # the ctx is usable
                assert st == OK and _guards_intact(b2) and _err(win, ref[2:6]) <= 2e-12 * n, (route, what)
            buf = np.full(2 * GUARD, -7.25 + 3.5j, dtype=np.complex128)
            rt = C.c_int32(-1)
            szs, q = np.asarray(sizes, dtype=np.int32), _qflat(Q)
            for first in (1, d, d + 5, 0):  # an empty window: OK wherever it "starts", nothing touched
                assert ctx._lib.sdpsr_basis_image_complex(ctx._h, n, _vp(lab), d, len(szs), _vp(szs), _vp(q), first, 0, -1.0,
                                                          C.c_void_p(buf.ctypes.data + 16 * GUARD), C.byref(rt), None, HOST) == OK
                assert np.all(buf == -7.25 + 3.5j) and rt.value == 0
            # a label beyond the window but within d is no error: it is the skipped class 0 of that call
            st, win, _, b2 = _call(ctx, lab, n, d, sizes, Q, 2, 3)
            assert st == OK and _guards_intact(b2) and _err(win, ref[1:4]) <= 2e-12 * n


# ------------------------------------------------------------------ 7. label widths and memory spaces
@pytest.mark.parametrize("route", ["outer", "chunk"])
def test_label_widths_and_memory_spaces_give_the_same_bits(pkg, route):
    import torch
    name = "Z16K5" if route == "outer" else "Z3K70"
    L, d = H.instance(name)
    n = L.shape[0]
    sizes, Q, ref = H.gaussian_case(name)
    S = sum(s * s for s in sizes)
    first, count = H.class_window(d, 3, 1)
    base = None
    for width in (32, 16, 8):
        dt = {8: np.uint8, 16: np.uint16, 32: np.uint32}[width]
        lab = _flat(L, dt)
        with pkg.Context(seed=28, label_width=width, **_kw(route)) as ctx:
            st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
            assert st == OK and _guards_intact(buf) and rt == _want_route(route, name)
            if base is None:
                base = win
                assert _err(base, ref[first - 1:first - 1 + count]) <= 2e-12 * n
            assert _same_bits(win, base), ("host", width)
            t_lab = torch.from_numpy(lab.view({8: np.uint8, 16: np.int16, 32: np.int32}[width]).copy()).cuda()
            t_q = torch.from_numpy(_qflat(Q)).cuda()
            t_sz = np.asarray(sizes, dtype=np.int32)
            t_out = torch.full((2 * GUARD + count * S,), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
            torch.cuda.synchronize()
            r2 = C.c_int32(-1)
            st = ctx._lib.sdpsr_basis_image_complex(ctx._h, n, C.c_void_p(t_lab.data_ptr()), d, len(sizes), _vp(t_sz), C.c_void_p(t_q.data_ptr()),
                                                    first, count, -1.0, C.c_void_p(t_out.data_ptr() + 16 * GUARD), C.byref(r2), None, DEVICE)
            assert st == OK and r2.value == rt
            got = t_out.cpu().numpy()
            assert _guards_intact(got) and _same_bits(got[GUARD:GUARD + count * S].reshape(count, S), base), ("device", width)
            assert np.array_equal(t_lab.cpu().numpy().view(dt), lab) and _same_bits(t_q.cpu().numpy(), _qflat(Q))  # inputs untouched


# ------------------------------------------------------------------ 8. reused workspaces, seeds
@pytest.mark.parametrize("route", ROUTES)
def test_smaller_call_after_a_larger_one_and_other_seeds(pkg, route):
    big, small = "Z3K70", "Z16K5"
    Lb, db = H.instance(big)
    Ls, ds = H.instance(small)
    sb, Qb, refb = H.gaussian_case(big)
    ss, Qs, refs = H.gaussian_case(small)
    with pkg.Context(seed=29, **_kw(route)) as ctx:
        st, fresh, _, _ = _call(ctx, _flat(Ls), Ls.shape[0], ds, ss, Qs, 1, ds)
        assert st == OK and _err(fresh, refs) <= 2e-12 * Ls.shape[0]
        st, fresh_win, _, _ = _call(ctx, _flat(Ls), Ls.shape[0], ds, ss, Qs, ds, 1)
        assert st == OK
    with pkg.Context(seed=30, **_kw(route)) as ctx:  # another seed: the entry draws no random numbers
        st, bigwin, _, buf = _call(ctx, _flat(Lb), Lb.shape[0], db, sb, Qb, 1, db)
        assert st == OK and _guards_intact(buf) and _err(bigwin, refb) <= 2e-12 * Lb.shape[0]
        st, after, _, buf = _call(ctx, _flat(Ls), Ls.shape[0], ds, ss, Qs, 1, ds)
        assert st == OK and _guards_intact(buf)
        assert _same_bits(after, fresh)
        st, after_win, _, buf = _call(ctx, _flat(Ls), Ls.shape[0], ds, ss, Qs, ds, 1)
        assert st == OK and _guards_intact(buf) and _same_bits(after_win, fresh_win)
        st, again, _, _ = _call(ctx, _flat(Lb), Lb.shape[0], db, sb, Qb, 1, db)
        assert st == OK and _same_bits(again, bigwin)


# ------------------------------------------------------------------ 9. the ctx's own block diagonalisations survive
def _diagonalize_complex(pkg, ctx, L, d):
    """sdpsr_block_diagonalize_complex through ctypes, retried as the reference asks ("try again"); (n, d_desym, sizes)."""
    n = L.shape[0]
    lab = _flat(L)
    for _ in range(4):
        dd, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        st = ctx._lib.sdpsr_block_diagonalize_complex(ctx._h, n, _vp(lab), d, pkg.api.RTOL_DEFAULT, None, C.byref(dd), C.byref(nb),
                                                      C.byref(ssq), C.byref(ss), HOST)
        if st == OK:
            return n, dd.value, ssq.value, ss.value
    pytest.fail(f"sdpsr_block_diagonalize_complex failed four times: {ctx._lib.sdpsr_last_error(ctx._h)}")


@pytest.mark.parametrize("route", ["outer", "chunk"])
def test_ctx_state_survives_the_new_entry(pkg, problems, route):
    Lo, do = H.instance("M4K17")
    so, Qo, refo = H.gaussian_case("M4K17")
    Ls3, ds3 = problems.kron_with_complete(H.s3_cayley_labels(), 12, seed=3)  # n = 72: the sorted-entries kernel of the old entry
    with pkg.Context(seed=31, **_kw(route)) as ctx:
        n, dd, S, S1 = _diagonalize_complex(pkg, ctx, np.asarray(Ls3), ds3)
        a, qa = np.empty(dd * S, dtype=np.complex128), np.empty(n * S1, dtype=np.complex128)
        b, qb = np.empty(dd * S, dtype=np.complex128), np.empty(n * S1, dtype=np.complex128)
        assert ctx._lib.sdpsr_block_images_complex(ctx._h, _vp(a), _vp(qa), HOST) == OK
        st, win, rt, buf = _call(ctx, _flat(Lo), Lo.shape[0], do, so, Qo, 2, do - 2)
        assert st == OK and _guards_intact(buf) and _err(win, refo[1:do - 1]) <= 2e-12 * Lo.shape[0]
        assert ctx._lib.sdpsr_block_images_complex(ctx._h, _vp(b), _vp(qb), HOST) == OK
        assert _same_bits(a, b) and _same_bits(qa, qb)
    Lr, dr, _ = problems.known_blocks_instance("K17")
    Lr = np.asarray(Lr, dtype=np.int64)
    nr = Lr.shape[0]
    with pkg.Context(seed=101, basis_image_kernel="outer") as ctx:  # (a forced kernel route: the real shortcuts draw a key per call)
        nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        lab = _flat(Lr)
        for _ in range(4):
            st = ctx._lib.sdpsr_block_diagonalize(ctx._h, nr, _vp(lab), dr, pkg.api.RTOL_DEFAULT, C.byref(nb), C.byref(ssq), C.byref(ss), None, HOST)
            if st == OK:
                break
        assert st == OK
        a, qa = np.empty(dr * ssq.value), np.empty(nr * ss.value)
        b, qb = np.empty(dr * ssq.value), np.empty(nr * ss.value)
        assert ctx._lib.sdpsr_block_images(ctx._h, _vp(a), _vp(qa), None, HOST) == OK
        st, win, rt, buf = _call(ctx, _flat(Lo), Lo.shape[0], do, so, Qo, 1, do)
        assert st == OK and _guards_intact(buf) and _err(win, refo) <= 2e-12 * Lo.shape[0]
        assert ctx._lib.sdpsr_block_images(ctx._h, _vp(b), _vp(qb), None, HOST) == OK
        assert _same_bits(a, b) and _same_bits(qa, qb)


# ------------------------------------------------------------------ 10. the ctx's own Q_hat: the two entries agree
@functools.lru_cache(maxsize=None)
def _own(name):
    """blockDiagonalize(P; complex=true) once per instance: (labels of the desymmetrized partition, d, sizes, Q, blks as rows)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    if name == "S3K12":
        Lm, _ = pkg.problems.kron_with_complete(H.s3_cayley_labels(), 12, seed=3)
    else:
        Lm, _ = H.instance(name)
    with pkg.Context(seed=32) as ctx:
        bd = pkg.blockDiagonalize(pkg.Partition.from_matrix(np.asarray(Lm), ctx=ctx), complex=True, ctx=ctx, retries=3)
    return bd


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["P4", "C3", "S3K12"])
def test_full_range_on_the_ctx_own_q_hat_equals_block_images_complex(pkg, name, route):
    bd = _own(name)
    Ld, d = np.asarray(bd.partition.matrix).astype(np.int64), bd.partition.nparts
    n = Ld.shape[0]
    if name != "S3K12":
        assert sorted(bd.blkSizes) == [1, 1, 1]
    Q = np.concatenate([np.asarray(q) for q in bd.Q_hat], axis=1)
    own = _rows(bd.blks)
    with pkg.Context(seed=33, **_kw(route)) as ctx:
        st, win, rt, buf = _call(ctx, _flat(Ld), n, d, bd.blkSizes, Q, 1, d)
    assert st == OK and _guards_intact(buf)
    err = _err(win, own.astype(np.clongdouble))
    print(f"basis_image_complex own Q_hat {name} {route} route={rt} n={n} d={d} err={err:.3e} bound={2e-12 * n:.3e}")
    assert err <= 2e-12 * n


# ------------------------------------------------------------------ 11. the Python entry
def test_python_entry_numpy_and_torch(pkg, problems):
    import torch
    L, d = H.instance("M4K17")
    n = L.shape[0]
    sizes, Q, ref = H.gaussian_case("M4K17")
    win = pkg.class_window(d, 3, 2)
    blocks, off = [], 0
    for s in sizes:
        blocks.append(Q[:, off:off + s])
        off += s
    want = ref[win[0] - 1:win[0] - 1 + win[1]]
    with pkg.Context(seed=34) as ctx:
        P = pkg.Partition(d, L.astype(np.uint32))
        out, rt = pkg.basis_image(blocks, P, classes=win, ctx=ctx, return_route=True)
        assert len(out) == win[1] and [b.shape for b in out[0]] == [(s, s) for s in sizes] and rt == OUTER
        assert all(b.dtype == np.complex128 for row in out for b in row)
        flat = _rows(out)
        assert _err(flat, want) <= 2e-12 * n
        out2 = pkg.basis_image((np.array(Q), list(sizes)), P, classes=win, ctx=ctx)
        assert _same_bits(_rows(out2), flat)
        out64 = pkg.basis_image([b.astype(np.complex64) for b in blocks], P, classes=win, ctx=ctx)  # complex64 is widened, not refused
        assert out64[0][0].dtype == np.complex128 and _err(_rows(out64), want) <= 1e-5
        assert len(pkg.basis_image(blocks, P, ctx=ctx)) == d
        assert pkg.basis_image(blocks, P, classes=(1, 0), ctx=ctx) == []
        Pt = pkg.Partition(d, torch.from_numpy(L.astype(np.int32)).cuda())
        out3 = pkg.basis_image([torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in blocks], Pt, classes=win, ctx=ctx)
        assert out3[0][0].is_cuda and out3[0][0].dtype == torch.complex128
        assert out3[0][0].untyped_storage().data_ptr() == out3[-1][-1].untyped_storage().data_ptr()  # views of one device tensor
        flat3 = np.array([np.concatenate([b.cpu().numpy().ravel(order="F") for b in row]) for row in out3])
        assert _same_bits(flat3, flat)
        out4 = pkg.basis_image(blocks, Pt, classes=win, ctx=ctx)  # a NumPy Q_hat with a device partition is moved there
        assert out4[0][0].is_cuda and _same_bits(np.array([np.concatenate([b.cpu().numpy().ravel(order="F") for b in row]) for row in out4]), flat)
        # a real Q_hat still reaches the real entry: it refuses this non-symmetric partition, and serves a symmetric one
        with pytest.raises(pkg.SdpsrError, match="not symmetric"):
            pkg.basis_image([b.real.copy() for b in blocks], P, ctx=ctx)
        Lr, dr, _ = problems.known_blocks_instance("DS")
        rq = gaussian_unit_columns(Lr.shape[0], 4, 41)
        outr, rtr = pkg.basis_image((rq, [3, 1]), pkg.Partition(dr, np.asarray(Lr).astype(np.uint32)), ctx=ctx, return_route=True)
        assert outr[0][0].dtype == np.float64 and (rtr & 0xFF) in (1, 2, 3, 4, 5)


# ------------------------------------------------------------------ 12. sdpsr_transfer_bytes
@pytest.mark.parametrize("width", [32, 8])
def test_transfer_bytes(pkg, width):
    import torch
    L, d = H.instance("Z16K5")
    n = L.shape[0]
    sizes, Q, _ = H.gaussian_case("Z16K5")
    S1, S = sum(sizes), sum(s * s for s in sizes)
    first, count = H.class_window(d, 3, 1)
    dt = {8: np.uint8, 32: np.uint32}[width]
    lab = _flat(L, dt)
    with pkg.Context(seed=35, label_width=width) as ctx:
        h0, d0 = ctx.transfer_bytes()
        st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
        h1, d1 = ctx.transfer_bytes()
        assert st == OK
        assert (h1 - h0, d1 - d0) == (n * n * width // 8 + n * S1 * 16, count * S * 16)
        t_lab = torch.from_numpy(lab.view({8: np.uint8, 32: np.int32}[width]).copy()).cuda()
        t_q = torch.from_numpy(_qflat(Q)).cuda()
        t_sz = np.asarray(sizes, dtype=np.int32)
        t_out = torch.empty(count * S, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        h1, d1 = ctx.transfer_bytes()
        st = ctx._lib.sdpsr_basis_image_complex(ctx._h, n, C.c_void_p(t_lab.data_ptr()), d, len(sizes), _vp(t_sz), C.c_void_p(t_q.data_ptr()),
                                                first, count, -1.0, C.c_void_p(t_out.data_ptr()), None, None, DEVICE)
        h2, d2 = ctx.transfer_bytes()
        assert st == OK and (h2 - h1, d2 - d1) == (0, 8)  # nothing up; the two label verdicts down
        assert _same_bits(t_out.cpu().numpy().reshape(count, S), win)
        st = ctx._lib.sdpsr_basis_image_complex(ctx._h, n, _vp(lab), d, len(sizes), _vp(t_sz), _vp(_qflat(Q)), first, 0, -1.0, _vp(buf), None, None, HOST)
        assert st == OK and ctx.transfer_bytes() == (h2, d2)  # an empty window moves nothing


# ------------------------------------------------------------------ 13. pkg.basis_image reproduces bd.blks
@pytest.mark.parametrize("name", ["P4", "C3"])
def test_python_basis_image_reproduces_the_complex_block_diagonalization(pkg, name):
    Lm, _ = H.instance(name)
    with pkg.Context(seed=36) as ctx:
        bd = pkg.blockDiagonalize(pkg.Partition.from_matrix(np.asarray(Lm), ctx=ctx), complex=True, ctx=ctx, retries=3)
        assert sorted(bd.blkSizes) == [1, 1, 1]
        out = pkg.basis_image(bd.Q_hat, bd.partition, ctx=ctx)
    n = Lm.shape[0]
    assert len(out) == bd.partition.nparts and all(b.dtype == np.complex128 and b.shape == (1, 1) for row in out for b in row)
    err = _err(_rows(out), _rows(bd.blks).astype(np.clongdouble))
    print(f"basis_image_complex python {name} err={err:.3e} bound={2e-12 * n:.3e}")
    assert err <= 2e-12 * n
