"""sdpsr_basis_image: basis_image(Q, P; atol) (src/diagonalize.jl:64-89) of a caller's Q_hat for a window of classes.
The reference is the projection formula in np.longdouble over the entries of each class (tests/basis_image_helpers.py).
The bound is the project's 2e-12 n: both sides zero entries below atol = 1e-12 n, so an entry may differ by atol; fp64
rounding is orders of magnitude below (for the arbitrary Q, unit-norm columns: sum |q_a[r]| |q_b[c]| <= n as for
orthonormal ones; tests/test_basis_image_window_cpu.py checks the fp64 evaluation against a tenth of the bound)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from basis_image_helpers import class_window, gaussian_unit_columns, reference_images

pytestmark = pytest.mark.gpu

OK, BAD_ARGUMENT = 0, 5
HOST, DEVICE = 0, 1
COMMUTATIVE, BLOCKS, TWO_STAGE, OUTER, CHUNK, REPAIRED, REFUSED = 1, 2, 3, 4, 5, 0x100, 0x200
ROUTE_OF = {"two_stage": TWO_STAGE, "outer": OUTER, "chunk": CHUNK}
FORCED = ["two_stage", "outer", "chunk"]
FULL = 1 << 10  # SDPSR_FLAG_FULL_BASIS_IMAGE
SEEDS = (101, 102, 103)  # blockDiagonalize fails at random as the reference does: the next seed then
GUARD = 5


def _kw(route):
    return {"auto": {}, "auto_full": {"flags": FULL}}.get(route, {"basis_image_kernel": route})


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _flat(L, dtype=np.uint32):
    return np.ascontiguousarray(np.asarray(L).ravel(order="F").astype(dtype))


def _call(ctx, lab, n, d, sizes, Q, first, count, atol=-1.0):
    """The C entry on host arrays; the output sits between GUARD NaNs on either side.
    Returns (status, window as count x S or None, route, whole buffer)."""
    sz = np.asarray(sizes, dtype=np.int32)
    S = int(sum(int(s) * int(s) for s in sizes))
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64).ravel(order="F"))
    buf = np.full(2 * GUARD + max(count, 0) * S, np.nan)
    route = C.c_int32(-1)
    st = ctx._lib.sdpsr_basis_image(ctx._h, n, _vp(lab), d, len(sz), _vp(sz), _vp(q), first, count, atol,
                                    C.c_void_p(buf.ctypes.data + 8 * GUARD), C.byref(route), None, HOST)
    win = buf[GUARD:GUARD + count * S].reshape(count, S) if st == OK and count >= 0 else None
    return st, win, route.value, buf


def _guards_intact(buf):
    return bool(np.isnan(buf[:GUARD]).all() and np.isnan(buf[len(buf) - GUARD:]).all())


def _err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max()) if got.size else 0.0


@functools.lru_cache(maxsize=None)
def _instance(name):
    from __graft_entry__ import load_package
    pr = load_package().problems
    if name == "COMM":  # commutative: eighteen 1 x 1 blocks, n = 80
        L, d = pr.kron_with_complete(pr.symmetric_circulant_labels(16), 5)
    elif name == "BIG":  # n = 248, d = 15 500: the class tables of two_stage do not fit LDS at full range
        L, d = pr.kron_with_complete(pr.sym_full_labels(124), 2)
    else:
        L, d, _ = pr.known_blocks_instance(name)
    return np.asarray(L, dtype=np.int64), int(d)


@functools.lru_cache(maxsize=None)
def _own(name, route="two_stage"):
    """(seed, sizes, Q matrix, blks as d x S) of blockDiagonalize on a fresh Context(seed, route): the library's own Q_hat."""
    from __graft_entry__ import load_package
    pkg = load_package()
    L, d = _instance(name)
    P = pkg.Partition(d, L.astype(np.uint32))
    for seed in SEEDS:
        try:
            with pkg.Context(seed=seed, **_kw(route)) as ctx:
                bd = pkg.blockDiagonalize(P, ctx=ctx)
        except (pkg.NumericalInconsistency, pkg.DimensionMismatch):
            continue
        Q = np.concatenate([np.asarray(q) for q in bd.Q_hat], axis=1)
        blks = np.array([np.concatenate([b.ravel(order="F") for b in row]) for row in bd.blks])
        return seed, tuple(bd.blkSizes), Q, blks
    pytest.fail(f"blockDiagonalize failed on every seed of {SEEDS} ({name}, {route})")


@functools.lru_cache(maxsize=None)
def _ref(name, qkind):
    """The longdouble reference, once per (labels, Q).  qkind: "own" or (sizes, seed) of a Gaussian Q."""
    L, d = _instance(name)
    if qkind == "own":
        _, sizes, Q, _ = _own(name)
    else:
        sizes, Q = qkind[0], gaussian_unit_columns(L.shape[0], sum(qkind[0]), qkind[1])
    ref = reference_images(L, d, Q, sizes)
    ref.setflags(write=False)
    return sizes, Q, ref


# ------------------------------------------------------------------ 1. full range == sdpsr_block_images
@pytest.mark.parametrize("route", FORCED + ["auto", "auto_full"])
@pytest.mark.parametrize("name", ["K17", "DS"])
def test_full_range_equals_block_images(pkg, name, route):
    L, d = _instance(name)
    n = L.shape[0]
    seed, sizes, Q, blks = _own(name, route)
    with pkg.Context(seed=seed, **_kw(route)) as ctx:
        bd = pkg.blockDiagonalize(pkg.Partition(d, L.astype(np.uint32)), ctx=ctx)  # same seed: the same Q_hat and images
        own = np.array([np.concatenate([b.ravel(order="F") for b in row]) for row in bd.blks])
        assert np.array_equal(own, blks)
        st, win, rt, buf = _call(ctx, _flat(L), n, d, sizes, Q, 1, d)
    assert st == OK and _guards_intact(buf)
    if route in FORCED:
        assert rt == ROUTE_OF[route]
        assert np.array_equal(win, blks), (name, route)
    else:
        err = _err(win, blks.astype(np.longdouble))
        print(f"basis_image_entry full {name} {route} route={rt:#x} err={err:.3e} bound={2e-12 * n:.3e}")
        assert err <= 2e-12 * n
        if route == "auto_full":
            assert rt in (TWO_STAGE, OUTER, CHUNK)


# ------------------------------------------------------------------ 2. windows
def _windows(L, d):
    counts = np.bincount(L.ravel(), minlength=d + 1)
    single = [int(i) for i in range(1, d + 1) if counts[i] == 1][:1]
    return [(1, 1), (d, 1)] + [(i, 1) for i in single] + [(2, d - 2)] + [class_window(d, 3, j) for j in range(3)]


@pytest.mark.parametrize("route", FORCED + ["auto"])
@pytest.mark.parametrize("name", ["DS", "K2"])
def test_windows_equal_the_slice_of_the_full_call(pkg, name, route):
    L, d = _instance(name)
    n = L.shape[0]
    sizes, Q, ref = _ref(name, "own")
    lab = _flat(L)
    wins = _windows(L, d)
    if name == "DS":
        assert len(wins) == 7 and (166, 1) in wins  # DS has a class of a single entry
    with pkg.Context(seed=5, **_kw(route)) as ctx:
        st, full, rt_full, buf = _call(ctx, lab, n, d, sizes, Q, 1, d)
        assert st == OK and _guards_intact(buf)
        assert _err(full, ref) <= 2e-12 * n
        for first, count in wins:
            st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
            assert st == OK, (first, count, ctx._lib.sdpsr_last_error(ctx._h))
            assert _guards_intact(buf), (name, route, first, count)
            assert not np.isnan(win).any()
            if route in FORCED:
                assert rt == ROUTE_OF[route]
                assert np.array_equal(win, full[first - 1:first - 1 + count]), (name, route, first, count)
            else:
                err = _err(win, ref[first - 1:first - 1 + count])
                print(f"basis_image_entry window {name} ({first},{count}) route={rt:#x} err={err:.3e}")
                assert err <= 2e-12 * n, (name, first, count, err)


# ------------------------------------------------------------------ 3. stale workspaces
@pytest.mark.parametrize("name,route", [("DS", "two_stage"), ("K2", "auto"), ("COMM", "auto")])
def test_reused_workspaces_after_a_larger_call(pkg, name, route):
    """bi_T and the class-sum workspaces are reused: after the full call the window (d, 1), then (1, 1) -- rows without
    an entry in the window must contribute zeros, not what the larger call left there."""
    L, d = _instance(name)
    n = L.shape[0]
    sizes, Q, ref = _ref(name, "own")
    lab = _flat(L)
    with pkg.Context(seed=6, **_kw(route)) as ctx:
        for first, count in [(1, d), (d, 1), (1, 1)]:
            st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
            assert st == OK and _guards_intact(buf)
            err = _err(win, ref[first - 1:first - 1 + count])
            assert err <= 2e-12 * n, (name, route, first, count, err)


# ------------------------------------------------------------------ 4. arbitrary Q
@pytest.mark.parametrize("route", FORCED + ["auto"])
@pytest.mark.parametrize("sizes", [(3, 1, 5), (2, 2)])
def test_arbitrary_q(pkg, sizes, route):
    """Unit-norm Gaussian columns on DS: sum s_k = 9 is odd (the VEC = 1 rows kernel), 4 is even (VEC = 2).  One entry of
    Q is set to 1e-7 in the row of DS's single-entry class, so that class's image of the first 1-column (or the (0, 0)
    entry of the first block) is 1e-14 < 1e-12 n: atol = 0 must leave it, atol < 0 must clamp it."""
    L, d = _instance("DS")
    n = L.shape[0]
    _, Q0, _ = _ref("DS", (sizes, 41))
    counts = np.bincount(L.ravel(), minlength=d + 1)
    cls = int(np.flatnonzero(counts[1:] == 1)[0]) + 1
    r = int(np.argwhere(L == cls)[0][0])
    k = sizes.index(1) if 1 in sizes else 0  # the 1 x 1 block where there is one, else entry (0, 0) of the first block
    col, off = sum(sizes[:k]), sum(s * s for s in sizes[:k])
    Q = Q0.copy()
    Q[r, col] = 1e-7
    ref = reference_images(L, d, Q, sizes)
    assert abs(float(ref[cls - 1, off]) - 1e-14) < 1e-20
    lab = _flat(L)
    with pkg.Context(seed=7, **_kw(route)) as ctx:
        st, raw, rt, buf = _call(ctx, lab, n, d, sizes, Q, 1, d, atol=0.0)
        assert st == OK and _guards_intact(buf)
        st, clamped, rt2, buf = _call(ctx, lab, n, d, sizes, Q, 1, d, atol=-1.0)
        assert st == OK and _guards_intact(buf)
    if route in FORCED:
        assert rt == rt2 == ROUTE_OF[route]
    e0, e1 = _err(raw, ref), _err(clamped, ref)
    print(f"basis_image_entry arbitrary Q sizes={sizes} {route} route={rt:#x} err(atol=0)={e0:.3e} err(default)={e1:.3e} bound={2e-12 * n:.3e}")
    assert e0 <= 2e-12 * n and e1 <= 2e-12 * n
    assert raw[cls - 1, off] != 0.0 and abs(raw[cls - 1, off] - 1e-14) < 1e-20
    assert clamped[cls - 1, off] == 0.0
    assert not np.any((clamped != 0.0) & (np.abs(clamped) < 1e-12 * n))


# ------------------------------------------------------------------ 5. a window makes two_stage fit
def test_a_window_makes_two_stage_fit(pkg):
    L, d = _instance("BIG")
    n = L.shape[0]
    assert (n, d) == (248, 15500)
    sizes, Q, ref = _ref("BIG", ((3, 2), 43))
    lab = _flat(L)
    wins = [(1, 4000), (4001, 4000), (8001, 4000), (12001, 3500)]
    with pkg.Context(seed=8, basis_image_kernel="two_stage") as ctx:
        st, full, rt, buf = _call(ctx, lab, n, d, sizes, Q, 1, d)
        assert st == OK and _guards_intact(buf)
        assert rt == OUTER  # not TWO_STAGE: 2 (d + 2) * 4 + 2 n bytes of tables exceed the 60 KiB of basis_image_two_stage_fits
        assert _err(full, ref) <= 2e-12 * n
        for first, count in wins:
            st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
            assert st == OK and _guards_intact(buf) and rt == TWO_STAGE, (first, count, rt)
            assert _err(win, ref[first - 1:first - 1 + count]) <= 2e-12 * n, (first, count)
    with pkg.Context(seed=8, basis_image_kernel="outer") as ctx:
        for first, count in wins:
            st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
            assert st == OK and _guards_intact(buf) and rt == OUTER, (first, count, rt)
            assert np.array_equal(win, full[first - 1:first - 1 + count]), (first, count)  # the full call ran `outer` too


# ------------------------------------------------------------------ 6. shortcuts taken and refused
def _run_auto(pkg, name, sizes, Q, flags=0, seed=9):
    L, d = _instance(name)
    n = L.shape[0]
    with pkg.Context(seed=seed, flags=flags) as ctx:
        st, win, rt, buf = _call(ctx, _flat(L), n, d, sizes, Q, 1, d)
    assert st == OK and _guards_intact(buf)
    return win, rt, _err(win, reference_images(L, d, Q, sizes)), 2e-12 * n


def test_commutative_shortcut_taken_repaired_refused(pkg):
    _, sizes, Q, _ = _own("COMM", "auto")
    assert sizes == (1,) * 18
    win, rt, err, bound = _run_auto(pkg, "COMM", sizes, Q)
    assert rt in (COMMUTATIVE, COMMUTATIVE | REPAIRED) and err <= bound, (hex(rt), err)
    mixed = Q.copy()  # two columns of different irreducibles mixed: q_a' A_i q_b = (lambda_1 - lambda_2) / 2
    mixed[:, 0], mixed[:, 1] = (Q[:, 0] + Q[:, 1]) / math.sqrt(2), (Q[:, 0] - Q[:, 1]) / math.sqrt(2)
    win, rt, err, bound = _run_auto(pkg, "COMM", sizes, mixed)
    assert rt & (REPAIRED | REFUSED) and err <= bound, (hex(rt), err)
    rnd = gaussian_unit_columns(Q.shape[0], 18, 44)
    win, rt, err, bound = _run_auto(pkg, "COMM", sizes, rnd)
    assert rt & REFUSED and (rt & 0xFF) in (TWO_STAGE, OUTER, CHUNK) and err <= bound, (hex(rt), err)
    for q in (Q, mixed, rnd):
        win, rt, err, bound = _run_auto(pkg, "COMM", sizes, q, flags=FULL)
        assert rt in (TWO_STAGE, OUTER, CHUNK) and err <= bound, (hex(rt), err)


def test_blocks_shortcut_taken_and_refused(pkg):
    _, sizes, Q, _ = _own("K2", "auto")
    assert sizes == (2, 2)
    win, rt, err, bound = _run_auto(pkg, "K2", sizes, Q)
    assert rt == BLOCKS and err <= bound, (hex(rt), err)
    swapped = Q.copy()  # one column of each block swapped: neither block spans an invariant subspace any more
    swapped[:, 1], swapped[:, 3] = Q[:, 3], Q[:, 1]
    win, rt, err, bound = _run_auto(pkg, "K2", sizes, swapped)
    assert rt != BLOCKS and err <= bound, (hex(rt), err)
    for q in (Q, swapped):
        win, rt, err, bound = _run_auto(pkg, "K2", sizes, q, flags=FULL)
        assert rt in (TWO_STAGE, OUTER, CHUNK) and err <= bound, (hex(rt), err)


# ------------------------------------------------------------------ 7. label widths and memory spaces
@pytest.mark.parametrize("bits", [8, 16])
def test_label_widths_and_memory_spaces(pkg, bits):
    import torch
    L, d = _instance("DS")
    n = L.shape[0]
    sizes, Q, ref = _ref("DS", "own")
    S1, S = sum(sizes), sum(s * s for s in sizes)
    first, count = class_window(d, 3, 1)
    with pkg.Context(seed=10, basis_image_kernel="two_stage") as ctx:
        st, base, _, _ = _call(ctx, _flat(L), n, d, sizes, Q, first, count)
        assert st == OK
    assert _err(base, ref[first - 1:first - 1 + count]) <= 2e-12 * n
    for width in (32, bits):
        dt = {8: np.uint8, 16: np.uint16, 32: np.uint32}[width]
        lab = _flat(L, dt)
        with pkg.Context(seed=10, basis_image_kernel="two_stage", label_width=width) as ctx:
            h0, d0 = ctx.transfer_bytes()
            st, win, rt, buf = _call(ctx, lab, n, d, sizes, Q, first, count)
            h1, d1 = ctx.transfer_bytes()
            assert st == OK and rt == TWO_STAGE and _guards_intact(buf)
            assert np.array_equal(win, base), width
            assert (h1 - h0, d1 - d0) == (n * n * width // 8 + n * S1 * 8, count * S * 8), width
            # device arrays
            t_lab = torch.from_numpy(lab.view({8: np.uint8, 16: np.int16, 32: np.int32}[width]).copy()).cuda()
            t_q = torch.from_numpy(np.ascontiguousarray(Q.ravel(order="F"))).cuda()
            t_sz = np.asarray(sizes, dtype=np.int32)
            t_out = torch.full((2 * GUARD + count * S,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            route = C.c_int32(-1)
            h1, d1 = ctx.transfer_bytes()
            st = ctx._lib.sdpsr_basis_image(ctx._h, n, C.c_void_p(t_lab.data_ptr()), d, len(sizes), _vp(t_sz), C.c_void_p(t_q.data_ptr()),
                                            first, count, -1.0, C.c_void_p(t_out.data_ptr() + 8 * GUARD), C.byref(route), None, DEVICE)
            h2, d2 = ctx.transfer_bytes()
            assert st == OK and route.value == TWO_STAGE
            got = t_out.cpu().numpy()
            assert _guards_intact(got) and np.array_equal(got[GUARD:GUARD + count * S].reshape(count, S), base), width
            assert h2 - h1 == 0 and 0 < d2 - d1 <= 64, (width, h2 - h1, d2 - d1)  # nothing up; the verdict words down
            assert np.array_equal(t_lab.cpu().numpy().view(dt), lab)  # inputs untouched


def test_python_entry_host_and_torch(pkg):
    import torch
    L, d = _instance("DS")
    n = L.shape[0]
    sizes, Q, ref = _ref("DS", "own")
    win = pkg.class_window(d, 3, 2)
    blocks, off = [], 0
    for s in sizes:
        blocks.append(Q[:, off:off + s])
        off += s
    want = ref[win[0] - 1:win[0] - 1 + win[1]]
    with pkg.Context(seed=11) as ctx:
        P = pkg.Partition(d, L.astype(np.uint32))
        out, rt = pkg.basis_image(blocks, P, classes=win, ctx=ctx, return_route=True)
        assert len(out) == win[1] and [b.shape for b in out[0]] == [(s, s) for s in sizes] and (rt & 0xFF) in (1, 2, 3, 4, 5)
        flat = np.array([np.concatenate([b.ravel(order="F") for b in row]) for row in out])
        assert _err(flat, want) <= 2e-12 * n
        out2 = pkg.basis_image((Q, list(sizes)), P, classes=win, ctx=ctx)
        assert np.array_equal(np.array([np.concatenate([b.ravel(order="F") for b in row]) for row in out2]), flat)
        assert len(pkg.basis_image(blocks, P, ctx=ctx)) == d
        assert pkg.basis_image(blocks, P, classes=(1, 0), ctx=ctx) == []
        Pt = pkg.Partition(d, torch.from_numpy(L.astype(np.int32)).cuda())
        out3 = pkg.basis_image([torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in blocks], Pt, classes=win, ctx=ctx)
        assert out3[0][0].is_cuda
        flat3 = np.array([np.concatenate([b.cpu().numpy().ravel(order="F") for b in row]) for row in out3])
        assert np.array_equal(flat3, flat)


# ------------------------------------------------------------------ 8. the ctx's own block diagonalisation survives
@pytest.mark.parametrize("route", ["two_stage", "outer"])
def test_ctx_state_survives_an_interleaved_call(pkg, route):
    L, d = _instance("K17")
    n = L.shape[0]
    seed, sizes, _, _ = _own("K17", route)
    S1, S = sum(sizes), sum(s * s for s in sizes)
    Ld, dd = _instance("DS")
    rsizes, RQ, rref = _ref("DS", ((3, 1, 5), 41))
    results = []
    for interleave in (False, True):
        with pkg.Context(seed=seed, **_kw(route)) as ctx:
            nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
            lab = _flat(L)
            assert ctx._lib.sdpsr_block_diagonalize(ctx._h, n, _vp(lab), d, pkg.api.RTOL_DEFAULT, C.byref(nb), C.byref(ssq), C.byref(ss), None, HOST) == OK
            assert (nb.value, ssq.value, ss.value) == (len(sizes), S, S1)
            if interleave:
                st, win, rt, buf = _call(ctx, _flat(Ld), Ld.shape[0], dd, rsizes, RQ, 2, dd - 2)
                assert st == OK and _guards_intact(buf) and _err(win, rref[1:dd - 1]) <= 2e-12 * Ld.shape[0]
            blks, qh, qh2 = np.empty(d * S), np.empty(n * S1), np.empty(n * S1)
            szs = np.zeros(len(sizes), dtype=np.int32)
            assert ctx._lib.sdpsr_block_images(ctx._h, _vp(blks), _vp(qh), None, HOST) == OK
            assert ctx._lib.sdpsr_q_hat(ctx._h, _vp(qh2), HOST) == OK
            assert ctx._lib.sdpsr_block_sizes(ctx._h, _vp(szs)) == OK
            results.append((blks, qh, qh2, szs))
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert np.array_equal(results[0][1], results[0][2])


# ------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_output_and_the_ctx_alone(pkg):
    L, d = _instance("DS")
    n = L.shape[0]
    sizes, Q, ref = _ref("DS", ((3, 1, 5), 41))
    lab = _flat(L)
    S = sum(s * s for s in sizes)
    notsym = lab.copy()
    notsym[1 + 0 * n] = notsym[1] % d + 1  # entry (1, 0) changed, (0, 1) not
    assert notsym.reshape(n, n)[0, 1] != notsym.reshape(n, n)[1, 0]

    def beyond(v):
        b = lab.copy().reshape(n, n)
        b[n - 1, 2] = b[2, n - 1] = v
        return b.ravel()

    cases = [("class_first = 0", dict(first=0), "window"),
             ("window end d + 1", dict(first=d, count=2), "window"),
             ("class_count = -1", dict(count=-1), "class_count"),
             ("s_k = 0", dict(sizes=(3, 0, 5)), "block size"),
             ("sum s_k = n + 1", dict(sizes=(n - 3, 4), Q=np.zeros((n, n + 1))), "more than n"),
             ("nblocks = 0", dict(nblocks=0), "nblocks"),
             ("NULL Q_hat", dict(null="Q"), "null pointer"),
             ("NULL P", dict(null="P"), "null pointer"),
             ("NULL blks", dict(null="blks"), "null pointer"),
             ("NULL blk_sizes", dict(null="sizes"), "null pointer"),
             ("not symmetric", dict(lab=notsym), "partition is not symmetric"),
             ("label d + 1", dict(lab=beyond(d + 1)), "a label exceeds d"),
             ("label 2^32 - 1", dict(lab=beyond(0xFFFFFFFF)), "a label exceeds d")]
    for route in ["two_stage", "outer", "chunk", "auto"]:
        with pkg.Context(seed=12, **_kw(route)) as ctx:
            for what, kw, msg in cases:
                if route != "two_stage" and "label" not in what and what != "not symmetric":
                    continue  # the argument checks run before any route is chosen: once is enough
                szs = np.asarray(kw.get("sizes", sizes), dtype=np.int32)
                q = np.ascontiguousarray(np.asarray(kw.get("Q", Q), dtype=np.float64).ravel(order="F"))
                la = kw.get("lab", lab)
                first, count = kw.get("first", 1), kw.get("count", d)
                buf = np.full(2 * GUARD + d * S, -7.25)
                null = kw.get("null")
                st = ctx._lib.sdpsr_basis_image(ctx._h, n, None if null == "P" else _vp(la), d, kw.get("nblocks", len(szs)),
                                                None if null == "sizes" else _vp(szs), None if null == "Q" else _vp(q), first, count, -1.0,
                                                None if null == "blks" else C.c_void_p(buf.ctypes.data + 8 * GUARD), None, None, HOST)
                err = ctx._lib.sdpsr_last_error(ctx._h).decode()
                assert st == BAD_ARGUMENT and msg in err, (route, what, st, err)
                assert np.all(buf == -7.25), (route, what)
                st, win, rt, b2 = _call(ctx, lab, n, d, sizes, Q, 3, 4)  # the ctx is usable
                assert st == OK and _guards_intact(b2) and _err(win, ref[2:6]) <= 2e-12 * n, (route, what)
            buf = np.full(2 * GUARD, -7.25)
            rt = C.c_int32(-1)
            szs = np.asarray(sizes, dtype=np.int32)
            q = np.ascontiguousarray(Q.ravel(order="F"))
            for first in (1, d, d + 5, 0):  # an empty window: OK wherever it "starts", nothing touched
                assert ctx._lib.sdpsr_basis_image(ctx._h, n, _vp(lab), d, len(szs), _vp(szs), _vp(q), first, 0, -1.0,
                                                  C.c_void_p(buf.ctypes.data + 8 * GUARD), C.byref(rt), None, HOST) == OK
                assert np.all(buf == -7.25)
