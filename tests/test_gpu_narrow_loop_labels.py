"""The 8-bit shadow of the loop's packed labels on the guessed-closed path (csrc/loop.cpp: LoopLabels::Lp8).

A reduction that checks the recorded initial partition instead of rebuilding it refines nothing, so its packed labels are those of
the previous reduction on the ctx; where they fit a byte (<= 255 classes) they are narrowed once and the pair check, the
dot-product pass, the channel gathers and the verify passes stream the bytes.  Only loads change: every result must be the wide
form's bit for bit.

Kernel tests: each consumer through libsdpsr_prof.so at width 32 and 8 on the same made-up symmetric labels (the library's own
narrowing pass makes the bytes), compared bit for bit; packed column offsets take every residue mod 4 over the orders used, which
is what byte addressing adds.  Needles: one changed entry must flip the verdict at width 8 too.  End to end: reductions on one ctx
with and without SDPSR_FLAG_WIDE_LOOP_LABELS give identical outputs and counters, and the narrowing launch happens once per
recorded partition."""
import ctypes as C

import numpy as np
import pytest

import narrow_loop_labels_ref as R
import test_gpu_initial_guess as IG
import test_gpu_verify_pair as VP

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 129, 200, 257]
CLASSES = [1, 34, 255]
KEY = 0x9E3779B97F4A7C15
ATOL = 1e-6
NBLK = 2048  # per-workgroup sums of the dot-product pass, as the loop launches it
BAD_ARGUMENT = 5


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def test_the_orders_cover_every_byte_offset_of_a_packed_column():
    assert {R.col_off(n, j) % 4 for n in SIZES for j in range(n)} == {0, 1, 2, 3}
    for n in (63, 65, 129, 257):  # each of them alone, so that ragged and diagonal tiles meet every residue
        assert {R.col_off(n, j) % 4 for j in range(n)} == {0, 1, 2, 3}, n


def _gather(pkg, ctx, n, T, d, Lp, width, guard=64):
    prof = pkg._lib.load_prof_library()
    ld = -(-n // 128) * 128
    X = [np.zeros(T * ld * ld, dtype=np.int8) for _ in range(2)]
    L = np.full(n * n + guard, 0xABCD1234, dtype=np.uint32)
    ctx.check(prof.sdpsr_profile_gather_packed_w(ctx._h, n, T, d, KEY, width, _vp(Lp), _vp(X[0]), _vp(X[1]), _vp(L), guard))
    return X[0], X[1], L


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("n", SIZES)
def test_gather_gives_the_same_bytes_and_labels_at_either_width(pkg, gpu_ctx, n, T):
    ld = -(-n // 128) * 128
    for d in CLASSES:
        for zero in (False, True):
            Lp, _, de = R.packed_labels(n, d, zero, seed=7 * n + d + zero)
            w = _gather(pkg, gpu_ctx, n, T, de, Lp, 32)
            b = _gather(pkg, gpu_ctx, n, T, de, Lp, 8)
            for x, y in zip(w, b):
                assert np.array_equal(x, y), (n, T, d, zero)
            assert np.array_equal(b[0], b[1])  # the writing form gathers what the plain form gathers
            Xc = b[0].reshape(T, ld, ld)
            assert not Xc[:, n:, :].any() and not Xc[:, :, n:].any()  # padding: zero, all T channels
            assert np.array_equal(b[2][:n * n].reshape(n, n), R.full_from_packed(n, Lp))  # (symmetric: either order)
            assert (b[2][n * n:] == 0xABCD1234).all()


def test_the_byte_forms_refuse_labels_that_do_not_fit(pkg, gpu_ctx):
    prof = pkg._lib.load_prof_library()
    n, T = 65, 2
    Lp, _, d = R.packed_labels(n, 256, False, seed=3)
    assert d == 256
    X = [np.zeros(T * 128 * 128, dtype=np.int8) for _ in range(2)]
    L = np.zeros(n * n, dtype=np.uint32)
    assert prof.sdpsr_profile_gather_packed_w(gpu_ctx._h, n, T, 255, KEY, 8, _vp(Lp), _vp(X[0]), _vp(X[1]), _vp(L), 0) == BAD_ARGUMENT
    assert not X[0].any() and not L.any()  # the narrowing pass found the label; nothing was gathered


@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("n", SIZES)
def test_dot_product_pass_gives_the_same_sums_at_either_width(pkg, gpu_ctx, n, r):
    prof = pkg._lib.load_prof_library()
    for d in CLASSES:
        for zero in (False, True):
            Lp, _, _ = R.packed_labels(n, d, zero, seed=11 * n + d + zero)
            rng = np.random.default_rng(n + r)
            U = rng.standard_normal((r, n, n))
            U = np.ascontiguousarray(U + U.transpose(0, 2, 1))
            got = {}
            for width in (32, 8):
                partial, coef = np.zeros(r * NBLK), np.zeros(r)
                gpu_ctx.check(prof.sdpsr_profile_proj_coef_lower(gpu_ctx._h, n, r, KEY, width, _vp(Lp), _vp(U), _vp(partial), _vp(coef)))
                got[width] = (partial.view(np.uint64), coef.view(np.uint64))
            assert np.array_equal(got[8][0], got[32][0]) and np.array_equal(got[8][1], got[32][1]), (n, r, d, zero)
            assert got[8][0].any() or n == 1  # (the pass ran: some workgroup's sum is not +0.0)


def _verify(pkg, ctx, n, T, d, r, width, Lp, first, Cm, U, coef):
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint32 * 2)()
    ctx.check(prof.sdpsr_profile_verify_w(ctx._h, n, T, d, r, width, _vp(Lp), _vp(first), _vp(Cm), _vp(U), _vp(coef), KEY, ATOL, out))
    return int(out[0])


def _verify_case(pkg, ctx, n, T, d, r, zero):
    """Clean inputs pass at both widths; one changed channel entry -- and, joint, one changed basis entry -- at each place does not."""
    ld = -(-n // 128) * 128
    Lp, first, de = R.packed_labels(n, d, zero, seed=13 * n + d + zero)
    Cm = R.class_constant_channels(n, ld, T, Lp, seed=n + T)
    U, coef = R.class_constant_basis(n, max(r, 0), Lp, seed=n + 5)
    coef = np.where(np.abs(coef) < 0.25, 0.5, coef)  # (a needle in U must move the projected value)
    for width in (32, 8):
        assert _verify(pkg, ctx, n, T, de, r, width, Lp, first, Cm, U, coef) == 0, (n, T, d, r, zero, width)
    for (i, j) in R.needle_places(n, Lp):
        C2 = Cm.copy()
        C2[T - 1, j, i] += 1
        for width in (32, 8):
            assert _verify(pkg, ctx, n, T, de, r, width, Lp, first, C2, U, coef) != 0, (n, T, d, r, zero, width, i, j)
        if r >= 1:
            U2 = U.copy()
            U2[r - 1, j, i] += 0.5
            U2[r - 1, i, j] = U2[r - 1, j, i]
            assert _verify(pkg, ctx, n, T, de, r, 8, Lp, first, Cm, U2, coef) != 0, (n, T, d, r, zero, i, j)


@pytest.mark.parametrize("r", [-1, 0, 1, 2, 4], ids=["channels", "joint_r0", "joint_r1", "joint_r2", "joint_r4"])
@pytest.mark.parametrize("T", [2, 4])
def test_verify_pass_verdicts_and_single_entry_needles(pkg, gpu_ctx, T, r):
    """Every order with one class count and zero-class choice each (rotating, so that all of them occur for every T and r).
    (Joint with r = 2 or 4 and T = 2 the launcher keeps the wide labels at width 8 too -- the byte form would lose a wave per SIMD,
    csrc/kernels_class_compare.hip: launch_verify_rt -- so those cases pin that the choice changes no verdict.)"""
    for k, n in enumerate(SIZES):
        _verify_case(pkg, gpu_ctx, n, T, CLASSES[(k + T + r) % 3], r, zero=(k + r) % 2 == 0)


def test_verify_passes_where_a_workgroup_walks_more_than_one_column(pkg, gpu_ctx):
    n = 2049  # 2048 workgroups: the first one takes columns 0 and 2048
    _verify_case(pkg, gpu_ctx, n, 2, 34, 1, zero=True)


def _pair(pkg, ctx, n, d, width, Lp, first, a, b):
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint32 * 2)()
    af, bf = np.asfortranarray(a), np.asfortranarray(b)
    ctx.check(prof.sdpsr_profile_verify_pair_w(ctx._h, n, d, width, _vp(Lp), _vp(first), _vp(af), _vp(bf), out))
    return int(out[0])


@pytest.mark.parametrize("with_zero", [False, True], ids=["no_zero_class", "zero_class"])
@pytest.mark.parametrize("d", CLASSES)
@pytest.mark.parametrize("n", [57, 256])
def test_pair_check_needles_at_width_8(pkg, gpu_ctx, n, d, with_zero):
    """The cases and the seven needles of test_gpu_verify_pair.py, and a changed entry at each of the places of needle_places."""
    Lp, first, a, b = VP._case(n, d, with_zero, seed=1000 * n + 2 * d + with_zero)
    assert VP._would_reproduce(n, a, b, Lp, first)
    assert _pair(pkg, gpu_ctx, n, d, 8, Lp, first, a, b) == 0 == _pair(pkg, gpu_ctx, n, d, 32, Lp, first, a, b)
    needles = VP._needles(n, d, with_zero, Lp, first, a, b)
    assert len(needles) == 4 + (d >= 2) + 2 * with_zero
    for (i, j) in R.needle_places(n, Lp):
        needles[f"place_{i}_{j}"] = (a, VP._flip(b, i, j))
    for name, (an, bn) in needles.items():
        assert not VP._would_reproduce(n, an, bn, Lp, first), name
        assert _pair(pkg, gpu_ctx, n, d, 8, Lp, first, an, bn) != 0, (n, d, with_zero, name)


@pytest.mark.parametrize("n", SIZES[2:] + [2049])
def test_pair_check_at_every_order(pkg, gpu_ctx, n):
    """Both widths pass the unchanged case and find one flipped bit at each place (n = 2049: more than one column per workgroup)."""
    Lp, first, d, a, b = R.pair_case(n, 34 if n != 127 else 255, n % 2 == 0, seed=n)
    for width in (32, 8):
        assert _pair(pkg, gpu_ctx, n, d, width, Lp, first, a, b) == 0, (n, width)
        for (i, j) in R.needle_places(n, Lp):
            assert _pair(pkg, gpu_ctx, n, d, width, Lp, first, a, VP._flip(b, i, j)) != 0, (n, width, i, j)


# ---- end to end ----
def _narrowings(pkg, ctx, restart=0):
    out = (C.c_uint64 * 1)()
    ctx.check(pkg._lib.load_prof_library().sdpsr_profile_narrow_labels(ctx._h, restart, out))
    return int(out[0])


def _reduce(pkg, ctx, setup, seed):
    n0 = _narrowings(pkg, ctx)
    out = IG._reduce(pkg, ctx, setup, seed)
    out["narrowed"] = _narrowings(pkg, ctx) - n0
    return out


def _same_with_counters(x, y):
    IG._same(x, y)
    for k in ("draws", "squares", "spec", "waits", "taken", "violated"):
        assert x[k] == y[k], (k, x[k], y[k])


@pytest.fixture(scope="module")
def e2e(pkg, problems):
    """order -> (setup of a closed input, its labels): partitions that the loop finds closed in one iteration."""
    out = {}
    for n in (256, 384):
        L, _ = problems.synthetic_jordan_partition(n, seed=3)
        out[n] = (pkg.admissible_setup(*problems.partition_as_sdp(L, seed=1)), L)
    for m in (508, 510):  # symmetric circulant schemes of 255 and 256 classes: the last count that fits a byte, and the first that does not
        L, d = problems.canonical_labels(problems.symmetric_circulant_labels(m))
        assert d == m // 2 + 1
        # (partition_as_sdp draws its d values from ~1000: at this many classes two of them coincide and C_L alone is coarser than L)
        c = np.concatenate([[0.0], 1.0 + np.random.default_rng(m).permutation(d)])
        out[m] = (pkg.admissible_setup(c[L].ravel(order="F"), np.eye(m).ravel(order="F")[None, :], np.array([1.0])), L)
    for s, _ in out.values():
        assert s.hint == 3
    return out


@pytest.mark.parametrize("confirm", [1, 2, 3])
@pytest.mark.parametrize("n", [256, 384])
def test_five_reductions_with_and_without_the_shadow(pkg, e2e, n, confirm):
    setup, L = e2e[n]
    with pkg.Context(seed=12, confirm_rounds=confirm) as ctx:
        a = [_reduce(pkg, ctx, setup, seed=31 + k) for k in range(5)]
    with pkg.Context(seed=12, confirm_rounds=confirm, flags=pkg._lib.FLAG_WIDE_LOOP_LABELS) as ctx:
        b = [_reduce(pkg, ctx, setup, seed=31 + k) for k in range(5)]
    for x, y in zip(a, b):
        assert x["status"] == 0 and np.array_equal(x["P"], L) and x["iterations"] == 1
        _same_with_counters(x, y)
    assert [x["taken"] for x in a] == [0, 1, 1, 1, 1]
    assert [x["narrowed"] for x in a] == [0, 1, 0, 0, 0]  # made once, by the first reduction that takes the guess
    assert [y["narrowed"] for y in b] == [0] * 5


def test_a_changed_entry_drops_the_shadow_and_a_new_record_makes_a_new_one(pkg, e2e):
    setup, L = e2e[256]
    needle = IG._with_needle(pkg, setup)
    with pkg.Context(seed=11) as fresh:
        ref = _reduce(pkg, fresh, needle, seed=83)
    with pkg.Context(seed=12) as ctx:
        _reduce(pkg, ctx, setup, seed=81)
        c2 = _reduce(pkg, ctx, setup, seed=82)
        assert (c2["taken"], c2["narrowed"]) == (1, 1)
        r = _reduce(pkg, ctx, needle, seed=83)  # streams the shadow, finds the entry, repeats without guesses
        assert (r["taken"], r["violated"], r["narrowed"]) == (1, 1, 0)
        IG._same(r, ref)
        c4 = _reduce(pkg, ctx, setup, seed=84)  # no record of this input: rebuilt
        c5 = _reduce(pkg, ctx, setup, seed=85)  # ... which leaves one: guessed, and narrowed anew
        c6 = _reduce(pkg, ctx, setup, seed=86)
    assert [(x["taken"], x["narrowed"]) for x in (c4, c5, c6)] == [(0, 0), (1, 1), (1, 0)]
    for x in (c2, c4, c5, c6):
        assert x["status"] == 0 and np.array_equal(x["P"], L)


def test_an_input_that_is_not_closed_behind_two_closed_ones(pkg, problems, e2e):
    """closed, closed, then an input of the same order that is NOT closed: the pair check (on the shadow) refuses the recorded
    partition, the reduction is repeated without guesses and its loop refines -- reading the wide labels; nothing reads the shadow
    afterwards, and the call leaves no record.  Every call equals the same call under SDPSR_FLAG_WIDE_LOOP_LABELS, counters included."""
    setup, L = e2e[256]
    Cv, A, b, Lo, do = problems.theta_prime_product_problem(problems.cycle_adjacency(16), problems.symmetric_circulant_labels(16), 16, seed=1)
    opened = pkg.admissible_setup(Cv, A, b)
    assert opened[0] == 256 and opened.hint == 3
    with pkg.Context(seed=11) as fresh:
        ref = _reduce(pkg, fresh, opened, seed=73)
    assert ref["status"] == 0 and np.array_equal(ref["P"], Lo) and ref["dim"] == do and ref["iterations"] > 1
    runs = {}
    for flags in (0, pkg._lib.FLAG_WIDE_LOOP_LABELS):
        with pkg.Context(seed=12, flags=flags) as ctx:
            runs[flags] = [_reduce(pkg, ctx, s, seed=71 + k) for k, s in enumerate((setup, setup, opened, setup, setup))]
    a, w = runs[0], runs[pkg._lib.FLAG_WIDE_LOOP_LABELS]
    for x, y in zip(a, w):
        _same_with_counters(x, y)
    IG._same(a[2], ref)
    assert [(x["taken"], x["violated"], x["narrowed"]) for x in a] == [(0, 0, 0), (1, 0, 1), (1, 1, 0), (0, 0, 0), (1, 0, 1)]
    assert [y["narrowed"] for y in w] == [0] * 5


def test_255_classes_take_the_shadow_and_256_the_wide_labels(pkg, e2e):
    for m, narrowed in ((508, [0, 1, 0]), (510, [0, 0, 0])):
        setup, L = e2e[m]
        with pkg.Context(seed=12) as ctx:
            a = [_reduce(pkg, ctx, setup, seed=41 + k) for k in range(3)]
        with pkg.Context(seed=12, flags=pkg._lib.FLAG_WIDE_LOOP_LABELS) as ctx:
            b = [_reduce(pkg, ctx, setup, seed=41 + k) for k in range(3)]
        for x, y in zip(a, b):
            assert x["status"] == 0 and np.array_equal(x["P"], L) and x["dim"] == m // 2 + 1 and x["iterations"] == 1
            _same_with_counters(x, y)
        assert [x["taken"] for x in a] == [0, 1, 1], m  # 256 classes: the guess is taken all the same
        assert [x["narrowed"] for x in a] == narrowed, m


def test_batch_restarts_keep_a_shadow_each(pkg, e2e):
    setup, L = e2e[256]
    n, Rn = 256, 2
    rtol = pkg.api.RTOL_DEFAULT
    res = {}
    for flags in (0, pkg._lib.FLAG_WIDE_LOOP_LABELS):
        with pkg.Context(seed=5, flags=flags) as ctx, pkg.Problem(setup=setup, ctx=ctx) as prob:
            got = []
            for sd_ in ([141, 142], [143, 144], [145, 146]):
                sd = (C.c_uint64 * Rn)(*sd_)
                Ps = [np.zeros(n * n, dtype=np.uint32) for _ in range(Rn)]
                Bs = [np.full(IG.CAP, np.nan) for _ in range(Rn)]
                pP = (C.c_void_p * Rn)(*[a.ctypes.data for a in Ps])
                pb = (C.c_void_p * Rn)(*[a.ctypes.data for a in Bs])
                caps = (C.c_int64 * Rn)(*[IG.CAP] * Rn)
                dd, it, nb = (C.c_int64 * Rn)(), (C.c_int32 * Rn)(), (C.c_int32 * Rn)()
                ssq, ss, st = (C.c_int64 * Rn)(), (C.c_int64 * Rn)(), (C.c_int32 * Rn)()
                ctx.check(ctx._lib.sdpsr_problem_reduce_batch(ctx._h, prob._h, Rn, C.cast(sd, C.c_void_p), rtol, rtol, C.cast(pP, C.c_void_p), dd, it, nb,
                                                              ssq, ss, C.cast(pb, C.c_void_p), caps, st, pkg._lib.MEM_HOST))
                for i in range(Rn):
                    assert st[i] == 0 and np.array_equal(Ps[i].reshape(n, n, order="F"), L)
                    got.append((Ps[i].copy(), dd[i], it[i], nb[i], Bs[i][:dd[i] * ssq[i]].copy(), IG._counts(pkg, ctx, i), _narrowings(pkg, ctx, i)))
            res[flags] = got
    for x, y in zip(res[0], res[pkg._lib.FLAG_WIDE_LOOP_LABELS]):
        assert np.array_equal(x[0], y[0]) and x[1:4] == y[1:4] and np.array_equal(x[4], y[4])
        assert x[5][:3] == y[5][:3] and x[5][4:] == y[5][4:]  # draws, squares, speculative squares, guesses (host waits are the batch's)
    assert [g[6] for g in res[0]] == [0, 0, 1, 1, 1, 1]  # running totals per restart: made in the second batch, kept in the third
    assert [g[6] for g in res[pkg._lib.FLAG_WIDE_LOOP_LABELS]] == [0] * 6
