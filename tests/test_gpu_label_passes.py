"""The integer passes over the packed labels that every round "expected not to refine" runs: the channel
gather in its plain and in its label-writing form, and the verify pass with its table of class representatives built in LDS
(one launch up to a class-count cap) or by a kernel of its own (above the cap).

The kernels are driven on made-up inputs through libsdpsr_prof.so (sdpsr_profile_gather_packed, sdpsr_profile_verify and, for
more than one basis matrix, sdpsr_profile_verify_w and sdpsr_profile_basis_constant); every expectation is a NumPy restatement.
The last test goes through the product ABI: the full label matrix that a gather wrote must be the call's output on every route that claims it valid -- in place in a device buffer filled with garbage, on the
guess, on the deferred guess, and on the wrong guess."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = 0x1234567890ABCDEF
GUARD = 4096  # words behind the n * n labels that the writing gather must leave alone
FILL = 0xA5A5A5A5
CAP = 256  # classes up to which the verify pass keeps its table of representatives in LDS (the entry reports it: checked below)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _col_off(n, j):
    return j * n - j * (j - 1) // 2


def _mirror(n, Lp):
    """Full symmetric matrix of the packed lower triangle (column j at offset j n - j (j - 1) / 2, rows j .. n - 1)."""
    L = np.zeros((n, n), dtype=np.uint32)
    for j in range(n):
        col = Lp[_col_off(n, j):_col_off(n, j) + n - j]
        L[j:, j] = col
        L[j, j:] = col
    return L


def _packed_labels(n, d, rng):
    """Packed labels 0 .. d with every class 1 .. d present where the triangle has room, label 0 included."""
    npk = n * (n + 1) // 2
    Lp = rng.integers(1, d + 1, size=npk).astype(np.uint32)
    Lp[rng.random(npk) < 0.05] = 0
    where = rng.permutation(npk)[:min(d, npk)]
    Lp[where] = np.arange(1, len(where) + 1, dtype=np.uint32)
    if npk > d:
        Lp[np.setdiff1d(np.arange(npk), where)[0]] = 0
    return Lp


# ---------------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 57, 64, 130, 256])
@pytest.mark.parametrize("T", [1, 2, 4])
def test_writing_gather_equals_plain_gather_and_mirrors_the_labels(pkg, gpu_ctx, n, T):
    """ld = 128, 128, 128, 256, 256; 57 and 130 leave ragged tiles (130: a ragged second tile row).  3 classes (the LDS table of
    class bits) and, from n = 64 on, more than GATHER_LUT = 2048 classes (bits hashed per entry)."""
    prof = pkg._lib.load_prof_library()
    ld = -(-n // 128) * 128
    rng = np.random.default_rng(1000 * n + T)
    for d in (3, 2049 + 30):
        if d > 3 and n < 64:
            continue
        Lp = _packed_labels(n, d, rng)
        Lm = _mirror(n, Lp)
        Lfull = np.asfortranarray(Lm).reshape(-1, order="F").copy()
        X = [np.zeros(T * ld * ld, dtype=np.int8) for _ in range(3)]
        Lw = np.full(n * n + GUARD, FILL, dtype=np.uint32)
        gpu_ctx.check(prof.sdpsr_profile_gather_packed(gpu_ctx._h, n, T, d, KEY, _vp(Lp), _vp(Lfull), _vp(X[0]), _vp(X[1]), _vp(X[2]), _vp(Lw),
                                                       GUARD))
        plain, writing, full = X
        assert np.array_equal(writing, plain), (n, T, d)  # byte for byte, padding rows and columns included
        assert np.array_equal(plain, full), (n, T, d)     # = the gather of the mirrored full labels
        Xc = plain.reshape(T, ld, ld)
        assert not Xc[:, n:, :].any() and not Xc[:, :, n:].any()  # (the padding is zero, not the buffer's fill)
        assert Xc[:, :n, :n].any()
        assert np.array_equal(Lw[:n * n].reshape(n, n, order="F"), Lm), (n, T, d)
        assert (Lw[n * n:] == FILL).all(), (n, T, d)


# ---------------------------------------------------------------------------------------------------------------------------
# verify
# ---------------------------------------------------------------------------------------------------------------------------
def _verify_case(n, T, d, rng):
    """Packed labels whose marked places lie in classes of at least two entries, values constant on the classes."""
    npk = n * (n + 1) // 2
    Lp = _packed_labels(n, d, rng)
    # the places a perturbation goes to: the first column, the last row, the diagonal entry of the last column -- each in class 1 or 2
    # together with one more entry, so that the class really splits
    first_col, last_row, last_diag = n // 2, _col_off(n, 3) + (n - 1 - 3), npk - 1
    Lp[first_col] = 1
    Lp[last_row] = min(2, d)
    Lp[last_diag] = 1
    Lp[_col_off(n, 5) + 7] = min(2, d)
    zero_at = _col_off(n, 9) + 11
    Lp[zero_at] = 0
    counts = np.bincount(Lp, minlength=d + 1)
    for l in np.flatnonzero(counts[1:] == 0) + 1:  # (the forced places may have taken a class's only entry)
        e = _col_off(n, 11) + np.flatnonzero((Lp[_col_off(n, 11):npk - 1] > 2) & (counts[Lp[_col_off(n, 11):npk - 1]] > 1))[0]
        counts[Lp[e]] -= 1
        Lp[e] = l
        counts[l] += 1
    first = np.array([np.flatnonzero(Lp == l)[0] for l in range(1, d + 1)], dtype=np.uint32)
    ld = -(-n // 128) * 128
    vals = rng.integers(-2**30, 2**30, size=(T, d + 1)).astype(np.int32)
    vals[:, 0] = 0
    uvals = rng.standard_normal(d + 1)
    uvals[0] = 0.0
    Cm = rng.integers(-2**30, 2**30, size=(T, ld, ld)).astype(np.int32)  # [t][column][row]; what lies outside the lower triangle is noise
    U = np.full((n, n), 12345.0)                                        # [column][row]
    for j in range(n):
        col = Lp[_col_off(n, j):_col_off(n, j) + n - j]
        Cm[:, j, j:n] = vals[:, col]
        U[j, j:] = uvals[col]
    places = {"first_column": first_col, "last_row": last_row, "last_diagonal": last_diag, "label_zero": zero_at}
    return Lp, first, Cm, U, places


def _ij(n, e):
    j = 0
    while _col_off(n, j + 1) <= e:
        j += 1
    return j + e - _col_off(n, j), j


def _expected(n, Lp, first, Cm, U, joint):
    """Does any entry differ from the first entry of its class (label 0: from zero), in packed column-major order?"""
    T = Cm.shape[0]
    cv = np.concatenate([Cm[:, j, j:n] for j in range(n)], axis=1)  # T x packed
    uv = np.concatenate([U[j, j:] for j in range(n)])
    ref_c = np.zeros((T, len(first) + 1), dtype=np.int32)
    ref_u = np.zeros(len(first) + 1)
    ref_c[:, 1:] = cv[:, first]
    ref_u[1:] = uv[first]
    bad = (cv != ref_c[:, Lp]).any()
    if joint:
        bad = bad or (uv != ref_u[Lp]).any()
    return int(bad)


def _run_verify(pkg, ctx, n, T, d, mode, Lp, first, Cm, U, coef=0.75):
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint32 * 2)()
    ctx.check(prof.sdpsr_profile_verify(ctx._h, n, T, d, mode, _vp(Lp), _vp(first), _vp(Cm), _vp(U), coef, KEY, 1e-6, out))
    return int(out[0]), int(out[1])


def test_the_cap_the_cases_are_built_around(pkg, gpu_ctx):
    Lp, first, Cm, U, _ = _verify_case(57, 2, 1, np.random.default_rng(0))
    assert _run_verify(pkg, gpu_ctx, 57, 2, 1, 0, Lp, first, Cm, U)[1] == CAP


@pytest.mark.parametrize("n", [57, 256])
@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("joint", [False, True], ids=["channels", "joint"])
@pytest.mark.parametrize("d", [1, 34, CAP, CAP + 1])
def test_verify_verdict(pkg, gpu_ctx, n, T, joint, d):
    """Verdict 0 on values constant on the classes; 1 when exactly one value is off, at each place where a column walk with
    peeled ends or an LDS table indexed off by one goes wrong."""
    rng = np.random.default_rng(n * 100000 + T * 10000 + d * 10 + joint)
    Lp, first, Cm, U, places = _verify_case(n, T, d, rng)
    mode = 1 if joint else 0
    assert _expected(n, Lp, first, Cm, U, joint) == 0
    assert _run_verify(pkg, gpu_ctx, n, T, d, mode, Lp, first, Cm, U)[0] == 0
    for name, e in places.items():
        i, j = _ij(n, e)
        t = (i + j) % T
        C2 = Cm.copy()
        C2[t, j, i] += 1 if name != "label_zero" else 5
        assert _expected(n, Lp, first, C2, U, joint) == 1, name
        assert _run_verify(pkg, gpu_ctx, n, T, d, mode, Lp, first, C2, U)[0] == 1, (name, i, j, t)
    if joint:
        for name in ("last_row", "label_zero"):
            i, j = _ij(n, places[name])
            U2 = U.copy()
            U2[j, i] += 0.5
            assert _expected(n, Lp, first, Cm, U2, True) == 1
            assert _run_verify(pkg, gpu_ctx, n, T, d, 1, Lp, first, Cm, U2)[0] == 1, (name, i, j)


@pytest.mark.parametrize("d", [1, 34, CAP, CAP + 1])
def test_basis_constant_on_classes_verdict(pkg, gpu_ctx, d):
    """The basis check has the same two forms: 0 for a U that is constant on the classes (0 on label 0), 1 for one entry off."""
    n = 57
    Lp, first, Cm, U, places = _verify_case(n, 2, d, np.random.default_rng(77 + d))
    assert _run_verify(pkg, gpu_ctx, n, 2, d, 2, Lp, first, Cm, U)[0] == 0
    for name, e in places.items():
        i, j = _ij(n, e)
        U2 = U.copy()
        U2[j, i] += 0.5
        assert _expected(n, Lp, first, Cm, U2, True) == 1
        assert _run_verify(pkg, gpu_ctx, n, 2, d, 2, Lp, first, Cm, U2)[0] == 1, (name, i, j)


# ---------------------------------------------------------------------------------------------------------------------------
# the instances of the compare kernel that the cases above do not launch: r basis matrices
# ---------------------------------------------------------------------------------------------------------------------------
COEF = np.array([0.75, -0.5, 1.25, 0.625])  # (a needle of 0.5 in any U_k moves the projected value by far more than the rounding)


def _basis_stack(n, d, r, Lp, rng):
    """r basis matrices [k][column][row], each constant on the classes of Lp and 0 on label 0 (noise above the diagonal)."""
    uvals = rng.standard_normal((r, d + 1))
    uvals[:, 0] = 0.0
    U = np.full((r, n, n), 12345.0)
    for j in range(n):
        U[:, j, j:] = uvals[:, Lp[_col_off(n, j):_col_off(n, j) + n - j]]
    return U


def _expected_stack(n, Lp, first, Cm, U, joint):
    """_expected for a stack of basis matrices: any of them off is off."""
    return int(_expected(n, Lp, first, Cm, U[0], False) or (joint and any(_expected(n, Lp, first, Cm, Uk, True) for Uk in U)))


def _run_step(pkg, ctx, n, T, d, r, Lp, first, Cm, U, width=32):
    """The step check: r = -1 the channels alone, r = 0 .. 4 joint with the first r matrices of U."""
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint32 * 2)()
    U = np.ascontiguousarray(U)
    ctx.check(prof.sdpsr_profile_verify_w(ctx._h, n, T, d, r, width, _vp(Lp), _vp(first), _vp(Cm), _vp(U), _vp(COEF), KEY, 1e-6, out))
    return int(out[0]), int(out[1])


def _run_basis(pkg, ctx, n, d, r, Lp, first, U):
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint32 * 2)()
    U = np.ascontiguousarray(U)
    ctx.check(prof.sdpsr_profile_basis_constant(ctx._h, n, r, d, _vp(Lp), _vp(first), _vp(U), 1e-6, out))
    return int(out[0]), int(out[1])


def _basis_needles(n, r, Lp, first, Cm, U, places, run):
    """One entry of one U_k off at each place, k going round so that every one of the r matrices is hit; run(U) = the GPU's verdict."""
    for idx, (name, e) in enumerate(places.items()):
        i, j = _ij(n, e)
        U2 = U.copy()
        U2[idx % r, j, i] += 0.5
        assert _expected_stack(n, Lp, first, Cm, U2, True) == 1, name
        assert run(U2) == 1, (name, i, j, idx % r)


@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("d", [1, 34, CAP, CAP + 1])
def test_basis_check_of_r_matrices(pkg, gpu_ctx, r, d):
    """Every instance of the basis check, in both forms (table in LDS up to CAP classes, a table kernel above): 0 on matrices that are
    constant on the classes and 0 on label 0; 1 with one entry of one U_k off, each k and each place at least once."""
    n = 57
    rng = np.random.default_rng(9000 + 10 * d + r)
    Lp, first, Cm, _, places = _verify_case(n, 2, d, rng)
    U = _basis_stack(n, d, r, Lp, rng)
    assert len(places) == 4 >= r
    assert _expected_stack(n, Lp, first, Cm, U, True) == 0
    assert _run_basis(pkg, gpu_ctx, n, d, r, Lp, first, U) == (0, CAP)
    _basis_needles(n, r, Lp, first, Cm, U, places, lambda U2: _run_basis(pkg, gpu_ctx, n, d, r, Lp, first, U2)[0])


def test_basis_check_where_a_workgroup_walks_two_columns(pkg, gpu_ctx):
    n, d = 2049, 34  # 2048 workgroups: the first one takes columns 0 and 2048
    rng = np.random.default_rng(2049)
    Lp, first, Cm, _, places = _verify_case(n, 2, d, rng)
    U = _basis_stack(n, d, 1, Lp, rng)
    assert _run_basis(pkg, gpu_ctx, n, d, 1, Lp, first, U)[0] == 0
    _basis_needles(n, 1, Lp, first, Cm, U, places, lambda U2: _run_basis(pkg, gpu_ctx, n, d, 1, Lp, first, U2)[0])


def _step_case(pkg, ctx, n, T, d, r, width, seed):
    """Clean -> 0; one channel entry off -> 1 at each place; r >= 1: one basis entry off -> 1.  The NumPy expectation flips first."""
    rng = np.random.default_rng(seed)
    Lp, first, Cm, _, places = _verify_case(n, T, d, rng)
    assert all(np.count_nonzero(Lp == Lp[e]) >= 2 for name, e in places.items() if name != "label_zero")
    joint = r >= 0
    U = _basis_stack(n, d, max(r, 1), Lp, rng)
    assert _expected_stack(n, Lp, first, Cm, U, joint) == 0
    verdict, cap = _run_step(pkg, ctx, n, T, d, r, Lp, first, Cm, U, width)
    assert verdict == 0
    for name, e in places.items():
        i, j = _ij(n, e)
        t = (i + j) % T
        C2 = Cm.copy()
        C2[t, j, i] += 1 if name != "label_zero" else 5
        assert _expected_stack(n, Lp, first, C2, U, joint) == 1, name
        assert _run_step(pkg, ctx, n, T, d, r, Lp, first, C2, U, width)[0] == 1, (name, i, j, t)
    if r >= 1:
        _basis_needles(n, r, Lp, first, Cm, U, places, lambda U2: _run_step(pkg, ctx, n, T, d, r, Lp, first, Cm, U2, width)[0])
    return cap


@pytest.mark.parametrize("r", [-1, 0, 2, 3, 4], ids=["channels", "joint_r0", "joint_r2", "joint_r3", "joint_r4"])
@pytest.mark.parametrize("T", [2, 4])
def test_two_launch_step_check_of_every_r(pkg, gpu_ctx, T, r):
    """One class above the cap, where a kernel of its own builds the table: the instances that test_verify_verdict (r = 1) leaves out.
    57 * 58 / 2 = 1653 packed entries hold 257 classes with the needle places in classes of two entries or more (_verify_case)."""
    d = CAP + 1
    assert d > _step_case(pkg, gpu_ctx, 57, T, d, r, 32, seed=7000 + 10 * T + r)


@pytest.mark.parametrize("width", [32, 8])
@pytest.mark.parametrize("T", [2, 4])
def test_one_launch_step_check_joint_with_three_matrices(pkg, gpu_ctx, T, width):
    """r = 3 in the one-launch form, at either label width: the only r that no other test launches there."""
    assert 34 <= _step_case(pkg, gpu_ctx, 57, T, 34, 3, width, seed=7300 + 10 * T + width)


# ---------------------------------------------------------------------------------------------------------------------------
# through the ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inst(pkg, problems, golden):
    Lc = golden["circ256_P"].astype(np.int64)
    Lo = golden["er7_P"].astype(np.int64)
    closed = pkg.admissible_setup(*problems.partition_as_sdp(Lc, seed=1))
    other = pkg.admissible_setup(*problems.partition_as_sdp(Lo, seed=1))
    Cv, A, b, Le, dopen = problems.theta_prime_product_problem(problems.cycle_adjacency(16), problems.symmetric_circulant_labels(16), 16, seed=1)
    open_ = pkg.admissible_setup(Cv, A, b)
    assert closed[0] == open_[0] == 256 and other[0] == 57
    return {"circ256": (closed, Lc), "er7": (other, Lo), "open": (open_, Le)}


def _call(pkg, ctx, setup, seed, entry, device):
    """One seeded call with P_out on the host, or in a device buffer that holds garbage when the call starts."""
    import torch
    n, CL, X0L, U = setup
    r = U.shape[1]
    lib, Lm = ctx._lib, pkg._lib
    ctx.set_seed(seed)
    if setup.hint:
        lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    if device:
        keep = [torch.from_numpy(CL).cuda(), torch.from_numpy(X0L).cuda(), torch.from_numpy(np.ascontiguousarray(U.T)).cuda()]
        tP = torch.full((n * n,), 0x5EEDBAD, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        args, pP, mem = [C.c_void_p(t.data_ptr()) for t in keep], C.c_void_p(tP.data_ptr()), Lm.MEM_DEVICE
    else:
        keep = [CL, X0L, np.asfortranarray(U)]
        P = np.full(n * n, 0x5EEDBAD, dtype=np.uint32)
        args, pP, mem = [_vp(a) for a in keep], _vp(P), Lm.MEM_HOST
    dd, it = C.c_int64(0), C.c_int32(0)
    rtol = pkg.api.RTOL_DEFAULT
    if entry == "admissible_subspace":
        ctx.check(lib.sdpsr_admissible_subspace(ctx._h, n, *args, r, rtol, pP, C.byref(dd), C.byref(it), None, mem))
    else:
        nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        st = lib.sdpsr_jordan_reduce(ctx._h, n, *args, r, rtol, rtol, pP, C.byref(dd), C.byref(it), C.byref(nb), C.byref(ssq), C.byref(ss), None, 0,
                                     None, 0, None, mem)
        assert st in (0, 2, 3), st  # (a randomized failure of blockDiagonalize leaves the labels as the loop made them)
    got = tP.cpu().numpy().view(np.uint32) if device else P
    return got.reshape(n, n, order="F"), dd.value


@pytest.mark.parametrize("confirm", [1, 3])
@pytest.mark.parametrize("device", [True, False], ids=["device_P_out", "host_P_out"])
@pytest.mark.parametrize("entry", ["admissible_subspace", "jordan_reduce"])
def test_labels_through_the_abi(pkg, inst, entry, device, confirm):
    """Three seeded calls per closed instance on one ctx (the second and third take the guess; inside sdpsr_jordan_reduce they
    defer the verdicts), then the open instance of the same order on that ctx: the wrong guess, deferred and not."""
    with pkg.Context(seed=1, confirm_rounds=confirm) as ctx:
        for name in ("er7", "circ256"):
            setup, want = inst[name]
            for k in range(3):
                got, dim = _call(pkg, ctx, setup, 7 + k, entry, device)
                assert dim == want.max() and np.array_equal(got, want), (name, k)
        setup, want = inst["open"]
        for k in range(2):  # (the second call has an open input behind it: no guess)
            got, dim = _call(pkg, ctx, setup, 7 + k, entry, device)
            assert dim == want.max() and np.array_equal(got, want), ("open", k)
