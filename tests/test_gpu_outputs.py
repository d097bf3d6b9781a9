"""The two outputs a caller hands to its SDP solver, entry by entry: the block images of sdpsr_block_images on every
basis_image route, and A * PMat of sdpsr_reduce_constraints.  The instances have blocks known by construction
(tests/problems.py, known_blocks_instance); references are formed on the host in extended or integer arithmetic."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, SOLVER_ERROR = 5, 7

# ------------------------------------------------------------------ basis_image
ROUTES = [("two_stage", {"basis_image_kernel": "two_stage"}),
          ("outer", {"basis_image_kernel": "outer"}),
          ("chunk", {"basis_image_kernel": "chunk"}),
          ("auto", {}),
          ("auto_full", {"flags": 1 << 10})]  # SDPSR_FLAG_FULL_BASIS_IMAGE: no shortcut, projection formula for everything
SEEDS = (101, 102, 103)  # blockDiagonalize fails at random as the reference does: the next seed then, three at the most


def _block_diagonalize(pkg, P, seeds, **ctx_kw):
    """blockDiagonalize on a fresh Context(seed) for the first of ``seeds`` that does not end in the reference's
    randomized failure (NumericalInconsistency / DimensionMismatch, "try again"); anything else propagates."""
    for seed in seeds:
        try:
            with pkg.Context(seed=seed, **ctx_kw) as ctx:
                return seed, pkg.blockDiagonalize(P, ctx=ctx)
        except (pkg.NumericalInconsistency, pkg.DimensionMismatch):
            continue
    pytest.fail(f"blockDiagonalize failed on every seed of {seeds} ({ctx_kw})")


def _reference_images(L, d, Q_hat):
    """ref[i][k] = Q_k' 1[P == i + 1] Q_k in np.longdouble, not clamped: per class, the entries (r, c) of the class
    as the product Q_k[r, :]' Q_k[c, :] summed over the class."""
    n = L.shape[0]
    flat = L.ravel(order="F")
    order = np.argsort(flat, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=d + 1))])
    rows, cols = order % n, order // n
    Ql = [np.asarray(q, dtype=np.longdouble) for q in Q_hat]
    ref = []
    for i in range(1, d + 1):
        r, c = rows[ptr[i]:ptr[i + 1]], cols[ptr[i]:ptr[i + 1]]
        ref.append([q[r].T @ q[c] for q in Ql])
    return ref


def _max_abs_diff(a, b):
    """Largest |a[i][k] - b[i][k]| over every class i and every block k (nothing sampled)."""
    worst = 0.0
    for ai, bi in zip(a, b):
        for x, y in zip(ai, bi):
            assert x.shape == y.shape
            worst = max(worst, float(np.abs(np.asarray(x, dtype=np.longdouble) - y).max()))
    return worst


def _check_run(bd, L, d, blocks, ref=None):
    """Block sizes, orthonormal Q_hat, and EVERY class and block against the host reference.
    Bound 2e-12 n: the library and the reference both zero entries below atol = 1e-12 n (src/diagonalize.jl:67), so an
    entry may legitimately differ by atol; the fp64 rounding of a sum over at most n^2 products of entries of
    orthonormal columns is orders of magnitude below that."""
    n = L.shape[0]
    assert sorted(bd.blkSizes) == blocks
    assert len(bd.blks) == d and all(len(row) == len(blocks) for row in bd.blks)
    for q, s in zip(bd.Q_hat, bd.blkSizes):
        q = np.asarray(q)
        assert q.shape == (n, s)
        assert np.abs(q.T @ q - np.eye(s)).max() < 1e-7
    if ref is None:
        ref = _reference_images(L, d, bd.Q_hat)
    err = _max_abs_diff(bd.blks, ref)
    return ref, err


@pytest.mark.parametrize("name", ["K17", "K2", "K40", "DS"])
def test_block_images_on_every_route(pkg, problems, name):
    """blks[i][k] == Q_k' 1[P==i] Q_k for every class and block, through the three forced kernels, the automatic
    choice (K2: the four-vector shortcut for blocks <= 3 x 3; the others: two_stage) and the automatic choice under
    SDPSR_FLAG_FULL_BASIS_IMAGE.  Blocks wider than one 16-wide MFMA tile (17, and 40 = 2 * 16 + 8 in `outer`'s
    MFMA form), classes of 9 900 and 19 800 entries (3 and 5 chunks of 4096 in `chunk`, the last one ragged), a class
    of one entry, label 0 next to large blocks and blocks of different sizes in one call (DS).
    One Context seed for all five routes: they diagonalise identically, so Q_hat is the same array bit for bit and
    the five images agree with each other to the same bound."""
    L, d, blocks = problems.known_blocks_instance(name)
    n = L.shape[0]
    P = pkg.Partition(d, L.astype(np.uint32))
    bound = 2e-12 * n
    seed, first, ref, runs = None, None, None, {}
    for route, kw in ROUTES:
        seed, bd = _block_diagonalize(pkg, P, SEEDS if seed is None else (seed,), **kw)
        if first is None:
            first = bd
        else:  # the routes read the same Q_hat
            assert bd.blkSizes == first.blkSizes, (name, route)
            for q, q0 in zip(bd.Q_hat, first.Q_hat):
                assert np.array_equal(np.asarray(q), np.asarray(q0)), (name, route)
        ref, err = _check_run(bd, L, d, blocks, ref)
        print(f"basis_image_max_err {name} {route} seed={seed} {err:.3e} bound={bound:.3e}")
        assert err <= bound, (name, route, err)
        runs[route] = bd
    for route, bd in runs.items():
        if route != "two_stage":
            err = _max_abs_diff(bd.blks, runs["two_stage"].blks)
            assert err <= bound, (name, route, "against two_stage", err)


@pytest.mark.parametrize("eig_driver", [4, 6])
@pytest.mark.parametrize("name", ["K17", "DS"])
def test_block_images_other_eigen_drivers(pkg, problems, name, eig_driver):
    """The same comparison with Q_hat from the forced dense driver (4), automatic basis_image route.
    The forced module-compression driver (6) does not apply to these two instances: it compresses to the cyclic module
    of a random vector, of dimension sum_k s_k min(s_k, m_k) -- 17 * 1 + 17 * 3 = 68 = n for K17, 1 + 4 + 25 + 34 = 64
    of n = 76 for DS -- and refuses modules beyond min(n / 2, 500, 2 d + 8) (compress.cpp).  What the library promises
    then is SOLVER_ERROR "requested driver not applicable" (blockdiag.cpp), never images of a wrong Q_hat; that is
    what is asserted for 6."""
    L, d, blocks = problems.known_blocks_instance(name)
    P = pkg.Partition(d, L.astype(np.uint32))
    if eig_driver == 6:
        with pkg.Context(seed=SEEDS[0], eig_driver=6) as ctx:
            with pytest.raises(pkg.SdpsrError) as ei:
                pkg.blockDiagonalize(P, ctx=ctx)
            assert ei.value.status == SOLVER_ERROR and "not applicable" in str(ei.value)
        return
    seed, bd = _block_diagonalize(pkg, P, SEEDS, eig_driver=eig_driver)
    _, err = _check_run(bd, L, d, blocks)
    bound = 2e-12 * L.shape[0]
    print(f"basis_image_max_err {name} auto/eig_driver={eig_driver} seed={seed} {err:.3e} bound={bound:.3e}")
    assert err <= bound, (name, eig_driver, err)


# ------------------------------------------------------------------ reduce_constraints
def _labels(n, d, seed):
    """Flat column-major labels 0..d of an n x n matrix: about 5 % label 0 (no column), and for d >= 7 class d confined
    to the LAST entry (the ragged tail of the last chunk) and class d - 1 absent from the first chunk of 4096."""
    rng = np.random.default_rng(seed)
    ln = n * n
    hi = d if d < 7 else d - 2
    lab = rng.integers(1, hi + 1, size=ln)
    lab[rng.random(ln) < 0.05] = 0
    if d >= 7:
        late = 4096 + rng.choice(ln - 1 - 4096, size=5, replace=False)
        lab[late] = d - 1
        lab[ln - 1] = d
        assert not np.any(lab[:4096] == d - 1) and np.count_nonzero(lab == d) == 1
    return lab.astype(np.uint32)


def _class_sums_int(lab, A_int, d):
    """A * PMat in integer arithmetic: column e of A added into column lab[e] - 1."""
    acc = np.zeros((d + 1, A_int.shape[0]), dtype=np.int64)
    np.add.at(acc, lab.astype(np.int64), A_int.T)
    return acc[1:].T


def _reduce(pkg, ctx, n, d, lab, A):
    return pkg.reduce_constraints(pkg.Partition(d, lab.reshape(n, n, order="F")), A, ctx=ctx)


@pytest.mark.parametrize("n", [65, 130])
def test_reduce_constraints_exact_integer_cases(pkg, gpu_ctx, n):
    """A with integer entries in [-8, 8]: every class sum is exact in fp64 whatever the order, so A * PMat must EQUAL
    integer arithmetic.  len = 4225 is two chunks of 4096, the last of 129 = 2 * 64 + 1 entries (a ragged group of
    64 lanes); len = 16900 is five.  m = 65 and 130 take the second (and third) pass over the rows: an r0 that did
    not advance, or LDS bins not re-zeroed between the passes, would put the sums of rows 0..63 into rows 64.. .
    m = 63, 64, 65 sit around the wave width; (d, m) = (119, 64 and more) fills the LDS accumulators exactly,
    (119 + 1) * 64 * 8 = 60 KiB."""
    rng = np.random.default_rng(n)
    ln = n * n
    for m in (1, 63, 64, 65, 130):
        A_int = rng.integers(-8, 9, size=(m, ln))
        for d in (1, 7, 119):
            lab = _labels(n, d, seed=1000 * n + d)
            got = _reduce(pkg, gpu_ctx, n, d, lab, A_int.astype(np.float64))
            assert got.shape == (m, d)
            assert np.array_equal(got, _class_sums_int(lab, A_int, d)), (n, m, d)
    # a vector (C' * PMat) takes the m = 1 path and comes back as a vector
    lab = _labels(n, 7, seed=n)
    c_int = rng.integers(-8, 9, size=ln)
    got = _reduce(pkg, gpu_ctx, n, 7, lab, c_int.astype(np.float64))
    assert got.shape == (7,) and np.array_equal(got, _class_sums_int(lab, c_int[None, :], 7)[0])


def test_reduce_constraints_lds_boundary(pkg, gpu_ctx):
    """The accumulators are (d + 1) * min(m, 64) doubles of LDS, 60 KiB at the most: (d, m) = (119, 65) fits exactly,
    (120, 64) does not and comes back as BAD_ARGUMENT with the ctx still usable; at m = 1, d = 7678 fits."""
    n = 65
    rng = np.random.default_rng(7)
    A_int = rng.integers(-8, 9, size=(65, n * n))
    lab = _labels(n, 119, seed=3)
    got = _reduce(pkg, gpu_ctx, n, 119, lab, A_int.astype(np.float64))
    assert np.array_equal(got, _class_sums_int(lab, A_int, 119))
    lab = _labels(n, 120, seed=4)
    with pytest.raises(pkg.SdpsrError) as ei:
        _reduce(pkg, gpu_ctx, n, 120, lab, A_int[:64].astype(np.float64))
    assert ei.value.status == BAD_ARGUMENT and "LDS" in str(ei.value)
    lab = _labels(n, 7, seed=5)  # the same ctx computes a small case correctly afterwards
    got = _reduce(pkg, gpu_ctx, n, 7, lab, A_int[:3].astype(np.float64))
    assert np.array_equal(got, _class_sums_int(lab, A_int[:3], 7))
    lab = _labels(n, 7678, seed=6)
    got = _reduce(pkg, gpu_ctx, n, 7678, lab, A_int[:1].astype(np.float64))
    assert got.shape == (1, 7678)
    assert np.array_equal(got, _class_sums_int(lab, A_int[:1], 7678))


@pytest.mark.parametrize("d", [7, 119])
def test_reduce_constraints_real_values(pkg, gpu_ctx, d):
    """Real-valued A, standard normal times 10^U(-6, 6), against math.fsum per class and row.  Bound
    count_i * 2^-53 * sum |a_e| over the class: the a-priori bound of a floating-point sum in ANY order
    ((count - 1) u / (1 - (count - 1) u) <= count u), so it does not depend on how the kernel walks the entries."""
    n, m = 65, 65
    ln = n * n
    rng = np.random.default_rng(d)
    A = rng.standard_normal((m, ln)) * 10.0 ** rng.uniform(-6, 6, size=(m, ln))
    lab = _labels(n, d, seed=50 + d)
    got = _reduce(pkg, gpu_ctx, n, d, lab, A)
    worst = 0.0
    for i in range(1, d + 1):
        idx = np.flatnonzero(lab == i)
        for r in range(m):
            vals = A[r, idx].tolist()
            bound = len(vals) * 2.0 ** -53 * math.fsum(abs(v) for v in vals)
            err = abs(got[r, i - 1] - math.fsum(vals))
            assert err <= bound, (d, i, r, err, bound)
            if bound:
                worst = max(worst, err / bound)
    print(f"reduce_constraints_real d={d} worst error / bound = {worst:.3e}")


def test_reduce_constraints_device_resident_arguments(pkg, gpu_ctx):
    """SDPSR_MEM_DEVICE: labels, A (m x len, column-major) and the output are torch tensors, used in place."""
    import torch
    n, m, d = 65, 65, 7
    ln = n * n
    rng = np.random.default_rng(21)
    A_int = rng.integers(-8, 9, size=(m, ln))
    lab = _labels(n, d, seed=22)
    t_lab = torch.from_numpy(lab.view(np.int32).copy()).cuda()
    t_A = torch.from_numpy(np.ascontiguousarray(A_int.astype(np.float64).ravel(order="F"))).cuda()
    t_out = torch.full((m * d,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = pkg.load_library()
    gpu_ctx.check(lib.sdpsr_reduce_constraints(gpu_ctx._h, ln, C.c_void_p(t_lab.data_ptr()), d, m, C.c_void_p(t_A.data_ptr()),
                                               C.c_void_p(t_out.data_ptr()), pkg.MEM_DEVICE))
    got = t_out.cpu().numpy().reshape(m, d, order="F")
    assert np.array_equal(got, _class_sums_int(lab, A_int, d))
    assert np.array_equal(t_lab.cpu().numpy().view(np.uint32), lab)  # inputs untouched


@pytest.mark.parametrize("bad", ["d + 1", "2^32 - 1"])
def test_reduce_constraints_rejects_labels_beyond_d(pkg, gpu_ctx, bad):
    """A label > d has no accumulator: the kernel skips the entry and raises a flag (as fill! does), the call returns
    BAD_ARGUMENT, and the ctx stays usable.  (Without the guard the label indexes LDS out of bounds.)"""
    n, m, d = 65, 65, 7
    rng = np.random.default_rng(31)
    A_int = rng.integers(-8, 9, size=(m, n * n))
    lab = _labels(n, d, seed=32)
    broken = lab.copy()
    broken[n * n - 2] = d + 1 if bad == "d + 1" else 0xFFFFFFFF  # in the ragged tail of the last chunk
    with pytest.raises(pkg.SdpsrError) as ei:
        _reduce(pkg, gpu_ctx, n, d, broken, A_int.astype(np.float64))
    assert ei.value.status == BAD_ARGUMENT and "label exceeds d" in str(ei.value)
    got = _reduce(pkg, gpu_ctx, n, d, lab, A_int.astype(np.float64))
    assert np.array_equal(got, _class_sums_int(lab, A_int, d))
