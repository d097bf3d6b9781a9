"""sdpsr_sdp_solve (the first-order solver of the reduced SDP) end to end: the reference's pinned optima from the device
pipeline, certificates from independent entries, the NumPy restatement (tests/sdp_admm_ref.py) and the contract of the header.

Pins (test/lovasz.jl:16,32,48, test/qap.jl:31 of the reference): theta' of Petersen 4, ER(3) 5.0, ER(5) 10.066926, ER(7) 15.743402
within 1e-6 relative at rho = 1, eps = 1e-9, 20 000 iterations at most; esc16j 7.7942186 within 5e-4 at rho = 10 and exactly
20 000 iterations (ADMM does not converge on it; the NumPy restatement reaches 6.3e-5)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from blockop_ref import adjoint_ref, apply_ref, block_offsets, flatten_blocks, full_entries, random_triplets
from sdp_admm_ref import admm_ref, dense_B

pytestmark = pytest.mark.gpu

OK, BAD_ARGUMENT, NOT_CONVERGED = 0, 5, 9
EPS = float(np.finfo(np.float64).eps)
PINS = {"petersen": (4.0, 1e-6), "er3": (5.0, 1e-6), "er5": (10.066926, 1e-6), "er7": (15.743402, 1e-6), "esc16j": (7.7942186, 5e-4)}


def _problem(pr, name):
    import pathlib
    if name == "petersen":
        return pr.theta_prime_problem(pr.petersen_adjacency()) + ("max",)
    if name.startswith("er"):
        return pr.theta_prime_problem(pr.er_graph_adjacency(int(name[2:]))) + ("max",)
    fa, fb = pr.read_qapdata(pathlib.Path(__file__).resolve().parent / "golden" / "esc16j.dat")
    return pr.qap_problem(fa, fb) + ("min",)


_CACHE = {}


def _reduced(pkg, ctx, name):
    """admissible_subspace -> blockDiagonalize(retries=2) -> reduced_sdp -> basis_image_sparse, once per instance."""
    if name not in _CACHE:
        Cv, A, b, sense = _problem(pkg.problems, name)
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
        bd = pkg.blockDiagonalize(P, retries=2, ctx=ctx)
        newA, newB, newC = pkg.reduced_sdp(P, A, b, Cv, ctx=ctx)
        sp = pkg.basis_image_sparse(bd.Q_hat, P, ctx=ctx)
        _CACHE[name] = dict(sense=sense, sizes=list(bd.blkSizes), newA=np.asarray(newA), newB=np.asarray(newB), newC=np.asarray(newC),
                            sp=sp, d=int(P.nparts))
    return _CACHE[name]


_SOLVED = {}


def _solved(pkg, ctx, name):
    if name not in _SOLVED:
        r = _reduced(pkg, ctx, name)
        kw = dict(rho=10.0, max_iters=20000) if name == "esc16j" else {}
        with pkg.BlockOperator(r["sp"], ctx=ctx) as op:
            sol = op.solve(r["newA"], r["newB"], r["newC"], sense=r["sense"], return_S=True, return_Y=True, **kw)
            Z = op.apply(sol.x)
            w = pkg.block_eigvals(Z, op.sizes, ctx=ctx)
        _SOLVED[name] = (sol, Z, w)
    return _SOLVED[name]


# ------------------------------------------------------------------ the pins, from the device pipeline itself
@pytest.mark.parametrize("name", list(PINS))
def test_pinned_optimum(pkg, gpu_ctx, name):
    pin, bound = PINS[name]
    sol, _, _ = _solved(pkg, gpu_ctx, name)
    rel = abs(sol.objective - pin) / pin
    print(f"{name}: objective {sol.objective:.10f} pin {pin} relative {rel:.2e} iters {sol.iters} status {sol.status} "
          f"r_p {sol.r_primal:.2e} r_d {sol.r_dual:.2e}")
    if name == "esc16j":
        assert sol.iters == 20000 and sol.status in ("converged", "iteration_limit")
    else:
        assert sol.status == "converged" and sol.iters <= 20000
    assert rel <= bound


@pytest.mark.parametrize("name", list(PINS))
def test_certificates_at_the_returned_x(pkg, gpu_ctx, name):
    """A x = b holds to the rounding of one d-length sum whatever the status; the cones hold to r_p, so their certificates
    (10 eps) are for the converged instances.  The report against recomputations from independent entries: the objective within
    1e-12 relative, min_x exactly, lambda_min within the eigenvalue bound 1e-12 max|Z| of sdpsr_blocks_syev, eq_residual -- itself
    a number at rounding level, so without relative accuracy of its own -- within 1e-12 (1 + |b|_inf)."""
    r = _reduced(pkg, gpu_ctx, name)
    sol, Z, w = _solved(pkg, gpu_ctx, name)
    x, eps = sol.x, 1e-9
    res = np.abs(r["newA"] @ x - r["newB"]).max()
    bscale = 1 + np.abs(r["newB"]).max()
    zmax = max(np.abs(z).max() for z in Z)
    lmin = min(float(wk.min()) for wk in w)
    assert res <= 1e-9 * bscale
    if sol.status == "converged":
        assert x.min() >= -10 * eps
        assert lmin >= -10 * eps * max(1.0, zmax)
    assert abs(sol.objective - float(r["newC"] @ x)) <= 1e-12 * abs(sol.objective)
    assert sol.min_x == x.min()
    assert abs(sol.eq_residual - res) <= 1e-12 * bscale
    assert abs(sol.lambda_min - lmin) <= 1e-12 * zmax
    assert [s.shape for s in sol.S] == [(k, k) for k in r["sizes"]] and [y.shape for y in sol.Y] == [(k, k) for k in r["sizes"]]
    for Sk in sol.S:  # the split variable is PSD by construction and symmetric bit for bit
        assert np.array_equal(Sk, Sk.T) and np.linalg.eigvalsh(Sk).min() >= -4e-12 * Sk.shape[0] * max(np.abs(Sk).max(), 1e-300)


# ------------------------------------------------------------------ against the NumPy restatement, a synthetic operator
SIZES, D, R = [1, 2, 64, 3], 37, 5


@functools.lru_cache(maxsize=None)
def _synthetic():
    """A feasible problem that is no reduction: random triplets, x* > 0, and x*_0 I added to class 0 so that Z(x*) is positive definite."""
    rng = np.random.default_rng(41)
    ptr, blk, row, col, val = random_triplets(SIZES, D, 0.05, 42)
    xs = rng.uniform(0.5, 1.5, D)
    full = full_entries(ptr, blk, row, col, val, SIZES)
    n = int(block_offsets(SIZES)[-1])
    Z = apply_ref(xs, full, n)[0]
    off = block_offsets(SIZES)
    shift = 1.0 + max(np.abs(np.linalg.eigvalsh(Z[off[k]:off[k + 1]].reshape(s, s, order="F"))).max() for k, s in enumerate(SIZES))
    eb = np.concatenate([np.full(s, k) for k, s in enumerate(SIZES)]).astype(np.int32)
    ei = np.concatenate([np.arange(s) for s in SIZES]).astype(np.int32)
    blk, row, col = (np.concatenate([e, a]) for e, a in ((eb, blk), (ei, row), (ei, col)))
    val = np.concatenate([np.full(eb.size, shift / xs[0]), val])
    ptr = np.concatenate([[0], ptr[1:] + eb.size]).astype(np.int64)
    A = rng.standard_normal((R, D))
    return (ptr, blk, row, col, val), xs, A, A @ xs, rng.standard_normal(D)


def _as_full(trip):
    """The same operator with TRI_FULL triplets: every off-diagonal entry followed by its mirror."""
    ptr, blk, row, col, val = trip
    cls = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    reps = 1 + (row != col).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(reps)[:-1]])
    b2, r2, c2, v2 = (np.repeat(a, reps) for a in (blk, row, col, val))
    m = first[reps == 2] + 1
    r2[m], c2[m] = col[reps == 2], row[reps == 2]
    p2 = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(cls, reps), minlength=ptr.size - 1))]).astype(np.int64)
    return p2, b2, r2, c2, v2


def test_two_hundred_iterations_against_the_numpy_restatement(pkg, gpu_ctx):
    """The iteration map is non-expansive, so rounding differences grow at most linearly in the iteration count; their scale is
    measured on the reference alone -- the restatement with B dense against the same restatement with B applied as apply_ref /
    adjoint_ref (another summation order) -- and the library is held to 10 times that, with a floor of 200 d eps (1 + |.|_inf).
    Measured on an MI355X (x / S / Y): library - restatement 5.4e-13 / 1.5e-12 / 1.2e-13; restatement dense - keyed 2.8e-14 /
    7.1e-14 / 3.7e-14; floor 4.5e-12 / 2.7e-11 / 1.7e-12 (DESIGN.md "Solving the reduced SDP").  Upper and full triplets: equal bytes."""
    trip, xs, A, b, c = _synthetic()
    full = full_entries(*trip, SIZES)
    n = int(block_offsets(SIZES)[-1])
    B = dense_B(full, n, D)
    kw = dict(rho=1.0, max_iters=200, check_every=200)
    ref = admm_ref(B, SIZES, A, b, c, **kw)
    alt = admm_ref(B, SIZES, A, b, c, apply=lambda x: apply_ref(x, full, n)[0], adjoint=lambda S: adjoint_ref(S, full, D)[0], **kw)
    bounds = {}
    for key in ("x", "S", "Y"):
        u, v = getattr(ref, key), getattr(alt, key)
        bounds[key] = (np.abs(u - v).max(), 200 * D * EPS * (1 + np.abs(u).max()))
    outs = []
    for upper, t in ((True, trip), (False, _as_full(trip))):
        sp = pkg.SparseBlocks(*t, SIZES, len(t[4]), upper=upper)
        with pkg.BlockOperator(sp, ctx=gpu_ctx) as op:
            sol = op.solve(A, b, c, return_S=True, return_Y=True, **kw)
        assert sol.iters == 200 and sol.status == "iteration_limit"
        got = {"x": sol.x, "S": flatten_blocks(sol.S), "Y": flatten_blocks(sol.Y)}
        for key in ("x", "S", "Y"):
            diff, floor = bounds[key]
            err = np.abs(got[key] - getattr(ref, key)).max()
            print(f"{'upper' if upper else 'full'} {key}: library - restatement {err:.3e}; restatement dense - keyed {diff:.3e}; floor {floor:.3e}")
            assert err <= max(10 * diff, floor)
        outs.append(got)
    for key in ("x", "S", "Y"):  # TRI_UPPER and TRI_FULL triplets: the same operator
        diff, floor = bounds[key]
        assert np.abs(outs[0][key] - outs[1][key]).max() <= max(10 * diff, floor)
    assert np.abs(A @ outs[0]["x"] - b).max() <= 1e-9 * (1 + np.abs(b).max())


# ------------------------------------------------------------------ contract
def _raw_solve(ctx, op, A, b, c, **o):
    """One call of the C entry on host arrays: (status, x, S, Y, info)."""
    from __graft_entry__ import load_package
    L = load_package()._lib
    d, n = op.d, op.sum_sq
    A = np.asfortranarray(np.asarray(A, dtype=np.float64).reshape(-1, d))
    r = A.shape[0]
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    opts = L.SdpOpts()
    for k, v in o.items():
        setattr(opts, k, v)
    x, S, Y, info = np.full(d, 7.0), np.full(n, 7.0), np.full(n, 7.0), L.SdpInfo()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    st = ctx._lib.sdpsr_sdp_solve(ctx._h, op._h, r, p(A) if r else None, p(b) if r else None, p(c), C.byref(opts), p(x), p(S), p(Y),
                                  C.byref(info), 0)
    return st, x, S, Y, info


def test_equal_bytes_from_two_calls_and_two_contexts(pkg, gpu_ctx):
    r = _reduced(pkg, gpu_ctx, "er3")
    outs = []
    with pkg.BlockOperator(r["sp"], ctx=gpu_ctx) as op:
        for _ in range(2):
            outs.append(_raw_solve(gpu_ctx, op, r["newA"], r["newB"], r["newC"], max_iters=300))
        with pkg.Context(seed=77) as other:
            outs.append(_raw_solve(other, op, r["newA"], r["newB"], r["newC"], max_iters=300))
    st0, x0, S0, Y0, i0 = outs[0]
    assert st0 == NOT_CONVERGED and i0.iters == 300
    for st, x, S, Y, info in outs[1:]:
        assert st == st0 and x.tobytes() == x0.tobytes() and S.tobytes() == S0.tobytes() and Y.tobytes() == Y0.tobytes()
        assert bytes(info) == bytes(i0)


def test_iteration_limit_writes_every_output(pkg, gpu_ctx):
    r = _reduced(pkg, gpu_ctx, "er7")
    with pkg.BlockOperator(r["sp"], ctx=gpu_ctx) as op:
        st, x, S, Y, info = _raw_solve(gpu_ctx, op, r["newA"], r["newB"], r["newC"], max_iters=100)
        assert st == NOT_CONVERGED and b"iteration limit" in gpu_ctx._lib.sdpsr_last_error(gpu_ctx._h)
        assert info.iters == 100 and info.rho == 1.0 and info.rho_changes == 0
        assert not np.any(x == 7.0) and not np.all(S == 7.0) and not np.all(Y == 7.0) and np.all(np.isfinite(np.concatenate([x, S, Y])))
        assert abs(info.objective - float(r["newC"] @ x)) <= 1e-12 * abs(info.objective) and info.r_primal > 1e-9
        sol = op.solve(r["newA"], r["newB"], r["newC"], max_iters=100)
        assert sol.status == "iteration_limit" and sol.iters == 100 and sol.S is None and sol.Y is None
        with pytest.raises(pkg.NotConverged):
            op.solve(r["newA"], r["newB"], r["newC"], max_iters=100, raise_on_limit=True)


def test_host_waits_follow_the_checks(pkg, gpu_ctx):
    """ceil(iters / check_every) + a constant of the setup path (include/sdpsr.h): the constant is read off one call and has to
    serve two others with other iteration counts and check intervals."""
    prof = pkg._lib.load_prof_library()
    r = _reduced(pkg, gpu_ctx, "er5")

    def waits(**o):
        w0, w1 = C.c_uint64(0), C.c_uint64(0)
        prof.sdpsr_profile_host_waits(gpu_ctx._h, C.byref(w0))
        st, _, _, _, info = _raw_solve(gpu_ctx, op, r["newA"], r["newB"], r["newC"], **o)
        prof.sdpsr_profile_host_waits(gpu_ctx._h, C.byref(w1))
        assert st == NOT_CONVERGED
        return w1.value - w0.value, info.iters

    with pkg.BlockOperator(r["sp"], ctx=gpu_ctx) as op:
        waits(max_iters=10)  # (buffers of this shape exist from here on)
        w, it = waits(max_iters=100, check_every=10)
        const = w - math.ceil(it / 10)
        print(f"host waits: {w} for {it} iterations checked every 10: constant {const}")
        assert const == 5
        assert waits(max_iters=95, check_every=10) == (const + 10, 95)
        assert waits(max_iters=400, check_every=50) == (const + 8, 400)


def test_residual_balancing_on_esc16j(pkg, gpu_ctx):
    pin, bound = PINS["esc16j"]
    r = _reduced(pkg, gpu_ctx, "esc16j")
    with pkg.BlockOperator(r["sp"], ctx=gpu_ctx) as op:
        sol = op.solve(r["newA"], r["newB"], r["newC"], sense="min", rho=10.0, max_iters=40000, adapt_rho=True)
    rel = abs(sol.objective - pin) / pin
    print(f"esc16j adapt_rho: objective {sol.objective:.8f} relative {rel:.2e} rho {sol.rho} changes {sol.rho_changes} iters {sol.iters}")
    assert sol.rho_changes > 0 and rel <= bound


def test_refusals_leave_the_ctx_and_the_handle_usable(pkg, gpu_ctx):
    r = _reduced(pkg, gpu_ctx, "er3")
    A, b, c = r["newA"], r["newB"], r["newC"]
    err = lambda: gpu_ctx._lib.sdpsr_last_error(gpu_ctx._h)  # noqa: E731
    with pkg.BlockOperator(r["sp"], ctx=gpu_ctx) as op:
        st, x, S, Y, _ = _raw_solve(gpu_ctx, op, np.vstack([A, A[:1]]), np.concatenate([b, b[:1]]), c)  # a duplicated row
        assert st == BAD_ARGUMENT and b"dependent" in err() and b"compress_constraints" in err()
        cn = c.copy()
        cn[3] = np.nan
        st, x, S, Y, _ = _raw_solve(gpu_ctx, op, A, b, cn)
        assert st == BAD_ARGUMENT and b"non-finite" in err() and np.all(x == 7.0) and np.all(S == 7.0) and np.all(Y == 7.0)
        assert _raw_solve(gpu_ctx, op, A, b, c, max_iters=-1)[0] == BAD_ARGUMENT
        assert _raw_solve(gpu_ctx, op, A, b, c, sense=2)[0] == BAD_ARGUMENT
        assert _raw_solve(gpu_ctx, op, np.zeros((op.d + 1, op.d)), np.zeros(op.d + 1), c)[0] == BAD_ARGUMENT  # r > d
        with pytest.raises(ValueError, match="dependent"):
            op.solve(np.vstack([A, A[:1]]), np.concatenate([b, b[:1]]), c)
        sol = op.solve(A, b, c)  # the handle and the ctx still serve
        assert sol.status == "converged" and abs(sol.objective - 5.0) <= 5e-6
    empty = np.zeros(0, dtype=np.int32)
    for sizes, d, what in (([2], 4097, b"4096"), ([65, 2], 3, b"64")):  # refused before any allocation: an empty operator is enough
        sp = pkg.SparseBlocks(np.zeros(d + 1, dtype=np.int64), empty, empty, empty, np.zeros(0), sizes, 0)
        with pkg.BlockOperator(sp, ctx=gpu_ctx) as op:
            st, x, _, _, _ = _raw_solve(gpu_ctx, op, np.zeros((0, d)), np.zeros(0), np.ones(d))
            assert st == BAD_ARGUMENT and what in err() and np.all(x == 7.0)


@pytest.mark.parametrize("sense,sign", [("max", -1.0), ("min", 1.0)])
def test_no_equality_constraint(pkg, gpu_ctx, sense, sign):
    """r = 0 is legal.  Every direction that improves the objective leaves x >= 0, so the optimum is x = 0."""
    trip, xs, _, _, _ = _synthetic()
    c = sign * np.random.default_rng(51).uniform(0.5, 1.5, D)
    sp = pkg.SparseBlocks(*trip, SIZES, len(trip[4]))
    with pkg.BlockOperator(sp, ctx=gpu_ctx) as op:
        sol = op.solve(None, None, c, sense=sense)
    print(f"r = 0, {sense}: iters {sol.iters} |x|_inf {np.abs(sol.x).max():.2e}")
    assert sol.status == "converged" and sol.eq_residual == 0.0 and np.abs(sol.x).max() <= 1e-8 and abs(sol.objective) <= 1e-7


def test_reduce_and_solve_er3(pkg, gpu_ctx):
    pr = pkg.problems
    Cv, A, b = pr.theta_prime_problem(pr.er_graph_adjacency(3))
    res = pkg.reduce_and_solve(Cv, A, b, ctx=gpu_ctx)
    assert abs(res.optVal - 5.0) <= 5e-6 and sorted(res.blkSize) == [2, 2, 3]
    assert (res.originalSize, res.newSize) == (13, 12) and res.jTime > 0 and res.blkTime > 0 and res.solveTime > 0
    small = pkg.reduce_and_solve(Cv, A, b, limit_size=5, ctx=gpu_ctx)  # above limitSize: the reference's zero-filled tuple
    assert small[1:7] == (0, 0, 0, 0, 13, 12)


# ------------------------------------------------------------------ the complex route: the real embedding needs nothing of its own
def _theta_rows(L, edge_classes):
    """(newA, newB, newC) of theta' over the classes 1..d of the labels L: <A_E, X> = 0, tr X = 1, maximise <J, X>."""
    d = int(L.max())
    size = np.bincount(L.ravel(), minlength=d + 1)[1:].astype(np.float64)
    diag = np.bincount(np.diag(L), minlength=d + 1)[1:].astype(np.float64)
    edge = np.where(np.isin(np.arange(1, d + 1), edge_classes), size, 0.0)
    return np.vstack([edge, diag]), np.asarray([0.0, 1.0]), size


def test_complex_embedding_gives_the_objective_of_its_real_twin(pkg, gpu_ctx):
    """theta' of a Cayley-type graph on C[S3] (x) K12 (n = 72), twice.  Complex: the variables are the classes of the
    non-symmetric partition, X symmetric is the constraint x_i = x_i' for every class and its transpose, and the PSD blocks are
    the real embeddings of blockDiagonalize(complex=True).  Real twin: the symmetrized partition (a class merged with its
    transpose: the symmetric elements of the algebra, a Jordan algebra) through the real blockDiagonalize.  Both describe the
    same feasible set of matrices X, so the optima agree; 1e-6 relative is 20 times the accuracy the theta' pins reach."""
    from basis_image_complex_helpers import s3_cayley_labels
    Lm, _ = pkg.problems.kron_with_complete(s3_cayley_labels(), 12, seed=3)
    bdc = pkg.blockDiagonalize(pkg.Partition.from_matrix(np.asarray(Lm), ctx=gpu_ctx), complex=True, ctx=gpu_ctx, retries=3)
    Pd = bdc.partition
    L = np.asarray(Pd.matrix).astype(np.int64)
    d = int(Pd.nparts)
    assert not np.array_equal(L, L.T) and L.min() >= 1
    transpose = np.zeros(d + 1, dtype=np.int64)
    transpose[L.ravel()] = L.T.ravel()  # class i' of the transposed positions
    assert np.array_equal(transpose[transpose[1:]], np.arange(1, d + 1))
    e = int(L[0, 1])
    edge = sorted({e, int(transpose[e])})
    assert e != L[0, 0]
    # the complex formulation
    A1, b1, c1 = _theta_rows(L, edge)
    pairs = [(i, int(transpose[i])) for i in range(1, d + 1) if i < transpose[i]]
    assert pairs
    sym = np.zeros((len(pairs), d))
    for k, (i, j) in enumerate(pairs):
        sym[k, i - 1], sym[k, j - 1] = 1.0, -1.0
    newA, newB = pkg.compress_constraints(np.vstack([A1, sym]), np.concatenate([b1, np.zeros(len(pairs))]), ctx=gpu_ctx)
    sp = pkg.basis_image_sparse(bdc.Q_hat, Pd, ctx=gpu_ctx)
    assert sp.sizes == [2 * s for s in bdc.blkSizes]
    with pkg.BlockOperator(sp, ctx=gpu_ctx) as op:
        cx = op.solve(newA, newB, c1)
    # the real twin
    rep = np.minimum(np.arange(d + 1), transpose)
    _, Ls = np.unique(rep[L], return_inverse=True)
    Ls = Ls.reshape(L.shape) + 1
    assert np.array_equal(Ls, Ls.T)
    Ps = pkg.Partition(int(Ls.max()), Ls.astype(np.uint32))
    bdr = pkg.blockDiagonalize(Ps, ctx=gpu_ctx, retries=3)
    A2, b2, c2 = _theta_rows(Ls, sorted({int(Ls[0, 1])}))
    with pkg.BlockOperator(pkg.basis_image_sparse(bdr.Q_hat, Ps, ctx=gpu_ctx), ctx=gpu_ctx) as op:
        re = op.solve(A2, b2, c2)
    print(f"complex {cx.objective:.10f} ({cx.iters} iterations, {cx.status}), real twin {re.objective:.10f} ({re.iters}, {re.status})")
    assert cx.status == re.status == "converged"
    assert abs(cx.objective - re.objective) <= 1e-6 * abs(re.objective)
    assert np.abs(cx.x - cx.x[transpose[1:] - 1]).max() <= 1e-9
