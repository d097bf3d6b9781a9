"""sdpsr_sdp_solve over blocks of order 65 .. 128 (a context with psd_max_order = 128): the fused form of psd_project_mid_kernel
inside the solver's wait-free loop.  Against the NumPy restatement (tests/sdp_admm_ref.py) on synthetic operators, to
convergence on the instances of tests/sdp_mid_instances.py with their dual certificates, and the contract of the header."""
import ctypes as C
import functools
import math
import time

import numpy as np
import pytest

from blockop_ref import adjoint_ref, apply_ref, block_offsets, flatten_blocks, full_entries, random_triplets
from sdp_admm_ref import admm_ref, dense_B
from sdp_mid_instances import SOLVER, instance, restatement
from test_gpu_sdp_solve import _as_full, _raw_solve

pytestmark = pytest.mark.gpu

OK, BAD_ARGUMENT, NOT_CONVERGED = 0, 5, 9
EPS = float(np.finfo(np.float64).eps)
D, R = 37, 5


@pytest.fixture(scope="module")
def mid_ctx(pkg, gpu_ctx):
    with pkg.Context(device=0, seed=4321, psd_max_order=128) as ctx:
        yield ctx


@functools.lru_cache(maxsize=None)
def _synthetic(sizes):
    """_synthetic of tests/test_gpu_sdp_solve.py for other block orders: random triplets at density 0.05, x* > 0, and a shifted
    identity added to class 0 so that Z(x*) is positive definite."""
    sizes = list(sizes)
    rng = np.random.default_rng(41)
    ptr, blk, row, col, val = random_triplets(sizes, D, 0.05, 42)
    xs = rng.uniform(0.5, 1.5, D)
    full = full_entries(ptr, blk, row, col, val, sizes)
    n = int(block_offsets(sizes)[-1])
    Z = apply_ref(xs, full, n)[0]
    off = block_offsets(sizes)
    shift = 1.0 + max(np.abs(np.linalg.eigvalsh(Z[off[k]:off[k + 1]].reshape(s, s, order="F"))).max() for k, s in enumerate(sizes))
    eb = np.concatenate([np.full(s, k) for k, s in enumerate(sizes)]).astype(np.int32)
    ei = np.concatenate([np.arange(s) for s in sizes]).astype(np.int32)
    blk, row, col = (np.concatenate([e, a]) for e, a in ((eb, blk), (ei, row), (ei, col)))
    val = np.concatenate([np.full(eb.size, shift / xs[0]), val])
    ptr = np.concatenate([[0], ptr[1:] + eb.size]).astype(np.int64)
    A = rng.standard_normal((R, D))
    return (ptr, blk, row, col, val), xs, A, A @ xs, rng.standard_normal(D)


# ------------------------------------------------------------------ against the NumPy restatement, synthetic operators
@pytest.mark.parametrize("sizes", [(1, 2, 97, 3), (128, 64, 1)])
def test_two_hundred_iterations_against_the_numpy_restatement(pkg, mid_ctx, sizes):
    """The bound rule of tests/test_gpu_sdp_solve.py: rounding differences of the non-expansive iteration map are measured on the
    restatement alone (B dense against B keyed: another summation order) and the library is held to 10 times that, with a floor
    of 200 D eps (1 + |.|_inf).  Upper and full triplets describe the same operator and agree within the same bound."""
    SIZES = list(sizes)
    trip, xs, A, b, c = _synthetic(sizes)
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
        with pkg.BlockOperator(sp, ctx=mid_ctx) as op:
            sol = op.solve(A, b, c, return_S=True, return_Y=True, **kw)
        assert sol.iters == 200 and sol.status == "iteration_limit"
        got = {"x": sol.x, "S": flatten_blocks(sol.S), "Y": flatten_blocks(sol.Y)}
        for key in ("x", "S", "Y"):
            diff, floor = bounds[key]
            err = np.abs(got[key] - getattr(ref, key)).max()
            print(f"{SIZES} {'upper' if upper else 'full'} {key}: library - restatement {err:.3e}; restatement dense - keyed {diff:.3e}; "
                  f"floor {floor:.3e}")
            assert err <= max(10 * diff, floor)
        outs.append(got)
    for key in ("x", "S", "Y"):
        diff, floor = bounds[key]
        assert np.abs(outs[0][key] - outs[1][key]).max() <= max(10 * diff, floor)
    assert np.abs(A @ outs[0]["x"] - b).max() <= 1e-9 * (1 + np.abs(b).max())


# ------------------------------------------------------------------ to convergence, with certificates
# Measured on an MI355X: (a) at s = 65 converges in 2.75 s (2500 iterations, 1.10 ms each), (a) at s = 97 takes 10.8 s (3600
# iterations, 3.01 ms each) and (b) 7.0 s (5450 iterations, 1.29 ms each) -- all three pass the checks below (relative gap to the
# dual bound 3.9e-10 / 4.3e-10 / 1.3e-9, to the restatement's objective 1.3e-14 / 4.2e-14 / 4.3e-14).  A test runs for seconds,
# so (a) at s = 97 and (b) are held to the restatement over 500 iterations instead; tools/psd_project_mid_time.py runs all to the end.
@functools.lru_cache(maxsize=None)
def _five_hundred(name):
    """The restatement over 500 iterations without a stop, B dense and B keyed (another summation order), once."""
    t = instance(name)
    kw = dict(sense=t.sense, nonneg=t.nonneg, rho=1.0, max_iters=500, check_every=500)
    apply, adjoint = t.apply, t.adjoint
    if apply is None:
        full, n = full_entries(*t.trip, t.sizes), t.sizes[0] ** 2
        apply, adjoint = (lambda x: apply_ref(x, full, n)[0]), (lambda S: adjoint_ref(S, full, t.d)[0])
    return admm_ref(t.B, t.sizes, t.A, t.b, t.c, **kw), admm_ref(t.B, t.sizes, t.A, t.b, t.c, apply=apply, adjoint=adjoint, **kw)


@pytest.mark.parametrize("name", ["lmin97", "theta66"])
def test_five_hundred_iterations_against_the_numpy_restatement(pkg, mid_ctx, name):
    """The bound rule of the 200-iteration test with the instance's own d: the larger of 10 x (restatement dense - restatement
    keyed) and 200 d eps (1 + |.|_inf), for x, S and Y."""
    t = instance(name)
    ref, alt = _five_hundred(name)
    sp = pkg.SparseBlocks(*t.trip, t.sizes, len(t.trip[4]))
    with pkg.BlockOperator(sp, ctx=mid_ctx) as op:
        t0 = time.perf_counter()
        sol = op.solve(t.A, t.b, t.c, sense=t.sense, nonneg=t.nonneg, rho=1.0, max_iters=500, check_every=500, return_S=True, return_Y=True)
        wall = time.perf_counter() - t0
    print(f"{name}: 500 iterations in {wall:.2f} s (setup included)")
    assert sol.iters == 500 and sol.status == "iteration_limit" and ref.iters == alt.iters == 500
    got = {"x": sol.x, "S": flatten_blocks(sol.S), "Y": flatten_blocks(sol.Y)}
    for key in ("x", "S", "Y"):
        u, v = getattr(ref, key), getattr(alt, key)
        diff, floor = np.abs(u - v).max(), 200 * t.d * EPS * (1 + np.abs(u).max())
        err = np.abs(got[key] - u).max()
        print(f"{name} {key}: library - restatement {err:.3e}; restatement dense - keyed {diff:.3e}; floor {floor:.3e}")
        assert err <= max(10 * diff, floor)
    assert sol.eq_residual <= 1e-9 * (1 + np.abs(t.b).max())
    for Sk in sol.S:
        assert np.array_equal(Sk, Sk.T)  # symmetric bit for bit


@pytest.mark.parametrize("name", ["lmin65"])
def test_convergence_and_certificates(pkg, mid_ctx, name):
    t, ref = instance(name), restatement(name)
    sp = pkg.SparseBlocks(*t.trip, t.sizes, len(t.trip[4]))
    with pkg.BlockOperator(sp, ctx=mid_ctx) as op:
        t0 = time.perf_counter()
        sol = op.solve(t.A, t.b, t.c, sense=t.sense, nonneg=t.nonneg, return_S=True, return_Y=True, **SOLVER)
        wall = time.perf_counter() - t0
        Z = op.apply(sol.x)
    bound = t.bound(flatten_blocks(sol.Y))
    obj = sol.objective
    zmax = max(np.abs(z).max() for z in Z)
    print(f"{name}: {sol.status} after {sol.iters} iterations in {wall:.2f} s ({1e3 * wall / sol.iters:.3f} ms / iteration, setup included); "
          f"objective {obj:.10f}, dual bound {bound:.10f} (relative gap {abs(obj - bound) / abs(obj):.2e}), restatement {ref.objective:.10f} "
          f"after {ref.iters} (relative {abs(obj - ref.objective) / abs(obj):.2e}); eq_residual {sol.eq_residual:.2e} lambda_min "
          f"{sol.lambda_min:.2e} min_x {sol.min_x:.2e}")
    assert sol.status == "converged"
    assert abs(obj - bound) <= 1e-6 * abs(obj)
    assert abs(obj - ref.objective) <= 1e-7 * abs(obj)
    assert sol.eq_residual <= 1e-9 * (1 + np.abs(t.b).max())
    assert sol.lambda_min >= -10 * SOLVER["eps"] * max(1.0, zmax)
    if t.nonneg:
        assert sol.min_x >= -10 * SOLVER["eps"]
    for Sk in sol.S:
        assert np.array_equal(Sk, Sk.T)  # symmetric bit for bit


# ------------------------------------------------------------------ contract
def _lmin_op(pkg, ctx):
    t = instance("lmin65")
    return t, pkg.BlockOperator(pkg.SparseBlocks(*t.trip, t.sizes, len(t.trip[4])), ctx=ctx)


def test_host_waits_follow_the_checks(pkg, mid_ctx):
    """ceil(iters / check_every) + the constant of the setup path, 5 for host arrays with d <= 64 and r > 0: the second launch
    adds no wait.  The constant is read off one call and has to serve two others."""
    prof = pkg._lib.load_prof_library()
    t, opn = _lmin_op(pkg, mid_ctx)

    def waits(**o):
        w0, w1 = C.c_uint64(0), C.c_uint64(0)
        prof.sdpsr_profile_host_waits(mid_ctx._h, C.byref(w0))
        st, _, _, _, info = _raw_solve(mid_ctx, op, t.A, t.b, t.c, nonneg=-1, **o)
        prof.sdpsr_profile_host_waits(mid_ctx._h, C.byref(w1))
        assert st == NOT_CONVERGED
        return w1.value - w0.value, info.iters

    with opn as op:
        waits(max_iters=10)  # (buffers of this shape exist from here on)
        w, it = waits(max_iters=100, check_every=10)
        const = w - math.ceil(it / 10)
        print(f"host waits: {w} for {it} iterations checked every 10: constant {const}")
        assert const == 5
        assert waits(max_iters=95, check_every=10) == (const + 10, 95)
        assert waits(max_iters=400, check_every=50) == (const + 8, 400)


def test_equal_bytes_from_two_calls_and_two_contexts(pkg, mid_ctx):
    t, opn = _lmin_op(pkg, mid_ctx)
    outs = []
    with opn as op:
        for _ in range(2):
            outs.append(_raw_solve(mid_ctx, op, t.A, t.b, t.c, nonneg=-1, max_iters=300))
        with pkg.Context(seed=77, psd_max_order=128) as other:
            outs.append(_raw_solve(other, op, t.A, t.b, t.c, nonneg=-1, max_iters=300))
    st0, x0, S0, Y0, i0 = outs[0]
    assert st0 == NOT_CONVERGED and i0.iters == 300
    for st, x, S, Y, info in outs[1:]:
        assert st == st0 and x.tobytes() == x0.tobytes() and S.tobytes() == S0.tobytes() and Y.tobytes() == Y0.tobytes()
        assert bytes(info) == bytes(i0)


def test_one_handle_refused_by_a_default_context_and_solved_by_an_opted_in_one(pkg, gpu_ctx, mid_ctx):
    t, opn = _lmin_op(pkg, gpu_ctx)
    with opn as op:
        st, x, S, Y, _ = _raw_solve(gpu_ctx, op, t.A, t.b, t.c, nonneg=-1, max_iters=50)
        assert st == BAD_ARGUMENT and b"64" in gpu_ctx._lib.sdpsr_last_error(gpu_ctx._h)
        assert np.all(x == 7.0) and np.all(S == 7.0) and np.all(Y == 7.0)
        with pytest.raises(ValueError, match="64"):
            op.solve(t.A, t.b, t.c, nonneg=False, max_iters=50)
        st, x, S, Y, info = _raw_solve(mid_ctx, op, t.A, t.b, t.c, nonneg=-1, max_iters=50)
        assert st == NOT_CONVERGED and info.iters == 50 and np.all(np.isfinite(np.concatenate([x, S, Y]))) and not np.any(x == 7.0)
        sol = op.solve(t.A, t.b, t.c, nonneg=False, max_iters=50, ctx=mid_ctx)
        assert sol.iters == 50 and sol.x.tobytes() == x.tobytes()


def test_order_129_is_refused_before_any_allocation(pkg, mid_ctx):
    empty = np.zeros(0, dtype=np.int32)
    d = 3
    sp = pkg.SparseBlocks(np.zeros(d + 1, dtype=np.int64), empty, empty, empty, np.zeros(0), [129, 2], 0)
    with pkg.BlockOperator(sp, ctx=mid_ctx) as op:
        st, x, _, _, _ = _raw_solve(mid_ctx, op, np.zeros((0, d)), np.zeros(0), np.ones(d))
        assert st == BAD_ARGUMENT and b"128" in mid_ctx._lib.sdpsr_last_error(mid_ctx._h) and np.all(x == 7.0)
