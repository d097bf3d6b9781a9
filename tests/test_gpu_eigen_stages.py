"""The stages of the dense symmetric eigensolver, one by one, through the test entry points of libsdpsr_prof.so (sdpsr_profile_sytrd,
_backtransform, _stedc) against the references of tests/eigen_stages_ref.py, and the whole solver (sdpsr_syev_f64) on the structured
and the badly scaled inputs that the Gaussian matrices of the other tests never produce.

No bound here is measured on a kernel.  The tridiagonalisation's backward error is held against LAPACK's dsytrd on the same input
under the same evaluator (16 x: four bits for the different summation orders); column 0 against dlarfg in longdouble; the exact
reflector families of the back-transformation with ==; the general one against a float64 reflector-by-reflector application; the
divide and conquer and the whole solver by the bounds test_gpu_parity.py already uses.  Every in/out array carries one NaN bit
pattern (SENT) behind its end and, where the entry's comment says so, inside.

SDPSR_EIGEN_STAGES_RATIOS=<file>: the measured ratios are appended there (profiles/r22_eigen_stages.txt was made so)."""
import ctypes as C
import os

import numpy as np
import pytest

import eigen_stages_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF85A5ADEADBEEF
GUARD = 300
MARGIN = 16.0
OK, SOLVER_ERROR = 0, 7


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _fill(count):
    return np.full(int(count), SENT, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((_bits(a) == np.uint64(SENT)).all())


def _written(a):
    return not bool((_bits(a) == np.uint64(SENT)).any())


def _ld(n):
    return (n + 127) // 128 * 128


def _padded(X, ld, guard=GUARD):
    """X (n x n) in a column-major ld x ld array with zero padding, SENT behind it; (buffer, ld x ld view indexed [row, col])"""
    n = X.shape[0]
    buf = _fill(ld * ld + guard)
    M = buf[:ld * ld].reshape(ld, ld).T
    M[:] = 0.0
    M[:n, :n] = X
    return buf, M


def _record(line):
    path = os.environ.get("SDPSR_EIGEN_STAGES_RATIOS")
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


@pytest.fixture(scope="module")
def ctxs(pkg):
    """one ctx per flag word for the whole module: the graphs of a shape are built once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(flags=0):
        if flags not in made:
            made[flags] = pkg.Context(device=0, seed=1, flags=flags)
        return made[flags]

    yield get
    for c in made.values():
        c.close()


def _flags(pkg, form):
    return {"rows": 0, "hybrid": 0, "panels": pkg._lib.FLAG_SYTRD_PANELS, "hybrid_one_launch": pkg._lib.FLAG_SYTRD_ONE_LAUNCH}[form]


# ---------------------------------------------------------------------------------------------------------------------------
# Tridiagonalisation
# ---------------------------------------------------------------------------------------------------------------------------
def run_sytrd(prof, ctx, A):
    """(d, e, tau, S, raw A buffer) of sdpsr_profile_sytrd on the lower triangle of A, after the checks of the written region"""
    n = A.shape[0]
    ld = _ld(n)
    a, M = _padded(R.poisoned_lower(A), ld)
    d, e, tau = _fill(n + GUARD), _fill(n + GUARD), _fill(n + GUARD)
    ctx.check(prof.sdpsr_profile_sytrd(ctx._h, n, ld, _vp(a), _vp(d), _vp(e), _vp(tau), GUARD))
    assert _untouched(a[ld * ld:]) and _untouched(d[n:]) and _untouched(e[n - 1:]) and _untouched(tau[n - 1:])
    assert _written(d[:n]) and _written(e[:n - 1]) and _written(tau[:n - 1])
    assert not _bits(M[n:, :]).any() and not _bits(M[:, n:]).any()  # the padding: never written, so still +0
    return d[:n].copy(), e[:n - 1].copy(), tau[:n - 1].copy(), M[:n, :n].copy(), a


def evaluate_device(A, d, e, tau, S):
    """The evaluator of eigen_stages_ref.py in float64 on the device (orders where a longdouble evaluation takes too long)."""
    import torch
    n = A.shape[0]
    dev = torch.device("cuda")
    V = torch.tril(torch.from_numpy(np.ascontiguousarray(S)).to(dev), -2)
    idx = torch.arange(n - 1, device=dev)
    V[idx + 1, idx] = 1.0
    Q = torch.eye(n, dtype=torch.float64, device=dev)
    for j in range(n - 2, -1, -1):
        if tau[j] == 0:
            continue
        v = V[j + 1:, j]
        blk = Q[j + 1:, j + 1:]
        blk -= float(tau[j]) * torch.outer(v, v @ blk)
    At = torch.from_numpy(np.array(A, dtype=np.float64)).to(dev)  # (a copy: the families are read-only arrays)
    B = Q.t() @ At @ Q
    B[idx + 1, idx] -= torch.from_numpy(np.ascontiguousarray(e)).to(dev)
    B[idx, idx + 1] -= torch.from_numpy(np.ascontiguousarray(e)).to(dev)
    B.diagonal().sub_(torch.from_numpy(np.ascontiguousarray(d)).to(dev))
    norm1 = float(At.abs().sum(dim=0).max())
    G = Q.t() @ Q
    G.diagonal().sub_(1.0)
    return float(B.abs().max()) / (norm1 if norm1 > 0 else 1.0), float(G.abs().max())


_lapack_device = {}


def _values(name, n, A, out):
    """(kernel's values, LAPACK's values) under one evaluator"""
    if n <= 300:
        return R.evaluate(A, *out), R.lapack_values(name, n)
    if (name, n) not in _lapack_device:
        _lapack_device[(name, n)] = evaluate_device(A, *R.lapack_sytrd(A))
    return evaluate_device(A, *out), _lapack_device[(name, n)]


SMALL = [("rows", n) for n in (129, 255, 256, 257, 640)] + [("panels", n) for n in (129, 160, 161, 257, 300)]
HYBRID = [(form, n) for form in ("hybrid", "hybrid_one_launch") for n in (2049, 2200)]
SYTRD_CASES = [(f, n, fam) for f, n in SMALL for fam in R.FAMILIES] + [(f, n, fam) for f, n in HYBRID for fam in ("gauss", "sum", "two", "scheme")]


@pytest.mark.parametrize("form,n,name", SYTRD_CASES)
def test_sytrd(pkg, prof, ctxs, form, n, name):
    """One form of the tridiagonalisation on one input family: backward error and orthogonality within 16 x LAPACK's, column 0 as
    dlarfg makes it, the exact structure of the structured families, the written region as sdpsr_prof.h documents it."""
    A = R.family(name, n)
    d, e, tau, S, _ = run_sytrd(prof, ctxs(_flags(pkg, form)), A)
    assert np.isfinite(d).all() and np.isfinite(e).all() and np.isfinite(tau).all()
    low = np.tril_indices(n, -2)
    assert np.isfinite(S[low]).all()
    # column 0 has no history: dlarfg's convention, to 4 ulp of the largest entry
    e0, tau0, v0 = R.column0(A)
    assert R.ulp_distance(e[0], e0) <= 4, (e[0], float(e0))
    assert R.ulp_distance(tau[0], tau0) <= 4, (tau[0], float(tau0))
    assert R.ulp_distance(S[2:, 0], v0) <= 4
    if name in ("tridiag", "diag", "zero"):
        assert (d == np.diag(A)).all() and (e == np.diag(A, -1)).all() and not tau.any() and not S[low].any()
    if name == "sum":
        for j in R.sum_boundaries(n):
            assert e[j] == 0 and tau[j] == 0, j
    (bk, ok), (bl, ol) = _values(name, n, A, (d, e, tau, S))
    _record(f"sytrd {form:18s} n={n:5d} {name:9s} backward {bk:.3e} / lapack {bl:.3e} = {bk / bl if bl else 0.0:6.2f}   "
            f"orthogonality {ok:.3e} / lapack {ol:.3e} = {ok / ol if ol else 0.0:6.2f}")
    assert bk <= MARGIN * bl and ok <= MARGIN * ol, (bk, bl, ok, ol)


@pytest.mark.parametrize("form,n", [("rows", 257), ("panels", 300), ("hybrid", 2049)])
def test_sytrd_replayed_graph_gives_a_fresh_contexts_bits(pkg, prof, form, n):
    """Two different matrices one after the other in one ctx -- the second call replays the graph the first one built, on buffers
    that hold the first one's results -- each give the bits a fresh ctx gives."""
    flags = _flags(pkg, form)
    mats = [R.family("gauss", n), R.family("scheme", n)]
    stats = (C.c_double * 3)()
    with pkg.Context(device=0, seed=1, flags=flags) as ctx:
        both = [run_sytrd(prof, ctx, A) for A in mats]
        ctx.check(prof.sdpsr_profile_sytrd_graphs(ctx._h, stats))
        assert (stats[0], stats[1]) == (1.0, 1.0), tuple(stats)  # one miss, then one hit
    for A, got in zip(mats, both):
        with pkg.Context(device=0, seed=1, flags=flags) as ctx:
            fresh = run_sytrd(prof, ctx, A)
        for x, y in zip(got, fresh):
            assert np.array_equal(_bits(x), _bits(y))


# ---------------------------------------------------------------------------------------------------------------------------
# Back-transformation
# ---------------------------------------------------------------------------------------------------------------------------
def run_backtransform(prof, ctx, S, tau, Z):
    n = S.shape[0]
    ld = _ld(n)
    a = R.poisoned_reflector_array(S, ld)
    z, M = _padded(Z, ld)
    t = np.ascontiguousarray(tau[:n - 1], dtype=np.float64)
    ctx.check(prof.sdpsr_profile_backtransform(ctx._h, n, ld, _vp(a), _vp(t), _vp(z), GUARD))
    assert _untouched(z[ld * ld:])
    assert not _bits(M[n:, :]).any() and not _bits(M[:, n:]).any()  # zero padding comes back as it was
    assert np.array_equal(_bits(M[0, :n]), _bits(np.ascontiguousarray(Z[0])))  # no reflector reaches row 0
    return M[:n, :n].copy()


@pytest.fixture(scope="module")
def used_ctx(pkg):
    """a ctx whose workspaces a full sdpsr_syev_f64 of a larger order (ld = 512, four blocks) has already used"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = pkg.load_library()
    n = 400
    A = np.asfortranarray(R.family("gauss", n))
    w, V = np.zeros(n), np.zeros((n, n), order="F")
    ctx = pkg.Context(device=0, seed=1)
    ctx.check(lib.sdpsr_syev_f64(ctx._h, n, _vp(A), _vp(w), _vp(V), 0))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", [129, 130, 257, 300])
def test_backtransform(prof, ctxs, used_ctx, n):
    """One full block of 128 reflectors (129), a second block of one reflector (130), two full blocks (257), a ragged last block
    (300); prepare and apply on the main stream.  The exact families with ==; the general one within 16 x the error of a float64 application."""
    Z = R.integer_z(n)
    exact = {make.__name__: (make(n), None) for make in (R.reflectors_signs, R.reflectors_swaps)}
    for key, ((S, tau), _) in list(exact.items()):
        exact[key] = ((S, tau), R.apply_reflectors(S, tau, Z))
    Sg, taug = R.reflectors_general(n)
    ref = R.apply_reflectors(Sg, taug, Z, R.LD)
    e_seq = float(np.abs(R.apply_reflectors(Sg, taug, Z) - ref).max())
    for label, ctx in (("fresh", ctxs(0)), ("used", used_ctx)):
        for key, ((S, tau), want) in exact.items():
            got = run_backtransform(prof, ctx, S, tau, Z)
            assert (got == want).all(), (label, key, int((got != want).sum()))
        got = run_backtransform(prof, ctx, Sg, taug, Z)
        e_k = float(np.abs(got - ref).max())
        _record(f"backtransform n={n:4d} {label:5s} general family: error {e_k:.3e} / float64 reflector by reflector {e_seq:.3e} = {e_k / e_seq:6.2f}")
        assert e_k <= MARGIN * e_seq, (label, e_k, e_seq)


# ---------------------------------------------------------------------------------------------------------------------------
# Divide and conquer
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 160, 255])
def test_stedc(prof, ctxs, n):
    """The tridiagonal solver alone at ld = 256 with 127, 96 and 1 padding rows, by the bounds of
    test_tridiagonal_divide_and_conquer_hard_cases."""
    ld = _ld(n)
    ctx = ctxs(0)
    for name in R.STEDC_CASES:
        d, e = R.stedc_case(name, n)
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        w = _fill(n + GUARD)
        z = _fill(ld * ld + GUARD)
        dd, ee = np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(e, dtype=np.float64)
        ctx.check(prof.sdpsr_profile_stedc(ctx._h, n, ld, _vp(dd), _vp(ee), _vp(w), _vp(z), GUARD))
        assert _untouched(w[n:]) and _untouched(z[ld * ld:]) and _written(w[:n]) and _written(z[:ld * ld])
        M = z[:ld * ld].reshape(ld, ld).T
        assert not M[n:, :].any() and not M[:, n:].any(), name
        V, wk = M[:n, :n], w[:n]
        wl = np.linalg.eigvalsh(T)
        sc = np.abs(wl).max()
        assert np.all(np.diff(wk) >= 0), (n, name)
        assert np.abs(wk - wl).max() <= 2e-13 * sc, (n, name, np.abs(wk - wl).max() / sc)
        assert np.abs(T @ V - V * wk).max() <= 1e-12 * sc, (n, name)
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12, (n, name)


# ---------------------------------------------------------------------------------------------------------------------------
# The whole solver
# ---------------------------------------------------------------------------------------------------------------------------
def _syev(pkg, ctx, A):
    """(status, w, V) of sdpsr_syev_f64 on host memory; the upper triangle handed over is poisoned"""
    lib = pkg.load_library()
    n = A.shape[0]
    B = np.asfortranarray(R.poisoned_lower(A))
    w, V = np.full(n, np.nan), np.full((n, n), np.nan, order="F")
    st = lib.sdpsr_syev_f64(ctx._h, n, _vp(B), _vp(w), _vp(V), 0)
    return st, w, V


STRUCTURED = [(n, "default", fam) for n in (100, 130, 300, 2200) for fam in ("sum", "sum_perm", "two", "diag", "zero")] + \
             [(300, "panels", fam) for fam in ("sum", "sum_perm", "two", "diag", "zero")]


@pytest.mark.parametrize("n,form,name", STRUCTURED)
def test_syev_structured(pkg, ctxs, n, form, name):
    """Direct sums (tau = 0 in the middle of panels and WY blocks), the two-eigenvalue scheme, diagonal and zero matrices through the
    Jacobi kernel (100), the row form (130, 300), the panel form (300) and the hybrid (2200): the bounds of
    test_syev_degenerate_spectrum_residual."""
    A = R.family(name, n)
    st, w, V = _syev(pkg, ctxs(pkg._lib.FLAG_SYTRD_PANELS if form == "panels" else 0), A)
    assert st == OK, st
    scale = np.abs(w).max()
    if name == "zero":
        assert not w.any()
    assert np.all(np.diff(w) >= 0)
    assert np.abs(A @ V - V * w).max() <= 1e-13 * scale * 8
    assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12
    assert np.abs(w - np.linalg.eigvalsh(A)).max() <= 1e-12 * scale


@pytest.mark.parametrize("n", [100, 130, 300])
@pytest.mark.parametrize("name", ["gauss", "scheme"])
def test_syev_scale(pkg, ctxs, name, n):
    """2^k A for k = -600 .. +480: LAPACK is right at every k (tests/test_eigen_stages_ref_cpu.py); the library either meets the same
    relative bounds or says it could not.  SDPSR_OK with anything else is the failure.  (Before the entry point scaled its copy,
    k = -600 came back SDPSR_OK with the input's diagonal (n = 100) or the eigenvalues of its tridiagonal part (130, 300), off by
    0.8 to 1.0 max |w|: every square in the reflector norms and in the Jacobi kernel's stopping rule had underflowed.)"""
    A = R.family(name, n)
    w0 = np.linalg.eigvalsh(A)
    scale = np.abs(w0).max()
    bad = []
    for k in R.SCALE_EXPONENTS:
        st, w, V = _syev(pkg, ctxs(0), np.ldexp(A, k))
        if st != OK:
            print(f"syev_scale {name} n={n} k={k}: status {st}")
            continue
        wu = np.ldexp(w, -k)  # exact: the eigenvalues are normal numbers at every k used
        err_w = np.abs(wu - w0).max() / scale
        res = np.abs(A @ V - V * wu).max() / scale
        orth = np.abs(V.T @ V - np.eye(n)).max()
        print(f"syev_scale {name} n={n} k={k}: status OK, |w - lapack| {err_w:.2e}, residual {res:.2e}, orthogonality {orth:.2e} (relative)")
        if not (np.isfinite(w).all() and err_w <= 1e-12 and res <= 8e-13 and orth < 1e-12):
            bad.append((k, err_w, res, orth))
    assert not bad, bad
