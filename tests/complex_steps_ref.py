"""Plain NumPy references for the steps of blockDiagonalize(P; complex = true) (csrc/kernels_complex.hip, csrc/complex.cpp), shared
by tests/test_complex_steps_ref_cpu.py and tests/test_gpu_complex_steps.py: the Hermitian test matrices, the restatements of the
gather, the block norms and the irreducible columns, the running error bound of each restatement, and the inputs of the GPU tests.

Bounds.  A sum of products evaluated in fp64, in any order, with or without FMA, is within gamma_k sum |terms| of its exact value,
gamma_k ~ k 2^-53, k the number of real terms.  The steps here are NESTED sums (V^H (H V), Q_j (Q_j^H (H q))): a leaf term passes
through one rounding per level, and the first-order bound is again (number of real leaf terms) 2^-53 times the same expression with
every factor replaced by its absolute value.  Every bound below is

    k 2^-53 * (the expression in absolute values),   k = TWICE the number of real leaf terms of one real component,

the factor 2 covering the second-order terms and the rounding of the long-double reference.  A complex factor z enters the
absolute expression as |Re z| + |Im z|, which bounds every real product a component of a complex product is made of; a complex
product doubles the number of real terms of a component.  Division and square root add their relative terms, written out where
they occur.  The bounds are judged on a float64 NumPy evaluation of the same formula (the CPU test), never on a kernel.

Nothing here touches the library."""
import functools

import numpy as np

import basis_image_complex_helpers as BH
import module_kernels_ref as MR
import syev_families as fam

U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
IM_KEY = 0xA5A5A5A55A5A5A5A  # cx_class_value: the imaginary part is drawn under key ^ IM_KEY

# ---------------------------------------------------------------------------------------------------------------------------
# The gather: H = A + A^H, A[r, c] = value(L[r, c])
# ---------------------------------------------------------------------------------------------------------------------------
GATHER_ORDERS = (1, 2, 17, 64, 65, 300)
GATHER_KEYS = (0x1234567, 0xFEDCBA9876543210)


def gather_labels(n):
    """Non-symmetric n x n labels 0..d with zeros (column-major, entry (r, c) at r + c n) and their d."""
    d = max(1, min(n * n // 3, 700))
    return MR.hashed_labels(n, d, salt=29), d


def gather_herm(n, L, key):
    """(Hr, Hi), n x n, of the Hermitian generic element: one fp64 addition resp. subtraction of two class values per entry, so
    the kernel's planes are these bit for bit."""
    Lm = np.asarray(L).reshape(n, n, order="F")
    ar, ai = MR.class_uniform(key, Lm), MR.class_uniform(key ^ IM_KEY, Lm)
    return ar + ar.T, ai - ai.T


# ---------------------------------------------------------------------------------------------------------------------------
# Hermitian test matrices
# ---------------------------------------------------------------------------------------------------------------------------
DRIVER_KEY = 0x5DEECE66D
OWN = ("imaginary antisymmetric", "unitary, two eigenvalues", "unitary, five eigenvalues", "driver Z_n", "driver C3", "driver S3")
# the families whose eigenvalues are simple with gaps far above the rounding level at every order used: the spectral projectors of
# single eigenvalues are compared between the routes on these
LOW_MULTIPLICITY = ("phased random symmetric", "real random symmetric", "phased arrow", "real arrow", "phased descending diagonal",
                    "real descending diagonal", "imaginary antisymmetric")
TWO_VALUES, FIVE_VALUES = (1.0, -2.0), (-1.5, -0.25, 0.5, 0.75, 2.0)


def names(n, extreme=True):
    """The Hermitian families that exist at order n: every family of syev_families.py as H = D A D^H ("phased") and as A itself
    ("real"), and the families of this file."""
    base = fam.names(n, extreme)
    out = ["phased " + f for f in base] + ["real " + f for f in base] + list(OWN[:4])
    return out + (["driver C3"] if n == 3 else []) + (["driver S3"] if n == 6 else [])


def is_extreme(name):
    return name.split(" ", 1)[-1] in fam.EXTREME


def _unitary(n, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return Q


def driver_labels(name, n):
    if name == "driver Z_n":
        return BH.directed(n)
    return {"driver C3": BH.C3, "driver S3": BH.s3_cayley_labels()}[name]


def _build(name, n):
    rng = np.random.default_rng([n, sum(map(ord, name)), 77])
    kind, _, base = name.partition(" ")
    if kind in ("phased", "real") and base in fam.FAMILIES:
        A, wl, _ = fam.reference(base, n)
        if kind == "real":
            return A.astype(np.complex128), wl
        D = np.exp(2j * np.pi * rng.random(n))  # H = D A D^H: the spectrum of A, complex off-diagonal entries
        H = D[:, None] * A * np.conj(D)[None, :]
        return H, wl
    if name == "imaginary antisymmetric":  # Hr = 0; the spectrum is symmetric about 0, with a zero eigenvalue at odd n
        S = rng.standard_normal((n, n))
        return 1j * (S - S.T), None
    if name.startswith("unitary"):
        vals = TWO_VALUES if "two" in name else FIVE_VALUES
        Q = _unitary(n, rng)
        return (Q * np.resize(vals, n)) @ Q.conj().T, None
    L = driver_labels(name, n)  # the driver's own element: A + A^H of the complex class values
    Hr, Hi = gather_herm(n, L.ravel(order="F"), DRIVER_KEY)
    return Hr + 1j * Hi, None


@functools.lru_cache(maxsize=None)
def hermitian(name, n):
    """(H complex128, exactly Hermitian; the reference spectrum; |H| = max |eigenvalue|, or 1 for the zero matrix).  The reference
    spectrum of a phased or real family is LAPACK's REAL spectrum of A (syev_families.reference); of the other families LAPACK's
    Hermitian one.  Made once, read-only."""
    H, wl = _build(name, n)
    H = (H + H.conj().T) / 2  # exactly Hermitian; a relative perturbation of one rounding
    H[np.diag_indices(n)] = H.diagonal().real
    if wl is None:
        wl = np.linalg.eigvalsh(H)
    H.setflags(write=False)
    wl = np.array(wl)
    wl.setflags(write=False)
    return H, wl, float(np.abs(wl).max()) or 1.0


def smallest_gap(name, n):
    """The smallest gap of the reference spectrum (inf at n = 1)."""
    wl = hermitian(name, n)[1]
    return float(np.diff(wl).min()) if wl.size > 1 else np.inf


HEEV_BOUNDS = (2e-13, 1e-12, 1e-12)  # eigenvalues / |H|, residual / |H|, orthogonality: the figures of the real twin
HEEV0_FAMILY_ORDERS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 33, 34, 63, 64)  # (6: the order of "driver S3")
HEEV1_ORDERS = (1, 2, 33, 64, 65, 96, 127, 128, 129, 200)
PROJECTOR_QUOTIENT = 1e-6


def heev0_cases():
    cases = [("phased random symmetric", n) for n in range(1, 65)]
    return cases + [(name, n) for n in HEEV0_FAMILY_ORDERS for name in names(n) if (name, n) not in cases]


def heev1_cases(n):
    return [(name, n) for name in names(n, extreme=False)]


def heev1_atol(sc):
    """The cluster tolerance handed to the embedding route: twice the eigenvalue bound of the real solver.  Each eigenvalue of H
    shows up twice in the embedding, each copy within HEEV_BOUNDS[0] |H| of it, so the two are never separated; and the eigenvectors
    of a cluster, which the route does not match to single eigenvalues, keep a residual of the order of this figure."""
    return 2 * HEEV_BOUNDS[0] * sc


def projector_cases():
    """(name, n) with both routes and simple, well-separated eigenvalues."""
    return [(name, n) for n in HEEV1_ORDERS if n <= 64 for name in LOW_MULTIPLICITY if name in names(n)]


# ---------------------------------------------------------------------------------------------------------------------------
# Block norms: norms[sa, sb] = max |(V^H H V)[a, b]| over a in space sa, b in space sb
# ---------------------------------------------------------------------------------------------------------------------------
NORM_ORDERS = {0: (1, 2, 5, 33, 64), 1: (1, 2, 5, 33, 64, 65, 128, 130, 200)}


def abs1(Z):
    """|Re z| + |Im z| entrywise."""
    return np.abs(Z.real) + np.abs(Z.imag)


def partitions(n):
    """name -> space_of (int32, n entries): one space, n spaces, spaces of sizes 1 / 2 / rest (as far as n goes)."""
    out = {"one space": np.zeros(n, dtype=np.int32), "n spaces": np.arange(n, dtype=np.int32)}
    if n >= 4:
        out["1 / 2 / rest"] = np.array([0, 1, 1] + [2] * (n - 3), dtype=np.int32)
    return out


def _block_max(X, space_of, neig):
    """max of the non-negative X over every pair of spaces; 0 for a pair with an empty space"""
    out = np.zeros((neig, neig), dtype=X.dtype)
    np.maximum.at(out, (space_of[:, None], space_of[None, :]), X)
    return out


def block_norms(H, V, space_of, neig, dtype=CLD):
    """(norms, bound), neig x neig, pair (sa, sb) at [sa, sb] -- the kernel's norms[sa * neig + sb].  One real component of
    (V^H H V)[a, b] = sum_k conj(V[k, a]) sum_l H[k, l] V[l, b] has 2n * 2n real leaf terms: k = 8 n^2, and both components are
    within  k 2^-53 (|V|^T |H| |V|)[a, b]  of the exact ones; the magnitude of a complex number moves by at most sqrt(2) < 2
    times that, and  sqrt(re^2 + im^2)  adds 4 roundings' worth of relative error:

        bound[a, b] = 2 * 8 n^2 2^-53 (|V|^T |H| |V|)[a, b] + 4 2^-53 |G[a, b]|,

    and a maximum moves by no more than the largest bound of its block."""
    n = H.shape[0]
    real = np.float64 if dtype == np.complex128 else LD
    G = V.astype(dtype).conj().T @ (H.astype(dtype) @ V.astype(dtype))
    mag = np.sqrt(G.real * G.real + G.imag * G.imag)
    entry = 2 * 8 * n * n * U * (abs1(V).T @ (abs1(H) @ abs1(V))) + 4 * U * mag.astype(np.float64)
    return _block_max(mag.astype(real), space_of, neig), _block_max(entry, space_of, neig)


def gaussian_integers(n, seed):
    """(H, V): small Gaussian-integer entries, H Hermitian, V any (not unitary): every entry of V^H H V is an exact integer pair."""
    rng = np.random.default_rng([n, seed])
    A = rng.integers(-3, 4, (n, n)) + 1j * rng.integers(-3, 4, (n, n))
    H = A + A.conj().T
    V = rng.integers(-2, 3, (n, n)) + 1j * rng.integers(-2, 3, (n, n))
    return H, V


def block_norms_exact(H, V, space_of, neig):
    """max (re^2 + im^2) per pair of spaces, exactly, in int64 (0 for a pair with an empty space): the norm is the correctly rounded
    square root of an integer below 2^53.  H need not be Hermitian."""
    def ints(Z):
        r, i = Z.real.astype(np.int64), Z.imag.astype(np.int64)
        assert np.array_equal(r, Z.real) and np.array_equal(i, Z.imag)
        return r, i
    (hr, hi), (vr, vi) = ints(H), ints(V)
    tr, ti = hr @ vr - hi @ vi, hr @ vi + hi @ vr  # T = H V
    gr, gi = vr.T @ tr + vi.T @ ti, vr.T @ ti - vi.T @ tr  # G = conj(V)' T
    sq = gr * gr + gi * gi
    # every partial sum of every order of summation is an integer below 2^53, and so are the squares: exact in fp64 too
    assert float((abs1(V).T @ (abs1(H) @ abs1(V))).max()) < 2 ** 53 and int(sq.max()) < 2 ** 53
    return _block_max(sq, space_of, neig)


def random_complex(n, seed):
    """(H, V): a Hermitian Gaussian H and a unitary V."""
    rng = np.random.default_rng([n, seed, 5])
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return A + A.conj().T, _unitary(n, rng)


# ---------------------------------------------------------------------------------------------------------------------------
# Irreducible columns
# ---------------------------------------------------------------------------------------------------------------------------
def _h_times(H, q, dtype):
    """H q in `dtype`, rows in chunks (H is not converted whole: 4096^2 long-double complex numbers are half a gigabyte)."""
    out = np.empty(H.shape[0], dtype=dtype)
    qd = q.astype(dtype)
    for r0 in range(0, H.shape[0], 512):
        out[r0:r0 + 512] = H[r0:r0 + 512].astype(dtype) @ qd
    return out


def irreducible(H, V, desc, atol, dtype=CLD):
    """(Q-hat n x ncols UNCLAMPED, bound n x ncols on each real component, norms) for desc rows {kind, i0, mi, j0, mj, col}.
    kind 0: column = V[:, i0], bound 0.  kind 1, with Q_i = V[:, i0:i0 + mi], Q_j = V[:, j0:j0 + mj], q_x1 their first columns:

        y = Q_j (Q_j^H (H q_i1)),   s = Q_i^H (H q_j1),   nrm = |s|_2,   column = y (1 / nrm).

    A component of y[r] has 2 mj * 2n * 2n real leaf terms (k = 16 mj n^2) under Y = |Q_j| (|Q_j|^T (|H| |q_i1|)); a component of
    s[a] has 2n * 2n (k = 8 n^2) under S = |Q_i|^T (|H| |q_j1|).  |s|_2 moves by at most the 2-norm of the error of s, which is
    sqrt(2) < 2 times the 2-norm of the component bounds; the sum of the 2 mi squares and the square root add (2 mi + 2) roundings:

        dnrm = 2 * 8 n^2 2^-53 |S|_2 + (2 mi + 2) 2^-53 nrm,
        bound[r] = 16 mj n^2 2^-53 Y[r] / nrm + |y[r]| / nrm * (dnrm / nrm + 4 2^-53)

    (the reciprocal, the product with it, and the first-order quotient rule; 4 instead of 2 roundings for the second order).
    The clamp: entries whose magnitude is < atol become +0.0; see clamp()."""
    n = H.shape[0]
    ncols = len(desc)
    Q = np.zeros((n, ncols), dtype=dtype)
    bound = np.zeros((n, ncols))
    nrms = np.zeros(ncols)
    Ha = None
    prod = {}

    def h_times(c0):
        if c0 not in prod:
            prod[c0] = (_h_times(H, V[:, c0], dtype), _h_times(Ha, abs1(V[:, c0]), np.float64))
        return prod[c0]
    for kind, i0, mi, j0, mj, col in desc:
        if kind == 0:
            Q[:, col] = V[:, i0]
            continue
        if Ha is None:
            Ha = abs1(H)
        Qi, Qj = V[:, i0:i0 + mi], V[:, j0:j0 + mj]
        (t, ta), (u, ua) = h_times(i0), h_times(j0)
        y = Qj.astype(dtype) @ (Qj.astype(dtype).conj().T @ t)
        s = Qi.astype(dtype).conj().T @ u
        nrm = np.sqrt((s.real * s.real + s.imag * s.imag).sum())
        Y = abs1(Qj) @ (abs1(Qj).T @ ta)
        S = abs1(Qi).T @ ua
        nrm64 = float(nrm)
        dnrm = 2 * 8 * n * n * U * float(np.sqrt((S * S).sum())) + (2 * mi + 2) * U * nrm64
        Q[:, col] = y * (1 / nrm)
        bound[:, col] = 16 * mj * n * n * U * Y / nrm64 + np.abs(y).astype(np.float64) / nrm64 * (dnrm / nrm64 + 4 * U)
        nrms[col] = nrm64
    return Q, bound, nrms


def clamp(Q, bound, atol):
    """(clamped Q as complex128, mask of the clamped entries, whether atol is SAFE): the kernel clamps on sqrt(re^2 + im^2) < atol of
    its own column; that magnitude is within 2 bound + 4 2^-53 |q| of the reference's, so the reference decides every entry as the
    kernel does when no reference magnitude is that close to atol."""
    mag = np.abs(Q).astype(np.float64)
    safe = bool((np.abs(mag - atol) > 2 * bound + 4 * U * mag).all())
    mask = mag < atol
    out = Q.astype(np.complex128)
    out[mask] = 0
    return out, mask, safe


def orthonormal_columns(n, cols, seed):
    rng = np.random.default_rng([n, cols, seed])
    Q, _ = np.linalg.qr(rng.standard_normal((n, cols)) + 1j * rng.standard_normal((n, cols)))
    return Q


def _choose_atol(mags, bound):
    """A threshold that clamps at least one and at most half of the entries: the midpoint between two consecutive magnitudes, the
    highest one that is as far from every magnitude as clamp() asks."""
    order = np.argsort(mags.ravel())
    m, tol = mags.ravel()[order], (2 * bound + 4 * U * mags).ravel()[order]
    hi = m.size // 2 + 1
    mid = (m[1:hi] + m[:hi - 1]) / 2
    for k in range(hi - 2, -1, -1):
        if (np.abs(m - mid[k]) > tol).all():
            return float(mid[k])
    raise AssertionError("no threshold is far enough from every magnitude")


def irreducible_case(n):
    """(H, V, desc int32 ncols x 6, atol, Q-hat reference clamped, bound, mask) of the irreducible test at order n.  Small orders: a
    Hermitian Gaussian H, V with orthonormal columns from a complex QR, a kind-0 column and kind-1 columns with
    (mi, mj) in {(1, 1), (2, 3), (3, 2), (n/2, n/2)} as far as they fit.  n = 600: (mi, mj) = (257, 300).  n >= 3370: Gaussian H
    and V (8 columns of norm ~1, nothing orthogonal: the formula needs no eigenvectors), a kind-0 column and (2, 3), (3, 2).
    atol clamps some entries of the columns and is safe (clamp()): asserted here.  (The large orders are made afresh at every call:
    a quarter of a gigabyte each.)"""
    return _irreducible_case(n) if n >= 3370 else _irreducible_case_kept(n)


def _irreducible_case(n):
    rng = np.random.default_rng([n, 41])
    large = n >= 3370
    if large:
        H = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        V = (rng.standard_normal((n, 8)) + 1j * rng.standard_normal((n, 8))) / np.sqrt(2 * n)
        rows = [(0, 7, 1, 0, 1), (1, 0, 2, 2, 3), (1, 2, 3, 0, 2)]
    else:
        A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        H = A + A.conj().T
        if n == 600:
            shapes = [(257, 300)]
        else:
            shapes = [s for s in ((1, 1), (2, 3), (3, 2), (n // 2, n // 2)) if s[0] + s[1] <= n and min(s) >= 1]
            shapes = list(dict.fromkeys(shapes))
        V = orthonormal_columns(n, max(mi + mj for mi, mj in shapes), 43)
        rows = [(0, V.shape[1] - 1, 1, 0, 1)] + [(1, 0, mi, mi, mj) for mi, mj in shapes]
        rows += [(1, mi, mj, 0, mi) for mi, mj in shapes[:1]]  # the root behind the member: i0 > j0
    desc = np.array([r + (c,) for c, r in enumerate(rows)], dtype=np.int32)
    Q, bound, nrms = irreducible(H, V, [tuple(int(x) for x in r) for r in desc], 0.0)
    assert (nrms[desc[:, 0] == 1] > 0).all()
    mags = np.abs(Q).astype(np.float64)
    atol = _choose_atol(mags, bound)
    ref, mask, safe = clamp(Q, bound, atol)
    assert safe and mask.any() and not mask.all(), (n, atol)
    for a in (H, V, desc, ref, bound, mask):
        a.setflags(write=False)
    return H, V, desc, atol, ref, bound, mask


_irreducible_case_kept = functools.lru_cache(maxsize=None)(_irreducible_case)
IRREDUCIBLE_BOTH = (2, 7, 64)
IRREDUCIBLE_GENERAL = (65, 600, 3370, 3371, 4096)
