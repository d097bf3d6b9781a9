"""References for the stages of the dense symmetric eigensolver (csrc/kernels_sytrd.hip, kernels_sytrd_look.hip, kernels_stedc.hip,
kernels_backtransform.hip and the driver in csrc/eigen.cpp), shared by tests/test_eigen_stages_ref_cpu.py (no GPU: the references
against LAPACK and against themselves) and tests/test_gpu_eigen_stages.py (the kernels against the references).

Conventions.  A tridiagonalisation is (d, e, tau, reflectors) in LAPACK's dsytrd layout for uplo = 'L': A = Q T Q' with
Q = H_0 ... H_{n-2}, H_j = I - tau_j v_j v_j', v_j = [0 .. 0, 1 in row j+1, S[j+2 .., j]] for the stored array S.  Nothing here
looks at a kernel's output to choose a bound."""
import functools

import numpy as np

LD = np.longdouble
FAMILIES = ("gauss", "sum", "sum_perm", "two", "scheme", "diag", "zero", "tridiag")
SUM_BLOCKS = (1, 40, 1, 60)  # then one block with the rest
POISON = 1e300               # the upper triangle handed to an entry point: only the lower one is referenced
SCALE_EXPONENTS = (-600, -300, 0, 300, 480)
LONGDOUBLE_MAX_N = 257       # above: float64 evaluations


def sum_blocks(n):
    """Orders of the direct summands at order n: 1, 40, 1, 60, n - 102, cut off at n (orders <= 102 lose the tail)."""
    out, left = [], n
    for b in SUM_BLOCKS + (max(n - sum(SUM_BLOCKS), 0),):
        b = min(b, left)
        if b > 0:
            out.append(b)
        left -= b
    return out


def sum_boundaries(n):
    """The columns j whose subdiagonal entry (j+1, j) lies between two summands."""
    return [int(j) for j in np.cumsum(sum_blocks(n))[:-1] - 1]


def _gauss(rng, m):
    G = rng.standard_normal((m, m))
    return (G + G.T) / 2


@functools.lru_cache(maxsize=None)
def _family(name, n):
    rng = np.random.default_rng(1000 * n + FAMILIES.index(name))
    if name == "gauss":
        A = _gauss(rng, n)
    elif name in ("sum", "sum_perm"):
        rng = np.random.default_rng(1000 * n + 1)  # the same summands for both
        A = np.zeros((n, n))
        o = 0
        for b in sum_blocks(n):
            A[o:o + b, o:o + b] = _gauss(rng, b)
            o += b
        if name == "sum_perm":
            p = np.random.default_rng(7).permutation(n)
            A = A[np.ix_(p, p)]
    elif name == "two":
        A = np.full((n, n), 0.25) + 0.5 * np.eye(n)
    elif name == "scheme":
        k = np.arange(n)
        dist = np.abs(k[:, None] - k[None, :])
        A = rng.random(n // 2 + 1)[np.minimum(dist, n - dist)]  # class of (i, j) in the cyclic scheme: the distance on the cycle
    elif name == "diag":
        A = np.diag(np.repeat(rng.standard_normal(5), n // 5 + 1)[:n])
    elif name == "zero":
        A = np.zeros((n, n))
    elif name == "tridiag":
        e = rng.standard_normal(n - 1)
        A = np.diag(rng.standard_normal(n)) + np.diag(e, 1) + np.diag(e, -1)
    else:
        raise KeyError(name)
    A = np.ascontiguousarray(A)
    assert np.array_equal(A, A.T)
    A.setflags(write=False)
    return A


def family(name, n):
    """The symmetric n x n matrix of an input family (float64, read-only, the same at every call)."""
    return _family(name, int(n))


def poisoned_lower(A):
    """A with the strict upper triangle replaced by POISON."""
    B = np.array(A, dtype=np.float64)
    B[np.triu_indices(B.shape[0], 1)] = POISON
    return B


# ---------------------------------------------------------------------------------------------------------------------------
# Tridiagonalisation
# ---------------------------------------------------------------------------------------------------------------------------
def _reflector(S, j, dtype):
    n = S.shape[0]
    v = np.zeros(n - j - 1, dtype=dtype)  # rows j+1 .. n-1
    v[0] = 1
    v[1:] = S[j + 2:, j]
    return v


def accumulate_q(tau, S, dtype):
    """Q = H_0 ... H_{n-2}: H_j applied to the identity, last reflector first (only the trailing block changes), in `dtype`."""
    n = S.shape[0]
    S = np.asarray(S)
    Q = np.eye(n, dtype=dtype)
    for j in range(n - 2, -1, -1):
        if tau[j] == 0:
            continue
        v = _reflector(S, j, dtype)
        Q[j + 1:, j + 1:] -= dtype(tau[j]) * np.outer(v, v @ Q[j + 1:, j + 1:])
    return Q


_SPLIT_BITS, _SPLIT_PIECES = 17, 4


def _split(X):
    """X (longdouble) = s * (X_1 + X_2 + X_3 + X_4) up to 2^-68 s: s a power of two >= max |X|, X_i float64 arrays that are integers
    of at most 17 bits on the grid 2^(-17 i)."""
    X = np.asarray(X, dtype=LD)
    big = float(np.abs(X).max())
    s = LD(2.0) ** int(np.ceil(np.log2(big))) if big > 0 else LD(1)
    rest = X / s
    out = []
    for i in range(1, _SPLIT_PIECES + 1):
        g = LD(2.0) ** (_SPLIT_BITS * i)
        p = np.rint(rest * g) / g
        rest = rest - p
        out.append(np.asarray(p, dtype=np.float64))
    return s, out


def matmul_ld(X, Y):
    """X @ Y in longdouble at the speed of float64 BLAS: both factors are split into 17-bit pieces, whose float64 products are
    EXACT (integers below 2^(34 + log2 k) <= 2^53 for an inner dimension k <= 2^19), and the piece products are added in longdouble.
    Dropped: piece pairs below 2^-102 of the result's scale.  (A plain longdouble matmul of order 640 takes seconds; a plain
    float64 one errs by 6e-15 on a column of 640 equal entries, more than what the evaluator is there to measure.)"""
    assert X.shape[1] <= 1 << 19
    sx, xs = _split(X)
    sy, ys = _split(Y)
    out = np.zeros((X.shape[0], Y.shape[1]), dtype=LD)
    for i, xi in enumerate(xs):
        for j, yj in enumerate(ys):
            if i + j <= _SPLIT_PIECES:
                out += xi @ yj
    return out * (sx * sy)


def evaluate_products(A, d, e, Q, matmul=matmul_ld):
    """(||Q'AQ - T||_max / ||A||_1, ||Q'Q - I||_max) from Q by three products (numpy arrays).  ||A||_1 = 0 divides by 1."""
    n = A.shape[0]
    dtype = Q.dtype.type
    A = np.asarray(A, dtype=dtype)
    T = np.zeros((n, n), dtype=dtype)
    idx = np.arange(n)
    T[idx, idx] = np.asarray(d[:n], dtype=dtype)
    T[idx[1:], idx[:-1]] = np.asarray(e[:n - 1], dtype=dtype)
    T[idx[:-1], idx[1:]] = np.asarray(e[:n - 1], dtype=dtype)
    norm1 = np.abs(A).sum(axis=0).max()
    bwd = np.abs(matmul(Q.T, matmul(A, Q)) - T).max() / (norm1 if norm1 > 0 else 1)
    orth = np.abs(matmul(Q.T, Q) - np.eye(n, dtype=dtype)).max()
    return float(bwd), float(orth)


def evaluate(A, d, e, tau, S):
    """The evaluator: Q = H_0 ... H_{n-2} from (tau, reflectors), then ||Q'AQ - T||_max / ||A||_1 and ||Q'Q - I||_max, all in
    longdouble (the products by matmul_ld).  Every entry of Q'AQ is kept: nothing is assumed to vanish.  Cost: n^3 / 3 longdouble
    operations for Q (0.15 s at n = 257, 1.5 s at 640); the orders of the hybrid form are evaluated in float64 on the device
    instead (test_gpu_eigen_stages.py)."""
    return evaluate_products(A, d, e, accumulate_q(tau, S, LD))


def lapack_sytrd(A):
    """(d, e, tau, S) of LAPACK's dsytrd, uplo = 'L'."""
    import scipy.linalg.lapack as ll
    c, d, e, tau, info = ll.dsytrd(np.asfortranarray(A), lower=1)
    assert info == 0
    return d, e, tau, c


@functools.lru_cache(maxsize=None)
def lapack_values(name, n):
    """The evaluator's two values for LAPACK's dsytrd on a family: the yardstick of the kernels' backward error."""
    A = family(name, n)
    return evaluate(A, *lapack_sytrd(A))


def column0(A):
    """(e_0, tau_0, v_0 below the unit entry) of the first reflector by dlarfg's convention, in longdouble."""
    a = np.asarray(A[1:, 0], dtype=LD)
    alpha, x = a[0], a[1:]
    xn2 = (x * x).sum()
    if xn2 == 0:  # H = I
        return alpha, LD(0), np.zeros(len(x), dtype=LD)
    beta = -np.copysign(np.sqrt(alpha * alpha + xn2), alpha)
    return beta, (beta - alpha) / beta, x / (alpha - beta)


def ulp_distance(got, ref):
    """max |got - ref| in units of the last place of the largest |ref| entry (float64 spacing)."""
    ref = np.atleast_1d(np.asarray(ref, dtype=LD))
    got = np.atleast_1d(np.asarray(got, dtype=LD))
    if ref.size == 0:
        return 0.0
    big = float(np.abs(ref).max())
    diff = float(np.abs(got - ref).max())
    if diff == 0:
        return 0.0
    return diff / float(np.spacing(big)) if big > 0 else np.inf


# ---------------------------------------------------------------------------------------------------------------------------
# Back-transformation
# ---------------------------------------------------------------------------------------------------------------------------
BT_BLOCK = 128


def reflectors_signs(n):
    """v_j = e_{j+1}, tau_j in {0, 2}: Q is a diagonal of +-1.  Returns (S, tau): S n x n with the stored entries (none), tau n-1."""
    tau = np.where(np.arange(n - 1) % 3 == 1, 0.0, 2.0)
    tau[n - 2] = 2.0
    return np.zeros((n, n)), tau


def reflectors_swaps(n):
    """v_j = e_{j+1} + e_{j+2}, tau_j = 1: H_j swaps rows j+1, j+2 with a sign; tau = 0 at every 37th column and at column n-2 (whose
    v has no second entry).  Q is a signed row permutation whose cycles run across the block boundaries."""
    S = np.zeros((n, n))
    j = np.arange(n - 2)
    S[j + 2, j] = 1.0
    tau = np.ones(n - 1)
    tau[36::37] = 0.0
    tau[n - 2] = 0.0
    return S, tau


def reflectors_general(n, seed=0):
    """Gaussian entries below the unit entry, scaled by 1/sqrt(n) so that v'v lies in [1, 2] and the product of n - 1 factors
    I - tau v v' (not orthogonal: the WY identity holds for any tau) stays far inside the range; tau from {0} and [0.5, 2]."""
    rng = np.random.default_rng(500 + n + seed)
    S = np.tril(rng.standard_normal((n, n)), -2) / np.sqrt(n)
    tau = rng.uniform(0.5, 2.0, n - 1)
    tau[rng.random(n - 1) < 0.15] = 0.0
    return S, tau


def integer_z(n, seed=0):
    return np.random.default_rng(900 + n + seed).integers(-9, 10, (n, n)).astype(np.float64)


def apply_reflectors(S, tau, Z, dtype=np.float64):
    """Q Z = H_0 (H_1 (... H_{n-2} Z)), reflector by reflector, in `dtype`."""
    n = S.shape[0]
    Z = np.array(Z, dtype=dtype)
    for j in range(n - 2, -1, -1):
        if tau[j] == 0:
            continue
        v = _reflector(S, j, dtype)
        Z[j + 1:, :] -= dtype(tau[j]) * np.outer(v, v @ Z[j + 1:, :])
    return Z


def block_wy(S, tau, Z, trace=None):
    """The library's block algorithm restated in float64: per block of 128 reflectors G = V'V, T by the dlarft recurrence
    (T[j, j] = tau_j, T[:j, j] = -tau_j T[:j, :j] G[:j, j]), X = T'V', W = V'Z, Z -= X'W; last block first.
    trace (a list) receives (T, W) per block."""
    n = S.shape[0]
    Z = np.array(Z, dtype=np.float64)
    nblk = (n - 1 + BT_BLOCK - 1) // BT_BLOCK
    for b in range(nblk - 1, -1, -1):
        V = np.zeros((n, BT_BLOCK))
        t = np.zeros(BT_BLOCK)
        for c in range(BT_BLOCK):
            j = BT_BLOCK * b + c
            if j <= n - 2:
                V[j + 1:, c] = _reflector(S, j, np.float64)
                t[c] = tau[j]
        G = V.T @ V
        T = np.zeros((BT_BLOCK, BT_BLOCK))
        for c in range(BT_BLOCK):
            T[:c, c] = -t[c] * (T[:c, :c] @ G[:c, c])
            T[c, c] = t[c]
        X = T.T @ V.T
        W = V.T @ Z
        Z -= X.T @ W
        if trace is not None:
            trace.append((T, W))
    return Z


def poisoned_reflector_array(S, ld):
    """ld x ld column-major array for an entry point: the stored reflector entries in place, POISON everywhere else inside n x n
    (the diagonal, the subdiagonal and the upper triangle are not the back-transformation's to read), zero padding."""
    n = S.shape[0]
    B = np.full((n, n), POISON)
    low = np.tril_indices(n, -2)
    B[low] = S[low]
    out = np.zeros((ld, ld))
    out[:n, :n] = B
    return np.asfortranarray(out)


# ---------------------------------------------------------------------------------------------------------------------------
# Divide and conquer
# ---------------------------------------------------------------------------------------------------------------------------
STEDC_CASES = ("1-2-1", "decoupled blocks", "glued wilkinson")


def stedc_case(name, n):
    """(d, e) of the hard tridiagonal matrices of test_tridiagonal_divide_and_conquer_hard_cases that the stage test uses."""
    rng = np.random.default_rng(n)
    if name == "1-2-1":
        return 2 * np.ones(n), -np.ones(n - 1)
    if name == "decoupled blocks":
        return rng.standard_normal(n), rng.standard_normal(n - 1) * (rng.random(n - 1) < 0.5)
    if name == "glued wilkinson":
        return np.tile(np.abs(np.arange(21) - 10.0), n // 21 + 1)[:n], np.where((np.arange(n - 1) + 1) % 21 == 0, 1e-8, 1.0)
    raise KeyError(name)
