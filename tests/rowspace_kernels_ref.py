"""Plain NumPy references for the row-space kernels of sdpsr_compress_constraints (csrc/kernels_rowspace.hip), the launchers' shape
rules restated, and the inputs of tests/test_gpu_rowspace_kernels.py -- shared with tests/test_rowspace_kernels_ref_cpu.py, which
checks the references and every precondition the GPU tests rely on.

Exact references: where the inputs are small integers (times a power of two) every partial sum of a product is an exactly
representable number whatever the order of summation, so the result is formed in int64 and compared bit for bit.  Real input:
the product is formed in np.longdouble and comes back with the matrix the rounding bound of a dot product is stated in,

    |fl(sum a_i b_i) - sum a_i b_i|  <=  gamma_n sum |a_i b_i|,   gamma_n = n u / (1 - n u),  u = 2^-53,

which holds for every order of summation, with or without FMA.

Nothing here touches the library."""
import numpy as np

U = 2.0 ** -53
DBL_MAX = float(np.finfo(np.float64).max)
LD_EPS = float(np.finfo(np.longdouble).eps) / 2  # the unit roundoff of the reference's own arithmetic (2^-64 with x87 long doubles)


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------------------
# the launchers' shape rules (csrc/kernels_rowspace.hip), restated
# ---------------------------------------------------------------------------------------------------------------------------
def gram_shape(m, ncols):
    """rowspace_gram_shape: (npairs, Z, cps) -- 64 x 64 block pairs of the lower triangle, K splits, columns per split."""
    nb = (m + 63) // 64
    npairs = nb * (nb + 1) // 2
    zmax = max(1, 2048 // npairs)
    z = min(max((ncols + 63) // 64, 1), zmax)
    cps = ((ncols + z - 1) // z + 3) // 4 * 4
    return npairs, max(1, (ncols + cps - 1) // cps), cps


def chunk(m, rotate=True):
    """rowspace_chunk: (cc, j_lds) -- columns per workgroup; J sits in LDS beside them while m * m + m <= 4000 doubles (the
    rotation only: the write-out stages no J)."""
    lds = 8000
    fits = rotate and m * m + m <= lds // 2
    room = lds - m * m if fits else lds
    return min(64, max(1, room // m)), int(fits)


def absmax_blocks(total):
    return min(1024, max(1, (total + 2047) // 2048))


# (m, ncols): (npairs, Z, cps) as the issue of these tests lists them; None = not listed there (Z capped by zmax)
GRAM_TABLE = {
    (1, 1): (1, 1, 4), (5, 2): (1, 1, 4), (15, 5): (1, 1, 8), (16, 64): (1, 1, 64), (17, 65): (1, 2, 36), (62, 130): (1, 3, 44),
    (63, 130): (1, 3, 44), (64, 256): (1, 4, 64), (65, 257): (3, 5, 52), (128, 67): (3, 2, 36), (129, 70): (6, 2, 36),
    (200, 1027): (10, 17, 64), (200, 13100): (10, None, None), (1024, 9): (136, 1, 12), (1024, 1000): (136, None, None),
    (3, 131075): (1, 1928, 68),
}
GRAM_SHAPES = tuple(GRAM_TABLE)
ROTATE_M = (1, 5, 62, 63, 64, 65, 200, 1024)
FINISH_M = (1, 63, 200, 1024)
FINISH_NCOLS = 300  # > 260, no multiple of 256, and no multiple of the chunk (64, 64, 40, 7) of any FINISH_M
DROPTOL = 1e-8


def rotate_ncols(m):
    """One ragged last chunk of every size 1, 2, 3 mod 4, a matrix narrower than four columns, and (cc = 7) a chunk of 4."""
    cc = chunk(m)[0]
    return (cc + 1, 2 * cc + 2, 3 * cc + 3, 2) + ((4,) if cc % 4 else ())


def last_chunk(ncols, cc):
    return ncols - (ncols - 1) // cc * cc


# ---------------------------------------------------------------------------------------------------------------------------
# scale
# ---------------------------------------------------------------------------------------------------------------------------
def scale_of(mx):
    """rowspace_scale_of: 2^-e, e the frexp exponent of mx, capped at 2^1000; 1 for mx = 0."""
    if not mx > 0.0:
        return 1.0
    e = -int(np.frexp(mx)[1])
    return float(np.ldexp(1.0, min(e, 1000)))


def scale_ref(M):
    """(M * scale, max |M| over the finite entries, 1.0 if an entry is not finite)."""
    M = np.asarray(M, dtype=np.float64)
    a = np.abs(M)
    ok = a <= DBL_MAX
    mx = float(a[ok].max()) if ok.any() else 0.0
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        W = M * scale_of(mx)
    return W, mx, 0.0 if ok.all() else 1.0


def scale_cases():
    """{name: M (m x ncols, the last column is b)}, all finite."""
    rng = np.random.default_rng(31)
    base = rng.standard_normal((7, 38))
    ints = rng.integers(-3, 4, size=(9, 5)).astype(np.float64)
    ints[0, 0] = 3.0
    big = rng.standard_normal((6, 11))
    big[4, 7] = -DBL_MAX
    zero = np.zeros((4, 7))
    zero[1, 2] = -0.0
    return {
        "order_one": base,
        "up_900": np.ldexp(base, 900),
        "down_900": np.ldexp(base, -900),
        "denormal": np.ldexp(ints, -1070),
        "dbl_max": big,
        "zeros": zero,
        "many_blocks": rng.standard_normal((5, 420001)),  # > 1024 * 2048 entries: the 1024 blocks take a second stride
    }


# ---------------------------------------------------------------------------------------------------------------------------
# Gram product
# ---------------------------------------------------------------------------------------------------------------------------
def gram_int_input(m, ncols, zero_lines=False):
    """(Wi, W): integers in [-8, 8] and W = Wi / 16; zero_lines: a few rows and columns (the first and last among them) all zero."""
    rng = np.random.default_rng(7000 * m + ncols + (1 if zero_lines else 0))
    Wi = rng.integers(-8, 9, size=(m, ncols)).astype(np.int64)
    if zero_lines:
        Wi[np.unique([0, m // 2, m - 1])] = 0
        Wi[:, np.unique([0, ncols // 3, ncols - 1])] = 0
    return Wi, Wi.astype(np.float64) / 16.0


def gram_int_ref(Wi):
    """W W' for W = Wi / 16, exactly: the int64 product over 256."""
    return (Wi @ Wi.T).astype(np.float64) / 256.0


def gram_real_inputs(m, ncols):
    """{name: W}: standard normal, and graded -- the row norms fall from 1 to 1e-12."""
    rng = np.random.default_rng(9000 * m + ncols)
    W = rng.standard_normal((m, ncols))
    grade = np.logspace(0, -12, m) if m > 1 else np.ones(1)
    G = rng.standard_normal((m, ncols))
    G *= (grade / np.sqrt((G * G).sum(axis=1)))[:, None]
    return {"normal": W, "graded": G}


def _ld_matmul_nt(A, B):
    """A B' in long double, in row blocks (NumPy has no BLAS for it: keep the temporaries small)."""
    A = np.ascontiguousarray(A, dtype=np.longdouble)
    Bt = np.ascontiguousarray(np.asarray(B, dtype=np.longdouble).T)
    return np.matmul(A, Bt)


SPLIT_ABOVE = 5e7  # m * m * ncols from which the long-double product goes through exact float64 pieces
SPLIT_BITS = 72    # bits of every row, counted from its largest entry, that the pieces keep


def split_rows(W, ncols):
    """W = P_0 + P_1 + ... + P_{K-1} + R exactly, row by row: P_k[r] holds multiples of 2^(e_r - beta (k + 1)) of magnitude
    <= 2^e_r 2^(-beta k) (e_r the frexp exponent of the row's largest entry), with beta so small that every sum of ncols products
    of piece entries is an integer below 2^53 in its unit -- float64 (BLAS, any order, FMA or not) multiplies two pieces out
    EXACTLY; |R[r]| <= 2^(e_r - beta K - 1).  Returns (pieces, e, beta)."""
    beta = (52 - int(np.ceil(np.log2(max(ncols, 2))))) // 2
    K = -(-SPLIT_BITS // beta)
    e = np.frexp(np.abs(W).max(axis=1))[1].astype(np.int64)
    rest = np.array(W, dtype=np.float64)
    pieces = []
    for k in range(K):
        q = np.ldexp(1.0, e - beta * (k + 1))[:, None]
        P = np.rint(rest / q) * q
        rest = rest - P
        pieces.append(P)
    return pieces, e, beta


def _gram_split(W):
    """W W' for a long W: the products of the exact pieces, added in long double from the smallest to the largest.  Left out: the
    piece pairs with k + l >= K and the remainder R, below 2^(e_p + e_q - SPLIT_BITS) (4 ncols) per entry."""
    pieces, _, _ = split_rows(W, W.shape[1])
    K = len(pieces)
    ref = np.zeros((W.shape[0], W.shape[0]), dtype=np.longdouble)
    for total in range(K - 1, -1, -1):
        for k in range(total + 1):
            ref += pieces[k] @ pieces[total - k].T
    return ref


def gram_real_ref(W, method="auto"):
    """(W W', |W| |W|') as long doubles.  "longdouble": NumPy's long-double product of the lower triangle, mirrored.  "split" (what
    "auto" takes from SPLIT_ABOVE on, where the former needs tens of seconds): exact float64 products of pieces of W summed in long
    double -- no less accurate on rows whose largest entry is within 2^6 of their r.m.s. (the CPU test checks that of the inputs) --
    with |W| |W|' from float64."""
    m, ncols = W.shape
    if method == "split" or (method == "auto" and m * m * ncols > SPLIT_ABOVE):
        return _gram_split(W), (np.abs(W) @ np.abs(W).T).astype(np.longdouble)
    ref = np.zeros((m, m), dtype=np.longdouble)
    ab = np.zeros((m, m), dtype=np.longdouble)
    A = np.abs(W)
    for i0 in range(0, m, 128):
        i1 = min(m, i0 + 128)
        ref[i0:i1, :i1] = _ld_matmul_nt(W[i0:i1], W[:i1])
        ab[i0:i1, :i1] = _ld_matmul_nt(A[i0:i1], A[:i1])
    low = np.tril_indices(m, -1)
    ref.T[low] = ref[low]
    ab.T[low] = ab[low]
    return ref, ab


def gram_bound(ab, ncols):
    """gamma_ncols |W||W|' for the kernel, plus ncols u_ld |W||W|' for the reference itself."""
    return (np.longdouble(gamma(ncols)) + np.longdouble(ncols * LD_EPS)) * ab


# ---------------------------------------------------------------------------------------------------------------------------
# rotation
# ---------------------------------------------------------------------------------------------------------------------------
def rotate_int_input(m, ncols):
    """(Ji, Wi, W): J = a signed permutation plus integers in [-3, 3]; W = Wi / 16, Wi integers in [-8, 8]."""
    rng = np.random.default_rng(11000 * m + ncols)
    Ji = rng.integers(-3, 4, size=(m, m)).astype(np.int64)
    Ji[np.arange(m), rng.permutation(m)] += rng.choice([-1, 1], size=m)
    Wi = rng.integers(-8, 9, size=(m, ncols)).astype(np.int64)
    return Ji, Wi, Wi.astype(np.float64) / 16.0


def rotate_int_ref(Ji, Wi):
    return (Ji @ Wi).astype(np.float64) / 16.0


def plane_rotations(m, seed):
    """J = a product of 3 m true plane rotations on random pairs of rows (the identity for m = 1)."""
    rng = np.random.default_rng(seed)
    J = np.eye(m)
    if m < 2:
        return J
    for _ in range(3 * m):
        p, q = rng.choice(m, size=2, replace=False)
        t = rng.uniform(-np.pi, np.pi)
        c, s = np.cos(t), np.sin(t)
        rp, rq = J[p].copy(), J[q].copy()
        J[p], J[q] = c * rp + s * rq, c * rq - s * rp
    return J


def rotate_real_ref(J, W):
    """(J W in long double, |J| |W| in long double)."""
    Jl = np.ascontiguousarray(J, dtype=np.longdouble)
    return np.matmul(Jl, W.astype(np.longdouble)), np.matmul(np.abs(Jl), np.abs(W).astype(np.longdouble))


# ---------------------------------------------------------------------------------------------------------------------------
# lead sign, write-out
# ---------------------------------------------------------------------------------------------------------------------------
def lead_index(W):
    """Per row: the first index of the largest magnitude."""
    return np.abs(W).argmax(axis=1)


def lead_ref(W, perm, sigma, r):
    """sig[k] = +-sigma[k], k < r: negative where the first largest-magnitude entry of row perm[k] is negative."""
    rows = W[perm[:r]]
    lead = rows[np.arange(r), lead_index(rows)] if r else np.zeros(0)
    return np.where(lead < 0, -sigma[:r], sigma[:r])


def write_ref(W, perm, sig, r, droptol):
    """(out, nnz): out[k] = W[perm[k]] / sig[k] (IEEE division), |v| <= droptol -> +0.0, rows >= r +0.0."""
    out = np.zeros_like(W)
    if r:
        with np.errstate(invalid="ignore", divide="ignore"):
            v = W[perm[:r]] / sig[:r, None]
        v[np.abs(v) <= droptol] = 0.0
        out[:r] = v
    return out, int(np.count_nonzero(out))


# the planted rows of the finish test: name -> ((column, value), ...); a negative column counts from the end
TIE = 0.75
FINISH_PATTERNS = (
    ("tie_7_260", ((7, TIE), (260, -TIE))),
    ("tie_260_7", ((7, -TIE), (260, TIE))),
    ("tie_255_256", ((255, TIE), (256, -TIE))),
    ("tie_256_255", ((255, -TIE), (256, TIE))),
    ("tie_first_last", ((0, -TIE), (-1, TIE))),
    ("last_column", ((-1, -0.9),)),
    ("zero_row", None),
    ("droptol", "drop"),
)
DROP_COLS = (3, 130, -2)  # exactly droptol, one ulp above, one ulp below (after the division), with alternating signs


def drop_targets():
    return (DROPTOL, float(np.nextafter(DROPTOL, 1.0)), float(np.nextafter(DROPTOL, 0.0)))


def _plant_quotient(t, s):
    """w with fl(w / s) == t exactly (s > 0), searched among the neighbours of t * s."""
    w = t * s
    for cand in (w, np.nextafter(w, np.inf), np.nextafter(w, -np.inf), np.nextafter(np.nextafter(w, np.inf), np.inf),
                 np.nextafter(np.nextafter(w, -np.inf), -np.inf)):
        if cand / s == t:
            return float(cand)
    raise AssertionError("no w divides to the target")


def finish_input(m, only=None):
    """(W, perm, sigma, planted): W m x FINISH_NCOLS with entries of magnitude < 0.5 and the patterns planted into the rows
    perm[0], perm[1], ... (as many as m holds; `only` = one pattern index, into row perm[0]); perm a permutation that is not the
    identity (m > 1); sigma in [1, 1.4).  planted: {name: k}."""
    ncols = FINISH_NCOLS
    rng = np.random.default_rng(13000 + m + (0 if only is None else 100 * (only + 1)))
    W = rng.uniform(-0.49, 0.49, size=(m, ncols))
    W[:, ::17] = np.ldexp(W[:, ::17], -40)  # (small entries too: some land under droptol after the division)
    perm = rng.permutation(m).astype(np.int32)
    if m > 1 and np.array_equal(perm, np.arange(m)):
        perm = np.roll(perm, 1)
    sigma = rng.uniform(1.0, 1.4, size=m)
    which = range(len(FINISH_PATTERNS)) if only is None else (only,)
    planted = {}
    for k, idx in zip(range(m), which):
        name, what = FINISH_PATTERNS[idx]
        row = W[perm[k]]
        planted[name] = k
        if what is None:
            row[:] = 0.0
        elif what == "drop":
            # this row's lead entry is positive (planted): sig = +sigma
            row[5] = 0.6
            for c, t, sign in zip(DROP_COLS, drop_targets(), (1.0, -1.0, 1.0)):
                row[c] = sign * _plant_quotient(t, sigma[k])
        else:
            for c, v in what:
                row[c] = v
    return np.asfortranarray(W), perm, sigma, planted


# ---------------------------------------------------------------------------------------------------------------------------
# the driver's inputs
# ---------------------------------------------------------------------------------------------------------------------------
def rows_70x300():
    """The 70 x 300, rank 40 matrix of tests/test_gpu_compress_constraints.py::test_more_than_one_block_of_rows."""
    rng = np.random.default_rng(21)
    B = rng.integers(-2, 3, size=(40, 300)).astype(np.float64)
    return np.asfortranarray(rng.integers(-1, 2, size=(70, 40)).astype(np.float64) @ B)


MORE_ROWS = ((129, 70, 70, 1), (200, 517, 90, 2))  # (m, ncols, rank, seed)


def more_rows(m, ncols, r, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.integers(-1, 2, (m, r)) @ rng.integers(-2, 3, (r, ncols))).astype(np.float64))
