"""Plain NumPy references for the steps of the real dense blockDiagonalize (csrc/eigdec.cpp, the head of csrc/kernels_blockdiag.hip),
shared by tests/test_dense_steps_ref_cpu.py, tests/test_gpu_dense_steps.py and tests/test_iso_classes_cpu.py: the coupling matrix
(T = A Q, M = Q' T, block maxima), the eigenvalue clustering, the Otsu chain from the coupling matrix to the classes, the irreducible
columns, copy_cols and clamptol; the input families of the GPU tests; and the error bound of every comparison that is not exact.

Exact families.  Integer inputs whose every partial sum, in any order of summation, fused or not, stays an integer below 2^53 give
the same float64 bits whatever the kernel does: compared as BITS.  `assert_exact_*` check the magnitudes on the absolute values.

Bounds (U = 2^-53).  A dot product of k terms evaluated in fp64 in any order, with or without FMA, is within gamma_k sum |terms| of
its exact value, gamma_k ~ k U; a product of two such stages (Q' (A Q), Q_j (Q_j' b)) passes every leaf term through at most
k1 + k2 roundings.  Every real-data bound below is

    2 (k1 + k2) U * (the same expression in absolute values),

the factor 2 covering the second-order terms and the rounding of the long-double reference.  Square root, reciprocal and the final
product add one rounding each, written out where they occur.  The bounds are judged on a float64 NumPy evaluation of the same
formulas (the CPU test), never on a kernel.

Nothing here touches the library."""
import functools
import math
import os
import sys

import numpy as np

import problems

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import sdpsr_oracle as O  # noqa: E402

U = 2.0 ** -53
LD = np.longdouble
ATOL = 1e-9
OK, NUMERICAL_INCONSISTENCY, BAD_ARGUMENT = 0, 2, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# Block norms: T = A Q, M = Q' T, norms[sa, sb] = max(norms[sa, sb], max |M[a, b]| over space_of[a] == sa, space_of[b] == sb)
# ---------------------------------------------------------------------------------------------------------------------------
SMALL_ORDERS = (1, 2, 31, 32, 33, 63, 64)  # route 0 (one workgroup)
LARGE_ORDERS = (1, 63, 64, 65, 127, 129, 200, 730)  # routes 1 and 2; 730^2 > 2048 * 256: the grid-stride loop's second trip


def layouts(n, non_monotone):
    """name -> space_of (int32): one space, n spaces, sizes 1 / 2 / rest, and (routes 1 and 2) a non-monotone assignment with runs
    that straddle the waves and the columns."""
    out = {"one space": np.zeros(n, dtype=np.int32), "n spaces": np.arange(n, dtype=np.int32)}
    if n >= 4:
        out["1 / 2 / rest"] = np.array([0, 1, 1] + [2] * (n - 3), dtype=np.int32)
    if non_monotone and n >= 3:
        out["non-monotone"] = ((np.arange(n) * 7 + 3) // 5 % 3).astype(np.int32)
        out["non-monotone"][n // 2] = 3 if n >= 4 else 2
        out["non-monotone"] = _dense_ids(out["non-monotone"])
    return out


def _dense_ids(s):
    """the same assignment with the ids 0 .. neig - 1 all in use, NOT in order of first occurrence"""
    ids = np.unique(s)
    return np.searchsorted(ids, s).astype(np.int32)


def block_max(X, space_of, neig):
    """max of the non-negative X over every pair of spaces; 0 for a pair with an empty space"""
    out = np.zeros((neig, neig), dtype=X.dtype)
    np.maximum.at(out, (space_of[:, None], space_of[None, :]), X)
    return out


@functools.lru_cache(maxsize=None)
def integer_family(n, seed=0):
    """(A symmetric, Q), integer entries |A| <= 2^10, |Q| <= 2^4 as float64; a zero row and column in A and a zero column in Q from
    order 3 on, so that M has zero entries.  Read-only."""
    rng = np.random.default_rng([n, seed, 19])
    A = np.triu(rng.integers(-2 ** 10, 2 ** 10 + 1, (n, n)))
    A = A + np.triu(A, 1).T
    Q = rng.integers(-2 ** 4, 2 ** 4 + 1, (n, n))
    if n >= 3:
        A[1, :] = A[:, 1] = 0
        Q[:, n - 1] = 0
    A, Q = A.astype(np.float64), Q.astype(np.float64)
    A.setflags(write=False)
    Q.setflags(write=False)
    return A, Q


@functools.lru_cache(maxsize=None)
def general_integer_family(n):
    """(A, Q) of the same magnitudes with a NON-symmetric A.  The kernels read the element by columns ("A symmetric: row i = column
    i"): they form T = A' Q and M = Q' T, which is not symmetric here, so that norms[sa, sb] and norms[sb, sa] differ and the
    layout of the result is pinned against its transpose (a symmetric element cannot tell the two apart)."""
    rng = np.random.default_rng([n, 29])
    A = rng.integers(-2 ** 10, 2 ** 10 + 1, (n, n)).astype(np.float64)
    Q = rng.integers(-2 ** 4, 2 ** 4 + 1, (n, n)).astype(np.float64)
    A.setflags(write=False)
    Q.setflags(write=False)
    return A, Q


def assert_exact_qtaq(A, Q, symmetric=True):
    """|A| <= 2^10, |Q| <= 2^4, n <= 1024: |T| <= 2^24 and |M| <= 2^38 on the absolute values, so every partial sum is an integer
    below 2^53."""
    n = A.shape[0]
    assert n <= 1024 and np.abs(A).max() <= 2 ** 10 and np.abs(Q).max() <= 2 ** 4
    assert np.array_equal(A, np.rint(A)) and np.array_equal(Q, np.rint(Q)) and (not symmetric or np.array_equal(A, A.T))
    Ta = np.abs(A).astype(np.int64) @ np.abs(Q).astype(np.int64)
    Ma = np.abs(Q).astype(np.int64).T @ Ta
    assert int(Ta.max()) <= 2 ** 24 and int(Ma.max()) <= 2 ** 38
    return int(Ta.max()), int(Ma.max())


def qtaq_exact(A, Q):
    """(T, M) = (A' Q, Q' T) in int64: A Q and Q' A Q for the symmetric elements of the driver"""
    Ai, Qi = A.astype(np.int64), Q.astype(np.int64)
    T = Ai.T @ Qi
    return T, Qi.T @ T


@functools.lru_cache(maxsize=None)
def real_family(n):
    """(A, Q): A the generic element of a permuted symmetric circulant partition (class values uniform in [0, 1), as the driver draws
    them), Q orthogonal from a QR factorisation.  Read-only."""
    rng = np.random.default_rng([n, 23])
    L = problems.permute_labels(problems.symmetric_circulant_labels(n), seed=n) if n > 1 else np.ones((1, 1), dtype=np.int64)
    L = np.asarray(L).reshape(n, n)
    vals = rng.random(int(L.max()) + 1)
    A = vals[L]
    assert np.array_equal(A, A.T)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A.setflags(write=False)
    Q.setflags(write=False)
    return A, Q


def _matmul(X, Y, dtype):
    """X Y in `dtype`, by column blocks (long double has no BLAS: the blocks bound the temporaries)"""
    Xd = X.astype(dtype)
    out = np.empty((X.shape[0], Y.shape[1]), dtype=dtype)
    for c0 in range(0, Y.shape[1], 128):
        out[:, c0:c0 + 128] = Xd @ Y[:, c0:c0 + 128].astype(dtype)
    return out


@functools.lru_cache(maxsize=None)
def real_qtaq(n, dtype=LD):
    """(|M| in `dtype`, entrywise bound) of the real family: an entry of M = Q' (A Q) passes through at most 2 n roundings, so it is
    within  2 * 2n U (|Q|' |A| |Q|)[a, b]  of the exact one, and |M| moves by no more."""
    A, Q = real_family(n)
    M = _matmul(Q.T, _matmul(A, Q, dtype), dtype)
    bound = 2 * 2 * n * U * (np.abs(Q).T @ (np.abs(A) @ np.abs(Q)))
    return np.abs(M), bound


def expected_norms(absM, space_of, neig, start):
    """elementwise maximum of the start values (neig x neig, non-negative) and the block maxima"""
    return np.maximum(np.asarray(start).reshape(neig, neig), block_max(absM, space_of, neig))


def start_values(name, neig, new):
    """the states of norms before a pass: the driver's zero fill, and a raise: values above and below the new maxima `new`"""
    if name == "zeros":
        return np.zeros((neig, neig))
    rng = np.random.default_rng([neig, 3])
    new = np.asarray(new, dtype=np.float64)
    return np.where(rng.random((neig, neig)) < 0.5, new * 2.0 + 1.0, new * 0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# Clustering of ascending eigenvalues: a new eigenspace where !(|dv| <= atol), so a NaN opens one on both sides
# ---------------------------------------------------------------------------------------------------------------------------
def cluster(evals, atol):
    """space_of (int32) of every eigenvalue"""
    sp = np.zeros(len(evals), dtype=np.int32)
    for i in range(1, len(evals)):
        sp[i] = sp[i - 1] + (0 if abs(float(evals[i]) - float(evals[i - 1])) <= atol else 1)
    return sp


def eigenvalue_lists(n, atol):
    """name -> n ascending values: all equal; all apart; gaps of exactly atol (no boundary) with one gap one ulp above atol (a
    boundary) where the values cross zero -- -atol / 2 and atol / 2 (1 + 2^-51) are atol (1 + 2^-52) apart, exactly --; a NaN.
    Whatever a difference rounds to, cluster() takes the same fp64 difference as the kernel."""
    out = {"all equal": np.full(n, 0.75), "all apart": np.arange(n) * 4 * atol}
    if n >= 2:
        h = n // 2
        neg = -atol / 2 - np.arange(h - 1, -1, -1) * atol  # multiples of atol / 2: exact
        pos = atol / 2 * (1 + 2.0 ** -51) + np.arange(n - h) * atol
        out["gaps atol and atol + ulp"] = np.concatenate([neg, pos])
        w = np.full(n, 0.5)
        w[h] = np.nan
        out["a NaN"] = w
    return out


CLUSTER_ATOL = 2.0 ** -30


def pack_layout(n):
    """byte offsets (space_of, values, norms, total) of the one-read-back pack"""
    o_space = 64
    o_vals = o_space + ((n * 4 + 63) // 64) * 64
    o_norms = o_vals + n * 8
    return o_space, o_vals, o_norms, o_norms + n * n * 8


# ---------------------------------------------------------------------------------------------------------------------------
# The Otsu chain: raw coupling matrix -> dimension rule -> extrema -> 17 edges -> counts -> threshold -> pair bits -> union-find
# ---------------------------------------------------------------------------------------------------------------------------
def _two_clusters(rng, dims, classes, lo=1e-7, hi=1.0):
    """Raw coupling matrix of eigenspaces with the given dimensions: large (hi * U(0.5, 1.5)) inside a class -- also between
    its eigenspaces of different dimension, which only the dimension rule separates --, small (lo * U(0.5, 1.5)) elsewhere; the
    lower triangle is large throughout: only the upper one may be read."""
    ne = len(dims)
    M = lo * rng.uniform(0.5, 1.5, size=(ne, ne))
    for i in range(ne):
        for j in range(ne):
            if classes[i] == classes[j]:
                M[i, j] = hi * rng.uniform(0.5, 1.5)
    M[np.tril_indices(ne, -1)] = hi * rng.uniform(0.5, 1.5, size=ne * (ne - 1) // 2)  # never read
    return M


def _matrix_cases():
    """(name, dims, raw matrix): neig = 1, 2, 17, 300; two well-separated clusters; all values equal; values below atol; a
    value equal to an edge; mixed dimensions; the inconsistent chain."""
    rng = np.random.default_rng(5)
    cases = [("one", [3], np.array([[1.0]])),  # (1.0: exact edges, as in `equal`)
             ("two_merged", [1, 1], _two_clusters(rng, [1, 1], [0, 0])),
             ("two_apart", [2, 2], _two_clusters(rng, [2, 2], [0, 1]))]
    dims17 = [1, 2, 1, 3, 2, 1, 1, 2, 3, 1, 2, 1, 1, 3, 2, 1, 1]
    cls17 = [i % 4 for i in range(17)]  # classes mix dimensions: the dimension rule zeroes entries and splits them
    cases.append(("mixed17", dims17, _two_clusters(rng, dims17, cls17)))
    cls300 = list(rng.integers(0, 40, size=300))
    cases.append(("clusters300", [1] * 300, _two_clusters(rng, [1] * 300, cls300)))
    # all values equal (1.0: log and exp are exact, every edge is 1.0): counts end in the last bin, every variance is 0 / 0,
    # Julia's argmax returns the first NaN
    cases.append(("equal", [1] * 5, np.ones((5, 5))))
    # values below atol (and zeros, from the dimension rule): the minimum is clamped to atol; one value EQUAL to atol, the first
    # edge, and the maximum equal to the last (exp(log(x)) may round to either side of x: both sides fall into the same bin, the
    # first and the last respectively)
    M = _two_clusters(rng, [1, 1, 2, 1, 1, 2], [0, 0, 1, 2, 2, 1], lo=1e-12)
    M[0, 3] = ATOL
    cases.append(("below_atol", [1, 1, 2, 1, 1, 2], M))
    # the inconsistent chain: 0-3, 1-2, 2-3 coupled -> union by rank makes 1 the root of {0, 1, 2, 3}, whose first member is 0
    M = 1e-7 * rng.uniform(0.5, 1.5, size=(5, 5))
    for i, j in ((0, 3), (1, 2), (2, 3)):
        M[i, j] = rng.uniform(0.5, 1.5)
    M[np.arange(5), np.arange(5)] = rng.uniform(0.5, 1.5, size=5)
    cases.append(("chain", [1] * 5, M))
    return cases


def _oracle_chain(dims, raw):
    """The oracle's own steps on a raw matrix: the dimension rule (block_norms_inf's), log_histogram, otsu_threshold, the
    merge order of isomorphism_partition, __isconsistent."""
    ne = len(dims)
    sym = np.zeros((ne, ne))
    for i in range(ne):
        for j in range(i, ne):
            sym[i, j] = sym[j, i] = 0.0 if dims[i] != dims[j] else raw[i, j]
    counts, edges = O.log_histogram(sym, 16, ATOL)
    thr = O.otsu_threshold(sym, ATOL)
    pdf = counts / counts.sum()  # the chosen bin, as otsu_threshold picks it
    w, mu0 = np.cumsum(pdf), np.cumsum(np.log(edges[:-1]) * pdf)
    with np.errstate(divide="ignore", invalid="ignore"):
        cand = ((mu0[-1] * w - mu0) ** 2 / (w * (1 - w)))[:-1]
    best = int(np.nonzero(np.isnan(cand))[0][0]) if np.isnan(cand).any() else int(np.argmax(cand))
    assert edges[best + 1] == thr
    K = O.IntDisjointSets(ne)
    for i in range(ne):
        for j in range(i + 1, ne):
            if sym[i, j] >= thr:
                K.union(i, j)
    return sym, counts, edges, best, thr, K


def _expected_classes(K, expect):
    kp = [K.find_root(i) for i in range(len(K))]
    roots = list(dict.fromkeys(kp))
    members = [[j for j, r in enumerate(kp) if r == i] for i in roots]
    sizes = [len(m) for m in members]
    S1, S, fd = sum(sizes), sum(s * s for s in sizes), sum(s * (s + 1) // 2 for s in sizes)
    col = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
    off = np.concatenate([[0], np.cumsum([s * s for s in sizes])[:-1]]).astype(int)
    da = [c + a for c, s in zip(col, sizes) for b in range(s) for a in range(s)]
    db = [c + b for c, s in zip(col, sizes) for b in range(s) for a in range(s)]
    return {"verdict": [int(O.is_consistent(K))], "kpart": kp, "roots": roots, "members": members, "sizes": sizes,
            "sums": [S1, S, fd, len(roots)], "settled": [int(fd == expect), 0, 1, 1, 1],
            "colsz": list(col) + sizes, "off": list(off), "laymax": [len(sizes), max(sizes)], "desc": da + db}


def _log(x):
    """the C library's log on every double (math.log raises where it returns -inf or NaN)"""
    if x != x:
        return x
    return -math.inf if x == 0 else math.log(x)


def _exp(t):
    """the C library's exp (math.exp raises where it returns inf)"""
    if t != t:
        return t
    try:
        return math.exp(t)
    except OverflowError:
        return math.inf


def otsu_edges(mn, mx, atol):
    """The 17 edges as the host forms them from the extrema: exp of 17 equidistant points between the logarithms, the last one
    exp(log(mx)) itself, in Python floats -- the same IEEE operations in the same order, log and exp from the same C library."""
    if mn < atol:
        mn = atol
    l0, l1 = _log(mn), _log(mx)
    return [_exp(l1 if i == 16 else l0 + (l1 - l0) * float(i) / 16.0) for i in range(17)]


def otsu_pick(edges, cnt):
    """(threshold, chosen bin) from the 17 edges and cnt[c] = number of values with exactly c edges <= them (c = 0..17): the counts
    per bin of log_histogram, then the first NaN, else the first maximum, of the between-class variance."""
    hist = [0] * 18
    for c in range(18):
        hist[min(c + 1, 17)] += int(cnt[c])
    counts = [0.0] * 16
    for f in range(1, 18):
        counts[min(max(f - 1, 1), 16) - 1] += float(hist[f])
    total = 0.0
    for v in counts:
        total += v
    w, mu, cw, cm = [], [], 0.0, 0.0
    for i in range(16):
        p = counts[i] / total if total else math.nan
        cw += p
        cm += _log(edges[i]) * p
        w.append(cw)
        mu.append(cm)
    best, bestv, have_nan = 0, -math.inf, False
    for i in range(15):
        num = mu[15] * w[i] - mu[i]
        den = w[i] * (1 - w[i])
        s2 = num * num / den if den != 0 else (math.nan if num * num == 0 or num != num else math.copysign(math.inf, den) * 1.0)
        if s2 != s2:
            if not have_nan:
                best, have_nan = i, True
        elif not have_nan and s2 > bestv:
            bestv, best = s2, i
    return edges[best + 1], best


def classes_expected(raw, dims, atol):
    """What isomorphism_classes_device returns for a raw neig x neig coupling matrix (float64, [i, j] at i * neig + j), every quantity
    an exact function of the entries: the symmetrised matrix, the 20 stat words, the edges, the threshold, the pair bits (neig x W
    words), kpart and the status.  The extrema skip NaNs (a < mn and mx < a are false); a NaN has 17 edges "not above" it; the
    union-find visits the pairs in the reference's order (i, then j > i)."""
    raw = np.asarray(raw, dtype=np.float64)
    ne = len(dims)
    d = np.asarray(dims)
    iu = np.triu_indices(ne)
    sym = np.zeros((ne, ne))
    up = np.where(d[iu[0]] != d[iu[1]], 0.0, raw[iu])
    sym[iu] = up
    sym[(iu[1], iu[0])] = up
    a = np.abs(up)
    a = a[~np.isnan(a)]
    mn = float(a.min()) if a.size else math.inf
    mx = float(a.max()) if a.size else 0.0
    stat = np.zeros(20, dtype=np.uint64)
    if mn < math.inf:
        stat[0] = ~np.array([mn]).view(np.uint64)[0]
    if mx > 0.0:
        stat[1] = np.array([mx]).view(np.uint64)[0]
    mn_h = ((~stat[:1]).view(np.float64)[0]) if stat[0] else math.inf  # the host reads the extrema back from the words
    mx_h = stat[1:2].view(np.float64)[0]
    edges = otsu_edges(float(mn_h), float(mx_h), atol)
    flat = sym.ravel()
    with np.errstate(invalid="ignore"):
        c = np.zeros(flat.size, dtype=np.int64)
        for e in edges:
            c += ~(e > flat)
    cnt = np.bincount(c, minlength=18)
    stat[2:20] = cnt.astype(np.uint64)
    thr, best = otsu_pick(edges, cnt)
    W = (ne + 63) // 64
    with np.errstate(invalid="ignore"):
        on = np.triu(sym >= thr, 1)
    words = np.zeros((ne, W), dtype=np.uint64)
    ii, jj = np.nonzero(on)  # row-major: i, then j > i
    np.bitwise_or.at(words, (ii, jj // 64), np.uint64(1) << (jj % 64).astype(np.uint64))
    K = O.IntDisjointSets(ne)
    for i, j in zip(ii.tolist(), jj.tolist()):
        K.union(i, j)
    kpart = [K.find_root(i) for i in range(ne)]
    status = OK if O.is_consistent(K) else NUMERICAL_INCONSISTENCY
    return {"sym": sym, "stat": stat, "edges": np.array(edges), "thr": thr, "best": best, "bits": words, "kpart": kpart, "status": status,
            "K": K}


CLASS_ORDERS = (1, 2, 63, 64, 65, 255, 256, 300, 1000)


def class_cases(ne):
    """(name, dims, raw) at neig = ne: clusters (an asymmetric raw matrix: the lower triangle is large throughout and never read);
    all zero; all equal; one NaN; unequal dimensions inside a coupled pair; an entry exactly at the threshold."""
    rng = np.random.default_rng([ne, 11])
    ones = [1] * ne
    cls = list(rng.integers(0, max(1, ne // 3), size=ne))
    base = _two_clusters_fast(rng, ne, cls)
    cases = [("clusters, asymmetric raw", ones, base), ("all zero", ones, np.zeros((ne, ne))), ("all equal", ones, np.full((ne, ne), 0.375))]
    M = base.copy()
    M[0, ne - 1] = np.nan
    cases.append(("one NaN", ones, M))
    if ne >= 2:
        dims = list(rng.integers(1, 3, size=ne))
        i, j = _coupled_pair(base, cls)
        dims[i], dims[j] = 1, 2  # a large entry between eigenspaces of different dimension: the dimension rule zeroes it
        cases.append(("unequal dims in a coupled pair", dims, base))
    if ne >= 3:
        # couplings spread log-uniformly over seven decades, so that every bin is in use: a value of the bin right above the
        # threshold is moved down onto it -- it keeps its number of edges below, so every count and the threshold stay
        M = np.exp(rng.uniform(math.log(1e-7), 0.0, size=(ne, ne)))
        ref = classes_expected(M, ones, ATOL)
        thr, nxt = ref["thr"], ref["edges"][ref["best"] + 2]
        up = np.triu(ref["sym"], 1)
        hit = np.argwhere((up > thr) & (up < nxt) & (up < ref["sym"].max()))
        if len(hit):
            M[tuple(hit[0])] = thr
            cases.append(("an entry exactly at the threshold", ones, M))
    return cases


def _two_clusters_fast(rng, ne, cls):
    """_two_clusters for one-dimensional eigenspaces, vectorised"""
    cls = np.asarray(cls)
    same = cls[:, None] == cls[None, :]
    M = np.where(same, rng.uniform(0.5, 1.5, size=(ne, ne)), 1e-7 * rng.uniform(0.5, 1.5, size=(ne, ne)))
    M[np.tril_indices(ne, -1)] = rng.uniform(0.5, 1.5, size=ne * (ne - 1) // 2)
    return M


def _coupled_pair(base, cls):
    for i in range(len(cls)):
        for j in range(i + 1, len(cls)):
            if cls[i] == cls[j]:
                return i, j
    return 0, len(cls) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# Irreducible columns: column = Q_j (Q_j' b_i) / |Q_i' b_j|_2
# ---------------------------------------------------------------------------------------------------------------------------
IRREDUCIBLE_ORDERS = (1, 64, 65, 255, 257, 1000)
LDS_RULE_M2 = 7678  # the largest m_i + m_j the pair kernel takes: (m2 + 2) * 8 <= 60 KiB


def round_up(n, m):
    return (n + m - 1) // m * m


def pair_shapes(n):
    """(m_i, m_j) from (1, 1), (1, n), (n, 1), (63, 65), (65, 63), (128, 1), as far as they fit in n columns each"""
    return [s for s in dict.fromkeys(((1, 1), (1, n), (n, 1), (63, 65), (65, 63), (128, 1))) if max(s) <= n]


def pair_descriptors(n, npairs, seed=0):
    """(desc int32 npairs x 7, vcols, nf, ncols): the shapes of pair_shapes(n) in turn, windows anywhere inside the n columns of Q
    (they may overlap: the formula needs no orthogonality), B columns drawn from nf = 5, output columns a shuffled subset of
    ncols = npairs + 3: three columns stay unnamed."""
    rng = np.random.default_rng([n, npairs, seed, 31])
    shapes = pair_shapes(n)
    ncols, nf = npairs + 3, 5
    cols = rng.permutation(ncols)[:npairs]
    desc = np.zeros((npairs, 7), dtype=np.int32)
    for p in range(npairs):
        mi, mj = shapes[p % len(shapes)]
        desc[p] = (rng.integers(0, n - mi + 1), mi, rng.integers(0, n - mj + 1), mj, rng.integers(0, nf), rng.integers(0, nf), cols[p])
    return desc, n, nf, ncols


def irreducible_integer_inputs(n, seed=0):
    """(Q ldq x n, Bf ldq x 5) as float64 integers, |Q| <= 8, |B| <= 2^10 (2^6 from n = 129 on, where m_i reaches n: the sum of
    m_i squares must stay below 2^53); rows >= n hold 12345.0, which no result may depend on."""
    rng = np.random.default_rng([n, seed, 37])
    ldq = round_up(n, 128)
    bmax = 2 ** 10 if n <= 128 else 2 ** 6
    Q = np.full((ldq, n), 12345.0)
    B = np.full((ldq, 5), 12345.0)
    Q[:n] = rng.integers(-8, 9, (n, n))
    B[:n] = rng.integers(-bmax, bmax + 1, (n, 5))
    if n == 1:  # a single product: keep it away from zero, the norm divides
        Q[0, 0], B[0] = 3.0, (5.0, -7.0, 11.0, 2.0, -1.0)
    return Q, B


def irreducible_exact(n, Q, B, desc):
    """per pair (y int64 of n entries, S = sum of the squares of Q_i' b_j as a Python int), after asserting on the absolute values
    that every partial sum of the dot products, of the sum of squares and of Q_j w stays below 2^53"""
    Qi, Bi = Q[:n].astype(np.int64), B[:n].astype(np.int64)
    assert np.array_equal(Qi, Q[:n]) and np.array_equal(Bi, B[:n]) and np.abs(Qi).max() <= 8 and n <= 1024
    Wa = np.abs(Qi).T @ np.abs(Bi)  # |Q|' |B|: every dot product in absolute values
    out = []
    for ci, mi, cj, mj, fi, fj, _ in desc.tolist():
        w = Qi[:, cj:cj + mj].T @ Bi[:, fi]
        c = Qi[:, ci:ci + mi].T @ Bi[:, fj]
        S = sum(int(x) * int(x) for x in c)
        assert sum(int(x) ** 2 for x in Wa[ci:ci + mi, fj]) < 2 ** 53 and int((np.abs(Qi[:, cj:cj + mj]) @ Wa[cj:cj + mj, fi]).max()) < 2 ** 53
        out.append((Qi[:, cj:cj + mj] @ w, S))
    return out


def irreducible_exact_columns(n, Q, B, desc):
    """(reference columns in long double, n x npairs in desc order; the 4 ulp allowance).  y and S are exact integers in fp64 too, so
    the kernel's column is  fl(y * fl(1 / fl(sqrt(S)))):  three roundings, each a relative 2^-53 at most, together below
    3 * 2^-53 (1 + 2^-52) |value| <= 3 ulp(value) -- an ulp is at least 2^-53 |value| --; one more ulp for the second order and for
    taking the ulp of the rounded reference: 4 ulp, derived, not measured."""
    ex = irreducible_exact(n, Q, B, desc)
    ref = np.zeros((n, len(ex)), dtype=LD)
    for p, (y, S) in enumerate(ex):
        assert S > 0
        ref[:, p] = y.astype(LD) / np.sqrt(LD(S))
    return ref, 4 * np.spacing(np.abs(ref.astype(np.float64)))


def irreducible_real_inputs(n, seed=0):
    """(Q ldq x n with orthonormal columns from a QR factorisation -- Gaussian columns of norm ~1 from n = 2048 on --, Bf ldq x 5
    Gaussian); rows >= n hold 12345.0."""
    rng = np.random.default_rng([n, seed, 41])
    ldq = round_up(n, 128)
    Q = np.full((ldq, n), 12345.0)
    B = np.full((ldq, 5), 12345.0)
    G = rng.standard_normal((n, n))
    Q[:n] = np.linalg.qr(G)[0] if n < 2048 else G / np.sqrt(n)
    B[:n] = rng.standard_normal((n, 5))
    return Q, B


def irreducible_real(n, Q, B, desc, dtype=LD):
    """(columns n x npairs in `dtype`, bound).  With Y = |Q_j| (|Q_j|' |b_i|), S = |Q_i|' |b_j|, y = Q_j (Q_j' b_i), nrm = |Q_i' b_j|_2:

        dnrm     = 2 n U |S|_2 + (m_i + 2) U nrm          (the dot products; the m_i squares, their sum and the root)
        bound[r] = 2 (n + m_j) U Y[r] / nrm + |y[r]| / nrm (dnrm / nrm + 4 U)

    (the reciprocal and the product with it: 2 roundings, 4 for the second order)."""
    Qd, Bd = Q[:n].astype(dtype), B[:n].astype(dtype)
    Qa, Ba = np.abs(Q[:n]), np.abs(B[:n])
    Wd, Wa = Qd.T @ Bd, Qa.T @ Ba  # every dot product any pair needs, once
    cols = np.zeros((n, len(desc)), dtype=dtype)
    bound = np.zeros((n, len(desc)))
    for p, (ci, mi, cj, mj, fi, fj, _) in enumerate(np.asarray(desc).tolist()):
        y = Qd[:, cj:cj + mj] @ Wd[cj:cj + mj, fi]
        c = Wd[ci:ci + mi, fj]
        nrm = np.sqrt((c * c).sum())
        Y = Qa[:, cj:cj + mj] @ Wa[cj:cj + mj, fi]
        S = Wa[ci:ci + mi, fj]
        nrm64 = float(nrm)
        dnrm = 2 * n * U * float(np.sqrt((S * S).sum())) + (mi + 2) * U * nrm64
        cols[:, p] = y * (1 / nrm)
        bound[:, p] = 2 * (n + mj) * U * Y / nrm64 + np.abs(y).astype(np.float64) / nrm64 * (dnrm / nrm64 + 4 * U)
    return cols, bound


# ---------------------------------------------------------------------------------------------------------------------------
# copy_cols and clamptol
# ---------------------------------------------------------------------------------------------------------------------------
COPY_COUNTS = (1, 128, 129, 257)
GRID_CAP = 2048 * 256  # threads of the largest grid: a longer array takes the grid-stride loop's second trip


def copy_cols(n, src, dst, src_cols, dst_cols):
    """dst with rows < n of column dst_cols[k] replaced by those of column src_cols[k] of src (distinct destinations)"""
    out = dst.copy()
    out[:n, dst_cols] = src[:n, src_cols]
    return out


def clamptol(a, atol):
    """+0.0 where |a| < atol; everything else, a NaN and |a| == atol included, as it is"""
    out = a.copy()
    out[np.abs(a) < atol] = 0.0
    return out
