"""NumPy side of tests/test_gpu_narrow_loop_labels.py: made-up symmetric labels in packed form, inputs on which the loop's verify
passes must find nothing (every value constant on the classes), and the places where the needles go.

Packed form: the lower triangle column by column, column j at offset j n - j (j - 1) / 2, rows j .. n - 1."""
import numpy as np


def col_off(n, j):
    return j * n - j * (j - 1) // 2


def packed_ij(n):
    """(rows, columns) of every packed index."""
    cols = np.arange(n)
    return np.concatenate([np.arange(j, n) for j in range(n)]), np.repeat(cols, n - cols)


def packed_labels(n, d, with_zero, seed):
    """Packed labels 1 .. min(d, what fits), every one of them present, plus label 0 when with_zero (and there is room); numbered by
    first occurrence in packed order, as a refinement numbers them.  Returns (Lp uint32, first uint32 per class, d_eff)."""
    rng = np.random.default_rng(seed)
    npk = n * (n + 1) // 2
    zero = with_zero and npk >= 2
    d_eff = max(1, min(d, npk - (1 if zero else 0)))
    g = np.concatenate([np.arange(1, d_eff + 1), [0] if zero else [], rng.integers(0 if zero else 1, d_eff + 1, size=npk - d_eff - (1 if zero else 0))])
    g = g[rng.permutation(npk)].astype(np.int64)
    _, first, inv = np.unique(g, return_index=True, return_inverse=True)
    vals = g[first]
    order = np.argsort(first[vals != 0], kind="stable")
    rank = np.zeros(len(first), dtype=np.uint32)
    rank[np.flatnonzero(vals != 0)[order]] = np.arange(1, d_eff + 1, dtype=np.uint32)
    Lp = rank[inv.reshape(-1)]
    fi = np.sort(first[vals != 0]).astype(np.uint32)
    assert int(Lp.max()) == d_eff and len(fi) == d_eff and np.array_equal(Lp[fi], np.arange(1, d_eff + 1))
    return np.ascontiguousarray(Lp), fi, d_eff


def full_from_packed(n, Lp):
    """The symmetric n x n matrix [row, column] of a packed triangle."""
    ii, jj = packed_ij(n)
    M = np.zeros((n, n), dtype=Lp.dtype)
    M[ii, jj] = Lp
    M[jj, ii] = Lp
    return M


def class_constant_channels(n, ld, T, Lp, seed):
    """T int32 channels of ld x ld (column-major, flat), constant on the classes of the lower triangle and 0 on label 0; the strict upper
    triangle and the padding hold a value no class has (nobody may read them)."""
    rng = np.random.default_rng(seed)
    ii, jj = packed_ij(n)
    C = np.full((T, ld, ld), -77777, dtype=np.int32)  # [t, column, row]
    for t in range(T):
        v = rng.integers(-2 ** 20, 2 ** 20, size=int(Lp.max()) + 1).astype(np.int32)
        v[0] = 0
        C[t, jj, ii] = v[Lp]
    return C


def class_constant_basis(n, r, Lp, seed):
    """r symmetric n x n matrices (flat, column-major), constant on the classes and 0 on label 0, and r coefficients."""
    rng = np.random.default_rng(seed)
    U = np.zeros((max(r, 1), n, n))
    for k in range(r):
        v = rng.standard_normal(int(Lp.max()) + 1) / n
        v[0] = 0.0
        U[k] = full_from_packed(n, v[Lp])
    return np.ascontiguousarray(U), rng.standard_normal(max(r, 1))


def pair_case(n, d, with_zero, seed):
    """Packed labels as above and n x n matrices a, b [row, column] whose pairs of values are constant on the classes, distinct between
    them and (+0.0, +0.0) exactly on label 0: the refinement of (a, b) writes these labels and first occurrences again.  The strict upper
    triangle holds NaNs nobody may read."""
    Lp, first, de = packed_labels(n, d, with_zero, seed)
    rng = np.random.default_rng(seed + 1)
    va = np.concatenate([[0.0], 1.0 + rng.permutation(de)])  # distinct, so are the pairs
    vb = np.concatenate([[0.0], rng.integers(1, 4, size=de).astype(np.float64)])
    ii, jj = packed_ij(n)
    a, b = np.full((n, n), np.nan), np.full((n, n), np.nan)
    a[ii, jj], b[ii, jj] = va[Lp], vb[Lp]
    return Lp, first, de, a, b


def needle_places(n, Lp):
    """(row, column), row >= column: first and last row of the first, the middle and the last column -- and, for a walk over column
    pairs (p, n - 1 - p), both columns of a pair and the unpaired middle column of an odd n are among them.  Only places whose class
    has another entry (or is label 0, which is compared with zero): the only entry of a class IS its representative, and changing it
    changes no partition."""
    cols = sorted({0, (n - 1) // 2, n // 2, n - 1})
    counts = np.bincount(Lp)
    out = []
    for (i, j) in sorted({(j, j) for j in cols} | {(n - 1, j) for j in cols}):
        l = int(Lp[col_off(n, j) + i - j])
        if l == 0 or counts[l] > 1:
            out.append((i, j))
    return out
