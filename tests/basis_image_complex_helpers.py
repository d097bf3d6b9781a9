"""Host side of the sdpsr_basis_image_complex tests (tests/test_gpu_basis_image_complex.py,
tests/test_basis_image_complex_cpu.py): the formula over the entries of each class in extended precision, the seeded
arbitrary complex Q, and the non-symmetric label generators, built from tests/problems.py."""
import functools

import numpy as np

import problems as pr


def reference_images_complex(L, d, Q, sizes, dtype=np.clongdouble):
    """ref[i - 1, :] = the images of class i, block after block, each block column-major -- the layout of
    sdpsr_block_images_complex -- from blks[i][k][a, b] = sum over the entries (r, c) with L[r, c] == i of
    conj(Q_k[r, a]) Q_k[c, b] = (Q_k^H 1[L == i] Q_k)[a, b] (src/diagonalize.jl:64-89), in ``dtype`` (np.clongdouble: the
    reference; np.complex128: what rounding alone does), not clamped.  L need not be symmetric; label 0 is skipped.
    Q: n x sum(sizes), blocks side by side."""
    L = np.asarray(L)
    n = L.shape[0]
    flat = L.ravel(order="F").astype(np.int64)
    order = np.argsort(flat, kind="stable")  # entries grouped by label, in linear (column-major) order inside a class
    lab = flat[order]
    rows, cols = order % n, order // n
    present, starts = np.unique(lab, return_index=True)
    Ql = np.asarray(Q, dtype=dtype)
    Qc = np.conj(Ql)
    S = sum(s * s for s in sizes)
    ref = np.zeros((d + 1, S), dtype=dtype)
    c0 = off = 0
    for s in sizes:
        for b in range(s):
            qb = Ql[cols, c0 + b]
            for a in range(s):
                ref[present, off + a + b * s] = np.add.reduceat(Qc[rows, c0 + a] * qb, starts)
        c0 += s
        off += s * s
    return ref[1:]


def gaussian_unit_columns_complex(n, cols, seed):
    """n x cols columns with standard normal real and imaginary parts, scaled to unit norm: nothing orthogonal, nothing
    invariant.  Then sum over any set of entries of |q_a[r]| |q_b[c]| <= ||q_a||_1 ||q_b||_1 <= n, as for orthonormal columns."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, cols)) + 1j * rng.standard_normal((n, cols))
    return Q / np.linalg.norm(Q, axis=0)


def fourier_columns(m):
    """F[r, k] = omega^(r k) / sqrt(m), omega = exp(2 pi i / m): the m one-dimensional blocks of Z_m."""
    r = np.arange(m)
    return np.exp(2j * np.pi * ((r[:, None] * r[None, :]) % m) / m) / np.sqrt(m)


def fourier_closed_form(m, sign=1):
    """want[t, k] = omega^(sign t k): the image of class 1 + t of directed(m) (sign = +1) -- sum over the m entries with
    c - r = t (mod m) of conj(omega^(r k)) omega^(c k) / m -- or of its transpose, C_3 as the reference writes it (sign = -1)."""
    t = np.arange(m)
    return np.exp(sign * 2j * np.pi * ((t[:, None] * t[None, :]) % m) / m)


# ---------------------------------------------------------------- labels
def directed(m):
    """L[r, c] = 1 + (c - r) mod m: the cyclic group Z_m, m classes of m entries, not symmetric for m >= 3."""
    i = np.arange(m)
    return 1 + (i[None, :] - i[:, None]) % m


def full(s):
    """L[p, q] = 1 + p + q s: every entry its own class, all of M_s."""
    p, q = np.indices((s, s))
    return 1 + p + q * s


C3 = np.array([[1, 3, 2], [2, 1, 3], [3, 2, 1]])                        # test/runtests.jl:50-54
P4 = np.array([[1, 2, 3, 2], [2, 1, 2, 3], [3, 2, 1, 2], [2, 3, 2, 1]])  # test/runtests.jl:43, Partition(3, ...)


def direct_sum_full(parts):
    """problems.direct_sum_labels with M_s in place of Sym(s): k diagonal copies of full(s) carrying the same labels, label
    ranges disjoint between parts, label 0 everywhere off the diagonal blocks.  Not symmetric."""
    n = sum(s * k for s, k in parts)
    L = np.zeros((n, n), dtype=np.int64)
    o = base = 0
    for s, k in parts:
        for _ in range(k):
            L[o:o + s, o:o + s] = full(s) + base
            o += s
        base += s * s
    return L


def s3_cayley_labels():
    """The group algebra of S3 (labels g^-1 h), as tests/test_gpu_parity.py builds it: not symmetric, C + C + M_2(C)."""
    import itertools
    perms = list(itertools.permutations(range(3)))
    idx = {p: i for i, p in enumerate(perms)}

    def mul(a, b):
        return tuple(a[b[i]] for i in range(3))

    def inv(a):
        r = [0] * 3
        for i, x in enumerate(a):
            r[x] = i
        return tuple(r)

    return np.array([[idx[mul(inv(g), h)] + 1 for h in perms] for g in perms])


# name -> (labels, sizes of the Gaussian Q, seed of the Gaussian Q); which kernel boundary each one hits is said where the
# GPU tests list them
GAUSSIAN_SIZES = {"Z3K70": ((1, 2, 5, 17), 51), "M4K17": ((40, 3), 52), "M4K17W": ((65, 3), 53), "Z16K5": ((1,) * 18, 54),
                  "DSF": ((3, 1, 5), 55), "N1": ((1,), 56), "C3": ((1, 1, 1), 57), "P4": ((1, 1, 1), 58)}


@functools.lru_cache(maxsize=None)
def instance(name):
    """(labels int64 n x n, d)."""
    if name == "Z3K70":
        L, d = pr.kron_with_complete(directed(3), 70, seed=3)
    elif name in ("M4K17", "M4K17W"):
        L, d = pr.kron_with_complete(full(4), 17, seed=5)
    elif name == "Z16K5":
        L, d = pr.kron_with_complete(directed(16), 5, seed=7)
    elif name == "DSF":
        L, d = pr.canonical_labels(pr.permute_labels(direct_sum_full([(1, 1), (2, 3), (5, 7), (17, 2)]), 76))
    elif name == "N1":
        L, d = np.array([[1]]), 1
    elif name == "C3":
        L, d = C3, 3
    elif name == "P4":
        L, d = P4, 3
    else:
        raise ValueError(name)
    L = np.asarray(L, dtype=np.int64)
    L.setflags(write=False)
    return L, int(d)


@functools.lru_cache(maxsize=None)
def gaussian_case(name):
    """(sizes, Q, clongdouble reference) of the instance's Gaussian Q, computed once and read-only."""
    L, d = instance(name)
    sizes, seed = GAUSSIAN_SIZES[name]
    Q = gaussian_unit_columns_complex(L.shape[0], sum(sizes), seed)
    ref = reference_images_complex(L, d, Q, sizes)
    Q.setflags(write=False)
    ref.setflags(write=False)
    return sizes, Q, ref


def class_window(d, parts, index):
    """What pkg.class_window must return, written independently: the first d % parts windows have one class more."""
    sizes = [d // parts + (1 if j < d % parts else 0) for j in range(parts)]
    return 1 + sum(sizes[:index]), sizes[index]
