"""Host side of the sdpsr_basis_image tests (tests/test_gpu_basis_image_entry.py, tests/test_basis_image_window_cpu.py):
the projection formula over the entries of each class, and the seeded arbitrary Q."""
import numpy as np


def reference_images(L, d, Q, sizes, dtype=np.longdouble):
    """ref[i - 1, :] = the images of class i, block after block, each block column-major -- the layout of
    sdpsr_block_images -- from blks[i][k][a, b] = sum over the entries (r, c) of class i of Q_k[r, a] Q_k[c, b]
    (src/diagonalize.jl:64-89), in ``dtype`` (np.longdouble: the reference; np.float64: what rounding alone does),
    not clamped.  Q: n x sum(sizes), blocks side by side."""
    n = L.shape[0]
    flat = np.asarray(L).ravel(order="F").astype(np.int64)
    idx = np.arange(n * n)
    rows, cols = idx % n, idx // n
    Ql = np.asarray(Q, dtype=dtype)
    S = sum(s * s for s in sizes)
    ref = np.zeros((d + 1, S), dtype=dtype)
    c0 = off = 0
    for s in sizes:
        for b in range(s):
            qc = Ql[cols, c0 + b]
            for a in range(s):
                np.add.at(ref[:, off + a + b * s], flat, Ql[rows, c0 + a] * qc)
        c0 += s
        off += s * s
    return ref[1:]


def gaussian_unit_columns(n, cols, seed):
    """n x cols standard normal columns scaled to unit norm: nothing orthogonal, nothing invariant.  Then
    sum over any set of entries of |q_a[r]| |q_b[c]| <= ||q_a||_1 ||q_b||_1 <= n, the same size as for orthonormal columns."""
    Q = np.random.default_rng(seed).standard_normal((n, cols))
    return Q / np.linalg.norm(Q, axis=0)


def class_window(d, parts, index):
    """What pkg.class_window must return, written independently: the first d % parts windows have one class more."""
    sizes = [d // parts + (1 if j < d % parts else 0) for j in range(parts)]
    return 1 + sum(sizes[:index]), sizes[index]
