"""Plain NumPy references for the kernels of the module-compression driver (csrc/kernels_module.hip, the class sums of
csrc/kernels_blockdiag.hip), shared by tests/test_module_kernels_ref_cpu.py and tests/test_gpu_module_kernels.py.

Products come back as (result, abs) with `result` formed in np.longdouble (or exactly, in int64, where the inputs are integers)
and abs = |A|'|B| (resp. |In||S|, |A(v)||W|), the matrix the rounding bound of a dot product is stated in:

    |fl(sum a_i b_i) - sum a_i b_i|  <=  gamma_k sum |a_i b_i|,   gamma_k ~ k 2^-53,

for every summation order, with or without FMA.  The GPU tests assert |got - ref| <= 2 k 2^-53 abs (the 2 covers the second-order
terms and the final rounding of the long-double reference).  abs is formed in float64: its own relative error (k 2^-53) is far
inside that factor.

Nothing here touches the library."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
U = 2.0 ** -53

# the keys of the GPU tests' label products (G of them per row) -- the CPU test checks the class values of each against sdpsr_hash.h
KEYS = (0x1234567, 0x89ABCDEF, 0x13579BDF0F1E2D3C, 0xFEDCBA9876543210)
RANDOM_VECTOR_KEYS = (0xC0FFEE, 0xFFFFFFFFFFFFFFFF)  # the keys of the random_vector test


def fmix64(z):
    """sdpsr_fmix64 on uint64 arrays (wrap-around arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def class_uniform(key, labels):
    """v(key, l) = (fmix(key + GOLDEN l) >> 11) / 2^53 for l >= 1, v(key, 0) = 0 (sdpsr_class_uniform; label 0 carries no value)."""
    lab = np.asarray(labels, dtype=np.uint64)
    with np.errstate(over="ignore"):
        bits = fmix64(np.uint64(key & M64) + np.uint64(GOLDEN) * lab)
    v = (bits >> np.uint64(11)).astype(np.float64) * U  # a 53-bit integer: exact in float64
    return np.where(lab == 0, 0.0, v)


def hashed_labels(n, d, salt=17):
    """Non-symmetric n x n labels 0..d, hashed from the linear index as profile kind 9 does; 0 and d are present where there is room."""
    e = np.arange(n * n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        L = (fmix64(e * np.uint64(2654435761) + np.uint64(salt)) % np.uint64(d + 1)).astype(np.uint32)
    if n * n >= 3:
        L[1] = 0
        L[2] = d
    elif d == 1:
        L[:] = 1
    return L  # column-major: entry (r, c) at r + c n


def tn_product(A, B):
    """A' B in long double with |A|'|B|."""
    ref = np.matmul(np.ascontiguousarray(A.T, dtype=np.longdouble), B.astype(np.longdouble))
    return ref, np.abs(A).T @ np.abs(B)


def _exact_int_matmul(X, Y):
    """X Y for integer-valued float64 matrices, exactly, as int64.  Every partial sum of every summation order is an integer of
    magnitude <= k max|X| max|Y| < 2^53, so the float64 product is exact whatever the BLAS does."""
    Xi, Yi = X.astype(np.int64), Y.astype(np.int64)
    assert np.array_equal(Xi, X) and np.array_equal(Yi, Y)
    assert X.shape[1] * max(1, np.abs(Xi).max()) * max(1, np.abs(Yi).max()) < 2 ** 53
    P = X @ Y
    Pi = P.astype(np.int64)
    assert np.array_equal(Pi, P)
    return Pi


def tn_product_int(A, B):
    """A' B exactly (int64) for integer-valued float64 inputs."""
    return _exact_int_matmul(np.ascontiguousarray(A.T), B)


def nn_product(In, S):
    """In S in long double with |In||S|."""
    return np.matmul(In.astype(np.longdouble), S.astype(np.longdouble)), np.abs(In) @ np.abs(S)


def nn_product_int(In, S):
    """In S exactly (int64) for integer-valued float64 inputs."""
    return _exact_int_matmul(In, S)


def label_product(n, L, keys, W):
    """Y[:, g w + j] = A_g W[:, j], A_g[r, c] = v(keys[g], L[r + c n]); W: n x w.  (result n x G w in long double, |A(v)||W|)."""
    Lm = np.asarray(L).reshape(n, n, order="F")
    Wl, Wa = W.astype(np.longdouble), np.abs(W)
    refs, sums = [], []
    for key in keys:
        A = class_uniform(key, Lm)
        refs.append(np.matmul(A.astype(np.longdouble), Wl))
        sums.append(A @ Wa)  # v >= 0
    return np.concatenate(refs, axis=1), np.concatenate(sums, axis=1)


def class_sums_int(n, d, L, x):
    """out[i - 1, r] = sum over c with L[c + r n] == i of x[c] -- COLUMN r of the labels -- exactly, for an integer-valued x."""
    Lm = np.asarray(L).reshape(n, n, order="F")
    xi = x.astype(np.int64)
    assert np.array_equal(xi, x)
    out = np.zeros((d, n), dtype=np.int64)
    for r in range(n):
        col = Lm[:, r]
        keep = col > 0
        np.add.at(out[:, r], col[keep].astype(np.int64) - 1, xi[keep])  # (label 0 contributes nowhere)
    return out


def label_form(n, d, G, w):
    """The selection rule of the label product (label_spmm_select, csrc/kernels_module.hip) restated: (mfma, tile, z, columns per
    workgroup) with tile = JT (matrix cores) or WMAX (VALU), or None where the launcher refuses."""
    if n < 1 or d < 0 or w < 1 or G not in (1, 2, 4) or G * w > 64 or d > 4000 or G * (d + 2) * 8 > 64 * 1024:
        return None
    rb = (n + 63) // 64
    zg = max(1, min(32, 2048 // rb))
    zg_cap = zg
    if n >= 64:
        JT = (w + 15) // 16
        stride = JT * 16 if (JT * 16) % 32 == 16 else JT * 16 + 16
        lds = G * ((d + 2) & ~1) * 8 + 2 * 64 * stride * 8
        best = None
        for R in (1, 2, 3):
            if R > (158 * 1024) // lds:
                break
            z0 = max(1, 256 * R // rb)
            if z0 * 32 > n:
                z0 = max(1, n // 32)
            if z0 * G * w > zg_cap * 64:
                z0 = zg_cap * 64 // (G * w)
            cp = (n + z0 - 1) // z0
            cp = (cp + 3) // 4 * 4
            z = (n + cp - 1) // cp
            per_cu = (rb * z + 255) // 256
            t_mfma = float(per_cu) * (cp // 4) * (JT * G) * 64.0 / 2400.0 * (1.5 if per_cu == 1 else 1.0)
            t_part = float(z) * n * G * w * 16.0 / 4.0e6
            cost = t_mfma + t_part
            if best is None or cost < best[0]:
                best = (cost, z, cp)
        if best is not None and lds <= (150 if JT == 4 else 64) * 1024:
            return (1, JT, best[1], best[2])
    cpb = (n + zg - 1) // zg
    cpb = (cpb + 7) // 8 * 8
    zg = (n + cpb - 1) // cpb
    if G == 1:
        tile = 8 if w <= 8 else 16 if w <= 16 else 32 if w <= 32 else 48 if w <= 48 else 64
    elif G == 2:
        tile = 8 if w <= 8 else 16 if w <= 16 else 32
    else:
        tile = 8 if w <= 8 else 16
    return (0, tile, zg, cpb)


# Every instantiation launch_label_spmm_multi can launch: (mfma, tile, G)
LABEL_INSTANTIATIONS = ([(0, t, 1) for t in (8, 16, 32, 48, 64)] + [(0, t, 2) for t in (8, 16, 32)] + [(0, t, 4) for t in (8, 16)] +
                        [(1, t, 1) for t in (1, 2, 3, 4)] + [(1, t, 2) for t in (1, 2)] + [(1, 1, 4)])

# The rows of the GPU test of the label product: (n, w, G, d) -> the (mfma, tile) each was written to reach.
LABEL_ROWS = [
    # VALU below 64 rows, every WMAX x G
    ((63, 5, 1, 7), (0, 8)), ((63, 16, 1, 7), (0, 16)), ((63, 17, 1, 7), (0, 32)), ((63, 33, 1, 7), (0, 48)), ((63, 64, 1, 7), (0, 64)),
    ((63, 8, 2, 7), (0, 8)), ((63, 9, 2, 7), (0, 16)), ((63, 32, 2, 7), (0, 32)),
    ((63, 8, 4, 7), (0, 8)), ((63, 16, 4, 7), (0, 16)),
    # a single ragged row block
    ((1, 1, 1, 1), (0, 8)), ((9, 3, 2, 4), (0, 8)),
    # VALU at n >= 64: the class table pushes the matrix-core form out of LDS
    ((200, 8, 4, 2000), (0, 8)), ((200, 20, 1, 3000), (0, 32)), ((200, 30, 2, 1200), (0, 32)), ((200, 40, 1, 3000), (0, 48)),
    # matrix cores, one element
    ((64, 16, 1, 3), (1, 1)), ((65, 17, 1, 3), (1, 2)), ((127, 33, 1, 9), (1, 3)), ((200, 49, 1, 9), (1, 4)),
    ((200, 64, 1, 4000), (1, 4)),  # the largest class table (the > 64 KiB LDS attribute)
    # matrix cores, batched
    ((130, 16, 2, 5), (1, 1)), ((130, 32, 2, 5), (1, 2)), ((130, 16, 4, 5), (1, 1)), ((333, 13, 4, 40), (1, 1)),
    # a workgroup with one whole 64-column slab followed by a partial one (72 columns = 18 steps)
    ((1062, 16, 4, 200), (1, 1)),
    # steps per workgroup an exact multiple of 16 (64 columns: one whole slab and nothing else)
    ((963, 33, 1, 9), (1, 3)),
]
# what the last two rows are there for: (column split z, columns per workgroup), asserted from the entry point's report and from label_form
LABEL_ROW_SPLIT = {(1062, 16, 4, 200): (15, 72), (963, 33, 1, 9): (16, 64)}
