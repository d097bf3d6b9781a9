"""The summation ORDER of the class-sum kernels with per-lane tables (class_sums_small_d_kernel, class_sums2_kernel of
csrc/kernels_blockdiag.hip), restated in NumPy for tests/test_gpu_class_sums_order.py.

A wave sums one column r of the labels: lane q owns the entries c = q, q + 64, q + 128, ... and adds x[c], c ascending, into its
own entry of class L[c + r n], every entry starting from +0.0; then the 64 lane sums of a class are added in lane order 0 .. 63,
again from +0.0.  Plain IEEE double additions, no FMA: the float64 additions below round the same way, so the result is the
kernel's bit for bit -- as long as the kernel keeps that order.

Nothing here touches the library."""
import numpy as np


def window(L, first, d):
    """class l - first + 1 inside the window of d classes that starts at `first`, 0 (no class) outside"""
    t = np.asarray(L).astype(np.int64) - first
    return np.where((t >= 0) & (t < d), t + 1, 0)


def mixed_magnitudes(rng, shape):
    """random signs, magnitudes 1e-8 .. 1e8: almost every addition rounds, so another order shows in the bits"""
    return rng.choice((-1.0, 1.0), size=shape) * 10.0 ** rng.uniform(-8.0, 8.0, size=shape)


def class_sums_in_order(n, d, L, X, first=1):
    """out[i - 1, r, :] = the sum over c with L[c + r n] == first + i - 1 of X[c, :] in the kernels' order.  L: n * n labels,
    column-major; X: (n, k) float64 (k = 1 for one vector, 2 for the pair kernel).  Returns (d, n, k) float64."""
    Lw = window(np.asarray(L).reshape(n, n, order="F"), first, d)  # Lw[c, r]
    X = np.asarray(X, dtype=np.float64).reshape(n, -1)
    k = X.shape[1]
    T = np.zeros((64, d + 1, n, k))  # [lane][class][column r]; class 0 collects what belongs nowhere
    rr = np.arange(n)
    for c in range(n):  # ascending: each lane meets its columns in ascending order
        T[c % 64, Lw[c], rr] += X[c]  # (one entry per r: no index repeats within the statement)
    out = np.zeros((d + 1, n, k))
    for lane in range(64):
        out += T[lane]
    return out[1:]
