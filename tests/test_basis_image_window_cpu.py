"""The host side of sdpsr_basis_image: class_window's arithmetic, the wrapper's checks that run before the library is
called, and the premise of the GPU tests' bound for an arbitrary Q (tests/test_gpu_basis_image_entry.py)."""
import numpy as np
import pytest

import basis_image_helpers as H


@pytest.mark.parametrize("d", [0, 1, 7, 27828])
@pytest.mark.parametrize("parts", [1, 3, 8, 64])
def test_class_window_tiles_the_classes(pkg, d, parts):
    wins = [pkg.class_window(d, parts, j) for j in range(parts)]
    assert wins == [H.class_window(d, parts, j) for j in range(parts)]
    nxt = 1
    for first, count in wins:  # disjoint, in order, nothing left out
        assert first == nxt and count >= 0
        nxt = first + count
    assert nxt == d + 1
    counts = [c for _, c in wins]
    assert max(counts) - min(counts) <= 1
    assert (0 in counts) == (parts > d)
    assert sum(counts) == d


def test_class_window_rejects_nonsense(pkg):
    for args in [(-1, 1, 0), (5, 0, 0), (5, 2, 2), (5, 2, -1)]:
        with pytest.raises(ValueError):
            pkg.class_window(*args)


class _NoLibrary:
    """A context whose library must not be reached: the wrapper has to refuse before it."""
    label_width = 32
    label_dtype = np.dtype(np.uint32)

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper went on to the library ({name})")


def test_wrapper_rejects_a_q_hat_that_does_not_fit_the_partition(pkg, problems):
    L, d, _ = problems.known_blocks_instance("DS")
    n = L.shape[0]
    P = pkg.Partition(d, L.astype(np.uint32))
    ctx = _NoLibrary()
    good = [np.zeros((n, 3)), np.zeros((n, 1))]
    with pytest.raises(ValueError, match="rows"):
        pkg.basis_image([np.zeros((n - 1, 3)), np.zeros((n - 1, 1))], P, ctx=ctx)
    with pytest.raises(ValueError, match="rows"):
        pkg.basis_image((np.zeros((n + 1, 4)), [3, 1]), P, ctx=ctx)
    with pytest.raises(ValueError, match="sum to"):
        pkg.basis_image((np.zeros((n, 4)), [3, 2]), P, ctx=ctx)
    with pytest.raises(ValueError, match=">= 1"):
        pkg.basis_image((np.zeros((n, 4)), [4, 0]), P, ctx=ctx)
    with pytest.raises(ValueError, match="> n"):
        pkg.basis_image((np.zeros((n, n + 1)), [n, 1]), P, ctx=ctx)
    with pytest.raises(ValueError, match="no blocks"):
        pkg.basis_image([], P, ctx=ctx)
    for classes in [(0, 1), (d, 2), (1, -1), (d + 1, 1)]:
        with pytest.raises(ValueError, match="window"):
            pkg.basis_image(good, P, classes=classes, ctx=ctx)


@pytest.mark.parametrize("sizes,seed", [((3, 1, 5), 41), ((2, 2), 41), ((1,) * 18, 44), ((3, 2), 43)])
def test_fp64_evaluation_is_far_inside_the_bound(problems, sizes, seed):
    """The GPU tests hold the library to 2e-12 n against the longdouble projection formula also for Gaussian columns of
    unit norm.  That presumes fp64 rounding of the same sums is negligible there as it is for orthonormal columns:
    the plain NumPy fp64 evaluation must stay within a tenth of the bound for the very Q the GPU tests use."""
    if len(sizes) == 18:
        L, d = problems.kron_with_complete(problems.symmetric_circulant_labels(16), 5)
    elif sizes == (3, 2):
        L, d = problems.kron_with_complete(problems.sym_full_labels(124), 2)
    else:
        L, d, _ = problems.known_blocks_instance("DS")
    L = np.asarray(L, dtype=np.int64)
    n = L.shape[0]
    Q = H.gaussian_unit_columns(n, sum(sizes), seed)
    assert np.allclose(np.linalg.norm(Q, axis=0), 1.0, atol=1e-15)
    ref = H.reference_images(L, d, Q, sizes)
    f64 = H.reference_images(L, d, Q, sizes, dtype=np.float64)
    err = float(np.abs(f64.astype(np.longdouble) - ref).max())
    assert err <= 0.1 * 2e-12 * n, (err, n)
    # and the formula itself: the classes partition the entries, so the images of all classes (label 0 included) add up to
    # Q_k' J Q_k = (column sums)(column sums)'
    if not (L == 0).any():
        tot, c0, off = ref.sum(axis=0), 0, 0
        for s in sizes:
            cs = Q[:, c0:c0 + s].sum(axis=0)
            assert np.allclose(np.asarray(tot[off:off + s * s], dtype=np.float64).reshape(s, s, order="F"), np.outer(cs, cs), atol=1e-9)
            c0 += s
            off += s * s
