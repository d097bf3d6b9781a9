"""The NumPy restatement of sdpsr_block_images_sparse (tests/sparse_images_ref.py) checked on its own: it is what the GPU
tests compare the library with."""
import numpy as np
import pytest
import scipy.sparse as sp

from sparse_images_ref import embed, max_asym_ref, sparse_ref, to_dense, virtual_blocks, virtual_sizes


def _random_flat(rng, sizes, count, density, cx):
    S = sum(s * s for s in sizes)
    v = rng.standard_normal(count * S)
    if cx:
        v = v + 1j * rng.standard_normal(count * S)
    return v * (rng.random(count * S) < density)


@pytest.mark.parametrize("cx", [False, True])
@pytest.mark.parametrize("sizes", [[1], [3], [1, 2, 3], [4, 1, 5]])
def test_full_triangle_round_trips(sizes, cx):
    rng = np.random.default_rng(7)
    flat = _random_flat(rng, sizes, 6, 0.5, cx)
    flat[:sum(s * s for s in sizes)] = 0  # an empty class
    r = sparse_ref(flat, sizes, upper=False, index_base=1)
    vs = virtual_sizes(sizes, cx)
    dense = to_dense(r, vs, 6, index_base=1)
    vb, count = virtual_blocks(flat, sizes)
    assert count == 6 and r["classptr"][0] == 0 and r["classptr"][1] == 0 and r["classptr"][-1] == r["nnz"]
    for i in range(6):
        for k in range(len(sizes)):
            assert np.array_equal(dense[i][k], vb[k][i])
    assert not (r["val"] == 0).any()


@pytest.mark.parametrize("upper", [True, False])
def test_agrees_with_scipy_per_block(upper):
    rng = np.random.default_rng(11)
    sizes = [5, 2, 7]
    flat = _random_flat(rng, sizes, 4, 0.4, False)
    r = sparse_ref(flat, sizes, upper=upper)
    vb, _ = virtual_blocks(flat, sizes)
    e = 0
    for i in range(4):
        assert r["classptr"][i] == e
        for k in range(len(sizes)):
            M = sp.csc_matrix(vb[k][i])  # column-major: sorted by column, then row
            M = sp.triu(M, format="csc") if upper else M
            M.sort_indices()
            M.eliminate_zeros()
            coo = M.tocoo()
            order = np.lexsort((coo.row, coo.col))
            n = coo.nnz
            assert np.array_equal(r["blk"][e:e + n], np.full(n, k))
            assert np.array_equal(r["row"][e:e + n], coo.row[order]) and np.array_equal(r["col"][e:e + n], coo.col[order])
            assert np.array_equal(r["val"][e:e + n], coo.data[order])
            e += n
    assert e == r["nnz"]


def test_tolerance_zeros_and_nan():
    tol = 1e-8
    flat = np.array([tol, -tol, np.nextafter(tol, 1), -np.nextafter(tol, 1), 0.0, -0.0, np.nan, 1.0])
    r = sparse_ref(flat, [1], upper=True, tol=tol)
    assert np.array_equal(np.diff(r["classptr"]), [0, 0, 1, 1, 0, 0, 1, 1])
    assert np.isnan(r["val"][2]) and r["nnz"] == 4
    r0 = sparse_ref(flat, [1], upper=True, tol=0.0)
    assert np.array_equal(np.diff(r0["classptr"]), [1, 1, 1, 1, 0, 0, 1, 1])


def test_embedding_of_a_hermitian_block_is_symmetric():
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    H = Z + Z.conj().T
    E = embed(H)
    assert np.array_equal(E, E.T)
    flat = H.ravel(order="F")
    assert max_asym_ref(flat, [4]) == 0.0
    up, full = sparse_ref(flat, [4], upper=True), sparse_ref(flat, [4], upper=False)
    d = to_dense(up, [8], 1)[0][0]
    assert np.array_equal(d + np.triu(d, 1).T, to_dense(full, [8], 1)[0][0])


def test_embedding_of_a_general_block_has_the_formula_s_asymmetry():
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
    A, B = Z.real, Z.imag
    # [A -B; B A] - transpose = [A - A', -(B + B'); B + B', A - A']
    want = max(np.abs(A - A.T).max(), np.abs(B + B.T).max())
    assert max_asym_ref(Z.ravel(order="F"), [3]) == want
    R = rng.standard_normal((5, 5))
    assert max_asym_ref(R.ravel(order="F"), [5]) == np.abs(R - R.T).max()
    assert max_asym_ref(np.zeros(0), [2]) == 0.0
