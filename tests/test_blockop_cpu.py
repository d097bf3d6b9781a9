"""The NumPy reference of the reduced PSD pencil (tests/blockop_ref.py) checked on its own, and the new symbols of the
library.  No GPU."""
import ctypes as C
import pathlib

import numpy as np
import pytest

from blockop_ref import EPS, adjoint_ref, apply_ref, block_offsets, flatten_blocks, full_entries, random_triplets, split_blocks
from sparse_images_ref import sparse_ref, to_dense

ROOT = pathlib.Path(__file__).resolve().parents[1]
SIZES = [3, 1, 4]
D = 5


def _symmetric_images(sizes, d, seed, density=0.6):
    """d * sum s_k^2 elements in the layout of sdpsr_block_images, every block symmetric, a share of the entries zero."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(d):
        for s in sizes:
            B = rng.standard_normal((s, s)) * (rng.random((s, s)) < density)
            B = np.triu(B) + np.triu(B, 1).T
            out.append(B.ravel(order="F"))
    return np.concatenate(out)


def _mirrored(sp, sizes, d):
    return [[B + np.triu(B, 1).T for B in row] for row in to_dense(sp, sizes, d)]


@pytest.fixture(scope="module")
def case():
    flat = _symmetric_images(SIZES, D, 3)
    up, fu = sparse_ref(flat, SIZES, upper=True), sparse_ref(flat, SIZES, upper=False)
    rng = np.random.default_rng(4)
    x = rng.standard_normal(D)
    S = [rng.standard_normal((s, s)) for s in SIZES]
    S = [A + A.T for A in S]
    return flat, up, fu, x, S


def _full(sp, upper):
    return full_entries(sp["classptr"], sp["blk"], sp["row"], sp["col"], sp["val"], SIZES, upper=upper)


def test_apply_ref_is_the_dense_sum(case):
    flat, up, fu, x, S = case
    dense = _mirrored(up, SIZES, D)
    Z, c, mag = apply_ref(x, _full(up, True), block_offsets(SIZES)[-1])
    for k, Zk in enumerate(split_blocks(Z, SIZES)):
        want = sum(x[i] * dense[i][k] for i in range(D))
        assert np.abs(Zk - want).max() <= (D + 2) * EPS * np.abs(split_blocks(mag, SIZES)[k]).max()
        assert np.array_equal(Zk, Zk.T)
    assert c.max() <= D and c.sum() == _full(up, True)[0].size


def test_adjoint_ref_is_the_inner_product(case):
    flat, up, fu, x, S = case
    dense = _mirrored(up, SIZES, D)
    g, c, mag = adjoint_ref(flatten_blocks(S), _full(up, True), D)
    for i in range(D):
        want = sum(np.vdot(dense[i][k], S[k]) for k in range(len(SIZES)))
        assert abs(g[i] - want) <= (c[i] + 2) * EPS * mag[i]


def test_upper_and_full_triplets_give_the_same_operator(case):
    flat, up, fu, x, S = case
    n = block_offsets(SIZES)[-1]
    Zu, cu, _ = apply_ref(x, _full(up, True), n)
    Zf, cf, mf = apply_ref(x, _full(fu, False), n)
    assert np.array_equal(cu, cf) and np.abs(Zu - Zf).max() <= (D + 2) * EPS * mf.max()
    gu = adjoint_ref(flatten_blocks(S), _full(up, True), D)[0]
    gf, cg, mg = adjoint_ref(flatten_blocks(S), _full(fu, False), D)
    assert np.all(np.abs(gu - gf) <= (cg + 2) * EPS * mg)


def test_duplicates_add_and_indices_shift():
    sizes = [2]
    ptr = np.asarray([0, 3, 4], dtype=np.int64)
    blk = np.asarray([1, 1, 1, 1], dtype=np.int32)
    row = np.asarray([1, 1, 1, 2], dtype=np.int32)
    col = np.asarray([2, 2, 1, 2], dtype=np.int32)
    val = np.asarray([1.5, 2.0, 7.0, -1.0])
    full = full_entries(ptr, blk, row, col, val, sizes, upper=True, index_base=1)
    assert full[0].tolist() == [0, 0, 0, 0, 0, 1] and full[1].tolist() == [2, 1, 2, 1, 0, 3]
    Z, c, mag = apply_ref([2.0, 3.0], full, 4)
    assert Z.tolist() == [14.0, 7.0, 7.0, -3.0] and c.tolist() == [1, 2, 2, 1] and mag.tolist() == [14.0, 7.0, 7.0, 3.0]
    g, cg, _ = adjoint_ref([1.0, 10.0, 100.0, 1000.0], full, 2)
    assert g.tolist() == [3.5 * 110.0 + 7.0, -1000.0] and cg.tolist() == [5, 1]


def test_adjoint_identity():
    for upper in (True, False):
        sizes = [2, 3]
        t = random_triplets(sizes, 6, 0.5, 11, upper=upper, empty_class=2, empty_block=None, zero_pos=(1, 0, 2))
        full = full_entries(*t, sizes, upper=upper)
        rng = np.random.default_rng(12)
        x = rng.standard_normal(6)
        S = flatten_blocks([A + A.T for A in (rng.standard_normal((s, s)) for s in sizes)])
        Z, c, _ = apply_ref(x, full, 13)
        g, cg, _ = adjoint_ref(S, full, 6)
        bound = (full[0].size + 2) * EPS * np.abs(x[full[0]] * full[2] * S[full[1]]).sum()
        assert abs(np.dot(Z, S) - np.dot(x, g)) <= bound
        assert cg[2] == 0 and g[2] == 0.0
        zp = block_offsets(sizes)[1] + 0 + 2 * 3
        assert c[zp] == 0 and Z[zp] == 0.0


def test_new_symbols_are_exported():
    lib = ROOT / "sdpsymmetryreduction.jl_amd" / "libsdpsr_hip.so"
    h = C.CDLL(str(lib))  # (loading initialises no device)
    for name in ("sdpsr_blockop_create", "sdpsr_blockop_destroy", "sdpsr_blockop_info", "sdpsr_blockop_apply",
                 "sdpsr_blockop_adjoint", "sdpsr_blocks_syev"):
        assert hasattr(h, name), name
    assert h.sdpsr_version() == 5
