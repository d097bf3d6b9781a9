"""sdpsr_psd_project (the batched projection onto the PSD cone) against numpy's eigh and a clamp (tests/sdp_admm_ref.py).

Bound: |P - P_ref|_F <= 4e-12 s max|Z_k| per block.  Derived from what the project already holds this Jacobi solver to
(tests/test_gpu_blockop.py: residual 8e-13 max|Z|, orthogonality 1e-12): the computed eigenpairs are exact for Z + E with
|E|_F <= s (8e-13 + 2e-12) max|Z|, and the projection is non-expansive in the Frobenius norm.  lambda_min: 1e-12 max|Z|."""
import ctypes as C

import numpy as np
import pytest

from blockop_ref import block_offsets, flatten_blocks, split_blocks
from sdp_admm_ref import psd_project_ref

pytestmark = pytest.mark.gpu

OK, BAD_ARGUMENT, SOLVER_ERROR = 0, 5, 7
HOST, DEVICE = 0, 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _p(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else C.c_void_p(a.ctypes.data)


def _project(ctx, sizes, Z, mem=HOST, alias=False, lam=True):
    """(status, P, lambda_min) of one call; the input is checked to be unmodified unless P aliases it."""
    sz = np.asarray(sizes, dtype=np.int32)
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    lm = np.full(len(sizes), 7.0) if lam else None
    if mem == DEVICE:
        import torch
        dZ = torch.from_numpy(Z).cuda()
        dP = dZ if alias else torch.full((Z.size,), 7.0, dtype=torch.float64, device="cuda")
        dl = torch.from_numpy(lm).cuda() if lam else None
        torch.cuda.synchronize()
        st = ctx._lib.sdpsr_psd_project(ctx._h, len(sizes), _p(sz), _p(dZ), _p(dP), _p(dl), DEVICE)
        if not alias:
            assert np.array_equal(_bits(dZ.cpu().numpy()), _bits(Z))
        return st, dP.cpu().numpy(), (dl.cpu().numpy() if lam else None)
    keep = Z.copy()
    P = Z if alias else np.full(Z.size, 7.0)
    st = ctx._lib.sdpsr_psd_project(ctx._h, len(sizes), _p(sz), _p(Z), _p(P), _p(lm), HOST)
    if not alias:
        assert np.array_equal(_bits(Z), _bits(keep))
    return st, P, lm


def _check(ctx, sizes, blocks, mem=HOST, alias=False):
    Z = flatten_blocks(blocks)
    ref, lref = psd_project_ref(Z, sizes, return_lambda_min=True)
    st, P, lm = _project(ctx, sizes, Z.copy(), mem, alias)
    assert st == OK, ctx._lib.sdpsr_last_error(ctx._h)
    worst = 0.0
    for k, (B, Pk, Rk) in enumerate(zip(blocks, split_blocks(P, sizes), split_blocks(ref, sizes))):
        s, scale = B.shape[0], np.abs(np.tril(B)).max()
        assert np.array_equal(_bits(Pk), _bits(Pk.T))  # exactly symmetric
        err = np.linalg.norm(Pk - Rk)
        assert err <= 4e-12 * s * scale, (k, s, err, scale)
        assert abs(lm[k] - lref[k]) <= 1e-12 * scale
        worst = max(worst, err / (s * scale) if scale > 0 else 0.0)
    return P, lm, worst


def _sym(rng, s):
    A = rng.standard_normal((s, s))
    return A + A.T


def _spectrum(rng, s, w):
    Q, _ = np.linalg.qr(rng.standard_normal((s, s)))
    B = (Q * np.asarray(w, dtype=np.float64)) @ Q.T
    return (B + B.T) / 2


@pytest.mark.parametrize("s", [1, 2, 3, 7, 33, 63, 64])
def test_one_indefinite_block(gpu_ctx, s):
    rng = np.random.default_rng(100 + s)
    for mem in (HOST, DEVICE):
        _, _, worst = _check(gpu_ctx, [s], [_sym(rng, s)], mem)
        print(f"order {s}: |P - P_ref|_F / (s max|Z|) = {worst:.2e}")


def test_mixed_batch(gpu_ctx):
    sizes = [1, 64, 2, 1, 17] * 3
    rng = np.random.default_rng(7)
    blocks = [_sym(rng, s) for s in sizes]
    for mem in (HOST, DEVICE):
        _check(gpu_ctx, sizes, blocks, mem)


def test_a_thousand_blocks_of_order_two(gpu_ctx):
    sizes = [2] * 1000
    rng = np.random.default_rng(8)
    blocks = [_sym(rng, 2) for _ in sizes]
    P, lm, _ = _check(gpu_ctx, sizes, blocks)
    w = np.asarray([np.linalg.eigvalsh(B) for B in blocks])
    assert 100 < np.count_nonzero(w[:, 0] > 0) + np.count_nonzero(w[:, 1] < 0) < 900  # definite blocks of both signs among them


def test_many_blocks_of_order_one(gpu_ctx):
    z = np.random.default_rng(9).standard_normal(300)
    z[:3] = [0.0, -0.0, 5.0]
    st, P, lm = _project(gpu_ctx, [1] * 300, z)
    assert st == OK and np.array_equal(_bits(P), _bits(np.where(z > 0, z, 0.0))) and np.array_equal(_bits(lm), _bits(z))


@pytest.mark.parametrize("s", [2, 7, 64])
def test_special_inputs(gpu_ctx, s):
    rng = np.random.default_rng(200 + s)
    w = rng.uniform(0.5, 2.0, s)
    psd, nd = _spectrum(rng, s, w), _spectrum(rng, s, -w)
    rank_one = np.outer(*(2 * [rng.standard_normal(s)]))
    rank_one_neg = -rank_one
    sizes = [s] * 6
    blocks = [psd, nd, np.zeros((s, s)), rank_one, rank_one_neg, _sym(rng, s)]
    P, lm, _ = _check(gpu_ctx, sizes, blocks)
    Pk = split_blocks(P, sizes)
    assert np.linalg.norm(Pk[0] - psd) <= 4e-12 * s * np.abs(psd).max()          # already PSD: P = Z within the bound
    assert np.array_equal(_bits(Pk[1]), _bits(np.zeros((s, s))))                  # negative definite: exactly +0.0
    assert np.array_equal(_bits(Pk[2]), _bits(np.zeros((s, s)))) and lm[2] == 0   # all-zero: +0.0 everywhere
    assert np.linalg.norm(Pk[3] - rank_one) <= 4e-12 * s * np.abs(rank_one).max()
    assert np.abs(Pk[4]).max() <= 4e-12 * s * np.abs(rank_one).max()


@pytest.fixture(scope="module")
def own_ctx(pkg):
    """A context of this module's own: tests/test_gpu_sdp_solve.py counts the host waits of the shared one, and those follow
    the number of uploads the context has made before (its pinned upload ring wraps every 32)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with pkg.Context(device=0, seed=4321) as ctx:
        yield ctx


@pytest.mark.parametrize("s", [2, 3, 16, 17, 63, 64])
def test_half_and_half_plus_one_positive(own_ctx, s):
    """Exactly s // 2 positive eigenvalues sums the positive columns, one more takes the complement (which re-reads Z, so
    it is run with P aliasing Z too), at even and odd orders on both sides of one wave per block."""
    rng = np.random.default_rng(300 + s)
    w = rng.uniform(0.5, 2.0, s)
    counts = [s // 2, s // 2 + 1]
    blocks = [_spectrum(rng, s, np.where(np.arange(s) < npos, w, -w)) for npos in counts]
    for B, npos in zip(blocks, counts):
        assert np.count_nonzero(np.linalg.eigvalsh(B) > 0) == npos
    P, lm, _ = _check(own_ctx, [s, s], blocks)
    for mem in (HOST, DEVICE):
        st, P2, l2 = _project(own_ctx, [s, s], flatten_blocks(blocks), mem, alias=True)
        assert st == OK and np.array_equal(_bits(P), _bits(P2)) and np.array_equal(_bits(lm), _bits(l2)), mem


def test_triple_eigenvalue_that_includes_zero(gpu_ctx):
    rng = np.random.default_rng(31)
    blocks = [_spectrum(rng, 6, [0.0, 0.0, 0.0, -1.0, 0.5, 3.0]), _spectrum(rng, 7, [2.0, 2.0, 2.0, 0.0, -1.0, -1.0, -1.0]),
              np.diag([3.0, -1.0, 0.0, 0.0, 0.0])]
    P, lm, _ = _check(gpu_ctx, [6, 7, 5], blocks)
    assert np.array_equal(split_blocks(P, [6, 7, 5])[2], np.diag([3.0, 0.0, 0.0, 0.0, 0.0]))


def test_result_scales_exactly_with_powers_of_two(gpu_ctx):
    rng = np.random.default_rng(32)
    sizes = [3, 1, 9]
    blocks = [_sym(rng, s) for s in sizes]
    st, P1, l1 = _project(gpu_ctx, sizes, flatten_blocks(blocks))
    assert st == OK
    for e in (-450, 450):
        f = 2.0 ** e
        st, P, lm = _project(gpu_ctx, sizes + sizes, flatten_blocks([B * f for B in blocks] + blocks))
        assert st == OK
        n = P1.size
        assert np.array_equal(_bits(P[:n]), _bits(P1 * f)) and np.array_equal(_bits(lm[:3]), _bits(l1 * f))
        assert np.array_equal(_bits(P[n:]), _bits(P1)) and np.array_equal(_bits(lm[3:]), _bits(l1))


def test_only_the_lower_triangle_is_read_and_P_may_alias_Z(gpu_ctx):
    rng = np.random.default_rng(33)
    sizes = [5, 2, 40, 1]
    blocks = [_sym(rng, s) for s in sizes]
    st, P, lm = _project(gpu_ctx, sizes, flatten_blocks(blocks))
    poisoned = [np.where(np.triu(np.ones_like(B), 1) > 0, np.nan, B) for B in blocks]
    for mem in (HOST, DEVICE):
        for alias in (False, True):
            st2, P2, l2 = _project(gpu_ctx, sizes, flatten_blocks(poisoned), mem, alias)
            assert st2 == OK and np.array_equal(_bits(P), _bits(P2)) and np.array_equal(_bits(lm), _bits(l2)), (mem, alias)
    st3, P3, _ = _project(gpu_ctx, sizes, flatten_blocks(blocks), lam=False)
    assert st3 == OK and np.array_equal(_bits(P), _bits(P3))  # lambda_min = NULL: the same P bits


def test_nan_poisons_its_block_alone(gpu_ctx):
    rng = np.random.default_rng(34)
    sizes = [4, 3, 1, 1, 20]
    blocks = [_sym(rng, s) for s in sizes]
    st, P, lm = _project(gpu_ctx, sizes, flatten_blocks(blocks))
    assert st == OK
    bad = [B.copy() for B in blocks]
    bad[1][2, 0] = np.nan
    bad[3][0, 0] = np.inf
    st2, P2, l2 = _project(gpu_ctx, sizes, flatten_blocks(bad))
    assert st2 == SOLVER_ERROR and b"NaN" in gpu_ctx._lib.sdpsr_last_error(gpu_ctx._h)
    off = block_offsets(sizes)
    for k in range(len(sizes)):
        a, b = P[off[k]:off[k + 1]], P2[off[k]:off[k + 1]]
        if k in (1, 3):
            assert np.all(np.isnan(b)) and np.isnan(l2[k])
        else:
            assert np.array_equal(_bits(a), _bits(b)) and l2[k] == lm[k]
    assert _project(gpu_ctx, sizes, flatten_blocks(blocks))[0] == OK  # the ctx stays usable


def test_refusals(gpu_ctx):
    f = gpu_ctx._lib.sdpsr_psd_project
    Z = np.zeros(65 * 65)
    P = np.full(65 * 65, 7.0)
    for sizes in ([65], [2, 65, 1]):
        sz = np.asarray(sizes, dtype=np.int32)
        assert f(gpu_ctx._h, len(sizes), _p(sz), _p(Z), _p(P), None, HOST) == BAD_ARGUMENT
        assert b"64" in gpu_ctx._lib.sdpsr_last_error(gpu_ctx._h) and np.all(P == 7.0)
    two, zero = np.asarray([2], dtype=np.int32), np.asarray([0], dtype=np.int32)
    assert f(gpu_ctx._h, 0, _p(two), _p(Z), _p(P), None, HOST) == BAD_ARGUMENT
    assert f(gpu_ctx._h, 1, _p(zero), _p(Z), _p(P), None, HOST) == BAD_ARGUMENT
    assert f(gpu_ctx._h, 1, None, _p(Z), _p(P), None, HOST) == BAD_ARGUMENT
    assert f(gpu_ctx._h, 1, _p(two), None, _p(P), None, HOST) == BAD_ARGUMENT
    assert f(gpu_ctx._h, 1, _p(two), _p(Z), None, None, HOST) == BAD_ARGUMENT
    assert f(gpu_ctx._h, 1, _p(two), _p(Z), _p(P), None, HOST) == OK


def test_equal_bytes_across_calls_and_contexts(pkg, gpu_ctx):
    sizes = [1, 64, 2, 1, 17, 3, 3]
    rng = np.random.default_rng(35)
    Z = flatten_blocks([_sym(rng, s) for s in sizes])
    st, P, lm = _project(gpu_ctx, sizes, Z)
    st2, P2, l2 = _project(gpu_ctx, sizes, Z, DEVICE)
    with pkg.Context(seed=99) as other:
        st3, P3, l3 = _project(other, sizes, Z)
    assert st == st2 == st3 == OK
    assert np.array_equal(_bits(P), _bits(P2)) and np.array_equal(_bits(P), _bits(P3))
    assert np.array_equal(_bits(lm), _bits(l2)) and np.array_equal(_bits(lm), _bits(l3))


def test_python_mirror(pkg, gpu_ctx):
    import torch
    sizes = [2, 3, 1]
    rng = np.random.default_rng(36)
    blocks = [_sym(rng, s) for s in sizes]
    flat = flatten_blocks(blocks)
    ref = psd_project_ref(flat, sizes)
    P = pkg.psd_project(blocks, sizes, ctx=gpu_ctx)
    assert [p.shape for p in P] == [(s, s) for s in sizes] and np.abs(flatten_blocks(P) - ref).max() <= 4e-12 * 3 * np.abs(flat).max()
    Pf, lm = pkg.psd_project(flat, sizes, return_lambda_min=True, ctx=gpu_ctx)
    assert np.array_equal(Pf, flatten_blocks(P)) and lm.shape == (3,)
    Pt, lt = pkg.psd_project(torch.from_numpy(flat).cuda(), sizes, return_lambda_min=True, ctx=gpu_ctx)  # torch in, torch out
    assert torch.is_tensor(Pt) and Pt.is_cuda and np.array_equal(Pt.cpu().numpy(), Pf) and np.array_equal(lt.cpu().numpy(), lm)
    with pytest.raises(ValueError, match="64"):
        pkg.psd_project(np.zeros(65 * 65), [65], ctx=gpu_ctx)
