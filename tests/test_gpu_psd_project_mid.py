"""sdpsr_psd_project on blocks of order 65 .. 128 (a context with psd_max_order = 128: psd_project_mid_kernel, one workgroup per
block on the Jacobi core of jacobi128.h) against numpy's eigh and a clamp (tests/sdp_admm_ref.py).

Bound: |P - P_ref|_F <= 4e-12 s |Z_k|_2 per block, |lambda_min - ref| <= 1e-12 |Z_k|_2.  Derived, not measured, the way
tests/test_gpu_psd_project.py derives its own: tests/test_gpu_small_syev.py (BOUNDS) holds this Jacobi at every order 65 .. 128 to a
residual of 1e-12 and an orthogonality of 1e-12 in units of max |lambda| = |Z|_2, so the computed eigenpairs are exact for
Z + E with |E|_F <= s (1e-12 + 2e-12) |Z|_2, the projection is non-expansive in the Frobenius norm, and the last 1e-12 s |Z|_2
is the rounding of the reconstruction's at most 64 terms; eigenvalues within 2e-13 |Z|_2 there, 1e-12 here as below order 64.
V sits in LDS up to order 97 and in global memory from 98 on, so the orders cover both sides (and the issue's 96 | 97)."""
import ctypes as C

import numpy as np
import pytest

from blockop_ref import block_offsets, flatten_blocks, split_blocks
from sdp_admm_ref import psd_project_ref
from test_gpu_psd_project import _bits, _p, _project, _spectrum, _sym

pytestmark = pytest.mark.gpu

OK, BAD_ARGUMENT, SOLVER_ERROR = 0, 5, 7
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def mid_ctx(pkg, gpu_ctx):
    with pkg.Context(device=0, seed=4321, psd_max_order=128) as ctx:
        assert ctx.psd_max_order == 128 and gpu_ctx.psd_max_order == 64
        yield ctx


def _norm2(B):
    L = np.tril(B)
    return float(np.abs(np.linalg.eigvalsh(L + np.tril(B, -1).T)).max())


def _check(ctx, sizes, blocks, mem=HOST, alias=False):
    Z = flatten_blocks(blocks)
    ref, lref = psd_project_ref(Z, sizes, return_lambda_min=True)
    st, P, lm = _project(ctx, sizes, Z.copy(), mem, alias)
    assert st == OK, ctx._lib.sdpsr_last_error(ctx._h)
    worst = {}
    for k, (B, Pk, Rk) in enumerate(zip(blocks, split_blocks(P, sizes), split_blocks(ref, sizes))):
        s, scale = B.shape[0], _norm2(B)
        assert np.array_equal(_bits(Pk), _bits(Pk.T))  # exactly symmetric
        err = np.linalg.norm(Pk - Rk)
        assert err <= 4e-12 * s * scale, (k, s, err, scale)
        assert abs(lm[k] - lref[k]) <= 1e-12 * scale, (k, s, lm[k], lref[k])
        if scale > 0:
            worst[s] = max(worst.get(s, (0.0, 0.0)), (err / (s * scale), abs(lm[k] - lref[k]) / scale))
    return P, lm, worst


@pytest.mark.parametrize("s", [65, 66, 95, 96, 97, 98, 127, 128])
def test_one_indefinite_block(mid_ctx, s):
    rng = np.random.default_rng(100 + s)
    for mem in (HOST, DEVICE):
        _, _, worst = _check(mid_ctx, [s], [_sym(rng, s)], mem)
        print(f"order {s}: |P - P_ref|_F / (s |Z|_2) = {worst[s][0]:.2e}, |lambda_min - ref| / |Z|_2 = {worst[s][1]:.2e}")


def test_mixed_batch_keeps_the_small_blocks_bits(mid_ctx, gpu_ctx):
    sizes = [1, 128, 2, 65, 64, 97, 17, 1]
    rng = np.random.default_rng(7)
    blocks = [_sym(rng, s) for s in sizes]
    small = [k for k, s in enumerate(sizes) if s <= 64]
    st, Ps, ls = _project(gpu_ctx, [sizes[k] for k in small], flatten_blocks([blocks[k] for k in small]))  # a DEFAULT context
    assert st == OK
    for mem in (HOST, DEVICE):
        P, lm, _ = _check(mid_ctx, sizes, blocks, mem)
        got = split_blocks(P, sizes)
        assert np.array_equal(_bits(flatten_blocks([got[k] for k in small])), _bits(Ps)) and np.array_equal(_bits(lm[small]), _bits(ls))


def test_three_hundred_blocks_of_order_65(mid_ctx):
    sizes = [65] * 300  # more workgroups than CUs
    rng = np.random.default_rng(8)
    _, _, worst = _check(mid_ctx, sizes, [_sym(rng, 65) for _ in sizes], DEVICE)
    print(f"300 x 65: worst |P - P_ref|_F / (s |Z|_2) = {worst[65][0]:.2e}")


@pytest.mark.parametrize("s", [65, 97, 128])
def test_special_inputs(mid_ctx, s):
    rng = np.random.default_rng(200 + s)
    w = rng.uniform(0.5, 2.0, s)
    psd, nd = _spectrum(rng, s, w), _spectrum(rng, s, -w)
    rank_one = np.outer(*(2 * [rng.standard_normal(s)]))

    def signs(npos):  # exactly npos positive values, the others negative
        return np.where(np.arange(s) < npos, w, -w)

    many = max(65, (3 * s) // 4)  # more than 64 positive values: their indices need the second ballot
    sizes = [s] * 9
    blocks = [psd, nd, np.zeros((s, s)), rank_one, -rank_one, _spectrum(rng, s, signs(s // 2)), _spectrum(rng, s, signs(s // 2 + 1)),
              _spectrum(rng, s, signs(many)), _sym(rng, s)]
    for k, npos in ((5, s // 2), (6, s // 2 + 1), (7, many)):
        assert np.count_nonzero(np.linalg.eigvalsh(blocks[k]) > 0) == npos
    P, lm, worst = _check(mid_ctx, sizes, blocks)
    Pk = split_blocks(P, sizes)
    assert np.linalg.norm(Pk[0] - psd) <= 4e-12 * s * _norm2(psd)                 # already PSD: P = Z within the bound
    assert np.array_equal(_bits(Pk[1]), _bits(np.zeros((s, s))))                  # negative definite: exactly +0.0
    assert np.array_equal(_bits(Pk[2]), _bits(np.zeros((s, s)))) and lm[2] == 0   # all-zero: +0.0 everywhere
    assert np.linalg.norm(Pk[3] - rank_one) <= 4e-12 * s * _norm2(rank_one)
    assert np.linalg.norm(Pk[4]) <= 4e-12 * s * _norm2(rank_one)
    print(f"special inputs at order {s}: worst |P - P_ref|_F / (s |Z|_2) = {worst[s][0]:.2e}")


def test_result_scales_exactly_with_powers_of_two(mid_ctx):
    rng = np.random.default_rng(32)
    sizes = [65, 1, 98]
    blocks = [_sym(rng, s) for s in sizes]
    st, P1, l1 = _project(mid_ctx, sizes, flatten_blocks(blocks))
    assert st == OK
    for e in (-450, 450):
        f = 2.0 ** e
        st, P, lm = _project(mid_ctx, sizes + sizes, flatten_blocks([B * f for B in blocks] + blocks))
        assert st == OK
        n = P1.size
        assert np.array_equal(_bits(P[:n]), _bits(P1 * f)) and np.array_equal(_bits(lm[:3]), _bits(l1 * f))
        assert np.array_equal(_bits(P[n:]), _bits(P1)) and np.array_equal(_bits(lm[3:]), _bits(l1))


def test_only_the_lower_triangle_is_read_and_P_may_alias_Z(mid_ctx):
    rng = np.random.default_rng(33)
    sizes = [66, 2, 99, 1]
    blocks = [_sym(rng, s) for s in sizes]
    blocks[2] = _spectrum(rng, 99, np.where(np.arange(99) < 80, 1.0, -1.0) * rng.uniform(0.5, 2.0, 99))  # the complement route re-reads Z
    st, P, lm = _project(mid_ctx, sizes, flatten_blocks(blocks))
    assert st == OK
    poisoned = [np.where(np.triu(np.ones_like(B), 1) > 0, np.nan, B) for B in blocks]
    for mem in (HOST, DEVICE):
        for alias in (False, True):
            st2, P2, l2 = _project(mid_ctx, sizes, flatten_blocks(poisoned), mem, alias)
            assert st2 == OK and np.array_equal(_bits(P), _bits(P2)) and np.array_equal(_bits(lm), _bits(l2)), (mem, alias)
    st3, P3, _ = _project(mid_ctx, sizes, flatten_blocks(blocks), lam=False)
    assert st3 == OK and np.array_equal(_bits(P), _bits(P3))  # lambda_min = NULL: the same P bits


def test_nan_poisons_its_block_alone(mid_ctx):
    rng = np.random.default_rng(34)
    sizes = [65, 3, 100, 1, 70]
    blocks = [_sym(rng, s) for s in sizes]
    st, P, lm = _project(mid_ctx, sizes, flatten_blocks(blocks))
    assert st == OK
    bad = [B.copy() for B in blocks]
    bad[2][40, 7] = np.nan
    st2, P2, l2 = _project(mid_ctx, sizes, flatten_blocks(bad))
    assert st2 == SOLVER_ERROR and b"NaN" in mid_ctx._lib.sdpsr_last_error(mid_ctx._h)
    off = block_offsets(sizes)
    for k in range(len(sizes)):
        a, b = P[off[k]:off[k + 1]], P2[off[k]:off[k + 1]]
        if k == 2:
            assert np.all(np.isnan(b)) and np.isnan(l2[k])
        else:
            assert np.array_equal(_bits(a), _bits(b)) and l2[k] == lm[k]
    assert _project(mid_ctx, sizes, flatten_blocks(blocks))[0] == OK  # the ctx stays usable


def test_equal_bytes_across_calls_memories_and_contexts(pkg, mid_ctx):
    sizes = [1, 65, 64, 128, 2, 97, 98]
    rng = np.random.default_rng(35)
    Z = flatten_blocks([_sym(rng, s) for s in sizes])
    outs = [_project(mid_ctx, sizes, Z), _project(mid_ctx, sizes, Z), _project(mid_ctx, sizes, Z, DEVICE)]
    with pkg.Context(seed=99, psd_max_order=128) as other:
        outs.append(_project(other, sizes, Z))
    st, P, lm = outs[0]
    assert st == OK
    for st2, P2, l2 in outs[1:]:
        assert st2 == OK and np.array_equal(_bits(P), _bits(P2)) and np.array_equal(_bits(lm), _bits(l2))


def test_refusals(mid_ctx, gpu_ctx):
    lib = mid_ctx._lib
    f = lib.sdpsr_psd_project
    Z = np.zeros(129 * 129 + 5)
    P = np.full(Z.size, 7.0)
    for sizes in ([129], [2, 129, 1]):
        sz = np.asarray(sizes, dtype=np.int32)
        assert f(mid_ctx._h, len(sizes), _p(sz), _p(Z), _p(P), None, HOST) == BAD_ARGUMENT
        assert b"128" in lib.sdpsr_last_error(mid_ctx._h) and np.all(P == 7.0)
    assert lib.sdpsr_set_psd_max_order(mid_ctx._h, 100) == BAD_ARGUMENT and lib.sdpsr_psd_max_order(mid_ctx._h) == 128
    for bad in (0, 65, 129, -1):
        assert lib.sdpsr_set_psd_max_order(mid_ctx._h, bad) == BAD_ARGUMENT
    assert lib.sdpsr_psd_max_order(mid_ctx._h) == 128
    s65 = np.asarray([65], dtype=np.int32)
    assert f(mid_ctx._h, 1, _p(s65), _p(Z), _p(P), None, HOST) == OK and np.all(P[:65 * 65] == 0.0) and np.all(P[65 * 65:] == 7.0)
    P[:] = 7.0
    assert f(gpu_ctx._h, 1, _p(s65), _p(Z), _p(P), None, HOST) == BAD_ARGUMENT  # a default context still refuses 65
    assert b"64" in lib.sdpsr_last_error(gpu_ctx._h) and np.all(P == 7.0) and lib.sdpsr_psd_max_order(gpu_ctx._h) == 64


def test_python_mirror(pkg, gpu_ctx):
    import torch
    sizes = [66, 3, 100]
    rng = np.random.default_rng(36)
    blocks = [_sym(rng, s) for s in sizes]
    flat = flatten_blocks(blocks)
    ref = psd_project_ref(flat, sizes)
    with pkg.Context(psd_max_order=128) as ctx:
        assert ctx.psd_max_order == 128
        P = pkg.psd_project(blocks, sizes, ctx=ctx)
        assert [p.shape for p in P] == [(s, s) for s in sizes]
        for Pk, Rk, B in zip(P, split_blocks(ref, sizes), blocks):
            assert np.linalg.norm(Pk - Rk) <= 4e-12 * B.shape[0] * _norm2(B)
        Pf, lm = pkg.psd_project(flat, sizes, return_lambda_min=True, ctx=ctx)
        assert np.array_equal(Pf, flatten_blocks(P)) and lm.shape == (3,)
        Pt, lt = pkg.psd_project(torch.from_numpy(flat).cuda(), sizes, return_lambda_min=True, ctx=ctx)  # torch in, torch out
        assert torch.is_tensor(Pt) and Pt.is_cuda and np.array_equal(Pt.cpu().numpy(), Pf) and np.array_equal(lt.cpu().numpy(), lm)
        with pytest.raises(ValueError, match="128"):
            pkg.psd_project(np.zeros(129 * 129), [129], ctx=ctx)
        with pytest.raises(ValueError):
            ctx.psd_max_order = 100
        ctx.psd_max_order = 64
        assert ctx.psd_max_order == 64
        with pytest.raises(ValueError, match="64"):
            pkg.psd_project(flat, sizes, ctx=ctx)
    with pytest.raises(ValueError, match="64"):
        pkg.psd_project(flat, sizes, ctx=gpu_ctx)
