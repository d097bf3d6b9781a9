"""blockDiagonalize with the invariance round's two label products as ONE pass over the labels (Module::growth_round,
launch_label_spmm_pair) against the two-launch route that SDPSR_FLAG_SPMM_ONE_BY_ONE keeps, through the public entry: the pair
gives each product bit for bit what its own launch gives and draws the two keys in the same order, so block sizes, Q_hat, the
images and the ctx's stream position afterwards are EQUAL, not close.  Orders just above 512, the smallest where the automatic
selection takes the module-compression driver; both partitions end their growth in a one-element (G = 1) round on a small module:
a commutative scheme (the class sums are the module, w = 10) and ER(7) (x) K_9 (non-commutative, growth rounds, w = 50)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _instances(problems, golden):
    return {"circulant512": problems.synthetic_jordan_partition(512, seed=3),
            "er7k9": problems.kron_with_complete(golden["er7_P"], 9, seed=5)}


def _run(pkg, L, d, seed, flags):
    prof = pkg._lib.load_prof_library()
    with pkg.Context(seed=seed, flags=flags) as ctx:
        bd = pkg.blockDiagonalize(pkg.Partition(d, L), ctx=ctx, retries=1)
        cnt = (C.c_uint64 * 4)()
        ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, cnt))
        return ([int(s) for s in bd.blkSizes], [np.asarray(q) for q in bd.Q_hat], [np.asarray(b) for row in bd.blks for b in row], int(cnt[0]))


@pytest.mark.parametrize("name", ["circulant512", "er7k9"])
def test_pair_route_equals_two_launch_route(pkg, gpu_ctx, problems, golden, name):
    L, d = _instances(problems, golden)[name]
    L = np.asarray(L).astype(np.uint32)
    n = L.shape[0]
    assert n >= 512 and 2 * d + 8 <= min(n // 2, 500)  # the automatic selection compresses
    for seed in (3, 4):
        sizes_a, Q_a, B_a, draws_a = _run(pkg, L, int(d), seed, 0)
        sizes_b, Q_b, B_b, draws_b = _run(pkg, L, int(d), seed, pkg._lib.FLAG_SPMM_ONE_BY_ONE)
        assert sum(s * s for s in sizes_a) <= 64  # the module's dimension: small, so the host tail, whose invariance round carries the rider
        assert sizes_a == sizes_b and draws_a == draws_b, (seed, sizes_a, sizes_b, draws_a, draws_b)
        assert len(Q_a) == len(Q_b) and len(B_a) == len(B_b) > 0
        for x, y in zip(Q_a + B_a, Q_b + B_b):
            assert x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)), (name, seed)
