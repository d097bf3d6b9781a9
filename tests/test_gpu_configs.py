"""BASELINE.json configs at (or near) their full sizes on the GPU.  Where the CPU oracle
finishes in seconds the comparison is bit-exact against it; at N >= 4096 the checks are the
size-independent properties of the domain: the generator's partition is a fixed point
(known closure), idempotence, seed independence, block sizes known by construction."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_config1_gnp1024_theta_prime(pkg, problems, oracle):
    """configs[1]: G(1024, 0.5) theta': trivial symmetry, the loop must end at
    dim = (n^2+n)/2 = 524800 with the oracle's canonical matrix; the eigen path on the generic
    element gives one isomorphism class of 1024 one-dimensional eigenspaces."""
    n = 1024
    Cv, A, b = problems.theta_prime_problem(problems.gnp_adjacency(n, 0.5, seed=11))
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0))
    assert ref.nparts == (n * n + n) // 2
    with pkg.Context(seed=21) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
        assert P.nparts == ref.nparts
        assert np.array_equal(P.matrix, ref.matrix)
        assert P.iterations <= 3
        ne, nc = pkg.eigen_decomposition(P, atol=1.4901161193847656e-8, ctx=ctx)
        assert ne == n and nc == 1
        Qh = pkg.diagonalize(P, atol=1.4901161193847656e-8, ctx=ctx)  # 1024*1025/2 = dim
        assert [q.shape for q in Qh] == [(n, n)]


@pytest.mark.parametrize("n", [2048, 4096])
def test_generic_theta_prime_fresh_call_needs_no_overflow_ladder(pkg, problems, oracle, n):
    """G(n, 1/2) theta' at n = 2048 / 4096 (configs[1] at the sizes where the relabel path matters): no symmetry, the loop
    jumps from 3 classes to (n^2 + n) / 2 in its first iteration.  A call has no class-count prediction (the loop resets
    it), so this is the path the round-3/4 ladder of overflowing hash tables (2^12 -> 2^16 -> 2^20 slots, 12.7 ms at
    n = 4096) used to take: the first table's overflow is now followed by a sample of the signatures and the grouping.
    Device-resident inputs and labels, second call on the ctx timed: <= 3 ms at 2048, <= 8 ms at 4096.
    The canonical matrix of a partition whose classes are the unordered pairs {i, j} is known in closed form (column-major
    first occurrence = the packed lower-triangle index + 1); at 2048 the oracle's loop is run as well."""
    import time
    import torch
    Cv, A, b = problems.theta_prime_problem(problems.gnp_adjacency(n, 0.5, seed=7))
    setup = pkg.admissible_setup(Cv, A, b)
    nn, CL, X0L, U = setup
    j, i = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    expect = (lo * n - lo * (lo - 1) // 2 + (hi - lo) + 1).astype(np.uint32)
    if n <= 2048:
        ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0))
        assert ref.nparts == (n * n + n) // 2 and np.array_equal(ref.matrix.astype(np.uint32), expect)
    tCL, tX0 = torch.from_numpy(CL).cuda(), torch.from_numpy(X0L).cuda()
    tU = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
    tP = torch.zeros(n * n, dtype=torch.int32, device="cuda")
    dd, it = C.c_int64(0), C.c_int32(0)
    with pkg.Context(seed=5) as ctx:
        times = []
        for rep in range(3):
            if getattr(setup, "hint", 0):
                ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.check(ctx._lib.sdpsr_admissible_subspace(ctx._h, n, C.c_void_p(tCL.data_ptr()), C.c_void_p(tX0.data_ptr()), C.c_void_p(tU.data_ptr()),
                                                        U.shape[1], 1.4901161193847656e-08, C.c_void_p(tP.data_ptr()), C.byref(dd), C.byref(it), None, 1))
            times.append((time.perf_counter() - t0) * 1e3)
            assert dd.value == (n * n + n) // 2 and it.value <= 3
            got = tP.cpu().numpy().view(np.uint32).reshape(n, n, order="F")
            assert np.array_equal(got, expect), rep
        print(f"G({n}, 1/2) theta' admissible_subspace, device-resident: {['%.2f' % t for t in times]} ms")
        assert min(times[1:]) <= (3.0 if n <= 2048 else 8.0), times


def test_config2_qap_grid30(pkg, problems, oracle):
    """configs[2]: QAP relaxation with n = 30 facilities, N = 900, sparse A (61 x 810000)."""
    flow, dist = problems.grid_qap_instance(5, 6, seed=4, symmetric_flow=True)
    Cv, A, b = problems.qap_problem(flow, dist)
    assert A.shape == (61, 810000)
    setup = pkg.admissible_setup(Cv, A, b)
    n, CL, X0L, U = setup
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0),
                                     setup=(n, U, CL.reshape(n, n, order="F"), X0L.reshape(n, n, order="F")))
    for mode in (pkg.SQUARE_I8, pkg.SQUARE_F64):
        with pkg.Context(seed=31, square_mode=mode) as ctx:
            P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
            assert P.nparts == ref.nparts
            assert np.array_equal(P.matrix, ref.matrix)
    assert ref.nparts < (n * n + n) // 2  # the grid symmetry gives a real reduction


def test_config3_noncommutative_n4104(pkg, problems, golden):
    """configs[3] variant: ER(7) Jordan algebra (x) {I, J-I} on 72 points, N = 4104, dim 36,
    blocks [2,2,2,2,3] twice (known by construction)."""
    L, d = problems.kron_with_complete(golden["er7_P"].astype(np.int64), 72, seed=5)
    n = L.shape[0]
    assert n == 4104 and d == 36
    Cv, A, b = problems.partition_as_sdp(L, seed=2)
    setup = pkg.admissible_setup(Cv, A, b)
    mats = []
    for seed in (1, 2):
        with pkg.Context(seed=seed) as ctx:
            P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
            assert P.nparts == d
            mats.append(P.matrix)
            if seed == 1:
                bd = pkg.blockDiagonalize(P, ctx=ctx)
                assert sorted(bd.blkSizes) == sorted([2, 2, 2, 2, 3] * 2)
                # spectrum invariant on the block side only (the full 4104^2 eigensolve on the
                # host is the oracle's job at small n): block spectra must be real symmetric
                x = np.random.default_rng(3).random(d)
                for k, s in enumerate(bd.blkSizes):
                    B = sum(x[i] * bd.blks[i][k] for i in range(d))
                    assert np.abs(B - B.T).max() < 1e-8
    assert np.array_equal(mats[0], L) and np.array_equal(mats[1], L)


def test_config4_n8192_fixed_point(pkg, problems):
    """configs[4]: N = 8192 of the same generator family: closure known by construction,
    idempotence, all blocks of size 1."""
    n = 8192
    L, d = problems.synthetic_jordan_partition(n, seed=8)
    Cv, A, b = problems.partition_as_sdp(L, seed=3)
    # trace-only A: the setup stage is analytic (saves a 67M x 1 QR on the host)
    U = (np.eye(n).ravel(order="F") / np.sqrt(n))[:, None]
    c = Cv - U[:, 0] * (U[:, 0] @ Cv)
    CL = pkg.api.clamp_round_host(c, pkg.api.RTOL_DEFAULT)
    X0L = pkg.api.clamp_round_host(U[:, 0] * (1.0 / np.sqrt(n)), pkg.api.RTOL_DEFAULT)
    with pkg.Context(seed=77) as ctx:
        P = pkg.admissible_subspace(None, None, None, ctx=ctx, setup=(n, CL, X0L, np.asfortranarray(U)))
        assert P.nparts == d
        assert np.array_equal(P.matrix, L)
        ne, nc = pkg.eigen_decomposition(P, atol=1.4901161193847656e-8, ctx=ctx)
        assert ne == d and nc == d  # commutative: every eigenspace its own class


@pytest.mark.parametrize("name", ["circ256", "er7xK8"])
def test_dense_driver_block_images(pkg, problems, oracle, golden, name):
    """eig_driver 4 = dense driver (hand-written tridiagonalisation, rocSOLVER stedc, own
    compact-WY back-transformation): pinned blkSizes, the spectrum invariant and
    blks == Q_k' 1[P==i] Q_k."""
    if name == "er7xK8":
        L, d = problems.kron_with_complete(golden["er7_P"].astype(np.int64), 8, seed=5)
        expect = sorted([2, 2, 2, 2, 3] * 2)
    else:
        L = golden[f"{name}_P"].astype(np.int64)
        d = int(L.max())
        expect = list(golden[f"{name}_blk"])
    P = pkg.Partition(d, L.astype(np.uint32))
    Po = oracle.Partition(d, L)
    x = np.random.default_rng(8).random(d)
    with pkg.Context(seed=3, eig_driver=4) as ctx:
        bd = pkg.blockDiagonalize(P, ctx=ctx)
    assert sorted(bd.blkSizes) == expect, name
    full, blk = oracle.spectrum_invariant(Po, bd.blks, x)
    assert len(full) == len(blk), name
    assert np.allclose(full, blk, rtol=1e-6, atol=1e-8), name
    ref = oracle.basis_image_fast([np.asarray(q) for q in bd.Q_hat], Po)
    for i in range(0, d, max(1, d // 7)):
        for k in range(len(bd.blkSizes)):
            assert np.allclose(bd.blks[i][k], ref[i][k], atol=1e-9)


def test_generic_partition_uses_dense_driver(pkg, problems):
    """No symmetry: n distinct eigenvalues; the default driver must take the dense path."""
    n = 300
    rng = np.random.default_rng(0)
    M = rng.integers(1, 40, size=(n, n))
    M = np.triu(M) + np.triu(M, 1).T
    P = pkg.Partition(int(M.max()), M.astype(np.uint32))
    with pkg.Context(seed=3) as ctx:
        ne, nc = pkg.eigen_decomposition(P, atol=1e-8, ctx=ctx)
        assert ne == n


@pytest.mark.parametrize("name", ["circ256", "er7xK8", "circ1024", "er5xK20"])
def test_module_compression_driver_agrees_with_dense(pkg, problems, oracle, golden, name):
    """eig_driver 4 = dense on the n x n generic element, 6 = module compression (dense on the
    w x w restriction to a cyclic module, w < 2 dim(P)), the default when dim(P) << n."""
    if name == "er7xK8":
        L, d = problems.kron_with_complete(golden["er7_P"].astype(np.int64), 8, seed=5)
        expect = sorted([2, 2, 2, 2, 3] * 2)
    elif name == "er5xK20":
        L, d = problems.kron_with_complete(golden["er5_P"].astype(np.int64), 20, seed=6)
        expect = sorted([2, 2, 2, 3] * 2)
    elif name == "circ1024":
        L, d = problems.synthetic_jordan_partition(1024, seed=4)
        expect = [1] * d
    else:
        L = golden[f"{name}_P"].astype(np.int64)
        d = int(L.max())
        expect = list(golden[f"{name}_blk"])
    P = pkg.Partition(d, L.astype(np.uint32))
    Po = oracle.Partition(d, L)
    x = np.random.default_rng(8).random(d)
    for drv in (4, 6):
        for seed in (3, 4):
            with pkg.Context(seed=seed, eig_driver=drv) as ctx:
                bd = pkg.blockDiagonalize(P, ctx=ctx)
            assert sorted(bd.blkSizes) == expect, (name, drv)
            full, blk = oracle.spectrum_invariant(Po, bd.blks, x)
            assert len(full) == len(blk), (name, drv)
            assert np.allclose(full, blk, rtol=1e-6, atol=1e-8), (name, drv)
            for q in bd.Q_hat:  # orthonormal columns inside every block
                q = np.asarray(q)
                assert np.abs(q.T @ q - np.eye(q.shape[1])).max() < 1e-7
            ref = oracle.basis_image_fast([np.asarray(q) for q in bd.Q_hat], Po)
            for i in range(0, d, max(1, d // 7)):
                for k in range(len(bd.blkSizes)):
                    assert np.allclose(bd.blks[i][k], ref[i][k], atol=1e-9)


@pytest.mark.parametrize("name", ["closed_scheme", "theta_c32xk128", "theta_er7xk72"])
def test_bench_instances_n4096(pkg, problems, oracle, golden, name):
    """The exact instances bench.py times (configs[3] at N = 4096 / 4104), checked against more
    than themselves: bit-exact partition vs the generator's closure (the theta' instances must get
    there from {diagonal, edges, non-edges} in 5 iterations), pinned block sizes,
    blks == Q_k' 1[P==i] Q_k on sampled classes (host products, atol 1e-9), and the spectrum
    invariant of SURVEY 8c (block eigenvalues of sum_i x_i blks[i][k] = distinct eigenvalues of
    sum_i x_i 1[P==i], rtol 1e-6) with the full N x N spectrum from LAPACK."""
    Cv, A, b, L, d, blocks, iters = problems.bench_instance(name, golden["er7_P"])
    n = L.shape[0]
    with pkg.Context(seed=1000) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, host_setup=True)
        assert P.nparts == d
        assert np.array_equal(P.matrix, L)
        assert P.iterations == iters
        bd = pkg.blockDiagonalize(P, ctx=ctx, retries=3)
    assert sorted(bd.blkSizes) == sorted(blocks)
    Q = [np.asarray(q) for q in bd.Q_hat]
    for i in sorted(set(np.linspace(1, d, 6).astype(int))):
        M = (L == i).astype(np.float64)
        for k, q in enumerate(Q):
            ref = q.T @ (M @ q)
            ref[np.abs(ref) < 1e-12 * n] = 0.0
            assert np.allclose(bd.blks[i - 1][k], ref, atol=1e-9), (name, i, k)
    x = np.random.default_rng(3).random(d)
    full, blk = oracle.spectrum_invariant(oracle.Partition(d, L), bd.blks, x)
    assert len(full) == len(blk), (name, len(full), len(blk))
    assert np.allclose(full, blk, rtol=1e-6, atol=1e-8 * np.abs(full).max())


def _device_resident_block_diagonalize(pkg, ctx, L, d, epsilon, nsample=6, seed=3):
    """blockDiagonalize with labels, images and Q_hat left on the device (the 12 GB of images of configs[2] never
    cross PCIe); checks that need no oracle run: check_block_sizes, orthonormal Q_hat, blks == Q_k' 1[P==i] Q_k on
    sampled classes with host products, and the spectrum invariant of SURVEY 8c with the block side summed on the
    device and the full n x n spectrum from an independent solver (LAPACK, or torch's on the GPU for n >= 4096)."""
    import ctypes as C
    import torch
    Lm = pkg._lib
    n = L.shape[0]
    dev = torch.device("cuda:0")
    tP = torch.from_numpy(np.ascontiguousarray(L.ravel(order="F")).astype(np.int32)).to(dev)
    nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    lib = ctx._lib
    for attempt in range(4):  # the reference's answer to its randomized failures is "try again"
        st = lib.sdpsr_block_diagonalize(ctx._h, n, C.c_void_p(tP.data_ptr()), d, float(epsilon), C.byref(nb), C.byref(ssq),
                                         C.byref(ss), None, Lm.MEM_DEVICE)
        if st not in (2, 3):
            break
    ctx.check(st)
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
    S, S1 = int(ssq.value), int(ss.value)
    assert sum(int(s) * (int(s) + 1) // 2 for s in sizes) == d and sum(int(s) ** 2 for s in sizes) == S
    buf = torch.empty(d * S, dtype=torch.float64, device=dev)
    qh = torch.empty(n * S1, dtype=torch.float64, device=dev)
    ctx.check(lib.sdpsr_block_images(ctx._h, C.c_void_p(buf.data_ptr()), C.c_void_p(qh.data_ptr()), None, Lm.MEM_DEVICE))
    Q = qh.cpu().numpy().reshape(n, S1, order="F")
    cols = np.concatenate([[0], np.cumsum(sizes)])
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64) ** 2)])
    for k in range(len(sizes)):
        q = Q[:, cols[k]:cols[k + 1]]
        assert np.abs(q.T @ q - np.eye(q.shape[1])).max() < 1e-7, k
    blks = buf.view(d, S)
    for i in sorted(set(np.linspace(1, d, nsample).astype(int))):
        R, Cc = np.nonzero(L == i)
        row = blks[i - 1].cpu().numpy()
        for k in range(len(sizes)):
            q = Q[:, cols[k]:cols[k + 1]]
            ref = q[R].T @ q[Cc]  # Q_k' 1[P==i] Q_k = sum over the entries (r, c) of class i of Q_k[r,:]' Q_k[c,:]
            ref[np.abs(ref) < 1e-12 * n] = 0.0
            got = row[offs[k]:offs[k + 1]].reshape(sizes[k], sizes[k], order="F")
            assert np.allclose(got, ref, atol=1e-9), (i, k, np.abs(got - ref).max())
    x = np.random.default_rng(seed).random(d)
    xb = (torch.from_numpy(x).to(dev) @ blks).cpu().numpy()  # sum_i x_i blks[i][:] on the device
    blk_vals = []
    for k in range(len(sizes)):
        B = xb[offs[k]:offs[k + 1]].reshape(sizes[k], sizes[k], order="F")
        blk_vals.append(np.linalg.eigvalsh((B + B.T) / 2))
    blk_vals = np.sort(np.concatenate(blk_vals))
    tA = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), torch.from_numpy(x).to(dev)])[tP.to(torch.int64)].view(n, n)
    if n >= 4096:
        full = torch.linalg.eigvalsh((tA + tA.T) / 2).cpu().numpy()
    else:
        A = tA.cpu().numpy()
        full = np.linalg.eigvalsh((A + A.T) / 2)

    def distinct(v, tol=1e-7):
        v = np.sort(v)
        scale = max(1.0, np.abs(v).max())
        keep = [v[0]]
        for t in v[1:]:
            if abs(t - keep[-1]) > tol * scale:
                keep.append(t)
        return np.array(keep)

    fd, bdv = distinct(full), distinct(blk_vals)
    assert len(fd) == len(bdv), (len(fd), len(bdv))
    assert np.allclose(fd, bdv, rtol=1e-6, atol=1e-8 * np.abs(fd).max())
    return [int(s) for s in sizes]


def test_config2_qap_grid30_block_diagonalize_full_size(pkg, problems):
    """configs[2] at full size THROUGH blockDiagonalize: the N = 900 QAP-type partition (dim 27 828, blocks 36 ... 81,
    12 GB of block images written by basis_image_outer_mfma_kernel) -- block sizes consistent with dim(P), orthonormal
    Q_hat, blks == Q_k' 1[P==i] Q_k on sampled classes, spectrum invariant.  Dense driver (dim(P) >> n)."""
    flow, dist = problems.grid_qap_instance(5, 6, seed=4)
    Cv, A, b = problems.qap_problem(flow, dist)
    setup = pkg.admissible_setup(Cv, A, b)
    with pkg.Context(seed=1) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, setup=setup)
        L = np.asarray(P.matrix).astype(np.int64)
        assert P.nparts > 20000 and L.shape == (900, 900) and np.array_equal(L, L.T)
        sizes = _device_resident_block_diagonalize(pkg, ctx, L, P.nparts, 1e-8, nsample=8)
    assert max(sizes) >= 36 and sum(sizes) <= 900


def test_coupling_classes_on_device_equal_host_classes(pkg, problems):
    """From 256 eigenspaces on, the isomorphism classes (Otsu threshold + union-find, src/eigen_decomposition.jl:83-139,
    205-217) are formed from extrema, histogram counts and pair bits computed on the device; SDPSR_FLAG_COUPLING_ON_HOST
    reads the coupling matrix back as before.  Same seed, same draws: the outcome (eigenspaces, classes, or the
    reference's NumericalInconsistency) must be the same run by run -- on the 900 one-dimensional eigenspaces in 16
    classes of configs[2] and on the single class of a partition without symmetry."""
    flow, dist = problems.grid_qap_instance(5, 6, seed=4)
    Cv, A, b = problems.qap_problem(flow, dist)
    with pkg.Context(seed=1) as ctx:
        P2 = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
    Cv, A, b = problems.theta_prime_problem(problems.gnp_adjacency(320, 0.5, seed=3))
    with pkg.Context(seed=1) as ctx:
        P1 = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
    assert P1.nparts == 320 * 321 // 2
    for P, atol in ((P2, 1e-8), (P1, 1.5e-8)):
        outcomes = []
        for flags in (0, pkg._lib.FLAG_COUPLING_ON_HOST):
            runs = []
            with pkg.Context(seed=5, flags=flags) as ctx:
                for _ in range(6):
                    try:
                        runs.append(pkg.eigen_decomposition(P, atol=atol, ctx=ctx))
                    except pkg.NumericalInconsistency:
                        runs.append("inconsistent")
            outcomes.append(runs)
        assert outcomes[0] == outcomes[1], outcomes
        assert any(r != "inconsistent" and r[0] >= 256 for r in outcomes[0]), outcomes


def test_config4_n8192_block_diagonalize_full_size(pkg, problems):
    """configs[4] through blockDiagonalize at N = 8192: all blocks of size 1 (commutative scheme), blks against host
    products on sampled classes, spectrum invariant with the full 8192 x 8192 spectrum from torch's solver."""
    n = 8192
    L, d = problems.synthetic_jordan_partition(n, seed=8)
    with pkg.Context(seed=78) as ctx:
        sizes = _device_resident_block_diagonalize(pkg, ctx, L, d, pkg.api.RTOL_DEFAULT, nsample=6)
    assert sizes == [1] * d


def test_generic_partition_failure_rate_matches_the_oracle(pkg, problems):
    """configs[1]'s kind of partition (no symmetry: every unordered pair its own class) makes the randomized
    eigen_decomposition fail with NumericalInconsistency in a two-digit percentage of the draws -- the reference's own
    behaviour ("try again", src/eigen_decomposition.jl:264-270).  CPU oracle, reference-literal, 300 runs each
    (tools/bd_failure_compare.py generic-oracle; profiles/r04_bd_failure_rates_generic.txt): 30 / 300 at n = 200,
    35 / 300 at n = 320, 30 / 300 at n = 512.  The device's dense driver with the reference's single coupling element
    (SDPSR_FLAG_SINGLE_COUPLING_ELEMENT) must fail at the SAME rate (binomial band of 4 sigma around 35 / 300), and the
    default driver (extra coupling elements on demand) must not fail more often than that."""
    n, runs, p_oracle = 320, 300, 35.0 / 300.0
    iu = np.triu_indices(n)
    L = np.zeros((n, n), dtype=np.int64)
    L[iu] = np.arange(1, len(iu[0]) + 1)
    L = np.maximum(L, L.T)
    L, d = problems.canonical_labels(L)
    P = pkg.Partition(d, L.astype(np.uint32))
    sigma = (runs * p_oracle * (1 - p_oracle)) ** 0.5
    rates = {}
    for flags in (pkg._lib.FLAG_SINGLE_COUPLING_ELEMENT, 0):
        fails = 0
        with pkg.Context(seed=77, flags=flags) as ctx:
            for _ in range(runs):
                try:
                    pkg.eigen_decomposition(P, ctx=ctx)
                except pkg.NumericalInconsistency:
                    fails += 1
        rates[flags] = fails
    lit = rates[pkg._lib.FLAG_SINGLE_COUPLING_ELEMENT]
    assert abs(lit - runs * p_oracle) <= 4 * sigma, (rates, runs * p_oracle, sigma)
    assert rates[0] <= runs * p_oracle + 4 * sigma, rates


# ------------------------------------------------ bench.py --gpus N: the launcher and the agreement step on device tensors
def _run_bench(extra_env, *flags):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    # one GPU on the box: both ranks on cuda:0, gloo instead of RCCL (which refuses two ranks on one device)
    env.update({"SDPSR_BENCH_SAME_DEVICE": "1", "SDPSR_BENCH_BACKEND": "gloo"})
    env.update(extra_env)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "2",
                          "--skip-roofline", "--n", "1024", *flags], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]  # rank 0 prints ONE JSON line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_gpus_2_starts_two_ranks():
    """`python bench.py --gpus 2` (the shape of the driver's command, no launcher, no WORLD_SIZE) must start two ranks
    itself and report n_gpus = 2 -- not one rank with n_gpus = 1."""
    js = _run_bench({})
    assert js["n_gpus"] == 2 and js["value"] > 0 and js["scaling"] == "weak"
    assert js["config"]["restarts_per_step"] == 2
    assert js["partition_meets"] == {"warmup": 0, "timed": 0, "note": js["partition_meets"]["note"]}


@pytest.mark.gpu
def test_bench_forced_disagreement_reaches_the_hash_meet():
    """Rank 1 reports a coarser partition in the warm-up steps: checksums differ, MIN/MAX all-reduce on the device
    label tensors, SUM all-reduce of the hashed labels, canonical relabel on the device (sdpsr_partition_from_u64);
    bench.py asserts after every warm-up step that the agreed partition is the generator's closure again."""
    js = _run_bench({"SDPSR_BENCH_FORCE_DISAGREE": "1"}, "--workload", "theta_c32xk128")
    assert js["n_gpus"] == 2 and js["value"] > 0
    assert js["partition_meets"]["warmup"] == 2 and js["partition_meets"]["timed"] == 0


@pytest.mark.gpu
def test_bench_batched_restarts_two_ranks_forced_disagreement():
    """`bench.py --gpus 2 --restarts-per-gpu 2` with restart 1 of rank 1 reporting a coarser partition in
    the warm-up steps.  The batched multi-rank step runs parallel.agree_partitions over all four restarts (the R x world
    checksum table; on a difference the hash-meet with the device relabel), never asserts on a randomized event, and the
    agreed partition of every restart must be the generator's closure again (bench.py checks it in the warm-up steps)."""
    js = _run_bench({"SDPSR_BENCH_FORCE_DISAGREE": "1"}, "--workload", "theta_c32xk128", "--restarts-per-gpu", "2")
    assert js["n_gpus"] == 2 and js["value"] > 0 and js["config"]["restarts_per_step"] == 4
    assert js["partition_meets"]["warmup"] == 2 and js["partition_meets"]["timed"] == 0
    js = _run_bench({"SDPSR_BENCH_FORCE_BD_FAIL": "0"}, "--restarts-per-gpu", "2")
    w = js["block_diagonalization_winner"]
    assert w["adopted_warmup"] == 2 and w["adopted_timed"] == 0 and w["all_failed"] == 0


@pytest.mark.gpu
def test_bench_forced_block_diagonalize_failure_adopts_the_winner():
    """rank 0 reports DimensionMismatch for its blockDiagonalize in the warm-up steps; the one-integer
    MIN all-reduce must pick rank 1, whose block sizes are broadcast and adopted (bench.py asserts them against the
    instance's pinned sizes on both ranks); the timed steps, where nobody fails, have rank 0 as the winner."""
    js = _run_bench({"SDPSR_BENCH_FORCE_BD_FAIL": "0"}, "--workload", "theta_c32xk128")
    assert js["n_gpus"] == 2 and js["value"] > 0
    w = js["block_diagonalization_winner"]
    assert w["adopted_warmup"] == 2 and w["adopted_timed"] == 0 and w["all_failed"] == 0


@pytest.mark.gpu
def test_bench_restarts_per_gpu_batches_in_one_call():
    """--restarts-per-gpu 2: every step is ONE sdpsr_jordan_reduce_batch call of two restarts (fibers of one host thread);
    bench.py checks every restart's partition against the generator's closure in the warm-up steps."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "2", "--skip-roofline", "--n", "1024",
                          "--restarts-per-gpu", "2"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    js = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert js["n_gpus"] == 1 and js["config"]["restarts_per_step"] == 2 and js["config"]["restarts_per_gpu"] == 2 and js["value"] > 0


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_instance_and_repeat(problems, tmp_path):
    """A plain `bench.py --dump-outputs DIR` times exactly --steps steps, measures nothing beyond the headline, and writes
    what its last timed step delivered: the generator's closure (labels at the seeded positions, class sizes), blocks of
    size 1, dim x sum_sq block images.  A second run with the same arguments writes the same partition outputs."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = 1024
    Ls, d = problems.synthetic_jordan_partition(n, seed=1)
    runs = []
    for k in range(2):
        out_dir = tmp_path / f"run{k}"
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "2", "--n", str(n),
                              "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        js = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
        assert js["steps"] == 3 and js["ms_per_step"] > 0 and js["value"] > 0
        assert js["variants"] == {} and js["kernels"] == {} and js["roofline"] is None and js["cpu_baseline"] is None
        assert list(js["workloads"]) == ["closed_scheme"] and js["phase_ms_per_step"] is None
        files = {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
        assert set(files) == {"labels_sample.npy", "class_sizes.npy", "block_sizes.npy", "block_images.npy", "summary.npy"}
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 * 1000 ** 2
        pick = np.sort(np.random.default_rng(1).choice(n * n, min(n * n, 1 << 20), replace=False))
        assert np.array_equal(files["labels_sample.npy"], Ls.ravel(order="F")[pick].astype(np.float32))
        assert np.array_equal(files["class_sizes.npy"], np.bincount(Ls.ravel(), minlength=d + 1).astype(np.float64))
        assert np.array_equal(files["block_sizes.npy"], np.ones(d))
        dim, nblocks, sum_sq, iters = files["summary.npy"]
        assert (dim, nblocks, sum_sq, iters) == (d, d, d, 1)
        assert files["block_images.npy"].shape == (d * d,) and np.isfinite(files["block_images.npy"]).all()
        runs.append(files)
    for f in ("labels_sample.npy", "class_sizes.npy", "block_sizes.npy", "summary.npy"):
        assert np.array_equal(runs[0][f], runs[1][f]), f


@pytest.mark.gpu
def test_rccl_backend_runs_the_agreement_collectives_single_rank():
    """gpurun exposes one GPU, so RCCL cannot be run with two ranks here (it refuses two ranks on one device; the two-rank
    flow is tested over gloo above).  What CAN be shown on this box is that the `nccl` (= RCCL) branch of the agreement
    step executes with the device tensors and dtypes it uses: process group with device_id, the 16-byte all_gather of the
    device checksum, the MIN / MAX all-reduce of int32 labels, the SUM all-reduce of int64 keys and the device relabel --
    here in a group of one rank, where every collective must return its input."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys
sys.path.insert(0, os.getcwd())
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29571", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
import numpy as np, torch, torch.distributed as dist
from __graft_entry__ import load_package
pkg = load_package()
dev = torch.device("cuda:0")
dist.init_process_group("nccl", device_id=dev)
assert dist.get_backend() == "nccl"
L, d = pkg.problems.synthetic_jordan_partition(512, seed=3)
tP = torch.from_numpy(np.asfortranarray(L).ravel(order="F").astype(np.int32)).to(dev)
with pkg.Context(seed=1) as ctx:
    words = pkg.partition_checksum(tP, ctx=ctx)
    assert pkg.parallel.checksums_agree(words, device=dev)          # all_gather of two int64 words on the device
    agreed, lab = pkg.parallel.agree_partition(tP, lambda sig: pkg.relabel_keys(sig, ctx=ctx), checksum=lambda t: pkg.partition_checksum(t, ctx=ctx))
    assert agreed and bool((lab == tP).all())
    lo, hi = tP.clone(), tP.clone()                                   # the collectives of a disagreement, issued directly
    dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    assert bool((lo == tP).all()) and bool((hi == tP).all())
    sig = (tP.to(torch.int64) + 1) * 0x1E3779B97F4A7C15
    ref = sig.clone()
    dist.all_reduce(sig, op=dist.ReduceOp.SUM)
    assert bool((sig == ref).all())
    new, nparts = pkg.relabel_keys(sig - 0x1E3779B97F4A7C15, ctx=ctx)  # zero stays zero, first-occurrence order: the same partition
    assert int(nparts) == d and bool((new == tP).all())
torch.cuda.synchronize()
dist.destroy_process_group()
print("RCCL_ONE_RANK_OK")
"""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RCCL_ONE_RANK_OK" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_four_restarts_in_flight_on_one_gpu(pkg, problems, golden):
    """Independent restarts on one GPU, one ctx per host thread (the bench's N_restarts_in_flight variants):
    four threads run the whole path concurrently -- two on the commutative scheme at N = 1024 (module compression), one on
    the non-commutative ER(7) algebra, one on a partition without symmetry at n = 512 (dense eigensolver: row
    tridiagonalisation, side-stream back-transformation, tridiagonal divide and conquer, device-side classes) -- and every
    run must end on its known answer: nothing is shared between the ctxs."""
    import threading
    Ls, ds = problems.synthetic_jordan_partition(1024, seed=4)
    Cs, As, bs = problems.partition_as_sdp(Ls, seed=1)
    Le = golden["er7_P"].astype(np.int64)
    de = int(Le.max())
    Ce, Ae, be = problems.partition_as_sdp(Le, seed=2)
    Cg, Ag, bg = problems.theta_prime_problem(problems.gnp_adjacency(512, 0.5, seed=9))
    errs = []

    def scheme(seed):
        try:
            with pkg.Context(seed=seed) as ctx:
                for _ in range(4):
                    P = pkg.admissible_subspace(Cs, As, bs, ctx=ctx)
                    assert P.nparts == ds and np.array_equal(P.matrix, Ls)
                    bd = pkg.blockDiagonalize(P, ctx=ctx, retries=3)
                    assert sorted(bd.blkSizes) == [1] * ds
        except Exception as exc:  # noqa: BLE001
            errs.append(("scheme", seed, repr(exc)))

    def er7(seed):
        try:
            with pkg.Context(seed=seed) as ctx:
                for _ in range(6):
                    P = pkg.admissible_subspace(Ce, Ae, be, ctx=ctx)
                    assert P.nparts == de and np.array_equal(P.matrix, Le)
                    bd = pkg.blockDiagonalize(P, ctx=ctx, retries=3)
                    assert sorted(bd.blkSizes) == sorted(int(x) for x in golden["er7_blk"])
        except Exception as exc:  # noqa: BLE001
            errs.append(("er7", seed, repr(exc)))

    def generic(seed):
        try:
            with pkg.Context(seed=seed) as ctx:
                for _ in range(3):
                    P = pkg.admissible_subspace(Cg, Ag, bg, ctx=ctx)
                    assert P.nparts == 512 * 513 // 2
                    Qh = None
                    for attempt in range(8):  # one class of 512 coupled eigenspaces: the reference's own consistency check
                        try:                   # rejects a fair share of the draws ("simply try again")
                            Qh = pkg.diagonalize(P, ctx=ctx)
                            break
                        except (pkg.NumericalInconsistency, pkg.DimensionMismatch):
                            continue
                    assert Qh is not None
                    assert [q.shape for q in Qh] == [(512, 512)]
                    assert np.abs(Qh[0].T @ Qh[0] - np.eye(512)).max() < 1e-9
        except Exception as exc:  # noqa: BLE001
            errs.append(("generic", seed, repr(exc)))

    ths = [threading.Thread(target=scheme, args=(11,)), threading.Thread(target=scheme, args=(12,)),
           threading.Thread(target=er7, args=(13,)), threading.Thread(target=generic, args=(14,))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
