"""The element-wise and reduction kernels behind the AbstractPartition primitives of include/sdpsr.h, the full-matrix channel gathers of the
square step, the projection's dot products on labels with their symmetry probe, and the vector kernels of the device setup -- each past
the cap of grid_for() (csrc/kernel_util.h: 2048 workgroups of 256 threads), where a kernel relies on its grid-stride loop, and at the
small lengths where one wave or one workgroup is ragged.  References: tests/primitives_ref.py (ports held against csrc/sdpsr_hash.h by
tests/test_primitives_ref_cpu.py), the oracle, exact integer arithmetic.

Everything is bit for bit but two bounds, neither fitted to a kernel's output:
  * the dot products on class draws (x = a 53-bit uniform per class): |got - exact| <= 2 len 2^-53 sum_e |U[k, e] x_e|, the bound
    gamma_len of a float64 dot product of len terms summed in any order, with the factor 2 for 1 / (1 - len u).  The exact value comes
    from integers (2^53 x and the entries of U are integers);
  * the device setup against the NumPy setup: the bounds of csr_setup_helpers._compare_with_host_setup as they stand.
Every case past the cap asserts that its work items exceed the threads of its launch."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import primitives_ref as P
from csr_setup_helpers import _compare_with_host_setup
from module_kernels_ref import hashed_labels
from refine_source_ref import canonical

pytestmark = pytest.mark.gpu

ATOL = 2.0 ** -26
G = P.GRID_THREADS
OK, LABEL_OVERFLOW, BAD_ARGUMENT = 0, 4, 5
HOST, DEVICE = 0, 1


def _vp(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else C.c_void_p(a.ctypes.data)


def _past_cap(length, work_items=None):
    """A length of the lists below runs past the launch exactly when it is one of the long ones -- and those do."""
    work = length if work_items is None else work_items
    assert (work > G) == (length in (P.LEN_W, P.LEN_P)), (length, work)
    return work > G


def _labels(length, d, seed, canonical_numbering=False):
    """Labels 0 .. d (uint32), every one of them present where there is room, label 0 in a run in the middle as well."""
    rng = np.random.default_rng(seed)
    l = rng.integers(0, d + 1, size=length)
    if length > 2 * d:
        l[rng.permutation(length)[:d]] = np.arange(1, d + 1)
    l[length // 2:length // 2 + max(1, length // 16)] = 0
    if canonical_numbering:
        l = canonical([l.astype(np.uint64)], l == 0)[0]
    return np.ascontiguousarray(l, dtype=np.uint32)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def prof(pkg):
    return pkg._lib.load_prof_library()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch


LENS_W = P.SMALL_LENS + (P.LEN_W,)
LENS_P = P.SMALL_LENS + (P.LEN_P,)


# ------------------------------------------------------------------ fill / randomize
@pytest.mark.parametrize("length", LENS_W)
def test_fill(lib, gpu_ctx, length):
    d = 1000
    past = _past_cap(length)
    rng = np.random.default_rng(length)
    lab = _labels(length, d, seed=length)
    values = rng.standard_normal(d)
    values[:3] = [-0.0, 5e-324, -1e300]
    out = np.full(length, np.nan)
    assert lib.sdpsr_fill(gpu_ctx._h, length, _vp(lab), _vp(values), d, _vp(out), HOST) == OK
    want = np.concatenate([[0.0], values])[lab]
    assert np.array_equal(out.view(np.uint64), want.view(np.uint64))
    # a label beyond d: where only a second trip of the loop reads it, and at the last entry
    for pos in ([G + 5, length - 1] if past else [length - 1]):
        bad = lab.copy()
        bad[pos] = d + 1
        assert lib.sdpsr_fill(gpu_ctx._h, length, _vp(bad), _vp(values), d, _vp(out), HOST) == BAD_ARGUMENT, pos
    # d = 0: no values at all, all-zero labels
    out[:] = np.nan
    assert lib.sdpsr_fill(gpu_ctx._h, length, _vp(np.zeros(length, dtype=np.uint32)), None, 0, _vp(out), HOST) == OK
    assert np.array_equal(out.view(np.uint64), np.zeros(length, dtype=np.uint64))


@pytest.mark.parametrize("length", LENS_W)
def test_randomize(pkg, gpu_ctx, length):
    d = 1000 if length > 2000 else min(length, 40)
    _past_cap(length)
    lab = _labels(length, d, seed=7 + length, canonical_numbering=True)
    part = pkg.Partition(int(lab.max()), lab)
    R = pkg.randomize(part, ctx=gpu_ctx)
    assert R.shape == (length,)
    assert np.array_equal(R[lab == 0].view(np.uint64), np.zeros(int((lab == 0).sum()), dtype=np.uint64))  # +0.0 exactly
    assert ((R >= 0) & (R < 1)).all()
    first = np.full(part.nparts + 1, -1.0)
    first[lab[::-1]] = R[::-1]  # the value at the first entry of every class ...
    assert np.array_equal(R, first[lab])  # ... is the value of every entry of the class
    assert len(np.unique(first[1:])) == part.nparts and (first[1:] > 0).all()  # distinct between classes, none the zero class's
    assert pkg.Partition.from_matrix(R, ctx=gpu_ctx) == part


# ------------------------------------------------------------------ clamp_round
@pytest.fixture(scope="module", params=["nearest", "trunc"])
def mode_ctx(pkg, request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with pkg.Context(device=0, seed=5, round_mode=request.param) as ctx:
        yield request.param, ctx


@pytest.mark.parametrize("length", LENS_W)
def test_clamp_round(lib, mode_ctx, length):
    mode, ctx = mode_ctx
    past = _past_cap(length)
    a = P.clamp_values(length, ATOL, seed=length)
    want = P.clamp_round(a, ATOL, mode)
    got = a.copy()
    assert lib.sdpsr_clamp_round(ctx._h, length, _vp(got), ATOL, HOST) == OK
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (mode, len(bad), bad[:5], a[bad[:5]], got[bad[:5]], want[bad[:5]])
    if past:  # the planted ties were read on a later trip, and the two rules part on them
        t = P.tie_values()
        assert np.array_equal(a[G + 5:G + 5 + len(t)], t) and np.array_equal(a[2 * G + 5:2 * G + 5 + len(t)], t)
        assert a[-1] == -1e-300 and a[-16] == 0.0625  # (the fourth trip reads the end of the planted block)
        other = P.clamp_round(t, ATOL, "trunc" if mode == "nearest" else "nearest")
        assert (got[G + 5:G + 5 + len(t)] != other).any()


def test_clamp_round_keeps_non_finite_values_non_finite(lib, mode_ctx):
    """NaN and +-inf come back non-finite of the same kind, their neighbours rounded as ever.  This pins what the kernel does: the reference's
    unsafe_round throws on them."""
    mode, ctx = mode_ctx
    for length in (257, P.LEN_W):
        a = P.clamp_values(length, ATOL, seed=1)
        spots = [0, 63, 64, length - 1] + ([G + 5, 3 * G + 70] if length > G else [])
        kinds = [np.nan, np.inf, -np.inf]
        for k, pos in enumerate(spots):
            a[pos] = kinds[k % 3]
        got = a.copy()
        assert lib.sdpsr_clamp_round(ctx._h, length, _vp(got), ATOL, HOST) == OK
        for k, pos in enumerate(spots):
            v = kinds[k % 3]
            assert np.isnan(got[pos]) if np.isnan(v) else got[pos] == v, (mode, pos, got[pos])
        rest = np.ones(length, dtype=bool)
        rest[spots] = False
        assert np.array_equal(got[rest].view(np.uint64), P.clamp_round(a[rest], ATOL, mode).view(np.uint64))


# ------------------------------------------------------------------ project_out
def _int_basis(rng, r, length):
    return np.ascontiguousarray(rng.integers(-8, 9, size=max(r, 1) * length).astype(np.float64))


def _project_out_exact(x, U, r, length):
    """x - sum_k U_k <U_k, x> in int64.  |<U_k, x>| <= 64 len < 2^28, |U coef| < 2^31, three of them: no overflow, and every partial sum of
    every summation order is an integer below 2^53 -- exact in float64 with or without fma."""
    xi = x.astype(np.int64)
    y = xi.copy()
    for k in range(r):
        uk = U[k * length:(k + 1) * length].astype(np.int64)
        y -= uk * int((uk * xi).sum())
    return y


@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("length", LENS_P)
def test_project_out_is_exact_on_integers(lib, gpu_ctx, length, r):
    _past_cap(length)
    assert 64 * length < 2 ** 53
    rng = np.random.default_rng(1000 * r + length % 1000)
    U = _int_basis(rng, r, length)
    x = rng.integers(-8, 9, size=length).astype(np.float64)
    y = x.copy()
    assert lib.sdpsr_project_out(gpu_ctx._h, length, _vp(y), _vp(U) if r else None, r, HOST) == OK
    want = _project_out_exact(x, U, r, length)
    assert np.array_equal(y, want.astype(np.float64)) and np.array_equal(y.astype(np.int64), want)


def test_project_out_needles(lib, gpu_ctx):
    """x = the unit vector at p, U[k, p] = k + 1: the dot products are coef[k] = k + 1 exactly when entry p is read once and only once,
    and y[e] = x[e] - sum_k (k + 1) U[k, e] shows them.  p in the unrolled body's four streams, in the first and in the second trip of its
    tail, and at both ends."""
    length, r = P.LEN_P, 3
    assert _past_cap(length) and length > 5 * G
    rng = np.random.default_rng(11)
    U = _int_basis(rng, r, length)
    S = sum((k + 1) * U[k * length:(k + 1) * length].astype(np.int64) for k in range(r))
    for p in (0, 255, 256, G - 1, G, 2 * G + 5, 3 * G + 5, 4 * G + 5, 5 * G + 5, length - 1):
        keep = [U[k * length + p] for k in range(r)]
        for k in range(r):
            U[k * length + p] = k + 1
        x = np.zeros(length)
        x[p] = 1.0
        assert lib.sdpsr_project_out(gpu_ctx._h, length, _vp(x), _vp(U), r, HOST) == OK
        want = -S
        want[p] = 1 - sum((k + 1) ** 2 for k in range(r))
        bad = np.flatnonzero(x != want)
        assert len(bad) == 0, (p, len(bad), bad[:3], x[bad[:3]], want[bad[:3]])
        for k in range(r):
            U[k * length + p] = keep[k]


# ------------------------------------------------------------------ checksum, refine!, the constructors
def test_partition_checksum_past_the_cap(pkg, gpu_ctx):
    length = P.LEN_W
    assert _past_cap(length)
    lab = _labels(length, 50, seed=3)
    want = P.checksum(lab)
    assert pkg.partition_checksum(lab, ctx=gpu_ctx) == want
    for pos in (length - 1, G + 5):
        other = lab.copy()
        other[pos] += 1
        got = pkg.partition_checksum(other, ctx=gpu_ctx)
        assert got == P.checksum(other) and got[0] != want[0] and got[1] != want[1], pos


@pytest.mark.parametrize("length", P.SMALL_LENS)
def test_partition_checksum_small_lengths(pkg, gpu_ctx, length):
    assert not _past_cap(length)
    lab = _labels(length, 50, seed=4)
    assert pkg.partition_checksum(lab, ctx=gpu_ctx) == P.checksum(lab)


def test_refine_and_u64_constructor_past_the_cap(pkg, oracle, gpu_ctx):
    length = P.LEN_W
    assert _past_cap(length)
    a, b = _labels(length, 40, seed=5, canonical_numbering=True), _labels(length, 30, seed=6, canonical_numbering=True)
    ref = oracle.refine(oracle.Partition(int(a.max()), a.astype(np.int64)), oracle.Partition(int(b.max()), b.astype(np.int64)))
    got = pkg.refine(pkg.Partition(int(a.max()), a.copy()), pkg.Partition(int(b.max()), b), ctx=gpu_ctx)
    assert got.nparts == ref.nparts and np.array_equal(got.matrix, ref.matrix)
    base = _labels(length, 70, seed=8).astype(np.int64)
    keys = base * (2 ** 40 + 12345)
    keys[-1] = 71 * (2 ** 40 + 12345)  # a class of the last entry alone
    base[-1] = 71
    Pk = pkg.Partition.from_matrix(keys, ctx=gpu_ctx)
    Rk = oracle.partition_from_labels(base)
    assert Pk.nparts == Rk.nparts == 71 and np.array_equal(Pk.matrix, Rk.matrix)


def test_label_overflow_of_the_pair_code_past_the_cap(pkg, lib, oracle):
    """label_bits = 16: refine! decides on the largest pair code l1 + l2 (dim(P1) + 1).  d1 = 200 and l2 <= 300: at most 60 500, no overflow;
    ONE l2 = 327 (327 * 201 = 65 727) where only a second trip of the maximum's loop reads it, or at the last entry: LABEL_OVERFLOW."""
    length, d1 = P.LEN_W, 200
    assert _past_cap(length)
    p1 = _labels(length, d1, seed=9, canonical_numbering=True)
    p2 = _labels(length, 300, seed=10, canonical_numbering=True)
    assert int(p1.max()) == d1 and int(p2.max()) == 300
    assert int((p1.astype(np.int64) + p2.astype(np.int64) * (d1 + 1)).max()) <= 60500
    with pkg.Context(seed=1, label_bits=16) as ctx:
        a, dd = p1.copy(), C.c_int64(d1)
        assert lib.sdpsr_refine(ctx._h, length, _vp(a), C.byref(dd), _vp(p2), 300, HOST) == OK
        ref = oracle.refine(oracle.Partition(d1, p1.astype(np.int64)), oracle.Partition(300, p2.astype(np.int64)), 16)
        assert dd.value == ref.nparts and np.array_equal(a, ref.matrix)
        for pos in (G + 5, length - 1):
            big = p2.copy()
            big[pos] = 327
            a, dd = p1.copy(), C.c_int64(d1)
            assert lib.sdpsr_refine(ctx._h, length, _vp(a), C.byref(dd), _vp(big), 327, HOST) == LABEL_OVERFLOW, pos
            with pytest.raises(oracle.LabelOverflow):
                oracle.refine(oracle.Partition(d1, p1.astype(np.int64)), oracle.Partition(327, big.astype(np.int64)), 16)
            assert np.array_equal(a, p1) and dd.value == d1  # (P1 untouched)


# ------------------------------------------------------------------ the same primitives on device memory
def test_primitives_on_device_memory(pkg, lib, oracle, gpu_ctx, torch_dev):
    """MEM_DEVICE: no staging copies, clamp_round and project_out in place, refine! in place in P1."""
    torch = torch_dev
    length, d = 5003, 300
    rng = np.random.default_rng(21)
    lab = _labels(length, d, seed=22, canonical_numbering=True)
    d = int(lab.max())
    dl = torch.from_numpy(lab.view(np.int32)).cuda()
    # fill
    values = rng.standard_normal(d)
    dv, dm = torch.from_numpy(values).cuda(), torch.full((length,), float("nan"), dtype=torch.float64, device="cuda")
    gpu_ctx.wait_for(dm)
    assert lib.sdpsr_fill(gpu_ctx._h, length, _vp(dl), _vp(dv), d, _vp(dm), DEVICE) == OK
    assert np.array_equal(dm.cpu().numpy().view(np.uint64), np.concatenate([[0.0], values])[lab].view(np.uint64))
    # randomize
    dm.fill_(float("nan"))
    gpu_ctx.wait_for(dm)
    assert lib.sdpsr_randomize(gpu_ctx._h, length, _vp(dl), _vp(dm), DEVICE) == OK
    R = dm.cpu().numpy()
    assert ((R >= 0) & (R < 1)).all() and not R[lab == 0].any()
    assert pkg.Partition.from_matrix(R, ctx=gpu_ctx) == pkg.Partition(d, lab)
    # clamp_round, in place
    a = P.clamp_values(length, ATOL, seed=23)
    da = torch.from_numpy(a).cuda()
    gpu_ctx.wait_for(da)
    assert lib.sdpsr_clamp_round(gpu_ctx._h, length, _vp(da), ATOL, DEVICE) == OK
    assert np.array_equal(da.cpu().numpy().view(np.uint64), P.clamp_round(a, ATOL, "nearest").view(np.uint64))
    # project_out, in place
    r = 3
    U = _int_basis(rng, r, length)
    x = rng.integers(-8, 9, size=length).astype(np.float64)
    dx, du = torch.from_numpy(x).cuda(), torch.from_numpy(U).cuda()
    gpu_ctx.wait_for(dx, du)
    assert lib.sdpsr_project_out(gpu_ctx._h, length, _vp(dx), _vp(du), r, DEVICE) == OK
    assert np.array_equal(dx.cpu().numpy().astype(np.int64), _project_out_exact(x, U, r, length))
    assert np.array_equal(du.cpu().numpy(), U)
    # checksum
    assert pkg.partition_checksum(dl, ctx=gpu_ctx) == P.checksum(lab)
    # refine!, in place in P1
    lab2 = _labels(length, 17, seed=24, canonical_numbering=True)
    d1, d2 = torch.from_numpy(lab.view(np.int32).copy()).cuda(), torch.from_numpy(lab2.view(np.int32)).cuda()
    dd = C.c_int64(d)
    gpu_ctx.wait_for(d1, d2)
    assert lib.sdpsr_refine(gpu_ctx._h, length, _vp(d1), C.byref(dd), _vp(d2), int(lab2.max()), DEVICE) == OK
    ref = oracle.refine(oracle.Partition(d, lab.astype(np.int64)), oracle.Partition(int(lab2.max()), lab2.astype(np.int64)))
    assert dd.value == ref.nparts and np.array_equal(d1.cpu().numpy().view(np.uint32), ref.matrix)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), lab2)
    # the u64 constructor
    keys = torch.from_numpy(lab.astype(np.int64) * (2 ** 40 + 12345)).cuda()
    got, nk = pkg.relabel_keys(keys, ctx=gpu_ctx)
    assert nk == d and np.array_equal(got.cpu().numpy().view(np.uint32), lab)


# ------------------------------------------------------------------ the full-matrix channel gathers
KIND_I8, KIND_F32, KIND_F64 = 0, 1, 2
GUARD = 64
KEY = 0x5DEECE66D1234567
_DT = {KIND_I8: np.int8, KIND_F32: np.float32, KIND_F64: np.float64}
_SENTINEL = {KIND_I8: 0x5A, KIND_F32: -12345.0, KIND_F64: -12345.0}
_PER_THREAD = {KIND_I8: 16, KIND_F32: 4, KIND_F64: 2}


def _gather_labels(n, dmax, seed):
    """Non-symmetric n x n labels (flat, column-major): 0 .. dmax where the gather is told a bound, 0 .. 5000 where it is not."""
    d = dmax if dmax > 0 else 5000
    L = hashed_labels(n, d, salt=seed)
    if n > 1:
        M = L.reshape(n, n, order="F")
        assert not np.array_equal(M, M.T)
    return L


def _gather(prof, ctx, kind, n, T, vmax, dmax, L, key=KEY):
    ld = -(-n // 128) * 128
    X = np.full(T * ld * ld + GUARD, _SENTINEL[kind], dtype=_DT[kind])
    out = (C.c_uint64 * 2)()
    st = prof.sdpsr_profile_gather_full(ctx._h, kind, n, T, vmax, dmax, C.c_uint64(key), _vp(L), _vp(X), GUARD, out)
    assert st == OK, ctx._lib.sdpsr_last_error(ctx._h)
    assert out[0] == (ld // _PER_THREAD[kind]) * ld and out[1] == min(-(-out[0] // 256), 2048) * 256
    assert (X[T * ld * ld:] == _SENTINEL[kind]).all(), "the guard behind the channels was written"
    return X[:T * ld * ld].reshape(T, ld, ld), int(out[0]), int(out[1])  # [t, column, row]


def _gather_expected(kind, n, T, vmax, L, key=KEY):
    ld = -(-n // 128) * 128
    lab = L.reshape(n, n)  # [column, row]: flat column-major
    bits = np.where(lab == 0, np.uint64(0), P.class_bits(key, lab))
    E = np.zeros((T, ld, ld), dtype=_DT[kind])
    for t in range(T):
        if kind == KIND_I8:
            E[t, :n, :n] = P.class_i8(bits, t)
        elif kind == KIND_F32:
            E[t, :n, :n] = np.where(lab == 0, 0, P.class_small(bits, t, vmax)).astype(np.float32)
        else:
            E[t, :n, :n] = P.class_uniform(key, lab)
    return E


def _same_bits(X, E):
    return np.array_equal(X.view(np.uint8), E.view(np.uint8))


@pytest.mark.parametrize("n", [1, 3, 16, 20, 28, 130])
def test_gather_i8_every_channel_count_and_table(prof, gpu_ctx, n):
    """Byte t of class_bits(key, l); zeros for label 0 and for every padding row and column.  n & 3 != 0: scalar label loads; n = 16: the
    16-byte loads; n = 20 and 28: a 16-byte column whose last chunk is ragged (4 and 12 rows of it: the nearest miss of "i0 + 16 <= n");
    n = 130: two tile columns with padding.  dmax 3 / 2048: the LDS
    table of class bits and its last admissible size; 2049 and 0: hashed per entry."""
    for dmax in (0, 3, 2048, 2049):
        L = _gather_labels(n, dmax, seed=n + dmax)
        for T in range(1, 9):
            X, work, threads = _gather(prof, gpu_ctx, KIND_I8, n, T, 0, dmax, L)
            assert work <= threads
            E = _gather_expected(KIND_I8, n, T, 0, L)
            assert _same_bits(X, E), (n, dmax, T, np.argwhere(X != E)[:4])


@pytest.mark.parametrize("n", [1, 3, 16, 20, 28, 130])
def test_gather_f32_and_f64(prof, gpu_ctx, n):
    """fp32: class_small of byte t, EVERY t (the eighth channel spans [-vmax, vmax] like the others), as a float; fp64: class_uniform."""
    L = _gather_labels(n, 0, seed=40 + n)
    for T in (1, 2, 4, 8):
        for vmax in (1, 64, 127):
            X, work, threads = _gather(prof, gpu_ctx, KIND_F32, n, T, vmax, 0, L)
            assert work <= threads
            E = _gather_expected(KIND_F32, n, T, vmax, L)
            for t in range(T):
                assert _same_bits(X[t], E[t]), (n, T, vmax, t, np.argwhere(X[t] != E[t])[:4])
    X, _, _ = _gather(prof, gpu_ctx, KIND_F64, n, 1, 0, 0, L)
    assert _same_bits(X, _gather_expected(KIND_F64, n, 1, 0, L))


@pytest.mark.parametrize("kind,n,T,vmax,dmax", [(KIND_I8, 2900, 8, 0, 2049), (KIND_I8, 2900, 3, 0, 2048), (KIND_F32, 1500, 8, 64, 0),
                                                (KIND_F64, 1100, 1, 0, 0)])
def test_gathers_past_the_cap(prof, gpu_ctx, kind, n, T, vmax, dmax):
    L = _gather_labels(n, dmax, seed=n)
    X, work, threads = _gather(prof, gpu_ctx, kind, n, T, vmax, dmax, L)
    assert threads == G and work > threads  # the shape really exceeded the launch
    E = _gather_expected(kind, n, T, vmax, L)
    for t in range(T):
        assert _same_bits(X[t], E[t]), (kind, n, t, np.argwhere(X[t] != E[t])[:4])
    if kind == KIND_F32:  # what the defect of the eighth channel looked like: no value below zero
        assert X[7].min() == -vmax and X[7].max() == vmax


def test_gather_f32_eighth_channel_takes_every_value(prof, gpu_ctx):
    n, vmax = 130, 64
    L = _gather_labels(n, 0, seed=77)
    X, _, _ = _gather(prof, gpu_ctx, KIND_F32, n, 8, vmax, 0, L)
    for t in range(8):
        seen = np.unique(X[t, :n, :n][L.reshape(n, n) != 0])
        assert len(seen) == 2 * vmax + 1, (t, len(seen))  # ~3900 classes over 129 values: every one of them occurs


# ------------------------------------------------------------------ the dot products on labels, and the symmetry probe
PROJ_N = (1, 16, 57, 1620)
_RATIOS = {}


def _proj_coef(prof, ctx, form, n, r, key, L, U):
    out = np.full(2 * r, np.nan)
    st = prof.sdpsr_profile_proj_coef(ctx._h, form, n * n, n, r, C.c_uint64(key), _vp(L), _vp(U), _vp(out))
    assert st == OK, ctx._lib.sdpsr_last_error(ctx._h)
    return out


def _note(name, ratio):
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), float(ratio))
    print(f"[ratio to bound] {name}: {ratio:.3g} (largest so far {_RATIOS[name]:.3g})")


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("n", PROJ_N)
def test_proj_coef_on_labels(prof, gpu_ctx, n, r):
    """<U_k, x>, x the class draws: U in {+-1, +-2} without a zero, so that no dropped or doubled stride class can hide (one entry of the
    n = 1620 sum is ~1e-6 of it, the bound ~6e-10)."""
    length = n * n
    assert (length > 5 * G) == (n == 1620) and (length > G) == (n == 1620)
    rng = np.random.default_rng(100 * n + r)
    L = hashed_labels(n, 50, salt=r)
    U = np.ascontiguousarray(rng.choice([-2.0, -1.0, 1.0, 2.0], size=r * length))
    xi = P.uniform_ints(KEY, L)
    got = _proj_coef(prof, gpu_ctx, 0, n, r, KEY, L, U)
    for k in range(r):
        s, sa = P.exact_dot_ints(P.integer_basis(U[k * length:(k + 1) * length]), xi)
        bound = P.dot_bound(length, P.scaled(sa))
        err = abs(got[k] - P.scaled(s))
        _note("proj_coef", err / bound if bound else 0.0)
        assert err <= bound, (n, r, k, got[k], P.scaled(s), bound)
        if n == 1620:
            assert bound < 1e-9 * P.scaled(sa)  # (one entry of the sum is ~1e-6 of it)
    assert np.isnan(got[r:]).all()


def _symmetric_ints(rng, n, r):
    """r exactly symmetric n x n integer matrices with entries in {+-1, +-2}, flat."""
    out = []
    for _ in range(r):
        M = np.tril(rng.choice(np.array([-2, -1, 1, 2], dtype=np.int64), size=(n, n)))
        out.append((M + np.tril(M, -1).T).ravel(order="F"))
    return out


def _probe_scale(n, ui, wi):
    """The smallest q >= 10 with which the a-priori bound of every probe <ui 2^-q, w> lies under the loop's 1e-10: decided from the inputs.
    (The loop's basis is orthonormal, entries ~1 / n; with entries of order 1 the bound 2 len u sum |U w| is ~1e-3 at n = 1620.)"""
    worst = max(P.dot_bound(n * n, P.scaled(P.exact_dot_ints(u, wi)[1])) for u in ui)
    q = 10
    while np.ldexp(worst, -q) >= 1e-10:
        q += 1
    return q


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("n", PROJ_N)
def test_symmetry_probe(prof, gpu_ctx, n, r):
    """probe_k = <U_k, W - W'>, w(e) = the port's weights.  Exactly symmetric U_k: |probe_k| under the a-priori bound (weights in place of
    x), and that bound under the loop's 1e-10.  One entry (i, j) raised by 2^-10 over (j, i): probe_k = 2^-10 w_ij within the bound, and
    above 1e-10; the other probes stay under their bounds.  The entries of U are {+-1, +-2} 2^-q, q chosen from the inputs so that
    the bound can lie under 1e-10 at all (see _probe_scale)."""
    length = n * n
    assert (length > 5 * G) == (n == 1620)
    key = P.probe_key(n)
    L = hashed_labels(n, 50, salt=9)
    wi, xi = P.probe_weight_ints(key, n), P.uniform_ints(key, L)
    ui = _symmetric_ints(np.random.default_rng(300 * n + r), n, r)
    q = _probe_scale(n, ui, wi)
    U = np.ascontiguousarray(np.concatenate([np.ldexp(u.astype(np.float64), -q) for u in ui]))
    assert all(np.array_equal(P.integer_basis(U[k * length:(k + 1) * length], q), ui[k]) for k in range(r))
    bounds = [P.dot_bound(length, P.scaled(P.exact_dot_ints(ui[k], wi)[1], q)) for k in range(r)]
    assert all(b < 1e-10 for b in bounds)
    got = _proj_coef(prof, gpu_ctx, 1, n, r, key, L, U)
    for k in range(r):
        assert P.exact_dot_ints(ui[k], wi)[0] == 0  # (symmetric against antisymmetric: exactly zero)
        _note("probe_symmetric", abs(got[r + k]) / bounds[k] if bounds[k] else 0.0)
        assert abs(got[r + k]) <= bounds[k], (n, r, k, got[r + k], bounds[k])
        s, sa = P.exact_dot_ints(ui[k], xi)  # the dot products ride along: the same pass forms them
        assert abs(got[k] - P.scaled(s, q)) <= P.dot_bound(length, P.scaled(sa, q))
    for (i, j) in P.probe_pairs(n):
        k = r - 1
        e = i + j * n
        V = U.copy()
        V[k * length + e] += 2.0 ** -10
        w_e = int(wi[e])
        assert 2 * abs(w_e) / 2.0 ** 53 > 0.1
        want = P.scaled(w_e << (q - 10), q)  # 2^-10 w(e): the symmetric rest cancels exactly
        s_abs = P.exact_dot_ints(ui[k], wi)[1] + (abs(w_e) << (q - 10))
        bound = P.dot_bound(length, P.scaled(s_abs, q))
        got = _proj_coef(prof, gpu_ctx, 1, n, r, key, L, V)
        _note("probe_planted", abs(got[r + k] - want) / bound)
        assert abs(got[r + k] - want) <= bound and abs(got[r + k]) > 1e-10, (n, r, i, j, got[r + k], want, bound)
        for k2 in range(r - 1):
            assert abs(got[r + k2]) <= bounds[k2]


# ------------------------------------------------------------------ the setup's vector kernels past the cap
@pytest.fixture(scope="module")
def setup_problem(problems):
    """The circulant scheme at n = 768 (len = 589 824 > 524 288) as an SDP, its trace row joined by the indicator of one class (a symmetric
    0/1 row inside the partition's span: the admissible subspace stays the generator's), the sum of the two, and the 0/1 row again."""
    n = 768
    Lm, d = problems.synthetic_jordan_partition(n)
    Cv, A, b = problems.partition_as_sdp(Lm, seed=1)
    assert n * n > G and np.array_equal(Lm, Lm.T)
    cls = int(Lm[1, 0])
    assert cls != int(Lm[0, 0])
    E = (Lm == cls).astype(np.float64).ravel(order="F")[None, :]
    # the duplicate LAST and the sum first: the pivoted MGS takes the sum (largest norm), and the duplicate is the row whose rank-one
    # updates decide what its coefficients -- and through them x0 -- come out as
    A4 = np.vstack([A, A + E, E, E])
    b4 = np.array([1.0, 1.5, 0.5, 0.5])
    return n, Lm, d, Cv, A4, b4


def test_device_setup_past_the_cap(pkg, setup_problem):
    n, Lm, d, Cv, A4, b4 = setup_problem
    m = A4.shape[0]
    Sh = pkg.admissible_setup(Cv, A4, b4)
    with pkg.Context(seed=7) as ctx:
        S = pkg.admissible_setup_csr(Cv, sp.csr_matrix(A4), b4, ctx=ctx)
        assert S.info == pkg._lib.SETUP_MGS  # the duplicate forces the pivoted MGS
        assert S[3].shape[1] == Sh[3].shape[1] == m - 2
        seen = _compare_with_host_setup(pkg, S, Sh)
        for name, ratio in seen.items():
            _note("setup_" + name, ratio)
        Pc = pkg.admissible_subspace(Cv, sp.csr_matrix(A4), b4, ctx=ctx, csr_setup=True)
        Pd = pkg.admissible_subspace(Cv, A4, b4, ctx=ctx)  # the dense entry: its rows go through transpose_rows_kernel
    for got in (Pc, Pd):
        assert got.nparts == d and np.array_equal(got.matrix, Lm)
