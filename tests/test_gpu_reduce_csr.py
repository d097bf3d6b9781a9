"""Reduced-SDP assembly from a sparse A (sdpsr_reduce_constraints_csr; README.md:57-60, test/sd_problems.jl:32-37,113-118):
exact integer cases for every row shape and every d regime, agreement with the dense entry, real values against the
any-order bound, reproducible bits, input forms, device-resident arguments, errors, the reference's problems and the
grid QAP at full size."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 5


def _labels(n, d, seed):
    """Flat column-major labels 0..d of an n x n matrix: about 5 % label 0 (no column), and for d >= 7 class d confined
    to the LAST entry (the ragged tail of the last chunk) and class d - 1 absent from the first chunk of 4096."""
    rng = np.random.default_rng(seed)
    ln = n * n
    hi = d if d < 7 else d - 2
    lab = rng.integers(1, hi + 1, size=ln)
    lab[rng.random(ln) < 0.05] = 0
    if d >= 7:
        late = 4096 + rng.choice(ln - 1 - 4096, size=5, replace=False)
        lab[late] = d - 1
        lab[ln - 1] = d
        assert not np.any(lab[:4096] == d - 1) and np.count_nonzero(lab == d) == 1
    return lab.astype(np.uint32)


def _own_labels(n, seed):
    """Every entry its own class (in shuffled order), about 5 % label 0: d = number of non-zero labels."""
    rng = np.random.default_rng(seed)
    ln = n * n
    keep = np.flatnonzero(rng.random(ln) >= 0.05)
    lab = np.zeros(ln, dtype=np.uint32)
    lab[keep] = rng.permutation(keep.size) + 1
    return lab, int(keep.size)


def _row_columns(kind, ln, lab, rng):
    """Sorted column indices of one row of the given shape."""
    if kind == "all":                      # the QAP's all-ones row
        return np.arange(ln)
    if kind == "empty":
        return np.arange(0)
    if kind == "label0":                   # every entry in a column without a class
        z = np.flatnonzero(lab == 0)
        return z[:max(1, z.size // 2)]
    if kind == "one_class":                # confined to the largest class
        big = np.bincount(lab[lab > 0]).argmax()
        return np.flatnonzero(lab == big)
    if kind == "random":
        return np.flatnonzero(rng.random(ln) < rng.uniform(0.01, 0.3))
    return np.sort(rng.choice(ln, size=int(kind), replace=False))


ROW_KINDS = ["all", "empty", 4097, 1, 63, "label0", 64, 65, 4095, 4096, "one_class"]


def _matrix(ln, m, lab, seed, real=False):
    """m x ln CSR with the row shapes of ROW_KINDS (as many as fit m, then random rows)."""
    rng = np.random.default_rng(seed)
    kinds = (ROW_KINDS + ["random"] * m)[:m]
    cols = [_row_columns(k, ln, lab, rng) for k in kinds]
    rowptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    colind = np.concatenate(cols).astype(np.int64)
    if real:
        val = rng.standard_normal(colind.size) * 10.0 ** rng.uniform(-6, 6, size=colind.size)
    else:
        val = rng.integers(1, 9, size=colind.size) * rng.choice([-1, 1], size=colind.size)  # [-8, 8] without zeros
    return sp.csr_matrix((val.astype(np.float64), colind, rowptr), shape=(m, ln))


def _class_sums_int(lab, A, d):
    """A * PMat in integer arithmetic."""
    coo = A.tocoo()
    acc = np.zeros((A.shape[0], d + 1), dtype=np.int64)
    np.add.at(acc, (coo.row, lab[coo.col].astype(np.int64)), np.rint(coo.data).astype(np.int64))
    return acc[:, 1:]


def _P(pkg, n, d, lab):
    return pkg.Partition(d, lab.reshape(n, n, order="F"))


def _pmat(lab, d):
    idx = np.flatnonzero(lab > 0)
    return sp.csr_matrix((np.ones(idx.size), (idx, lab[idx].astype(np.int64) - 1)), shape=(lab.size, d))


def _check_any_order_bound(got, A, lab, what):
    """|got - fsum| <= count * 2^-53 * sum |a| per (row, class): the a-priori bound of a floating-point sum in ANY order."""
    coo = A.tocoo()
    keys = coo.row.astype(np.int64) * (int(lab.max()) + 1) + lab[coo.col].astype(np.int64)
    order = np.argsort(keys, kind="stable")
    keys, vals, rows, labs = keys[order], coo.data[order], coo.row[order], lab[coo.col][order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    ends = np.r_[starts[1:], keys.size]
    expect_zero = np.ones(got.shape, dtype=bool)
    worst = 0.0
    for a, b in zip(starts, ends):
        if labs[a] == 0:
            continue
        v = vals[a:b].tolist()
        bound = len(v) * 2.0 ** -53 * math.fsum(abs(x) for x in v)
        err = abs(got[rows[a], labs[a] - 1] - math.fsum(v))
        assert err <= bound, (what, int(rows[a]), int(labs[a]), err, bound)
        expect_zero[rows[a], labs[a] - 1] = False
        if bound:
            worst = max(worst, err / bound)
    assert np.all(got[expect_zero] == 0.0) and not np.any(np.signbit(got[expect_zero]))
    print(f"reduce_constraints_csr {what}: worst error / bound = {worst:.3e}")


# ------------------------------------------------------------------ 1. exact integer cases
@pytest.mark.parametrize("n", [65, 130])
def test_exact_integer_cases(pkg, gpu_ctx, n):
    """Integer values in [-8, 8]: every sum is exact in any order, so the result must EQUAL integer arithmetic.  len = 4225 is
    two chunks of 4096 with a ragged tail of 129 = 2 * 64 + 1; d = 120 with m = 65 and d = 8000 with m = 1 are the first
    shapes the dense entry refuses; with every entry its own class no two entries share an output."""
    ln = n * n
    cases = [(d, _labels(n, d, seed=1000 * n + d)) for d in (1, 7, 119, 120)]
    if n == 130:
        cases.append((8000, _labels(n, 8000, seed=8000)))
    lab_own, d_own = _own_labels(n, seed=n)
    cases.append((d_own, lab_own))
    for m in (1, 3, 65):
        for d, lab in cases:
            A = _matrix(ln, m, lab, seed=100 * m + d % 97)
            got = pkg.reduce_constraints_csr(_P(pkg, n, d, lab), A, ctx=gpu_ctx)
            assert got.shape == (m, d) and got.dtype == np.float64
            assert np.array_equal(got, _class_sums_int(lab, A, d)), (n, m, d)
    # a vector (C' * PMat) comes back as a vector: 1-D dense, and a SciPy column
    d, lab = cases[1]
    c_int = np.random.default_rng(n).integers(-8, 9, size=ln).astype(np.float64)
    want = _class_sums_int(lab, sp.csr_matrix(c_int[None, :]), d)[0]
    for form in (c_int, sp.csr_matrix(c_int[:, None])):
        got = pkg.reduce_constraints_csr(_P(pkg, n, d, lab), form, ctx=gpu_ctx)
        assert got.shape == (d,) and np.array_equal(got, want)


def test_empty_inputs(pkg, gpu_ctx):
    n, d = 65, 7
    lab = _labels(n, d, seed=1)
    got = pkg.reduce_constraints_csr(_P(pkg, n, d, lab), sp.csr_matrix((0, n * n)), ctx=gpu_ctx)
    assert got.shape == (0, d)
    got = pkg.reduce_constraints_csr(_P(pkg, n, d, lab), sp.csr_matrix((3, n * n)), ctx=gpu_ctx)
    assert got.shape == (3, d) and np.all(got == 0.0) and not np.any(np.signbit(got))


# ------------------------------------------------------------------ 2. agreement with the dense entry
@pytest.mark.parametrize("m,d,n", [(65, 7, 65), (65, 119, 65), (1, 7678, 130)])
def test_agrees_with_dense_entry(pkg, gpu_ctx, m, d, n):
    lab = _labels(n, d, seed=7 * d + m)
    A = _matrix(n * n, m, lab, seed=d)
    P = _P(pkg, n, d, lab)
    got = pkg.reduce_constraints_csr(P, A, ctx=gpu_ctx)
    dense = pkg.reduce_constraints(P, A.toarray(), ctx=gpu_ctx)
    assert np.array_equal(got, dense)
    assert np.array_equal(got, _class_sums_int(lab, A, d))


# ------------------------------------------------------------------ 3. / 4. real values, reproducible bits
@pytest.fixture(scope="module")
def real_case():
    n, m, d = 65, 65, 120
    lab = _labels(n, d, seed=50 + d)
    return n, d, lab, _matrix(n * n, m, lab, seed=3, real=True)


def test_real_values_any_order_bound(pkg, gpu_ctx, real_case):
    """Standard normal times 10^U(-6, 6) against math.fsum per (row, class); bound count * 2^-53 * sum |a| over the run
    ((count - 1) u / (1 - (count - 1) u) <= count u): a-priori for ANY summation order, so it is derived, not measured."""
    n, d, lab, A = real_case
    got = pkg.reduce_constraints_csr(_P(pkg, n, d, lab), A, ctx=gpu_ctx)
    _check_any_order_bound(got, A, lab, f"real n={n} m={A.shape[0]} d={d}")


def test_bits_do_not_depend_on_the_ctx_or_its_history(pkg, problems, gpu_ctx, real_case):
    n, d, lab, A = real_case
    P = _P(pkg, n, d, lab)
    a = pkg.reduce_constraints_csr(P, A, ctx=gpu_ctx)
    b = pkg.reduce_constraints_csr(P, A, ctx=gpu_ctx)
    with pkg.Context(seed=987) as ctx:
        # unrelated calls first: another problem through the CSR setup and the loop, another reduction of other sizes
        Cv, A2, b2 = problems.theta_prime_problem(problems.er_graph_adjacency(3))
        P2 = pkg.admissible_subspace(Cv, A2, b2, ctx=ctx, csr_setup=True)
        pkg.reduce_constraints_csr(P2, sp.csr_matrix(A2), ctx=ctx)
        pkg.randomize(P2, ctx=ctx)
        c = pkg.reduce_constraints_csr(P, A, ctx=ctx)
    assert a.tobytes() == b.tobytes() == c.tobytes()


# ------------------------------------------------------------------ 5. input forms
def test_input_forms_give_identical_bits(pkg, gpu_ctx):
    n, m, d = 65, 65, 119
    lab = _labels(n, d, seed=5)
    A = _matrix(n * n, m, lab, seed=6)
    P = _P(pkg, n, d, lab)
    want = _class_sums_int(lab, A, d)
    coo = A.tocoo()
    rng = np.random.default_rng(8)
    # every 7th entry split into two integer duplicates, then everything shuffled
    r, c, v = coo.row.copy(), coo.col.copy(), coo.data.copy()
    dup = np.arange(0, v.size, 7)
    v[dup] -= 3.0
    r, c, v = np.r_[r, r[dup]], np.r_[c, c[dup]], np.r_[v, np.full(dup.size, 3.0)]
    perm = rng.permutation(v.size)
    shuffled = sp.coo_matrix((v[perm], (r[perm], c[perm])), shape=A.shape)
    forms = {"csr": A, "coo shuffled + duplicates": shuffled, "dense": A.toarray(),
             "1-based arrays": ((A.indptr + 1).astype(np.int64), (A.indices + 1).astype(np.int64), A.data)}
    for name, form in forms.items():
        got = pkg.reduce_constraints_csr(P, form, ctx=gpu_ctx, index_base=1 if name.startswith("1-based") else 0)
        assert got.tobytes() == want.astype(np.float64).tobytes(), name
    # the same unsorted, duplicated arrays straight through the C entry (the library's own canonicalisation)
    order = np.lexsort((rng.random(v.size), r))  # rows grouped, columns shuffled inside
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64)
    ci, va = np.ascontiguousarray(c[order], dtype=np.int64), np.ascontiguousarray(v[order])
    out = np.full((m, d), np.nan, order="F")
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    gpu_ctx.check(gpu_ctx._lib.sdpsr_reduce_constraints_csr(gpu_ctx._h, n * n, p(lab), d, m, p(rp), p(ci), p(va), 0, p(out), pkg.MEM_HOST))
    assert out.tobytes() == np.asfortranarray(want.astype(np.float64)).tobytes()


# ------------------------------------------------------------------ 6. device-resident labels and out
def test_device_resident_labels_and_out(pkg, gpu_ctx):
    import torch
    n, m, d = 65, 65, 120
    ln = n * n
    lab = _labels(n, d, seed=22)
    A = _matrix(ln, m, lab, seed=23)
    t_lab = torch.from_numpy(lab.view(np.int32).copy()).cuda()
    t_out = torch.full((m * d,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rp, ci, va = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    gpu_ctx.check(gpu_ctx._lib.sdpsr_reduce_constraints_csr(gpu_ctx._h, ln, C.c_void_p(t_lab.data_ptr()), d, m, p(rp), p(ci), p(va), 0,
                                                            C.c_void_p(t_out.data_ptr()), pkg.MEM_DEVICE))
    got = t_out.cpu().numpy().reshape(m, d, order="F")
    want = _class_sums_int(lab, A, d)
    assert not np.any(np.isnan(got))
    assert np.array_equal(got, want)
    assert np.count_nonzero(want == 0) > 0 and not np.any(np.signbit(got[want == 0]))  # exact +0.0 where a class misses a row
    assert np.array_equal(t_lab.cpu().numpy().view(np.uint32), lab)
    # the Python mirror with a device-resident partition
    P = pkg.Partition(d, t_lab.view(n, n).t())
    assert np.array_equal(pkg.reduce_constraints_csr(P, A, ctx=gpu_ctx), want)


# ------------------------------------------------------------------ 7. errors
def test_errors_leave_the_ctx_usable(pkg, gpu_ctx):
    n, m, d = 65, 3, 7
    ln = n * n
    lab = _labels(n, d, seed=31)
    A = _matrix(ln, m, lab, seed=32)
    want = _class_sums_int(lab, A, d)

    def small_case_ok():
        assert np.array_equal(pkg.reduce_constraints_csr(_P(pkg, n, d, lab), A, ctx=gpu_ctx), want)

    for bad_label, where in ((d + 1, ln - 1), (2 ** 32 - 1, ln - 2), (d + 1, 4096 + 64)):
        lab2 = lab.copy()
        lab2[where] = bad_label  # in the ragged tail; row 0 holds every column
        with pytest.raises(pkg.SdpsrError) as ei:
            pkg.reduce_constraints_csr(_P(pkg, n, d, lab2), A, ctx=gpu_ctx)
        assert ei.value.status == BAD_ARGUMENT and "label exceeds d" in str(ei.value)
        small_case_ok()
    # malformed CSR straight through the C entry (the Python mirror would raise ValueError first)
    rp, ci, va = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    out = np.zeros((m, d), order="F")

    def call(rp_, ci_, va_, base):
        return gpu_ctx._lib.sdpsr_reduce_constraints_csr(gpu_ctx._h, ln, p(lab), d, m, p(rp_), p(ci_), p(va_), base, p(out), pkg.MEM_HOST)

    ci_bad = ci.copy()
    ci_bad[-1] = ln
    va_bad = va.copy()
    va_bad[5] = np.inf
    rp_bad = rp.copy()
    rp_bad[2] = rp[1] - 1  # non-monotone
    for args in ((rp, ci_bad, va, 0), (rp, ci, va, 1), (rp + 1, ci + 1, va, 0), (rp, ci, va_bad, 0), (rp_bad, ci, va, 0), (rp, ci, va, 2)):
        assert call(*args) == BAD_ARGUMENT
        small_case_ok()
    assert call(rp + 1, ci + 1, va, 1) == 0 and np.array_equal(out, want)


# ------------------------------------------------------------------ 8. the reference's problems
def _problem(problems, name):
    if name.startswith("er"):
        return problems.theta_prime_problem(problems.er_graph_adjacency(int(name[2:])))
    fa, fb = problems.read_qapdata(ROOT / "tests" / "golden" / "esc16j.dat")
    return problems.qap_problem(fa, fb)


@pytest.mark.parametrize("name", ["er3", "er5", "er7", "esc16j"])
def test_reference_problems_equal_scipy_product(pkg, problems, golden, gpu_ctx, name):
    """newA = A * PMat and newC = C' * PMat of test/sd_problems.jl:32-37,113-118 on the golden partitions."""
    Cv, A, b = _problem(problems, name)
    L = golden[f"{name}_P"]
    d = int(L.max())
    P = pkg.Partition(d, L.astype(np.uint32))
    lab = np.asarray(L).ravel(order="F")
    PMat = _pmat(lab, d)
    A = sp.csr_matrix(A)
    newA = pkg.reduce_constraints_csr(P, A, ctx=gpu_ctx)
    assert np.array_equal(newA, (A @ PMat).toarray())
    c = np.asarray(Cv, dtype=np.float64).reshape(-1)
    newC = pkg.reduce_constraints_csr(P, c, ctx=gpu_ctx)
    assert newC.shape == (d,) and np.array_equal(newC, PMat.T @ c)


# ------------------------------------------------------------------ 9. the grid QAP at full size
def test_grid_qap_full_size(pkg, problems):
    flow, dist = problems.grid_qap_instance(5, 6, seed=4, symmetric_flow=True)
    Cv, A, b = problems.qap_problem(flow, dist)
    assert A.shape == (61, 810000)
    with pkg.Context(seed=31) as ctx:
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, csr_setup=True)
        d = P.nparts
        assert d > 119  # beyond the dense entry's LDS accumulators at m = 61
        h0 = ctx.transfer_bytes()[0]
        newA = pkg.reduce_constraints_csr(P, A, ctx=ctx)
        h2d = ctx.transfer_bytes()[0] - h0
        newC = pkg.reduce_constraints_csr(P, Cv, ctx=ctx)
    lab = np.asarray(P.matrix).ravel(order="F")
    PMat = _pmat(lab, d)
    A = sp.csr_matrix(A)
    assert np.array_equal(newA, (A @ PMat).toarray())
    assert h2d <= 12 * A.nnz + 4 * lab.size + 8 * 62 + 64, h2d  # the CSR and the labels, not a dense A
    c = np.asarray(Cv, dtype=np.float64).reshape(-1)
    _check_any_order_bound(newC[None, :], sp.csr_matrix(c[None, :]), lab, f"grid QAP C' * PMat d={d}")
