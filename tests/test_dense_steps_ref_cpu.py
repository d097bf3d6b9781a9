"""The references of tests/test_gpu_dense_steps.py (tests/dense_steps_ref.py) checked without a GPU: the restatements agree with
Python-integer arithmetic and with the oracle on small cases, the float64 evaluation of every real-data reference lies inside the
reference's own bound on every input the GPU tests use, and every family of which exactness is claimed keeps its intermediate
magnitudes below 2^53 -- the bounds and the exactness are judged here, never on a kernel."""
import math

import numpy as np
import pytest

import dense_steps_ref as R

O = R.O


def test_block_norms_restatement_in_python_integers():
    """T, M and the block maxima of the integer family at n = 5 and 9 against nested Python-integer loops; the layouts name every
    space and the non-monotone one is not sorted"""
    for n in (5, 9):
        A, Q = R.integer_family(n)
        T, M = R.qtaq_exact(A, Q)
        a, q = [[int(x) for x in r] for r in A], [[int(x) for x in r] for r in Q]
        t = [[sum(a[i][k] * q[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
        m = [[sum(q[k][i] * t[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
        assert T.tolist() == t and M.tolist() == m
        for name, sp in R.layouts(n, True).items():
            neig = int(sp.max()) + 1
            assert sorted(set(sp.tolist())) == list(range(neig)), name
            want = [[max([abs(m[i][j]) for i in range(n) for j in range(n) if sp[i] == sa and sp[j] == sb]) for sb in range(neig)] for sa in range(neig)]
            assert R.block_max(np.abs(M), sp, neig).tolist() == want, name
        assert (np.diff(R.layouts(n, True)["non-monotone"]) < 0).any()
    for n in (2, 5, 33, 64, 65, 200):  # the non-symmetric element: exact, and its M tells the layout from its transpose
        A, Q = R.general_integer_family(n)
        R.assert_exact_qtaq(A, Q, symmetric=False)
        T, M = R.qtaq_exact(A, Q)
        assert np.array_equal(T, A.astype(np.int64).T @ Q.astype(np.int64)) and not np.array_equal(np.abs(M), np.abs(M).T)
    start = np.array([[0.0, 9.0], [1.0, 4.0]])
    assert R.expected_norms(np.array([[3.0, 2.0], [5.0, 4.0]]), np.array([0, 1], dtype=np.int32), 2, start).tolist() == [[3.0, 9.0], [5.0, 4.0]]


@pytest.mark.parametrize("n", sorted(set(R.SMALL_ORDERS + R.LARGE_ORDERS)))
def test_block_norm_families(n):
    """the integer family is exact (|T| <= 2^24, |M| <= 2^38 on the absolute values) and has the zero row and column the GPU test
    relies on; the float64 evaluation of the real family's |Q'AQ| is inside the bound, with room"""
    A, Q = R.integer_family(n)
    ta, ma = R.assert_exact_qtaq(A, Q)
    assert ta <= 2 ** 24 and ma <= 2 ** 38 < 2 ** 53
    M = R.qtaq_exact(A, Q)[1]
    assert n < 3 or (not M[n - 1].any() and not M[:, n - 1].any() and np.abs(M).max() > 0)
    ref, bound = R.real_qtaq(n)
    Ar, Qr = R.real_family(n)
    assert np.array_equal(Ar, Ar.T) and np.abs(Qr.T @ Qr - np.eye(n)).max() < 1e-12
    err = np.abs(np.abs(Qr.T @ (Ar @ Qr)).astype(R.LD) - ref)
    assert (err <= bound).all() and float((err / bound).max()) < 0.5, (n, float((err / bound).max()))
    for name in ("zeros", "raise"):
        start = R.start_values(name, 3, np.array([[1.0, 2.0, 0.0]] * 3))
        assert (start >= 0).all() and (name == "zeros" or ((start > 2).any() and (start < 2).any()))


def test_clustering_rule():
    """a new space where !(|dv| <= atol): the oracle's boundaries; the lists hold a gap of exactly atol (no boundary), one an ulp
    above it (a boundary) and a NaN (a boundary on both sides)"""
    atol = R.CLUSTER_ATOL
    for n in (1, 2, 33, 64):
        for name, ev in R.eigenvalue_lists(n, atol).items():
            assert len(ev) == n
            sp = R.cluster(ev, atol)
            ptrs, _ = O.eigenspace_ptrs(list(ev), atol)
            assert [int(np.argmax(sp == b)) for b in range(sp.max() + 1)] + [n] == ptrs, (n, name)
        lists = R.eigenvalue_lists(n, atol)
        assert R.cluster(lists["all equal"], atol).max() == 0 and R.cluster(lists["all apart"], atol).max() == n - 1
        if n >= 3:
            ev = lists["gaps atol and atol + ulp"]
            d = np.diff(ev)
            assert (d == atol).any() and (d == np.nextafter(atol, 1.0)).sum() == 1 and (np.diff(ev) > 0).all()
            assert R.cluster(ev, atol).max() >= 1
            h = n // 2
            sp = R.cluster(lists["a NaN"], atol)
            assert sp[h] == sp[h - 1] + 1 and (h + 1 >= n or sp[h + 1] == sp[h] + 1)
    o_space, o_vals, o_norms, total = R.pack_layout(33)
    assert (o_space, o_vals, o_norms, total) == (64, 64 + 192, 64 + 192 + 264, 64 + 192 + 264 + 33 * 33 * 8)


def test_otsu_chain_against_the_oracle():
    """classes_expected on the matrices of test_iso_classes_cpu.py: the symmetrised matrix, the counts per bin, the chosen bin, kpart
    and the verdict are the oracle's; the threshold to a relative 1e-12 (the two sides differ in how exp(linspace(log .)) rounds)"""
    for name, dims, raw in R._matrix_cases():
        sym, counts, edges, best, thr, K = R._oracle_chain(dims, raw)
        got = R.classes_expected(raw, dims, R.ATOL)
        assert np.array_equal(got["sym"], sym), name
        cnt = got["stat"][2:].astype(np.int64)
        hist = np.zeros(16, dtype=np.int64)  # counts per bin from the counts per number of edges below
        for c in range(18):
            hist[min(max(min(c + 1, 17) - 1, 1), 16) - 1] += cnt[c]
        assert hist.tolist() == counts.tolist() and int(cnt.sum()) == len(dims) ** 2, name
        assert got["best"] == best and abs(got["thr"] - thr) <= 1e-12 * thr, (name, got["best"], best)
        want = R._expected_classes(K, 0)
        assert got["kpart"] == want["kpart"] and got["status"] == (R.OK if want["verdict"][0] else R.NUMERICAL_INCONSISTENCY), name
        assert np.abs(got["edges"] - edges).max() <= 1e-12 * edges.max()


def test_otsu_chain_in_python_integers():
    """the stat words and the pair bits of a 70 x 70 case against plain Python loops over the entries"""
    name, dims, raw = R.class_cases(70)[4]
    assert name.startswith("unequal dims")
    got = R.classes_expected(raw, dims, R.ATOL)
    ne = 70
    sym = [[0.0 if dims[min(i, j)] != dims[max(i, j)] else float(raw[min(i, j), max(i, j)]) for j in range(ne)] for i in range(ne)]
    assert got["sym"].tolist() == sym
    flat = [x for r in sym for x in r]
    assert int(got["stat"][0]) == (~int(np.array([min(flat)]).view(np.uint64)[0])) & (2 ** 64 - 1)
    assert int(got["stat"][1]) == int(np.array([max(flat)]).view(np.uint64)[0])
    edges = R.otsu_edges(min(flat), max(flat), R.ATOL)
    assert edges == got["edges"].tolist() and all(a <= b for a, b in zip(edges, edges[1:]))
    cnt = [0] * 18
    for x in flat:
        cnt[sum(1 for e in edges if not e > x)] += 1
    assert cnt == [int(x) for x in got["stat"][2:]]
    words = [[0, 0] for _ in range(ne)]
    for i in range(ne):
        for j in range(i + 1, ne):
            if sym[i][j] >= got["thr"]:
                words[i][j // 64] |= 1 << (j % 64)
    assert [[int(x) for x in r] for r in got["bits"]] == words and any(any(r) for r in words)


@pytest.mark.parametrize("ne", R.CLASS_ORDERS)
def test_class_cases(ne):
    """the cases of every neig: all named kinds present, the NaN and the zeroed coupled pair where they should be, the threshold
    entry equal to the threshold, the bits beyond neig zero, and special values through the chain without an exception"""
    cases = {name: (dims, raw) for name, dims, raw in R.class_cases(ne)}
    want = {"clusters, asymmetric raw", "all zero", "all equal", "one NaN"} | ({"unequal dims in a coupled pair"} if ne >= 2 else set())
    want |= {"an entry exactly at the threshold"} if ne >= 3 else set()
    assert set(cases) == want
    for name, (dims, raw) in cases.items():
        got = R.classes_expected(raw, dims, R.ATOL)
        W = (ne + 63) // 64
        assert got["bits"].shape == (ne, W) and got["stat"][2:].sum() == ne * ne
        full = np.zeros((ne, W * 64), dtype=bool)
        for b in range(64):
            full[:, b::64] = (got["bits"] >> np.uint64(b)) & np.uint64(1)
        assert not full[:, ne:].any() and not np.tril(full[:, :ne]).any()
        if name == "clusters, asymmetric raw":
            assert ne < 2 or not np.array_equal(raw, raw.T)
            assert np.array_equal(got["sym"], got["sym"].T)
        if name == "one NaN":
            assert np.isnan(got["sym"][0, ne - 1]) and np.isnan(got["sym"][ne - 1, 0]) and got["stat"][19] >= 1
        if name == "all equal":
            assert got["thr"] == 0.375 and len(set(got["kpart"])) == 1
        if name == "all zero":
            assert not got["stat"][1] and not got["bits"].any() or got["thr"] == 0.0
        if name == "an entry exactly at the threshold":
            assert (np.triu(got["sym"], 1) == got["thr"]).sum() == 1
        if name == "unequal dims in a coupled pair":
            i, j = np.argwhere((np.triu(raw, 1) > 0.4) & (got["sym"] == 0))[0]
            assert dims[i] != dims[j] and not full[i, j]


def test_irreducible_restatement_in_python_integers():
    """y and the sum of squares at n = 6 against nested Python-integer loops; the 4 ulp allowance holds for the float64 evaluation
    of the same three roundings"""
    n = 6
    rng = np.random.default_rng(2)
    Q = np.full((128, n), 12345.0)
    B = np.full((128, 5), 12345.0)
    Q[:n], B[:n] = rng.integers(-8, 9, (n, n)), rng.integers(-1024, 1025, (n, 5))
    desc = np.array([[0, 2, 3, 3, 1, 4, 0], [4, 1, 0, 6, 0, 0, 2]], dtype=np.int32)
    q, b = [[int(x) for x in r] for r in Q[:n]], [[int(x) for x in r] for r in B[:n]]
    for (y, S), (ci, mi, cj, mj, fi, fj, _) in zip(R.irreducible_exact(n, Q, B, desc), desc.tolist()):
        w = [sum(q[r][cj + t] * b[r][fi] for r in range(n)) for t in range(mj)]
        c = [sum(q[r][ci + t] * b[r][fj] for r in range(n)) for t in range(mi)]
        assert y.tolist() == [sum(q[r][cj + t] * w[t] for t in range(mj)) for r in range(n)] and S == sum(x * x for x in c)
    ref, ulp4 = R.irreducible_exact_columns(n, Q, B, desc)
    for p, (y, S) in enumerate(R.irreducible_exact(n, Q, B, desc)):
        f64 = y.astype(np.float64) * (1.0 / math.sqrt(float(S)))
        assert (np.abs(f64.astype(R.LD) - ref[:, p]) <= ulp4[:, p]).all()


@pytest.mark.parametrize("n", R.IRREDUCIBLE_ORDERS)
def test_irreducible_families(n):
    """every (n, number of pairs) of the GPU test: the descriptors stay inside their arrays, name every shape that fits and leave
    three columns unnamed; the integer family is exact (asserted inside irreducible_exact on the absolute values) with a positive
    norm; the float64 evaluation of the real family is inside its bound, with room"""
    Qi, Bi = R.irreducible_integer_inputs(n)
    Qr, Br = R.irreducible_real_inputs(n)
    assert Qi.shape == (R.round_up(n, 128), n) and (Qi[n:] == 12345.0).all() and (Br[n:] == 12345.0).all()
    for npairs in (1, 2, 300):
        desc, vcols, nf, ncols = R.pair_descriptors(n, npairs)
        assert vcols == n and ncols == npairs + 3 and len(set(desc[:, 6].tolist())) == npairs and desc[:, 6].max() < ncols
        assert (desc[:, 0] + desc[:, 1] <= n).all() and (desc[:, 2] + desc[:, 3] <= n).all() and desc[:, 4:6].max() < nf and desc.min() >= 0
        if npairs == 300:
            assert {(int(r[1]), int(r[3])) for r in desc} == set(R.pair_shapes(n)) and not np.array_equal(desc[:, 6], np.sort(desc[:, 6]))
        ref, ulp4 = R.irreducible_exact_columns(n, Qi, Bi, desc)
        assert np.isfinite(ref.astype(np.float64)).all()
        ref, bound = R.irreducible_real(n, Qr, Br, desc)
        f64, _ = R.irreducible_real(n, Qr, Br, desc, dtype=np.float64)
        err = np.abs(f64.astype(R.LD) - ref)
        assert (err <= bound).all() and float((err / bound).max()) < 0.5, (n, npairs, float((err / bound).max()))
    assert (7678 + 2) * 8 == 60 * 1024 and R.LDS_RULE_M2 == 7678
    shapes = R.pair_shapes(n)
    assert (1, 1) in shapes and ((63, 65) in shapes) == (n >= 65) and ((128, 1) in shapes) == (n >= 128) and ((n, 1) in shapes)


def test_copy_cols_and_clamptol_restatements():
    src = np.arange(12.0).reshape(4, 3)
    dst = np.full((5, 4), -1.0)
    got = R.copy_cols(3, src, dst, np.array([2, 2, 0]), np.array([3, 0, 1]))
    assert got[:3, 3].tolist() == src[:3, 2].tolist() == got[:3, 0].tolist() and got[:3, 1].tolist() == src[:3, 0].tolist()
    assert (got[3:] == -1).all() and (got[:, 2] == -1).all()
    a = np.array([-0.5, 0.5, -1.0, 1.0, np.nan, -0.0, 2.0])
    out = R.clamptol(a, 1.0)
    assert R.bits(out).tolist() == R.bits(np.array([0.0, 0.0, -1.0, 1.0, np.nan, 0.0, 2.0])).tolist()
    assert R.GRID_CAP == 2048 * 256 and R.COPY_COUNTS == (1, 128, 129, 257)
