"""The references of tests/test_gpu_rowspace_kernels.py (tests/rowspace_kernels_ref.py) checked without a GPU: the restated shape
rules against the table of shapes the GPU tests run and against the rule's text in csrc/kernels_rowspace.hip, the products against
exact rational arithmetic, and every precondition the GPU tests rely on -- exactness of the integer inputs, exactness of the
power-of-two scalings, what the planted rows of the finish test hold, rank unambiguity of the driver inputs."""
import pathlib
import re
from fractions import Fraction

import numpy as np
import pytest

import compress_ref as CR
import rowspace_kernels_ref as R

ROOT = pathlib.Path(__file__).resolve().parents[1]
SRC = (ROOT / "sdpsymmetryreduction.jl_amd" / "csrc" / "kernels_rowspace.hip").read_text()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------
def test_gram_shape_table():
    """The restated rule gives the listed (npairs, Z, cps); the two shapes listed without Z are the ones the cap zmax = 2048 / npairs
    cuts, and the last one is cut at 2048 splits."""
    for (m, ncols), (npairs, Z, cps) in R.GRAM_TABLE.items():
        got = R.gram_shape(m, ncols)
        assert got[0] == npairs, (m, ncols)
        if Z is not None:
            assert got[1:] == (Z, cps), (m, ncols, got)
        assert (got[1] - 1) * got[2] < ncols <= got[1] * got[2] and got[2] % 4 == 0  # every split holds a column, none is left out
    assert R.gram_shape(200, 13100) == (10, 193, 68) and (13100 + 63) // 64 > 2048 // 10 == 204
    assert R.gram_shape(1024, 1000) == (136, 15, 68) and (1000 + 63) // 64 > 2048 // 136 == 15
    assert (131075 + 63) // 64 == 2049 > 2048
    assert 1027 - 16 * 64 == 3  # (200, 1027): the last split holds 3 columns
    # the properties the table is there for
    pairs = {R.gram_shape(m, n)[0] for m, n in R.GRAM_SHAPES}
    assert {1, 3, 6, 10, 136} <= pairs
    assert any(n - (R.gram_shape(m, n)[1] - 1) * R.gram_shape(m, n)[2] in (1, 2, 3) for m, n in R.GRAM_SHAPES)  # a ragged tail < 4
    assert all(m * n * 8 <= 25 << 20 for m, n in R.GRAM_SHAPES)


def test_the_rules_text_is_the_restated_one():
    """The constants the restatement copies, where the source states them: a change to either side shows here."""
    assert "const int64_t zmax = std::max<int64_t>(1, 2048 / *npairs);" in SRC
    assert "*cps = round_up((ncols + z - 1) / z, 4);" in SRC
    assert "const int64_t lds = 8000;" in SRC and "const bool fits = m * m + m <= lds / 2;" in SRC
    assert "return (int)std::min<int64_t>(64, std::max<int64_t>(1, room / m));" in SRC
    assert "std::min<int64_t>(1024, std::max<int64_t>(1, (total + 2047) / 2048))" in SRC
    assert re.search(r"if \(e > 1000\) e = 1000;", SRC)


def test_chunk_rule():
    assert [R.chunk(m) for m in (1, 5, 62, 63, 64, 65, 200, 1024)] == [(64, 1), (64, 1), (64, 1), (64, 0), (64, 0), (64, 0), (40, 0), (7, 0)]
    assert [R.chunk(m, rotate=False)[0] for m in R.FINISH_M] == [64, 64, 40, 7]
    for m in R.ROTATE_M:
        cc, j_lds = R.chunk(m)
        assert (cc * m + (m * m if j_lds else 0)) * 8 <= 64000  # what the launch asks of the 64 KiB
        # the sizes nc of the chunks that run: the last one of each matrix, and the full chunk in front of it
        sizes = {R.last_chunk(n, cc) for n in R.rotate_ncols(m)} | {cc}
        assert {t % 4 for t in sizes} == {0, 1, 2, 3}, m
        assert any(n < 4 for n in R.rotate_ncols(m)) and any(R.last_chunk(n, cc) != cc and n > cc for n in R.rotate_ncols(m))
    for m, cc in zip(R.FINISH_M, (64, 64, 40, 7)):
        assert R.FINISH_NCOLS % cc and R.FINISH_NCOLS % 256 and R.FINISH_NCOLS > 260


# ---------------------------------------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------------------------------------
def _frac(a):
    return [[Fraction(float(x)) for x in row] for row in a]


def _ld_frac(x):
    """a long double, exactly"""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


def test_int_references_against_rationals():
    Wi, W = R.gram_int_input(5, 7, zero_lines=True)
    F = _frac(W)
    exact = [[sum(F[p][c] * F[q][c] for c in range(7)) for q in range(5)] for p in range(5)]
    assert [[Fraction(float(x)) for x in row] for row in R.gram_int_ref(Wi)] == exact
    assert not Wi[0].any() and not Wi[:, 0].any() and not Wi[-1].any() and not Wi[:, -1].any()
    Ji, Wi, W = R.rotate_int_input(6, 5)
    FJ, FW = _frac(Ji.astype(np.float64)), _frac(W)
    exact = [[sum(FJ[i][k] * FW[k][c] for k in range(6)) for c in range(5)] for i in range(6)]
    assert [[Fraction(float(x)) for x in row] for row in R.rotate_int_ref(Ji, Wi)] == exact


def test_real_references_against_rationals():
    """The long-double products lie within n u_ld |.||.| of the exact value -- the term the GPU tests add to the kernel's bound."""
    W = R.gram_real_inputs(6, 9)["graded"]
    ref, ab = R.gram_real_ref(W)
    F = _frac(W)
    for p in range(6):
        for q in range(6):
            exact = sum(F[p][c] * F[q][c] for c in range(9))
            assert abs(_ld_frac(ref[p, q]) - exact) <= Fraction(9 * R.LD_EPS) * sum(abs(F[p][c] * F[q][c]) for c in range(9))
            assert ref[p, q] == ref[q, p] and ab[p, q] == ab[q, p]
    assert np.allclose(np.asarray(ab, dtype=np.float64), np.abs(W) @ np.abs(W).T, rtol=1e-14, atol=0)
    J = R.plane_rotations(5, 3)
    assert np.abs(J @ J.T - np.eye(5)).max() <= 1e-14 and np.count_nonzero(J) > 5
    X = np.random.default_rng(0).standard_normal((5, 4))
    ref, ab = R.rotate_real_ref(J, X)
    assert np.abs(np.asarray(ref, dtype=np.float64) - J @ X).max() <= 1e-14
    assert R.LD_EPS <= 2.0 ** -63  # an 80-bit (or wider) long double: the reference is finer than the kernel's arithmetic


def test_split_reference_of_the_long_products():
    """The two largest Gram shapes take the reference through exact float64 pieces.  Its pieces add up to W and are integers of few
    enough bits; on a small input it is exact to the last bit of a long double; on a mid-sized one it agrees with NumPy's long-double
    product within that product's own ncols u_ld |W||W|'; and on the inputs that take it, what it leaves out (< 4 ncols
    2^(e_p + e_q - 72) per entry) and its ten long-double additions stay under half the ncols u_ld |W||W|' the GPU test grants."""
    W = R.gram_real_inputs(6, 9)["graded"]
    pieces, e, beta = R.split_rows(W, 9)
    assert beta * len(pieces) >= R.SPLIT_BITS and 9 * 4 ** beta < 2 ** 53
    rest = W - sum(pieces[1:], pieces[0])
    assert np.abs(rest).max(axis=1).tolist() <= np.ldexp(1.0, e - beta * len(pieces) - 1).tolist()
    for k, P in enumerate(pieces):
        units = P / np.ldexp(1.0, e - beta * (k + 1))[:, None]
        assert np.array_equal(units, np.rint(units)) and np.abs(units).max() <= 2 ** beta
    ref, _ = R.gram_real_ref(W, "split")
    F = _frac(W)
    for p in range(6):
        for q in range(6):
            exact = sum(F[p][c] * F[q][c] for c in range(9))
            assert abs(_ld_frac(ref[p, q]) - exact) <= Fraction(2.0 ** -62) * abs(exact) + Fraction(2.0 ** -66) * Fraction(float(np.ldexp(1.0, e[p] + e[q])))
    for name, W in R.gram_real_inputs(65, 257).items():
        a, ab = R.gram_real_ref(W, "longdouble")
        b, ab64 = R.gram_real_ref(W, "split")
        assert np.all(np.abs(a - b) <= np.longdouble(257 * R.LD_EPS) * ab), name
        assert np.all(np.abs(ab - ab64) <= 1e-13 * ab)
    took = [(m, n) for m, n in R.GRAM_SHAPES if m * m * n > R.SPLIT_ABOVE]
    assert took == [(200, 13100), (1024, 1000)]
    for m, n in took:
        for name, W in R.gram_real_inputs(m, n).items():
            e = np.frexp(np.abs(W).max(axis=1))[1]
            left_out = 4.0 * n * np.ldexp(1.0, e[:, None] + e[None, :] - R.SPLIT_BITS) + 10 * R.LD_EPS * (np.abs(W) @ np.abs(W).T)
            assert np.all(left_out <= 0.5 * n * R.LD_EPS * (np.abs(W) @ np.abs(W).T)), (m, n, name)


def test_integer_inputs_are_exact():
    """Every partial sum of the integer products, in any order, is an integer below 2^53 (in units of 2^-8 resp. 2^-4)."""
    for m, ncols in R.GRAM_SHAPES:
        assert 8 * 8 * ncols < 2 ** 53
    Wi, W = R.gram_int_input(17, 65)
    assert np.abs(Wi).max() <= 8 and np.array_equal(W * 16, Wi)
    for m in R.ROTATE_M:
        assert (3 + 1) * 8 * m < 2 ** 53
    Ji, Wi, W = R.rotate_int_input(64, 9)
    assert np.abs(Ji).max() <= 4 and np.abs(Wi).max() <= 8 and np.array_equal(W * 16, Wi)
    assert (np.abs(Ji) >= 1).sum(axis=1).min() >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# scale
# ---------------------------------------------------------------------------------------------------------------------------
def test_scale_reference_and_its_cases():
    cases = R.scale_cases()
    assert R.scale_of(0.0) == 1.0 and R.scale_of(1.0) == 0.5 and R.scale_of(0.75) == 1.0 and R.scale_of(3.0) == 0.25
    assert R.scale_of(R.DBL_MAX) == 2.0 ** -1024 and 0 < R.scale_of(R.DBL_MAX) < np.finfo(np.float64).tiny  # the scale is a denormal
    assert R.scale_of(2.0 ** -1074) == 2.0 ** 1000
    base = cases["order_one"]
    for name, k in (("up_900", 900), ("down_900", -900)):
        assert np.array_equal(_bits(np.ldexp(cases[name], -k)), _bits(base))  # the scaling lost nothing
        assert np.array_equal(_bits(R.scale_ref(cases[name])[0]), _bits(R.scale_ref(base)[0]))  # W is the same
    W, mx, bad = R.scale_ref(base)
    assert 0.5 <= np.abs(W).max() < 1.0 and mx == np.abs(base).max() and bad == 0.0
    den = cases["denormal"]
    assert 0 < np.abs(den).max() < np.finfo(np.float64).tiny and R.scale_of(np.abs(den).max()) == 2.0 ** 1000
    ints = np.ldexp(den, 1070)
    assert np.array_equal(ints, np.round(ints)) and np.array_equal(R.scale_ref(den)[0], np.ldexp(ints, -70))
    W, mx, bad = R.scale_ref(cases["dbl_max"])
    assert mx == R.DBL_MAX and np.abs(W).max() == 1.0 - 2.0 ** -53 and bad == 0.0
    W, mx, bad = R.scale_ref(cases["zeros"])
    assert mx == 0.0 and np.array_equal(_bits(W), _bits(cases["zeros"])) and np.signbit(W[1, 2])
    assert cases["many_blocks"].size > 1024 * 2048 and R.absmax_blocks(cases["many_blocks"].size) == 1024
    X = base.copy()
    X[3, 3] = np.nan
    X[0, 0] = np.inf
    W, mx, bad = R.scale_ref(X)
    assert bad == 1.0 and mx == np.abs(base[np.isfinite(X)]).max()


# ---------------------------------------------------------------------------------------------------------------------------
# finish
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.FINISH_M)
def test_finish_inputs_hold_what_the_gpu_test_needs(m):
    onlys = range(len(R.FINISH_PATTERNS)) if m == 1 else (None,)
    seen = {}
    for only in onlys:
        W, perm, sigma, planted = R.finish_input(m, only)
        ncols = W.shape[1]
        assert sorted(perm) == list(range(m)) and (m == 1 or not np.array_equal(perm, np.arange(m)))
        sig = R.lead_ref(W, perm, sigma, m)
        out, nnz = R.write_ref(W, perm, sig, m, R.DROPTOL)
        for name, k in planted.items():
            row = W[perm[k]]
            seen[name] = True
            if name.startswith("tie"):
                a, b = dict(R.FINISH_PATTERNS)[name]
                ca, cb = a[0] % ncols, b[0] % ncols
                assert row[ca] == -row[cb] and abs(row[ca]) == np.abs(row).max() and np.count_nonzero(np.abs(row) == abs(row[ca])) == 2
                assert (sig[k] < 0) == (row[min(ca, cb)] < 0)  # the smaller column decides
                assert (ca % 256 != cb % 256) or name == "tie_first_last"  # two threads of the 256 hold the pair
            elif name == "last_column":
                assert R.lead_index(row[None])[0] == ncols - 1 and sig[k] == -sigma[k]
            elif name == "zero_row":
                assert not row.any() and sig[k] == sigma[k] and not _bits(out[k]).any()
            else:
                t0, up, down = R.drop_targets()
                assert sig[k] == sigma[k] and down < t0 < up
                c0, c1, c2 = (c % ncols for c in R.DROP_COLS)
                q = row / sig[k]
                assert (q[c0], q[c1], q[c2]) == (t0, -up, down)
                assert _bits(out[k, [c0, c2]]).tolist() == [0, 0] and out[k, c1] == -up
        assert nnz == np.count_nonzero(out) and nnz < out.size
        if W.any():  # (m = 1 with the zero row: nothing else is there)
            assert nnz > 0 and np.any((out == 0) & (W[perm] != 0))  # the drop rule removes something
    assert len(seen) == len(R.FINISH_PATTERNS)  # every pattern sits in a kept row at r = m


def test_lead_and_write_references():
    W = np.array([[1.0, -3.0, 3.0, 0.5], [0.0, -0.0, 0.0, 0.0], [-2.0, 2.0, 1e-9, -1e-9]])
    assert R.lead_index(W).tolist() == [1, 0, 0]
    perm, sigma = np.array([2, 0, 1], dtype=np.int32), np.array([2.0, 3.0, 5.0])
    sig = R.lead_ref(W, perm, sigma, 3)
    assert sig.tolist() == [-2.0, -3.0, 5.0]
    out, nnz = R.write_ref(W, perm, sig, 2, 1e-9)
    assert out[0].tolist() == [1.0, -1.0, 0.0, 0.0] and out[1].tolist() == [-1.0 / 3.0, 1.0, -1.0, 0.5 / -3.0] and nnz == 6
    assert not _bits(out[2]).any() and not _bits(out[0, 2:]).any()  # +0.0, never -0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the driver's inputs
# ---------------------------------------------------------------------------------------------------------------------------
def test_driver_inputs(problems, golden):
    cases = CR.inputs(problems, golden)
    mats = {name: CR.stack(*cases[name][:2]) for name in ("graded_6x37", "duplicates_6x70")}
    mats["rows_70x300"] = R.rows_70x300()
    for name, M in mats.items():
        for k in (900, -900):
            S = np.ldexp(M, k)
            assert np.isfinite(S).all() and np.array_equal(_bits(np.ldexp(S, -k)), _bits(M)), name  # ldexp(ldexp(M, k), -k) == M
            assert np.array_equal(_bits(R.scale_ref(S)[0]), _bits(R.scale_ref(M)[0])), name  # W after the scale copy is the same
        assert CR.rank_is_unambiguous(CR.reference(M)[0]), name
    Mi = CR.stack(*cases["integer_9x5"][:2])
    D = np.ldexp(Mi, -1070)
    assert np.array_equal(np.ldexp(D, 1070), Mi) and np.abs(D).max() < np.finfo(np.float64).tiny
    s, r, _ = CR.reference(Mi)
    assert r == 5 and CR.rank_is_unambiguous(s)
    for m, ncols, rank, seed in R.MORE_ROWS:
        M = R.more_rows(m, ncols, rank, seed)
        s, r, rows = CR.reference(M)
        assert M.shape == (m, ncols) and r == rank and CR.rank_is_unambiguous(s)
        assert CR.orth(rows) <= 1e-14 and CR.resid(M, rows) <= 1e-14
