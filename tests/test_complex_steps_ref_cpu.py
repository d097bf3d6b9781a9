"""The references of tests/test_gpu_complex_steps.py (tests/complex_steps_ref.py) checked without a GPU: every Hermitian family has
the spectrum it declares, every restatement agrees with a second, independent wording, and a float64 NumPy evaluation of each
formula lies inside the restatement's own running error bound on every input the GPU tests use -- the bounds are judged here, on
the reference, never on a kernel."""
import numpy as np
import pytest

import complex_steps_ref as R
import module_kernels_ref as MR
import syev_families as fam

ALL_HEEV_CASES = sorted(set(R.heev0_cases()) | {c for n in R.HEEV1_ORDERS for c in R.heev1_cases(n)})


def test_families_have_the_declared_spectrum():
    """H is Hermitian bit for bit; LAPACK's Hermitian spectrum of H is the reference spectrum (for a phased or real family: LAPACK's
    real spectrum of A) to 2e-14 |H|, a tenth of the eigenvalue bound of the GPU tests; the planes that should vanish do; the
    constructed spectra are the declared ones."""
    assert {name.split(" ", 1)[1] for name, _ in ALL_HEEV_CASES if name.split(" ", 1)[0] in ("phased", "real")} == set(fam.FAMILIES)
    for own in R.OWN:
        assert any(name == own for name, _ in ALL_HEEV_CASES), own
    worst = 0.0
    for name, n in ALL_HEEV_CASES:
        H, wl, sc = R.hermitian(name, n)
        assert H.shape == (n, n) and wl.shape == (n,) and np.array_equal(H, H.conj().T) and not H.diagonal().imag.any(), (name, n)
        assert np.all(np.diff(wl) >= 0) and sc == (np.abs(wl).max() or 1.0)
        dev = float(np.abs(np.linalg.eigvalsh(H) - wl).max() / sc)
        worst = max(worst, dev)
        assert dev <= 2e-14, (name, n, dev)
        if name.startswith("real "):
            assert not H.imag.any() and np.array_equal(H.real, (fam.matrix(name[5:], n) + fam.matrix(name[5:], n).T) / 2)
        if name.startswith("phased ") and n >= 3 and name[7:] in ("random symmetric", "rank one, ones"):
            assert np.abs(H.imag).max() > 1e-3 * sc  # complex off-diagonal entries
        if name == "imaginary antisymmetric":
            assert not H.real.any()
            assert np.abs(wl + wl[::-1]).max() <= 1e-14 * sc  # symmetric about 0 ...
            assert n % 2 == 0 or abs(wl[n // 2]) <= 1e-14 * sc  # ... with a zero eigenvalue at odd n
        if name.startswith("unitary"):
            vals = np.sort(np.resize(R.TWO_VALUES if "two" in name else R.FIVE_VALUES, n))
            assert np.abs(wl - vals).max() <= 1e-13, (name, n)
        if name.startswith("driver"):
            L = R.driver_labels(name, n)
            v = MR.class_uniform(R.DRIVER_KEY, np.arange(n * n + 1)) + 1j * MR.class_uniform(R.DRIVER_KEY ^ R.IM_KEY, np.arange(n * n + 1))
            A = v[L]
            assert np.array_equal(H, A + A.conj().T) and (n < 3 or np.abs(H.imag).max() > 0), (name, n)
    print("largest |eigvalsh(H) - reference spectrum| / |H| = %.2e" % worst)


def test_projector_cases_have_well_separated_spectra():
    """residual bound / smallest gap < 1e-6 on every case whose spectral projectors the GPU test compares between the routes"""
    cases = R.projector_cases()
    assert {n for _, n in cases} == {n for n in R.HEEV1_ORDERS if n <= 64} and {name for name, _ in cases} == set(R.LOW_MULTIPLICITY)
    for name, n in cases:
        sc = R.hermitian(name, n)[2]
        assert R.HEEV_BOUNDS[1] * sc / R.smallest_gap(name, n) < R.PROJECTOR_QUOTIENT, (name, n)


def test_heev_case_lists():
    """what the case lists must contain: every order 1..64 on route 0, every family at the listed orders, the extreme scales only
    on route 0"""
    c0 = R.heev0_cases()
    assert {n for _, n in c0} == set(range(1, 65)) and len(set(c0)) == len(c0)
    for n in (1, 2, 3, 4, 5, 7, 8, 16, 17, 33, 34, 63, 64):
        assert {name for name, m in c0 if m == n} == set(R.names(n)), n
    assert any(R.is_extreme(name) for name, _ in c0) and ("driver C3", 3) in c0 and ("driver S3", 6) in c0
    assert R.HEEV1_ORDERS == (1, 2, 33, 64, 65, 96, 127, 128, 129, 200)
    for n in R.HEEV1_ORDERS:
        got = {name for name, _ in R.heev1_cases(n)}
        assert got == {name for name in R.names(n) if not R.is_extreme(name)} and len(R.names(n)) - len(got) == 4


@pytest.mark.parametrize("n", R.GATHER_ORDERS)
def test_gather_restatement(n):
    """the labels are non-symmetric with zeros; the planes are those of A + A^H from a table of the class values, and entry by entry
    at the small orders"""
    L, d = R.gather_labels(n)
    Lm = L.reshape(n, n, order="F")
    assert L.dtype == np.uint32 and int(L.max()) <= d and (n < 2 or ((L == 0).any() and not np.array_equal(Lm, Lm.T)))
    for key in R.GATHER_KEYS:
        Hr, Hi = R.gather_herm(n, L, key)
        table = MR.class_uniform(key, np.arange(d + 1)) + 1j * MR.class_uniform(key ^ 0xA5A5A5A55A5A5A5A, np.arange(d + 1))
        A = table[Lm.astype(np.int64)]
        H = A + A.conj().T
        assert np.array_equal(Hr.view(np.uint64), np.ascontiguousarray(H.real).view(np.uint64))
        assert np.array_equal(Hi.view(np.uint64), np.ascontiguousarray(H.imag).view(np.uint64))
        if n <= 17:
            for r in range(n):
                for c in range(n):
                    a, b = table[int(L[r + c * n])], table[int(L[c + r * n])]
                    assert Hr[r, c] == a.real + b.real and Hi[r, c] == a.imag - b.imag


def _norm_inputs(n):
    return (("integers", R.gaussian_integers(n, 3)), ("random", R.random_complex(n, 3)))


@pytest.mark.parametrize("n", R.NORM_ORDERS[1])
def test_block_norms_restatement_and_bound(n):
    """the long-double norms against (1) entry-by-entry bilinear forms, (2) the exact integers; the float64 evaluation inside the
    bound"""
    for kind, (H, V) in _norm_inputs(n):
        for pname, space_of in R.partitions(n).items():
            neig = int(space_of.max()) + 1
            ref, bound = R.block_norms(H, V, space_of, neig)
            assert ref.shape == bound.shape == (neig, neig)
            f64, _ = R.block_norms(H, V, space_of, neig, dtype=np.complex128)
            assert (np.abs(f64.astype(np.longdouble) - ref) <= bound).all(), (n, kind, pname)
            assert bound.max() <= 1e-6 * float(ref.max())  # the bound means something at the scale of the norms
            if kind == "integers":
                sq = R.block_norms_exact(H, V, space_of, neig)
                assert np.array_equal(np.rint(ref * ref).astype(np.int64), sq), (n, pname)
            if n <= 33:  # second wording: one bilinear form per entry, maxima by loops
                Hl, Vl = H.astype(R.CLD), V.astype(R.CLD)
                want = np.zeros((neig, neig), dtype=R.LD)
                for a in range(n):
                    for b in range(n):
                        g = np.sum(np.conj(Vl[:, a])[:, None] * Hl * Vl[:, b][None, :])
                        want[space_of[a], space_of[b]] = max(want[space_of[a], space_of[b]], abs(g))
                assert np.allclose(ref.astype(np.float64), want.astype(np.float64), rtol=1e-14, atol=0), (n, kind, pname)


def test_block_norms_exact_against_python_integers():
    for n in (1, 2, 5):
        for hermitian in (True, False):
            H, V = R.gaussian_integers(n, 3)
            if not hermitian:
                H = np.triu(H) + 2 * np.tril(H, -1)
            space_of = R.partitions(n)["n spaces"]
            sq = R.block_norms_exact(H, V, space_of, n)
            for a in range(n):
                for b in range(n):
                    g = sum(complex(V[k, a]).conjugate() * complex(H[k, l]) * complex(V[l, b]) for k in range(n) for l in range(n))
                    assert int(sq[a, b]) == int(round(g.real)) ** 2 + int(round(g.imag)) ** 2


@pytest.mark.parametrize("n", R.IRREDUCIBLE_BOTH + R.IRREDUCIBLE_GENERAL)
def test_irreducible_restatement_and_bound(n):
    """the case is well made (shapes of the issue, a safe atol that clamps); the float64 evaluation lies inside the bound and
    clamps the same entries; at the small orders the columns agree with the projector wording  P_j H q_i1 / |Q_i^H H q_j1|"""
    H, V, desc, atol, ref, bound, mask = R.irreducible_case(n)
    rows = [tuple(int(x) for x in r) for r in desc]
    assert sorted(r[5] for r in rows) == list(range(len(rows))) and any(r[0] == 0 for r in rows)
    shapes = {(r[2], r[4]) for r in rows if r[0] == 1}
    if n in R.IRREDUCIBLE_BOTH or n == 65:
        assert {s for s in ((1, 1), (2, 3), (3, 2), (n // 2, n // 2)) if s[0] + s[1] <= n} <= shapes
    elif n == 600:
        assert shapes == {(257, 300), (300, 257)}
    else:
        assert shapes == {(2, 3), (3, 2)} and len(rows) == 3
    assert mask.any() and not mask.all() and not ref[mask].any() and (np.abs(ref[~mask]) >= atol).all()
    q64, _, _ = R.irreducible(H, V, rows, atol, dtype=np.complex128)
    c64, m64, _ = R.clamp(q64, bound, atol)
    assert np.array_equal(m64, mask)
    assert (np.abs(c64.real - ref.real) <= bound).all() and (np.abs(c64.imag - ref.imag) <= bound).all()
    kind0 = [r for r in rows if r[0] == 0]
    for r in kind0:
        assert np.array_equal(ref[:, r[5]][~mask[:, r[5]]], V[:, r[1]][~mask[:, r[5]]])
    if n <= 65:
        Hl, Vl = H.astype(R.CLD), V.astype(R.CLD)
        for kind, i0, mi, j0, mj, col in rows:
            if kind == 1:
                Qi, Qj = Vl[:, i0:i0 + mi], Vl[:, j0:j0 + mj]
                y = ((Qj @ Qj.conj().T) @ Hl) @ Vl[:, i0]
                want = (y / np.linalg.norm((Hl @ Vl[:, j0]).conj() @ Qi)).astype(np.complex128)
                want[np.abs(want) < atol] = 0
                assert np.allclose(ref[:, col], want, rtol=0, atol=1e-14), (n, col)
