"""The pair check of the loop's guessed initial partition (csrc/kernels_class_compare.hip: class_compare_kernel with ChkPair), driven on made-up
inputs through libsdpsr_prof.so (sdpsr_profile_verify_pair).

The check answers "would the refinement of the value pairs (a, b) over the packed lower triangle write these labels and these
representatives again?" with one word: 0 exactly when it would.  The reference is a NumPy restatement of that refinement: group the
packed entries by the pair of bit patterns, number the groups by first occurrence in packed order (the group of (+0.0, +0.0) is
label 0), and compare labels and first occurrences with what was handed in.  Labels are canonical (a refinement made them), every
class has at least two entries, so a change at ONE entry always changes the partition: each needle alone must raise the word.

Sizes: n = 57 (one ragged trip per column, fewer columns than workgroups) and 256 (every thread of a workgroup busy in the first
column); d = 1, 34 and the cap of the one-launch form, one more is refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 256  # VERIFY_LDS_CAP
BAD_ARGUMENT = 5


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _col_off(n, j):
    return j * n - j * (j - 1) // 2


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _packed(n, M):
    """The lower triangle of the n x n matrix M[row, column], column by column."""
    return np.concatenate([M[j:, j] for j in range(n)])


def _refine_reference(pa, pb):
    """Canonical labels and first occurrences of the pairs of bit patterns, in packed order; (+0.0, +0.0) is label 0."""
    ka, kb = _bits(pa), _bits(pb)
    key = np.stack([ka, kb], axis=1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    zero = (ka[first] == 0) & (kb[first] == 0)
    order = np.argsort(first[~zero], kind="stable")
    lab_of_group = np.zeros(len(first), dtype=np.uint32)
    lab_of_group[np.flatnonzero(~zero)[order]] = np.arange(1, len(order) + 1, dtype=np.uint32)
    return lab_of_group[inv], np.sort(first[~zero]).astype(np.uint32)


def _would_reproduce(n, a, b, Lp, first):
    lab, fi = _refine_reference(_packed(n, a), _packed(n, b))
    return np.array_equal(lab, Lp) and np.array_equal(fi, first)


def _case(n, d, with_zero, seed):
    """Canonical packed labels of d classes (plus label 0 when with_zero), each of at least two entries, and symmetric-by-construction
    a, b (only the lower triangle is meaningful: the strict upper triangle holds NaNs nobody may read) whose value pairs are
    constant on the classes and distinct between them -- while neither a nor b alone tells the classes apart."""
    rng = np.random.default_rng(seed)
    npk = n * (n + 1) // 2
    groups = d + (1 if with_zero else 0)
    assert npk >= 2 * groups
    g = np.concatenate([np.repeat(np.arange(groups), 2), rng.integers(0, groups, size=npk - 2 * groups)])
    g = g[rng.permutation(npk)]  # group 0 is the zero class when with_zero
    # distinct pairs from few distinct values per operand
    side = int(np.ceil(np.sqrt(groups + 4)))
    va_pool = np.concatenate([[0.0, -0.0], rng.standard_normal(side)])
    vb_pool = np.concatenate([[0.0, 1.5], rng.standard_normal(side)])
    pairs = [(i, k) for i in range(len(va_pool)) for k in range(len(vb_pool)) if not (i == 0 and k == 0)]
    pick = rng.permutation(len(pairs))[:groups]
    va = np.array([va_pool[pairs[p][0]] for p in pick])
    vb = np.array([vb_pool[pairs[p][1]] for p in pick])
    if with_zero:
        va[0], vb[0] = 0.0, 0.0
    pa, pb = va[g], vb[g]
    Lp, first = _refine_reference(pa, pb)
    assert int(Lp.max()) == d and len(first) == d and (Lp == 0).any() == with_zero
    a = np.full((n, n), np.nan)
    b = np.full((n, n), np.nan)
    for j in range(n):
        a[j:, j] = pa[_col_off(n, j):_col_off(n, j) + n - j]
        b[j:, j] = pb[_col_off(n, j):_col_off(n, j) + n - j]
    return Lp, first, a, b


_IJ = {}


def _ij(n, e=None):
    """(row, column) of packed index e (all packed indices when e is None)."""
    if n not in _IJ:
        cols = np.arange(n)
        _IJ[n] = (np.concatenate([np.arange(j, n) for j in range(n)]), np.repeat(cols, n - cols))
    ii, jj = _IJ[n]
    return (ii, jj) if e is None else (int(ii[e]), int(jj[e]))


def _run(pkg, ctx, n, d, Lp, first, a, b):
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint32 * 2)()
    af, bf = np.asfortranarray(a), np.asfortranarray(b)
    ctx.check(prof.sdpsr_profile_verify_pair(ctx._h, n, d, _vp(Lp), _vp(first), _vp(af), _vp(bf), out))
    return int(out[0]), int(out[1])


def _flip(M, i, j):
    M = M.copy()
    v = _bits(M[i, j]).copy()
    v ^= np.uint64(1)
    M[i, j] = v.view(np.float64)[0]
    return M


def _needles(n, d, with_zero, Lp, first, a, b):
    """name -> (a, b) that differ from the case at one place (or one class) each."""
    npk = n * (n + 1) // 2
    out = {"last_entry": (a, _flip(b, n - 1, n - 1)), "last_row_first_column": (a, _flip(b, n - 1, 0))}
    assert _col_off(n, n - 1) == npk - 1
    ri, rj = _ij(n, int(first[d // 2]))
    out["representative"] = (a, _flip(b, ri, rj))
    cls = d  # a whole non-zero class to (+0.0, +0.0)
    a5, b5 = a.copy(), b.copy()
    ii, jj = _ij(n)
    a5[ii[Lp == cls], jj[Lp == cls]] = 0.0
    b5[ii[Lp == cls], jj[Lp == cls]] = 0.0
    out["class_all_zero"] = (a5, b5)
    if d >= 2:  # class d takes the pair of class 1: the representatives are not distinct
        i1, j1 = _ij(n, int(first[0]))
        a6, b6 = a.copy(), b.copy()
        a6[ii[Lp == d], jj[Lp == d]] = a[i1, j1]
        b6[ii[Lp == d], jj[Lp == d]] = b[i1, j1]
        out["two_classes_one_pair"] = (a6, b6)
    if with_zero:
        z = np.flatnonzero(Lp == 0)
        i, j = _ij(n, int(z[len(z) // 2]))
        a4 = a.copy()
        a4[i, j] = -0.0
        out["negative_zero_in_zero_class"] = (a4, b)
        i, j = _ij(n, int(z[-1]))
        b7 = b.copy()
        b7[i, j] = 2.5
        out["label_zero_entry_non_zero"] = (a, b7)
    return out


@pytest.fixture(scope="module")
def cases():
    """Built once: (n, d, with_zero) -> case; nothing modifies them (the needles copy)."""
    return {(n, d, z): _case(n, d, z, seed=1000 * n + 2 * d + z) for n in (57, 256) for d in (1, 34, CAP) for z in (False, True)}


@pytest.mark.parametrize("with_zero", [False, True], ids=["no_zero_class", "zero_class"])
@pytest.mark.parametrize("d", [1, 34, CAP])
@pytest.mark.parametrize("n", [57, 256])
def test_unchanged_inputs_pass_and_every_needle_alone_is_found(pkg, gpu_ctx, cases, n, d, with_zero):
    Lp, first, a, b = cases[(n, d, with_zero)]
    assert _would_reproduce(n, a, b, Lp, first)
    verdict, cap = _run(pkg, gpu_ctx, n, d, Lp, first, a, b)
    assert cap == CAP
    assert verdict == 0, (n, d, with_zero)
    needles = _needles(n, d, with_zero, Lp, first, a, b)
    assert len(needles) == 4 + (d >= 2) + 2 * with_zero
    for name, (an, bn) in needles.items():
        assert not _would_reproduce(n, an, bn, Lp, first), name  # (the reference agrees that the partition has changed)
        assert _run(pkg, gpu_ctx, n, d, Lp, first, an, bn)[0] != 0, (n, d, with_zero, name)


def test_more_classes_than_the_cap_are_refused(pkg, gpu_ctx):
    n, d = 57, CAP + 1
    Lp, first, a, b = _case(n, d, False, seed=5)
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint32 * 2)(7, 7)
    af, bf = np.asfortranarray(a), np.asfortranarray(b)
    assert prof.sdpsr_profile_verify_pair(gpu_ctx._h, n, d, _vp(Lp), _vp(first), _vp(af), _vp(bf), out) == BAD_ARGUMENT
    assert int(out[0]) == 7  # nothing ran
