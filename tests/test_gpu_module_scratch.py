"""The module growth without whole-buffer fills, scratch matrix, copy or glue launches (csrc/compress.cpp, DESIGN.md "module
scratch"): whatever the small-module route reads it has written in the same call, the row-owning tall product may write behind
the basis it reads, the lift stores Q_hat clamped in both layouts, the seed is one launch -- each bit for bit what the separate
launches under SDPSR_FLAG_MODULE_SCRATCH_FILLS give.  Correctness against the recorded table stays with test_gpu_module_paths.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = 0x7FF8C0FFEE0DD5ED   # what no kernel may touch (a NaN: it also shows in any sum it enters)
POISON = 0x7FF8BADC0DEBAD00  # padding a kernel may not read
BAD_ARGUMENT = 5


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _fill(count, pattern=SENT):
    return np.full(int(count), pattern, dtype=np.uint64).view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a, pattern=SENT):
    return bool((_bits(a) == np.uint64(pattern)).all())


def _round_up(x, m):
    return -(-x // m) * m


@pytest.fixture(scope="module")
def prof(pkg, gpu_ctx):
    return pkg._lib.load_prof_library()


@pytest.fixture(scope="module")
def ctx_pair(pkg):
    """(default ctx, ctx under SDPSR_FLAG_MODULE_SCRATCH_FILLS): the kernel entries run the form the ctx's flags choose"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, b = pkg.Context(seed=1), pkg.Context(seed=1, flags=pkg._lib.FLAG_MODULE_SCRATCH_FILLS)
    yield a, b
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# poison: nothing of the scratch is read before the call at hand has written it
# ---------------------------------------------------------------------------------------------------------------------------
def _commutative(pr, n):
    """circulant (x) K, permuted: m k = n with (m // 2 + 1) * 2 <= 40 classes"""
    m = {520: 20, 1024: 32, 1030: 10}[n]
    L = pr.kron_labels(pr.symmetric_circulant_labels(m), pr.complete_scheme_labels(n // m))
    L, d = pr.canonical_labels(pr.permute_labels(L, 3))
    assert d <= 40
    return L.astype(np.uint32), d


def _er3_product(pr, golden, n):
    """golden ER(3) (13 points, dim 12, blocks up to 3 x 3: not commutative) (x) K_{n / 13}"""
    L, d = pr.kron_with_complete(golden["er3_P"], n // 13, seed=5)
    assert L.shape[0] == n and d == 24
    return np.asarray(L).astype(np.uint32), d


# The three orders of the commutative instance: ld = 640, ld == n, ld = 1152.  13 divides none of 1024 and 1030, so the ER(3)
# product runs at the same three kinds of order instead: 520 (ld 640), 1664 (ld == n) and 1027 (ld 1152).
POISON_CASES = [("circ", 520), ("circ", 1024), ("circ", 1030), ("er3", 520), ("er3", 1664), ("er3", 1027)]


def _two_calls(pkg, prof, L, d, flags, poison):
    with pkg.Context(seed=11, eig_driver=6, flags=flags) as ctx:
        first = pkg.blockDiagonalize(pkg.Partition(d, L), ctx=ctx, retries=1)
        if poison:
            ctx.check(prof.sdpsr_profile_poison_scratch(ctx._h))
        second = pkg.blockDiagonalize(pkg.Partition(d, L), ctx=ctx, retries=1)
        cur = C.c_int32(-1)
        ctx.check(prof.sdpsr_profile_qrm_current(ctx._h, C.byref(cur)))
    out = []
    for bd in (first, second):
        out.append(([int(s) for s in bd.blkSizes], _bits(np.hstack([np.asarray(q) for q in bd.Q_hat])).copy(),
                    [_bits(np.asarray(b)).copy() for row in bd.blks for b in row]))
    return out, cur.value


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("kind,n", POISON_CASES)
def test_second_call_reads_nothing_the_first_left(pkg, problems, golden, prof, kind, n):
    """Two fresh contexts with one seed: two calls of blockDiagonalize (sdpsr_block_diagonalize + sdpsr_block_images), and the
    same two calls with every "cm_*" buffer and "bd_qrm" filled with NaN in between.  The second calls agree bit for bit in
    Q_hat, block sizes and images -- with flag 0 and under SDPSR_FLAG_MODULE_SCRATCH_FILLS, and the two flags agree with each
    other in both calls.  The commutative instance is complete after the class sums (one orthogonalisation step), the ER(3)
    product needs growth rounds behind the class sums (dim <S> x = 34 > dim S = 24), whose pivot ratios keep the second step
    (compress.cpp, Module::absorb)."""
    L, d = _commutative(problems, n) if kind == "circ" else _er3_product(problems, golden, n)
    res = {}
    for flags in (0, pkg._lib.FLAG_MODULE_SCRATCH_FILLS):
        clean, cur0 = _two_calls(pkg, prof, L, d, flags, poison=False)
        dirty, cur1 = _two_calls(pkg, prof, L, d, flags, poison=True)
        assert not np.isnan(dirty[1][1].view(np.float64)).any()
        assert _same(clean[0], dirty[0]) and _same(clean[1], dirty[1]), (kind, n, flags)
        assert cur0 == cur1 == (0 if flags else 1)  # the lift left the row-major copy; under the flag block_images makes it
        res[flags] = clean
    a, b = res[0], res[pkg._lib.FLAG_MODULE_SCRATCH_FILLS]
    assert _same(a[0], b[0]) and _same(a[1], b[1]), (kind, n)
    assert sum(s * (s + 1) // 2 for s in a[1][0]) == d
    assert (max(a[1][0]) > 1) == (kind == "er3")


# ---------------------------------------------------------------------------------------------------------------------------
# the stacked product written in place
# ---------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _ordered_fma_rows(In, S, rows):
    """out[r, c] = fma(In[r, kk-1], S[kk-1, c], ... fma(In[r, 0], S[0, c], 0.0)) for the given rows: the kernel's order over t"""
    out = np.zeros((len(rows), S.shape[1]))
    for a, r in enumerate(rows):
        for c in range(S.shape[1]):
            acc = 0.0
            for t in range(In.shape[1]):
                acc = _fma(float(In[r, t]), float(S[t, c]), acc)
            out[a, c] = 0.0 + acc
    return out


@pytest.fixture(scope="module")
def stacked_inputs():
    """(n, kk) -> In (n x kk), S (kk x 64), the ordered-fma reference of a few rows: made once, left alone"""
    cache = {}

    def get(n, kk):
        if (n, kk) not in cache:
            rng = np.random.default_rng(1000 * n + kk)
            In, S = rng.standard_normal((n, kk)), rng.standard_normal((kk, 64))
            rows = sorted({0, n // 2, n - 1})
            cache[(n, kk)] = (In, S, rows, _ordered_fma_rows(In, S, rows))
        return cache[(n, kk)]

    return get


def _stacked(prof, ctx, n, ldi, kk, ncols, w, In, S):
    mcols = max(kk, w + ncols) + 2  # two sentinel columns behind everything
    lds, guard = kk + 3, 7
    M = _fill(ldi * mcols + guard)
    Mv = M[:ldi * mcols].reshape(mcols, ldi)
    Mv[:kk, :n] = In.T
    Sh = _fill(lds * ncols, POISON)
    Sh.reshape(ncols, lds)[:, :kk] = S[:, :ncols].T
    rep = (C.c_int32 * 1)(-1)
    ctx.check(prof.sdpsr_profile_stacked_in_place(ctx._h, n, ldi, kk, lds, ncols, w, mcols, _vp(M), _vp(Sh), guard, rep))
    return Mv, M[ldi * mcols:], rep[0]


@pytest.mark.parametrize("n", [5, 63, 64, 65, 1030])
def test_stacked_product_in_place(prof, ctx_pair, stacked_inputs, n):
    """M[:, w : w + ncols) = M[:, 0 : kk) S with the output inside the matrix that is read (w < kk: the new columns overwrite
    columns the product reads, as [W V] S overwrites V).  Bit for bit the ordered-fma sums, and bit for bit what the
    column-split kernel gives through a scratch matrix; rows >= n, the columns outside [w, w + ncols) that are not input, and
    the guard come back as they went in."""
    lean, parent = ctx_pair
    ldi = _round_up(n, 128)
    for kk in (2, 35, 69):
        In, S, rows, ref = stacked_inputs(n, kk)
        for ncols in (1, 8, 9, 34, 64):
            for w in (1, 35):
                where = (n, kk, ncols, w)
                got, guard, form = _stacked(prof, lean, n, ldi, kk, ncols, w, In, S)
                old, _, form_old = _stacked(prof, parent, n, ldi, kk, ncols, w, In, S)
                assert form == 1 and form_old == 0, where
                out = got[w:w + ncols, :n]
                assert np.array_equal(_bits(out[:, rows].T), _bits(ref[:, :ncols])), where
                assert np.array_equal(_bits(out), _bits(old[w:w + ncols, :n])), where
                assert _untouched(got[:, n:]) and _untouched(guard), where
                owned = [t for t in range(got.shape[0]) if w <= t < w + ncols]
                keep = [t for t in range(kk) if t not in owned]  # input columns the product does not own
                rest = [t for t in range(kk, got.shape[0]) if t not in owned]  # neither input nor output
                assert np.array_equal(_bits(got[keep, :n]), _bits(In.T[keep])), where
                assert len(rest) >= 2 and _untouched(got[rest]), where


def test_stacked_product_wider_than_the_form_runs_the_old_kernel(prof, ctx_pair, stacked_inputs):
    lean, parent = ctx_pair
    n, kk, w = 65, 69, 1
    In, _, _, _ = stacked_inputs(n, kk)
    S = np.random.default_rng(5).standard_normal((kk, 65))
    a, _, form_a = _stacked(prof, lean, n, 128, kk, 65, w, In, S)
    b, _, form_b = _stacked(prof, parent, n, 128, kk, 65, w, In, S)
    assert form_a == 0 and form_b == 0
    assert np.array_equal(_bits(a), _bits(b))
    ref = _ordered_fma_rows(In, S[:, 64:], [0, n - 1])
    assert np.array_equal(_bits(a[w + 64, [0, n - 1]]), _bits(ref[:, 0]))


# ---------------------------------------------------------------------------------------------------------------------------
# the lift
# ---------------------------------------------------------------------------------------------------------------------------
def _lift(prof, ctx, n, ldi, kk, S1, atol, In, S):
    lds, guard = kk + 1, 5
    Inh = _fill(ldi * kk, POISON)
    Inh.reshape(kk, ldi)[:, :n] = In.T
    Sh = _fill(lds * S1, POISON)
    Sh.reshape(S1, lds)[:, :kk] = S.T
    Qcm, Qrm = _fill(n * S1 + guard), _fill(n * S1 + guard)
    ctx.check(prof.sdpsr_profile_lift(ctx._h, n, ldi, kk, lds, S1, atol, _vp(Inh), _vp(Sh), _vp(Qcm), _vp(Qrm), guard))
    assert _untouched(Qcm[n * S1:]) and _untouched(Qrm[n * S1:])
    return Qcm[:n * S1].reshape(S1, n), Qrm[:n * S1].reshape(n, S1)


@pytest.mark.parametrize("S1", [1, 7, 34])
def test_lift_clamps_and_writes_both_layouts(prof, ctx_pair, S1):
    """Q_hat = clamp(W Q_small): the column-major output equals product-then-clamp bit for bit on products that straddle
    atol -- rows of W that select one coefficient each put -atol/2, +-atol, +-atol(1 -+ eps), -0.0 and denormals into the
    product exactly --, and the row-major copy is its exact transpose."""
    lean, parent = ctx_pair
    atol = 1e-9
    n, kk = 130, 9
    rng = np.random.default_rng(S1)
    In, S = rng.standard_normal((n, kk)), rng.standard_normal((kk, S1))
    special = [-atol / 2, atol / 2, atol, -atol, np.nextafter(atol, 0), -np.nextafter(atol, 0), np.nextafter(atol, 1), -0.0, 0.0, 5e-324, -1e-300]
    m = len(special)
    for r in range(m):  # rows 0 .. m-1 of W = e_0 and S[0, c] = special[c % m]: the product is that value itself
        In[r] = 0.0
        In[r, 0] = 1.0
    S[0, :] = [special[c % m] for c in range(S1)]
    for r, v in enumerate(special):  # rows 64 ..: W[64 + r, :] = v e_1 and S[1, c] = 1: the product is v in every column
        In[64 + r] = 0.0
        In[64 + r, 1] = v
    S[1, :] = 1.0
    cm, rm = _lift(prof, lean, n, 256, kk, S1, atol, In, S)
    cm_old, rm_old = _lift(prof, parent, n, 256, kk, S1, atol, In, S)
    assert np.array_equal(_bits(cm), _bits(cm_old)) and np.array_equal(_bits(rm), _bits(rm_old))
    assert np.array_equal(_bits(rm), _bits(cm.T))
    want = np.array([0.0 if abs(v) < atol else 0.0 + v for v in special])  # (+0.0 where clamped, bit for bit)
    for c in range(S1):
        assert np.array_equal(_bits(cm[c, :m]), _bits(np.full(m, want[c % m]))), c
        assert np.array_equal(_bits(cm[c, 64:64 + m]), _bits(want)), c
    assert (np.abs(cm) >= atol).any() and not np.signbit(cm[cm == 0]).any()


def test_lift_entry_refuses_more_columns_than_the_form(prof, ctx_pair):
    lean, _ = ctx_pair
    a = np.zeros(1 << 16)
    assert prof.sdpsr_profile_lift(lean._h, 8, 8, 4, 4, 65, 1e-9, _vp(a), _vp(a), _vp(a), _vp(a), 0) == BAD_ARGUMENT


def test_row_major_copy_is_void_after_a_dense_driver_call(pkg, problems, golden, prof):
    """The validity bit: set by the module lift, cleared by a call on the same ctx whose Q_hat the dense driver writes
    (n = 31 < 512: no module compression) -- whose images are then the ones a fresh ctx gives."""
    L, d = _commutative(problems, 1024)
    er5 = golden["er5_P"].astype(np.uint32)
    cur = C.c_int32(-1)
    with pkg.Context(seed=5) as ctx:
        pkg.blockDiagonalize(pkg.Partition(d, L), ctx=ctx, retries=1)
        ctx.check(prof.sdpsr_profile_qrm_current(ctx._h, C.byref(cur)))
        assert cur.value == 1
        bd = pkg.blockDiagonalize(pkg.Partition(15, er5), ctx=ctx, retries=1)
        ctx.check(prof.sdpsr_profile_qrm_current(ctx._h, C.byref(cur)))
        assert cur.value == 0
        for i, row in enumerate(bd.blks, start=1):  # blks == Q_k' 1[P == i] Q_k: the transpose ran on this Q_hat
            for Qk, b in zip(bd.Q_hat, row):
                assert np.allclose(np.asarray(b), np.asarray(Qk).T @ (er5 == i) @ np.asarray(Qk), atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------------
# the seed
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1024, 1030, 4099])
def test_seed_in_one_launch(prof, ctx_pair, n):
    """x, x / |x| and |x| bit for bit as random_vector + normalize_columns give them; nothing written behind n."""
    lean, parent = ctx_pair
    res = []
    for ctx in (lean, parent):
        x, h, nrm = _fill(n + 9), _fill(n + 9), _fill(1 + 9)
        ctx.check(prof.sdpsr_profile_seed_vector(ctx._h, n, C.c_uint64(0x1234ABCD5678 + n), _vp(x), _vp(h), _vp(nrm), 9))
        assert _untouched(x[n:]) and _untouched(h[n:]) and _untouched(nrm[1:])
        res.append((x[:n].copy(), h[:n].copy(), nrm[:1].copy()))
    for a, b in zip(*res):
        assert np.array_equal(_bits(a), _bits(b))
    x, h, nrm = res[0]
    assert (np.abs(x) < 1).all() and abs(nrm[0] - np.linalg.norm(x)) <= 1e-12 * nrm[0] and abs(np.linalg.norm(h) - 1) < 1e-12
