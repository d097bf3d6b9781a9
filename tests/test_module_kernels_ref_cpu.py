"""The references of tests/test_gpu_module_kernels.py (tests/module_kernels_ref.py) checked without a GPU: the vectorised class
values against sdpsr_hash.h (a tiny g++ program, nothing loaded into Python), the long-double and int64 products against brute-force
loops in exact rational arithmetic, and the label product's shape table against the Python restatement of its selection rule -- a
change to the rule that un-covers an instantiation fails here."""
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

import module_kernels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LABEL = 4000


def test_class_values_match_the_hash_header_bit_for_bit():
    keys = R.KEYS + R.RANDOM_VECTOR_KEYS
    src = r'''
    #include <stdio.h>
    #include <string.h>
    #include "sdpsr_hash.h"
    int main(){ const unsigned long long keys[] = {%s};
      for (unsigned i = 0; i < sizeof(keys) / sizeof(keys[0]); ++i)
        for (unsigned l = 1; l <= %d; ++l) {
          const double v = sdpsr_class_uniform(keys[i], l), x = 2.0 * v - 1.0;
          unsigned long long vb, xb; memcpy(&vb, &v, 8); memcpy(&xb, &x, 8);
          printf("%%llx %%llx %%llx\n", (unsigned long long)sdpsr_fmix64(keys[i] + l), vb, xb);
        }
      return 0; }
    ''' % (", ".join("0x%xULL" % k for k in keys), MAX_LABEL)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.check_call(["g++", "-O1", "-I", os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc"), os.path.join(d, "t.cpp"), "-o",
                               os.path.join(d, "t")])
        out = np.array([[int(t, 16) for t in line.split()] for line in subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()],
                       dtype=np.uint64).reshape(len(keys), MAX_LABEL, 3)
    labels = np.arange(1, MAX_LABEL + 1, dtype=np.uint64)
    for i, key in enumerate(keys):
        with np.errstate(over="ignore"):
            assert np.array_equal(R.fmix64(np.uint64(key) + labels), out[i, :, 0]), hex(key)
        v = R.class_uniform(key, labels)
        assert np.array_equal(v.view(np.uint64), out[i, :, 1]), hex(key)
        assert np.array_equal((2.0 * v - 1.0).view(np.uint64), out[i, :, 2]), hex(key)  # random_vector: exactly representable
        assert ((v >= 0) & (v < 1)).all()
    assert R.class_uniform(R.KEYS[0], np.array([0, 1, 0], dtype=np.uint32))[[0, 2]].tolist() == [0.0, 0.0]  # label 0 carries no value


def _exact(x):
    return Fraction(float(x))


def _close(ref, exact, scale, k):
    """a long-double sum of k products of doubles: within k 2^-63 of the exact value, relative to the sum of the absolute terms"""
    return abs(Fraction(float(ref)) - exact) <= Fraction(k + 2, 2 ** 63) * scale + abs(exact) * Fraction(1, 2 ** 52)


def test_products_against_brute_force():
    rng = np.random.default_rng(5)
    for (k, ma, nb) in ((1, 1, 1), (3, 2, 1), (7, 3, 4)):
        A, B = rng.standard_normal((k, ma)), rng.standard_normal((k, nb))
        ref, ab = R.tn_product(A, B)
        assert ref.dtype == np.longdouble and ref.shape == ab.shape == (ma, nb)
        for i in range(ma):
            for j in range(nb):
                ex = sum(_exact(A[t, i]) * _exact(B[t, j]) for t in range(k))
                sc = sum(abs(_exact(A[t, i]) * _exact(B[t, j])) for t in range(k))
                # (float(ref) rounds the long double to double: one more 2^-53, covered by the last term of _close)
                assert _close(ref[i, j], ex, sc, k), (k, i, j)
                assert abs(Fraction(float(ab[i, j])) - sc) <= sc * Fraction(k + 1, 2 ** 52)
        Ai, Bi = rng.integers(-8, 9, (k, ma)).astype(np.float64), rng.integers(-8, 9, (k, nb)).astype(np.float64)
        got = R.tn_product_int(Ai, Bi)
        assert got.dtype == np.int64
        assert got.tolist() == [[sum(int(Ai[t, i]) * int(Bi[t, j]) for t in range(k)) for j in range(nb)] for i in range(ma)]
    for (n, kk, nc) in ((1, 1, 1), (4, 3, 2)):
        In, S = rng.standard_normal((n, kk)), rng.standard_normal((kk, nc))
        ref, ab = R.nn_product(In, S)
        for i in range(n):
            for j in range(nc):
                ex = sum(_exact(In[i, t]) * _exact(S[t, j]) for t in range(kk))
                sc = sum(abs(_exact(In[i, t]) * _exact(S[t, j])) for t in range(kk))
                assert _close(ref[i, j], ex, sc, kk)
                assert abs(Fraction(float(ab[i, j])) - sc) <= sc * Fraction(kk + 1, 2 ** 52)
        Ii, Si = rng.integers(-8, 9, (n, kk)).astype(np.float64), rng.integers(-8, 9, (kk, nc)).astype(np.float64)
        assert R.nn_product_int(Ii, Si).tolist() == [[sum(int(Ii[i, t]) * int(Si[t, j]) for t in range(kk)) for j in range(nc)] for i in range(n)]


def test_label_product_and_class_sums_against_brute_force():
    n, d, w = 5, 3, 2
    L = R.hashed_labels(n, d)
    assert L.dtype == np.uint32 and L.max() == d and L.min() == 0
    Lm = L.reshape(n, n, order="F")
    assert not np.array_equal(Lm, Lm.T)  # non-symmetric: a transposed read shows
    rng = np.random.default_rng(6)
    W = rng.standard_normal((n, w))
    keys = R.KEYS[:2]
    ref, ab = R.label_product(n, L, keys, W)
    assert ref.shape == ab.shape == (n, 2 * w)
    for g, key in enumerate(keys):
        for r in range(n):
            for j in range(w):
                vals = [float(R.class_uniform(key, np.array([L[r + c * n]]))[0]) for c in range(n)]
                ex = sum(_exact(vals[c]) * _exact(W[c, j]) for c in range(n))
                sc = sum(abs(_exact(vals[c]) * _exact(W[c, j])) for c in range(n))
                assert _close(ref[r, g * w + j], ex, sc, n)
                assert abs(Fraction(float(ab[r, g * w + j])) - sc) <= sc * Fraction(n + 1, 2 ** 52)
    x = rng.integers(-8, 9, n).astype(np.float64)
    got = R.class_sums_int(n, d, L, x)
    want = [[sum(int(x[c]) for c in range(n) if L[c + r * n] == i) for r in range(n)] for i in range(1, d + 1)]  # COLUMN r of the labels
    assert got.tolist() == want
    assert got.tolist() != [[sum(int(x[c]) for c in range(n) if L[r + c * n] == i) for r in range(n)] for i in range(1, d + 1)]


def test_label_product_rows_cover_every_instantiation():
    reached = set()
    for (n, w, G, d), (mfma, tile) in R.LABEL_ROWS:
        form = R.label_form(n, d, G, w)
        assert form is not None and form[:2] == (mfma, tile), ((n, w, G, d), form)
        reached.add((mfma, tile, G))
        if n >= 64 and not mfma:  # VALU at n >= 64 only because the class table pushes the matrix-core form out of LDS
            assert R.label_form(n, 9, G, w)[0] == 1
    assert reached == set(R.LABEL_INSTANTIATIONS) and len(R.LABEL_INSTANTIATIONS) == 17
    for row, split in R.LABEL_ROW_SPLIT.items():
        n, w, G, d = row
        assert row in dict(R.LABEL_ROWS) and R.label_form(n, d, G, w)[2:] == split
    # one whole 64-column slab followed by a partial one; steps of four columns an exact multiple of 16
    assert 64 < R.LABEL_ROW_SPLIT[(1062, 16, 4, 200)][1] < 128 and R.LABEL_ROW_SPLIT[(963, 33, 1, 9)][1] % 64 == 0
    # every row so far has fewer than 16 steps per workgroup except those two
    assert all(R.label_form(n, d, G, w)[3] < 64 for (n, w, G, d), _ in R.LABEL_ROWS if (n, w, G, d) not in R.LABEL_ROW_SPLIT)
    # what the launcher refuses
    assert R.label_form(63, 7, 3, 8) is None and R.label_form(63, 7, 2, 33) is None and R.label_form(63, 4001, 1, 8) is None
    assert R.label_form(63, 7, 4, 17) is None and R.label_form(200, 2047, 4, 8) is None  # (four tables of 2049 values: > 64 KiB)
