"""The host side of the compressed eigenproblem (csrc/host_syev.cpp) alone: host_syev, host_count_edges17 and
host_gemm_tn, compiled with g++ into stand-alone programs -- under AddressSanitizer + UBSan at -O1, with the Makefile's
-O3 and at -O0 (the three sum in different orders, which decides whether rounding noise of low rank cascades) -- and run
as programs on record files (nothing is loaded into Python).  The references are NumPy's: LAPACK for the eigenvalues,
long-double products for residual and Gram matrix."""
import os
import struct
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import syev_families as fam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc")

# records in:  int32 kind, then  1: n lda ldz (int32), A (lda x n doubles)   2: len (int32), 17 edges, len values
#              3: m n k lda ldb ldc (int32), A (lda x m), B (ldb x n)
# records out: doubles only      1: info, w (n), Z (ldz x n, NaN before the call)   2: hist (18)   3: C (ldc x n, NaN before)
SRC = r'''
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
namespace sdpsr {
int host_syev(int n, const double* A, int lda, double* w, double* Z, int ldz);
void host_count_edges17(const double* x, size_t n, const double* ed, int64_t* hist);
void host_gemm_tn(int m, int n, int k, const double* A, int lda, const double* B, int ldb, double* C, int ldc);
}
static FILE *in, *out;
static bool get(void* p, size_t bytes) { return fread(p, 1, bytes, in) == bytes; }
static void put(const std::vector<double>& v) { fwrite(v.data(), sizeof(double), v.size(), out); }
int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int32_t kind;
    while (get(&kind, 4)) {
        if (kind == 1) {
            int32_t h[3];
            if (!get(h, sizeof h)) return 3;
            const int n = h[0], lda = h[1], ldz = h[2];
            std::vector<double> A((size_t)lda * n), w(n, nan), Z((size_t)ldz * n, nan);
            if (!get(A.data(), A.size() * 8)) return 3;
            const int info = sdpsr::host_syev(n, A.data(), lda, w.data(), Z.data(), ldz);
            put({(double)info});
            put(w);
            put(Z);
        } else if (kind == 2) {
            int32_t len;
            if (!get(&len, 4)) return 3;
            std::vector<double> ed(17), x(len);
            if (!get(ed.data(), 17 * 8) || !get(x.data(), x.size() * 8)) return 3;
            int64_t hist[18];
            sdpsr::host_count_edges17(x.data(), x.size(), ed.data(), hist);
            put(std::vector<double>(hist, hist + 18));
        } else if (kind == 3) {
            int32_t h[6];
            if (!get(h, sizeof h)) return 3;
            std::vector<double> A((size_t)h[3] * h[0]), B((size_t)h[4] * h[1]), C((size_t)h[5] * h[1], nan);
            if (!get(A.data(), A.size() * 8) || !get(B.data(), B.size() * 8)) return 3;
            sdpsr::host_gemm_tn(h[0], h[1], h[2], A.data(), h[3], B.data(), h[4], C.data(), h[5]);
            put(C);
        } else {
            return 4;
        }
    }
    return fclose(out) == 0 ? 0 : 5;
}
'''

BUILDS = {"asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "O3": ["-O3"], "O0": ["-O0"]}
ORDERS = (1, 2, 3, 4, 5, 7, 8, 16, 33, 34, 63, 64, 65, 72, 100, 128, 129, 256, 512)

def _slices(X, axis, beta):
    """X = S0 + S1 + S2 + rest, the S_k with multiples of 2^-beta of (the power of two above) the largest entry along axis, at most that entry: beta bits below the largest entry along axis."""
    out, R = [], X.copy()
    for _ in range(3):
        mu = np.abs(R).max(axis=axis, keepdims=True)
        sigma = np.where(mu > 0, 2.0 ** (np.ceil(np.log2(np.where(mu > 0, mu, 1.0))) + 53 - beta), 0.0)
        H = (R + sigma) - sigma
        R = R - H
        out.append(H)
    return out + [R]


def product_ld(X, Y):
    """X @ Y in long double.  Up to order 129 NumPy's own long-double product.  Above (1.1 s per product at order 512, 228
    of them): X (by rows) and Y (by columns) are cut into three slices of >= 21 bits plus a rest below 2^-63 of the row's /
    column's largest entry; a product of two slices is exact in double (integers below 2^53), the products with a rest are
    rounded at 2^-63 * 2^-53, and the sixteen are summed in long double, smallest first: at least long double's accuracy."""
    k = X.shape[1]
    if k <= 129:
        return X.astype(np.longdouble) @ Y.astype(np.longdouble)
    beta = int((53 - np.ceil(np.log2(k))) // 2)  # k products of two beta-bit integers stay below 2^53
    xs, ys = _slices(X, 1, beta), _slices(Y, 0, beta)
    acc = np.zeros((X.shape[0], Y.shape[1]), dtype=np.longdouble)
    for level in range(6, -1, -1):
        for i in range(4):
            if 0 <= level - i < 4:
                acc += xs[i] @ ys[level - i]
    return acc


def all_cases():
    """[(family, n, A, LAPACK's eigenvalues, |A|)] for every order."""
    return [(name, n) + fam.reference(name, n) for n in ORDERS for name in fam.names(n)]


def check_syev(tag, A, wl, sc, info, w, Z):
    """The bounds of test_tridiagonal_divide_and_conquer_hard_cases."""
    n = A.shape[0]
    assert info == 0, (tag, info)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(Z)), tag
    assert np.all(np.diff(w) >= 0), tag
    dw = np.abs(w - wl).max() / sc
    res = float(np.abs(product_ld(A, Z) - Z.astype(np.longdouble) * w.astype(np.longdouble)).max() / np.longdouble(sc))
    orth = float(np.abs(product_ld(np.ascontiguousarray(Z.T), Z) - np.eye(n, dtype=np.longdouble)).max())
    assert dw <= 2e-13 and res <= 1e-12 and orth < 1e-12, (tag, dw, res, orth)


@pytest.fixture(scope="module")
def programs():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(SRC)

        def build(name):
            subprocess.check_call(["g++", "-std=c++17", *BUILDS[name], os.path.join(CSRC, "host_syev.cpp"), os.path.join(d, "driver.cpp"),
                                   "-o", os.path.join(d, name)])
        with ThreadPoolExecutor(3) as pool:
            list(pool.map(build, BUILDS))

        def run(name, payload, count, job="0"):
            """Feeds one record file to one program; returns its output as doubles (count of them expected)."""
            fi, fo = os.path.join(d, name + job + ".in"), os.path.join(d, name + job + ".out")
            with open(fi, "wb") as f:
                f.write(payload)
            subprocess.run([os.path.join(d, name), fi, fo], check=True)
            got = np.fromfile(fo, dtype=np.float64)
            assert got.size == count, (name, got.size, count)
            return got
        yield run


@pytest.fixture(scope="module")
def solved(programs):
    """{(build, padded): [(info, w, Z buffer)] in the order of all_cases()}: every program on every case, the cases of one
    program dealt out to four processes (half a second per solve at order 512 even at -O3), all of them side by side."""
    cases, parts = all_cases(), 4
    by_cost = sorted(range(len(cases)), key=lambda i: -cases[i][1])

    def job(key):
        build, padded, part = key
        mine, payload, count = by_cost[part::parts], [], 0
        for i in mine:
            n, A = cases[i][1:3]
            lda, ldz = (n + 3, n + 5) if padded else (n, n)
            buf = np.full((lda, n), np.nan, order="F")
            buf[:n] = A
            payload.append(struct.pack("<4i", 1, n, lda, ldz) + buf.tobytes(order="F"))
            count += 1 + n + ldz * n
        got, pos, out = programs(build, b"".join(payload), count, "_%d_%d" % (padded, part)), 0, {}
        for i in mine:
            n = cases[i][1]
            ldz = n + 5 if padded else n
            out[i] = (int(got[pos]), got[pos + 1:pos + 1 + n], got[pos + 1 + n:pos + 1 + n + ldz * n].reshape((ldz, n), order="F"))
            pos += 1 + n + ldz * n
        return out
    keys = [(b, p, part) for b in BUILDS for p in (False, True) for part in range(parts)]
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        outs = list(pool.map(job, keys))
    res = {}
    for (b, p, _), out in zip(keys, outs):
        res.setdefault((b, p), {}).update(out)
    return {k: [v[i] for i in range(len(cases))] for k, v in res.items()}


def test_product_ld_slices_match_numpy_long_double():
    """The sliced product of the larger orders against NumPy's long-double product, at an order where that is quick: a
    matrix with 30 orders of magnitude inside every row, and one at 1e145."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((130, 130)) * 10.0 ** rng.uniform(-30, 0, (130, 130))
    Y = rng.standard_normal((130, 130)) * 1e145
    ref = X.astype(np.longdouble) @ Y.astype(np.longdouble)
    bound = np.abs(X).astype(np.longdouble) @ np.abs(Y).astype(np.longdouble) * np.longdouble(2.0 ** -60)
    assert np.all(np.abs(product_ld(X, Y) - ref) <= bound)


@pytest.mark.parametrize("build", list(BUILDS))
def test_host_syev_families(solved, build):
    """Every family at every order, once with lda = ldz = n and once with lda = n + 3, ldz = n + 5 (the padding NaN: that of
    Z comes back NaN, and that of A changes no bit of the result).  info = 0, w ascending, |w - w_lapack| <= 2e-13 |A|,
    |A Z - Z diag(w)| <= 1e-12 |A|, |Z'Z - I| < 1e-12, |A| = max |eigenvalue| (1 for the zero matrix).
    The solver before its drop and deflation rules fails here in the kron and rank-one families on all three builds."""
    failures = []
    for (name, n, A, wl, sc), (info, w, Zb), (info_p, w_p, Zb_p) in zip(all_cases(), solved[build, False], solved[build, True]):
        try:
            assert Zb_p.shape == (n + 5, n) and np.all(np.isnan(Zb_p[n:])), (build, name, n, "padding of Z")
            assert info_p == info and np.array_equal(w_p, w, equal_nan=True) and np.array_equal(Zb_p[:n], Zb, equal_nan=True), (build, name, n, "padded != tight")
            check_syev((build, name, n), A, wl, sc, info, w, Zb)
        except AssertionError as e:
            failures.append(str(e))
    print("\n".join(failures))
    assert not failures, (len(failures), failures[:10])


def test_host_count_edges17_and_gemm_tn(programs):
    """host_count_edges17 against a plain loop: lengths around the eight-wide step, values equal to an edge, below the
    first, above the last, and NaN (counts as 17).  host_gemm_tn against long double at ragged shapes with lda, ldb > k."""
    rng = np.random.default_rng(3)
    edges = np.sort(rng.standard_normal(17))
    payload, expect, count = [], [], 0
    for length in (0, 1, 7, 8, 9, 1000):
        x = rng.standard_normal(length) * 2
        special = np.concatenate([edges[[0, 8, 16]], [edges[0] - 1.0, edges[16] + 1.0, np.nan, -np.inf, np.inf]])
        x[:special.size] = rng.permutation(special)[:length]
        hist = [0] * 18
        for v in x:
            hist[sum(0 if t > v else 1 for t in edges)] += 1
        assert sum(hist) == length and (length < 8 or hist[17] >= 3)
        payload.append(struct.pack("<2i", 2, length) + edges.tobytes() + x.tobytes())
        expect.append(("edges", np.array(hist, dtype=float)))
        count += 18
    for m, n, k, lda, ldb, ldc in ((1, 1, 1, 2, 3, 1), (3, 5, 7, 9, 8, 4), (6, 2, 13, 14, 17, 6), (4, 4, 4, 5, 6, 7), (34, 9, 70, 72, 71, 40)):
        A = np.full((lda, m), np.nan, order="F")
        B = np.full((ldb, n), np.nan, order="F")
        A[:k], B[:k] = rng.standard_normal((k, m)), rng.standard_normal((k, n))
        payload.append(struct.pack("<7i", 3, m, n, k, lda, ldb, ldc) + A.tobytes(order="F") + B.tobytes(order="F"))
        expect.append(("gemm", (A[:k].T.astype(np.longdouble) @ B[:k].astype(np.longdouble), np.abs(A[:k]).T @ np.abs(B[:k]), m, ldc)))
        count += ldc * n
    for build in BUILDS:
        got = programs(build, b"".join(payload), count)
        pos = 0
        for kind, ref in expect:
            if kind == "edges":
                assert np.array_equal(got[pos:pos + 18], ref), (build, ref)
                pos += 18
            else:
                prod, mag, m, ldc = ref
                Cb = got[pos:pos + ldc * prod.shape[1]].reshape((ldc, prod.shape[1]), order="F")
                pos += Cb.size
                assert np.all(np.isnan(Cb[m:])), build
                # a dot product of length k in any order: k eps sum |a||b|
                assert np.all(np.abs(Cb[:m] - prod) <= 70 * 2.3e-16 * mag), build
