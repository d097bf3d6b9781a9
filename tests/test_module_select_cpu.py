"""The rank decisions of the module-compression driver (csrc/module_select.h) alone: plain host arithmetic, compiled with
g++ under AddressSanitizer + UBSan into a program of its own and run as a program (nothing is loaded into Python)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# W: n x w orthonormal, N: r further orthonormal directions.  V = [W N] M for a well-scaled M: the r independent columns sit LAST,
# with N-coefficients A0 = (I + 0.6 R) diag(1 + k / r) (R uniform in [-1, 1]: not orthogonal to each other, norms growing towards
# the end, so the pivot search permutes) and O(1) components along W; in front of them a W-only column and combinations
# A0 c with |c| <= 0.3 (smaller than every independent column).  The padding rows of the product (ap > w + mc) hold NaN.
SRC = r'''
#include <cstdio>
#include <limits>
#include "module_select.h"
using namespace sdpsr;
typedef std::vector<double> vec;
static unsigned long long state = 12345;
static double rnd() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(state >> 11) / 9007199254740992.0 * 2 - 1; }
static vec gram(const vec& A, int ka, const vec& B, int kb, int n, int ld) {  // A'B, leading dimension ld, NaN below row ka
    vec G((size_t)ld * kb, std::numeric_limits<double>::quiet_NaN());
    for (int j = 0; j < kb; ++j)
        for (int i = 0; i < ka; ++i) {
            long double s = 0;
            for (int t = 0; t < n; ++t) s += (long double)A[t + (size_t)i * n] * B[t + (size_t)j * n];
            G[i + (size_t)j * ld] = (double)s;
        }
    return G;
}
static double max_dev(const vec& G, int ka, int kb, int ld, bool identity) {
    double m = 0;
    for (int j = 0; j < kb; ++j)
        for (int i = 0; i < ka; ++i) m = std::max(m, std::fabs(G[i + (size_t)j * ld] - (identity && i == j ? 1.0 : 0.0)));
    return m;
}
static int run(int n, int w, int mc, int r) {
    vec Q((size_t)n * (w + r));  // [W N], orthonormal: Gram-Schmidt twice
    for (double& x : Q) x = rnd();
    for (int j = 0; j < w + r; ++j)
        for (int pass = 0; pass < 3; ++pass) {
            for (int i = 0; i < j && pass < 2; ++i) {
                long double s = 0;
                for (int t = 0; t < n; ++t) s += (long double)Q[t + (size_t)i * n] * Q[t + (size_t)j * n];
                for (int t = 0; t < n; ++t) Q[t + (size_t)j * n] -= (double)s * Q[t + (size_t)i * n];
            }
            long double s = 0;
            for (int t = 0; t < n; ++t) s += (long double)Q[t + (size_t)j * n] * Q[t + (size_t)j * n];
            for (int t = 0; t < n; ++t) Q[t + (size_t)j * n] /= std::sqrt((double)s);
        }
    vec WV((size_t)n * (w + mc), 0.0), A0((size_t)r * r);  // [W V]; A0: N-coefficients of the independent columns
    std::copy(Q.begin(), Q.begin() + (size_t)n * w, WV.begin());
    for (int k = 0; k < r; ++k)
        for (int i = 0; i < r; ++i) A0[i + (size_t)k * r] = ((i == k ? 1.0 : 0.0) + 0.6 * rnd()) * (1.0 + (double)k / r);
    for (int j = 0; j < mc; ++j) {
        double* v = &WV[(size_t)n * (w + j)];
        vec a(r, 0.0);  // this column's coefficients on N
        if (j >= mc - r) {
            for (int i = 0; i < r; ++i) a[i] = A0[i + (size_t)(j - (mc - r)) * r];
        } else if (j > 0) {
            for (int k = 0; k < r; ++k) {
                const double ck = 0.3 * rnd() / std::sqrt((double)r);
                for (int i = 0; i < r; ++i) a[i] += ck * A0[i + (size_t)k * r];
            }
        }
        for (int k = 0; k < r; ++k)
            for (int t = 0; t < n; ++t) v[t] += a[k] * Q[t + (size_t)(w + k) * n];
        for (int k = 0; k < w; ++k) {
            const double b = rnd();
            for (int t = 0; t < n; ++t) v[t] += b * Q[t + (size_t)k * n];
        }
    }
    const int ap = w + mc + 3;
    const vec V(WV.begin() + (size_t)n * w, WV.end());
    const vec hG = gram(WV, w + mc, V, mc, n, ap);
    const Selection sel = select_directions(hG.data(), ap, w, mc, 1e-10, true);
    double ref = 0;  // the largest |V_j|^2
    for (int j = 0; j < mc; ++j) ref = std::max(ref, hG[w + j + (size_t)j * ap]);
    // the pieces: the largest projected diagonal entry is the first pivot; the coefficient matrix is zero outside the pivot rows
    vec G1((size_t)mc * mc);
    double dmax = 0;
    for (int j = 0; j < mc; ++j)
        for (int i = 0; i < mc; ++i) G1[i + (size_t)j * mc] = projected_entry(hG.data(), ap, w, i, j);
    for (int j = 0; j < mc; ++j) dmax = std::max(dmax, G1[j + (size_t)j * mc]);
    const Selection gs = gram_select(G1.data(), mc, mc, 1e-10 * sel.ref);
    int nonzero_rows = 0;
    for (int i = 0; i < mc; ++i) {
        bool nz = false;
        for (int cc = 0; cc < std::max(gs.rank, 1); ++cc) nz = nz || gs.coef[i + (size_t)cc * mc] != 0.0;
        nonzero_rows += nz;
    }
    const bool pieces = gs.rank == sel.rank && nonzero_rows == gs.rank && (gs.rank == 0 || (gs.piv_max == sel.piv_max && gs.piv_min == sel.piv_min && std::fabs(dmax - gs.piv_max) <= 4e-16 * dmax)) &&
                        (int)sel.coef.size() == (w + mc) * sel.rank && gs.coef.size() == (size_t)mc * std::max(gs.rank, 1);
    // V_new = [W V] S: orthonormal, orthogonal to W; a second step on it (unit scale, absolute tolerance) keeps every column
    vec WN((size_t)n * (w + sel.rank), 0.0);
    std::copy(Q.begin(), Q.begin() + (size_t)n * w, WN.begin());
    for (int cc = 0; cc < sel.rank; ++cc)
        for (int k = 0; k < w + mc; ++k)
            for (int t = 0; t < n; ++t) WN[t + (size_t)(w + cc) * n] += WV[t + (size_t)k * n] * sel.coef[k + (size_t)cc * (w + mc)];
    double orth = 0, wdot = 0;
    int rank2 = 0;
    if (sel.rank > 0) {
        const vec Vn(WN.begin() + (size_t)n * w, WN.end());
        const int ap2 = w + sel.rank + 1;
        const vec h2 = gram(WN, w + sel.rank, Vn, sel.rank, n, ap2);
        wdot = max_dev(h2, w, sel.rank, ap2, false);
        orth = max_dev(vec(h2.begin() + w, h2.end()), sel.rank, sel.rank, ap2, true);
        const Selection s2 = select_directions(h2.data(), ap2, w, sel.rank, 1e-6, false);
        rank2 = s2.ref == 0 ? s2.rank : -1;
    }
    int first = 0;  // the first pivot's position: not the front
    for (int j = 1; j < mc; ++j) if (G1[j + (size_t)j * mc] > G1[first + (size_t)first * mc]) first = j;
    printf("case n=%d w=%d mc=%d r=%d first=%d rank=%d rank2=%d orth=%.3e wdot=%.3e piv_max=%.17g piv_min=%.17g ref_ok=%d pieces=%d\n", n, w, mc, r, first, sel.rank, rank2,
           orth, wdot, sel.piv_max, sel.piv_min, (int)(sel.ref == ref), (int)pieces);
    return 0;
}
int main() {
    const int cases[][4] = {{40, 5, 7, 3}, {40, 5, 7, 0}, {40, 5, 7, 7}, {40, 5, 1, 1}, {40, 5, 1, 0}, {33, 3, 4, 2}, {40, 1, 12, 6}};
    for (const auto& k : cases) run(k[0], k[1], k[2], k[3]);
    vec A = {1, 2, 99, 4, 3, 99}, B(4);  // the symmetrising copy: 2 x 2 out of leading dimension 3
    symmetrize_copy(A.data(), 3, 2, B.data());
    printf("sym %g %g %g %g\n", B[0], B[1], B[2], B[3]);
    return 0;
}
'''


def test_module_select_finds_the_known_rank_and_an_orthonormal_basis():
    """Gram products [W V]'V with a known answer through select_directions and its pieces: the rank is r; [W V] S is
    orthonormal and orthogonal to W to 1e-12; first pivot >= last pivot; the coefficient matrix is zero outside the pivot
    rows; r = 0 takes the early exit; r = mc and mc = 1 work; the padding rows (NaN) are never read.  The selected columns
    are neither orthogonal to each other nor to W, and the first pivot is never the front column, so the permutation
    scatter, R11^-1 and the sign of -C X all carry the result.  Bound: the step's error is ~ eps (w |C|^2 + |V|^2) / piv_min
    (cancellation in G - C'C, then Cholesky QR on a Gram matrix of condition piv_max / piv_min); with |V|^2 < 15 and
    piv_min >= 0.05 (asserted) that is < 1e-13."""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                               os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc"), os.path.join(d, "t.cpp"), "-o", os.path.join(d, "t")])
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.splitlines()
    print("\n".join(out))
    cases = [dict(kv.split("=") for kv in line.split()[1:]) for line in out if line.startswith("case ")]
    assert [(int(c["n"]), int(c["w"]), int(c["mc"]), int(c["r"])) for c in cases] == [
        (40, 5, 7, 3), (40, 5, 7, 0), (40, 5, 7, 7), (40, 5, 1, 1), (40, 5, 1, 0), (33, 3, 4, 2), (40, 1, 12, 6)]
    for c in cases:
        r = int(c["r"])
        assert int(c["rank"]) == r and int(c["rank2"]) == r, c
        assert float(c["orth"]) <= 1e-12 and float(c["wdot"]) <= 1e-12, c
        assert float(c["piv_max"]) >= float(c["piv_min"]) and (r == 0) == (float(c["piv_min"]) == 0.0), c
        assert c["pieces"] == "1" and c["ref_ok"] == "1", c
        assert r == 0 or (float(c["piv_min"]) >= 0.05 and float(c["piv_max"]) < 15), c
        assert r == 0 or int(c["mc"]) == 1 or int(c["first"]) > 0, c  # the pivot search had to permute
    assert out[-1] == "sym 1 3 3 3"
