// The rank decisions of the module-compression driver (compress.cpp) as plain host arithmetic on a few KiB: plain
// C++17, no HIP, tested alone (tests/test_module_select_cpu.py).  All matrices column-major.  The input of a step is the
// product hG = [W V]'V ((w + mc) x mc, leading dimension ap) of the orthonormal basis W (w columns) and the candidates V.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

namespace sdpsr {

// dst (m x m, compact) = (src + src') / 2 of the leading m x m block of src (leading dimension lds), like _symmetrize!
inline void symmetrize_copy(const double* src, int64_t lds, int m, double* dst) {
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) dst[(size_t)i + (size_t)j * m] = 0.5 * (src[(size_t)i + (size_t)j * lds] + src[(size_t)j + (size_t)i * lds]);
}

struct Selection {
    int rank = 0;
    double piv_max = 0, piv_min = 0;  // first / last accepted pivot (diagonal pivoting: decreasing)
    double ref = 0;                   // select_directions with take_ref: squared scale of the candidates before projection
    // gram_select: X = R11^-1 scattered to the pivot rows, m x max(rank, 1); select_directions: S = [-C X; X], (w + mc) x rank
    std::vector<double> coef;
};

// pivoted Cholesky of the m x m Gram matrix G (leading dimension ldg), pivots > tol_abs: the rank, the pivots and X
inline Selection gram_select(const double* G, int64_t ldg, int m, double tol_abs) {
    Selection out;
    std::vector<double> Gm((size_t)m * m);
    symmetrize_copy(G, ldg, m, Gm.data());
    std::vector<int> perm(m);
    std::iota(perm.begin(), perm.end(), 0);
    std::vector<double> R((size_t)m * m, 0.0);
    int r = 0;
    for (int kk2 = 0; kk2 < m; ++kk2) {
        int p = kk2;
        for (int i = kk2 + 1; i < m; ++i)
            if (Gm[(size_t)i + (size_t)i * m] > Gm[(size_t)p + (size_t)p * m]) p = i;
        if (!(Gm[(size_t)p + (size_t)p * m] > tol_abs)) break;
        if (p != kk2) {
            for (int i = 0; i < m; ++i) std::swap(Gm[(size_t)i + (size_t)kk2 * m], Gm[(size_t)i + (size_t)p * m]);
            for (int j = 0; j < m; ++j) std::swap(Gm[(size_t)kk2 + (size_t)j * m], Gm[(size_t)p + (size_t)j * m]);
            for (int i = 0; i < kk2; ++i) std::swap(R[(size_t)i + (size_t)kk2 * m], R[(size_t)i + (size_t)p * m]);
            std::swap(perm[kk2], perm[p]);
        }
        const double rkk = std::sqrt(Gm[(size_t)kk2 + (size_t)kk2 * m]);
        if (kk2 == 0) out.piv_max = rkk * rkk;
        out.piv_min = rkk * rkk;
        R[(size_t)kk2 + (size_t)kk2 * m] = rkk;
        for (int j = kk2 + 1; j < m; ++j) R[(size_t)kk2 + (size_t)j * m] = Gm[(size_t)kk2 + (size_t)j * m] / rkk;
        for (int j = kk2 + 1; j < m; ++j) {
            const double rj = R[(size_t)kk2 + (size_t)j * m];
            for (int i = kk2 + 1; i <= j; ++i) {
                Gm[(size_t)i + (size_t)j * m] -= R[(size_t)kk2 + (size_t)i * m] * rj;
                Gm[(size_t)j + (size_t)i * m] = Gm[(size_t)i + (size_t)j * m];
            }
        }
        ++r;
    }
    // X = R11^-1 (upper triangular r x r), column by column
    std::vector<double> X((size_t)r * r, 0.0);
    for (int cc = 0; cc < r; ++cc) {
        for (int i = cc; i >= 0; --i) {
            double sum = (i == cc) ? 1.0 : 0.0;
            for (int t = i + 1; t <= cc; ++t) sum -= R[(size_t)i + (size_t)t * m] * X[(size_t)t + (size_t)cc * r];
            X[(size_t)i + (size_t)cc * r] = sum / R[(size_t)i + (size_t)i * m];
        }
    }
    out.coef.assign((size_t)m * std::max(r, 1), 0.0);
    for (int cc = 0; cc < r; ++cc)
        for (int i = 0; i <= cc; ++i) out.coef[(size_t)perm[i] + (size_t)cc * m] = X[(size_t)i + (size_t)cc * r];
    out.rank = r;
    return out;
}

// entry (i, j) of the projected Gram matrix G - C'C of the candidates (C = W'V the top w rows, G = V'V below them)
inline double projected_entry(const double* hG, int64_t ap, int w, int i, int j) {
    double v = hG[(size_t)(w + i) + (size_t)j * ap];
    for (int t = 0; t < w; ++t) v -= hG[(size_t)t + (size_t)i * ap] * hG[(size_t)t + (size_t)j * ap];
    return v;
}

// S = [-C X; X] ((w + mc) x r, compact) with V_new = [W V] S for the selection X (mc x r, leading dimension mc)
inline std::vector<double> stacked_coefficients(const double* hG, int64_t ap, int w, int mc, const std::vector<double>& X, int r) {
    std::vector<double> stacked((size_t)(w + mc) * r, 0.0);
    for (int cc = 0; cc < r; ++cc) {
        double* col = stacked.data() + (size_t)cc * (w + mc);
        for (int i = 0; i < mc; ++i) {
            const double xi = X[(size_t)i + (size_t)cc * mc];
            col[w + i] = xi;
            if (xi != 0.0)
                for (int t = 0; t < w; ++t) col[t] -= hG[(size_t)t + (size_t)i * ap] * xi;
        }
    }
    return stacked;
}

// One orthonormalisation step's host part: the new directions among the mc candidates.  take_ref: tol is relative to THIS
// round's candidates before projection, the largest diagonal entry of V'V (after it, a complete module leaves only rounding
// noise and a relative test would compare noise with noise).  Rank 0 is decided by the largest projected diagonal entry
// alone: the invariance round of a complete module stops there, without the mc^2 w products of the full matrix.
inline Selection select_directions(const double* hG, int64_t ap, int w, int mc, double tol, bool take_ref) {
    Selection out;
    double ref = 0, dmax = 0;
    for (int i = 0; i < mc && take_ref; ++i) ref = std::max(ref, hG[(size_t)(w + i) + (size_t)i * ap]);
    const double tol_abs = take_ref ? tol * ref : tol;
    for (int i = 0; i < mc; ++i) dmax = std::max(dmax, projected_entry(hG, ap, w, i, i));  // (diagonal pivoting: the first pivot)
    if (dmax > tol_abs) {
        std::vector<double> G1((size_t)mc * mc);
        for (int j = 0; j < mc; ++j)
            for (int i = 0; i < mc; ++i) G1[(size_t)i + (size_t)j * mc] = projected_entry(hG, ap, w, i, j);
        out = gram_select(G1.data(), mc, mc, tol_abs);
    }
    out.coef = stacked_coefficients(hG, ap, w, mc, out.coef, out.rank);
    out.ref = ref;
    return out;
}

}  // namespace sdpsr
