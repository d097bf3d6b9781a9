// Cyclic two-sided Jacobi on a Gram matrix, for the HOST side of sdpsr_compress_constraints (rowspace.cpp): plain C++,
// no HIP, compiled by the host compiler.
//
// G = W W' (m x m) comes from the device; this file finds the rotations J that make J G J' diagonal and hands J back, the
// device forms W <- J W and the NEXT G from the new W (docs/src/examples/ReduceAndSolveJuMP.jl:44-50 asks for the row
// space of [A * PMat, b] and its rank; DESIGN.md "Dependent reduced constraints").  Two rules make that iteration find
// singular values far below sqrt(eps) sigma_1, which one eigen-decomposition of G cannot:
//   relative rule  (p, q) is rotated only while |g_pq| > tau sqrt(g_pp g_qq): the test does not see the size of the
//                  rows, so a row of norm 1e-9 is made orthogonal to the others as carefully as a row of norm 1.
//   floor          a row with g_pp <= floor2 max_q g_qq takes no part: rows that ARE dependent leave rounding noise
//                  behind, and noise is never orthogonal to anything in the relative sense.
// The largest |g_pq| / sqrt(g_pp g_qq) that was rotated away is reported: once it is inside the rounding error of G itself, the
// rows are orthogonal as far as any G can tell, and the caller stops.
// No vector clones and no reassociation: the rotations are a function of (m, G, tau, floor2) alone on every host.
#include <cmath>
#include <cstdint>
#include <vector>

namespace sdpsr {

// G: m x m, symmetric, both triangles stored (overwritten with J G J').  J: m x m, column-major (J[i + k * m] = J_ik), the
// product of all rotations: row i of the new W is sum_k J_ik (row k of the old W).  The sweeps end after the first
// one without a rotation, or after max_sweeps.  Returns the number of rotations made; *sweeps_out: sweeps run; *max_rel_out:
// the largest |g_pq| / sqrt(g_pp g_qq) among the rotated pairs, at the time of their rotation (0 without a rotation).
int64_t host_gram_jacobi(int m, double* G, double* J, double tau, double floor2, int max_sweeps, int* sweeps_out, double* max_rel_out) {
    const size_t n = (size_t)(m > 0 ? m : 0);
    std::vector<double> R(n * n, 0.0);  // the rotations by rows: R[p * m + k] = J_pk
    for (size_t p = 0; p < n; ++p) R[p * n + p] = 1.0;
    int64_t total = 0;
    int sweep = 0;
    double max_rel = 0.0;
    while (sweep < max_sweeps) {
        ++sweep;
        double gmax = 0.0;
        for (size_t p = 0; p < n; ++p)
            if (G[p * n + p] > gmax) gmax = G[p * n + p];
        const double fl = floor2 * gmax;
        int64_t rot = 0;
        for (size_t p = 0; p + 1 < n; ++p) {
            for (size_t q = p + 1; q < n; ++q) {
                const double gpp = G[p * n + p], gqq = G[q * n + q], gpq = G[p * n + q];
                // (written so that a negative or NaN diagonal -- noise of a dependent row -- counts as below the floor)
                if (!(gpp > fl) || !(gqq > fl)) continue;
                const double size = std::sqrt(gpp) * std::sqrt(gqq);
                if (!(std::fabs(gpq) > tau * size)) continue;
                if (std::fabs(gpq) > max_rel * size) max_rel = std::fabs(gpq) / size;
                const double zeta = (gqq - gpp) / (2.0 * gpq);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                double* gp = G + p * n;
                double* gq = G + q * n;
                for (size_t r = 0; r < n; ++r) {
                    const double a = gp[r], b = gq[r];
                    gp[r] = c * a - s * b;
                    gq[r] = s * a + c * b;
                }
                for (size_t r = 0; r < n; ++r) {
                    G[r * n + p] = gp[r];
                    G[r * n + q] = gq[r];
                }
                gp[p] = gpp - t * gpq;
                gq[q] = gqq + t * gpq;
                gp[q] = gq[p] = 0.0;
                double* rp = R.data() + p * n;
                double* rq = R.data() + q * n;
                for (size_t k = 0; k < n; ++k) {
                    const double a = rp[k], b = rq[k];
                    rp[k] = c * a - s * b;
                    rq[k] = s * a + c * b;
                }
                ++rot;
            }
        }
        total += rot;
        if (rot == 0) break;
    }
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < n; ++k) J[i + k * n] = R[i * n + k];
    if (sweeps_out) *sweeps_out = sweep;
    if (max_rel_out) *max_rel_out = max_rel;
    return total;
}

}  // namespace sdpsr
