// The setup stage of admissible_subspace on the device, src/partitions.jl:117-142: the pieces shared by the dense entry (below) and
// the CSR entries (setup_csr.cpp), and the dense entry.
#include <cmath>

#include "host_internal.h"

using namespace sdpsr;

namespace sdpsr {
// Pivoted modified Gram-Schmidt on the device rows R (len x m, column-major, overwritten by the residuals):
// pivot = the unused row of largest residual norm, one re-orthogonalisation pass against the basis so far, rank
// decided at 1e-12 of the largest row norm.  U (len x m capacity) receives the basis, *r_out its size, piv the rows
// taken in order and coeffs[i][j] the coefficient of u_j in row i (A[piv]' = U R with R[j][k] = coeffs[piv[k]][j]).
int setup_mgs(sdpsr_ctx* c, int64_t len, int64_t m, double* R, double* U, double* partial, int nblk, double* coef,
              std::vector<std::vector<double>>& coeffs, std::vector<int64_t>& piv, int64_t* r_out) {
    hipStream_t s = c->stream;
    const int64_t mm = std::max<int64_t>(m, 1);
    coeffs.assign(m, std::vector<double>(mm, 0.0));
    piv.clear();
    std::vector<char> used(m, 0);
    std::vector<double> hd(mm);
    double maxnorm = 0;
    int64_t r = 0;
    int st = SDPSR_OK;
    for (int64_t step = 0; step < m; ++step) {
        launch_col_norms2(s, len, m, R, partial, nblk, coef);  // |R_i|^2 for every row
        st = d2h_sync(c, hd.data(), coef, (size_t)m * 8);
        if (st) return st;
        if (step == 0)
            for (int64_t i = 0; i < m; ++i) maxnorm = std::max(maxnorm, std::sqrt(hd[i]));
        int64_t best = -1;
        double bestn = -1;
        for (int64_t i = 0; i < m; ++i)
            if (!used[i] && hd[i] > bestn) {
                bestn = hd[i];
                best = i;
            }
        if (best < 0 || std::sqrt(std::max(bestn, 0.0)) <= 1e-12 * maxnorm) break;
        used[best] = 1;
        double* v = R + (size_t)best * len;
        if (r > 0) {  // re-orthogonalise against the basis so far
            launch_proj_coef(s, len, r, U, nullptr, 0, v, partial, nblk, coef);
            st = d2h_sync(c, hd.data(), coef, (size_t)r * 8);
            if (st) return st;
            for (int64_t j = 0; j < r; ++j) coeffs[best][j] += hd[j];
            launch_proj_apply(s, len, r, U, nullptr, 0, v, coef, 0, 1, 0, v, nullptr);
        }
        launch_col_norms2(s, len, 1, v, partial, nblk, coef);
        double nn = 0;
        st = d2h_sync(c, &nn, coef, 8);
        if (st) return st;
        nn = std::sqrt(std::max(nn, 0.0));
        if (nn <= 1e-12 * maxnorm) continue;
        double* ur = U + (size_t)r * len;
        launch_scale_copy(s, len, v, 1.0 / nn, ur);
        coeffs[best][r] = nn;
        // remaining residual rows: R_i -= (u . R_i) u
        launch_proj_coef(s, len, m, R, nullptr, 0, ur, partial, nblk, coef);  // dots of every row with u
        st = d2h_sync(c, hd.data(), coef, (size_t)m * 8);
        if (st) return st;
        std::vector<double> dots(m, 0.0);
        for (int64_t i = 0; i < m; ++i)
            if (!used[i]) {
                dots[i] = hd[i];
                coeffs[i][r] += hd[i];
            }
        st = h2d_sync(c, coef, dots.data(), (size_t)m * 8);
        if (st) return st;
        launch_rank1_update(s, len, m, R, ur, coef);
        piv.push_back(best);
        ++r;
    }
    *r_out = r;
    return SDPSR_OK;
}

// min-norm solution x0 = U y with R' y = b(piv): forward substitution (Krylov.craig, :137)
std::vector<double> min_norm_coefficients(int64_t r, const std::vector<int64_t>& piv, const std::vector<std::vector<double>>& coeffs,
                                          const double* b) {
    std::vector<double> y(std::max<int64_t>(r, 1), 0.0);
    for (int64_t k = 0; k < r; ++k) {
        double s2 = b[piv[k]];
        for (int64_t j = 0; j < k; ++j) s2 -= coeffs[piv[k]][j] * y[j];
        y[k] = s2 / coeffs[piv[k]][k];
    }
    return y;
}

// C_L and X0_L from the basis U (len x r, device) and the coefficients y of x0 = U y (:129-142); v1 holds c on entry.
// Everything stays in stream order (no host wait).
int setup_tail(sdpsr_ctx* c, int64_t n, int64_t r, const double* U, const std::vector<double>& y, double atol, double* v1, double* v2,
               double* dCL, double* dX0, double* partial, int nblk, double* coef) {
    hipStream_t s = c->stream;
    const int64_t len = n * n;
    int st = SDPSR_OK;
    const double scale = round_scale(c, atol);
    // C_L (:129-134): v1 = c;  C_L = symmetrize(round(c - U U'c))
    launch_proj_coef(s, len, r, U, nullptr, 0, v1, partial, nblk, coef);
    launch_proj_apply(s, len, r, U, nullptr, 0, v1, coef, atol, scale, 1, dCL, nullptr);
    launch_symmetrize(s, n, n, dCL);
    // X0_L (:137-142): x0 = U y -> symmetrize -> U U' x0 -> round
    if (r > 0) {
        st = h2d_sync(c, coef, y.data(), (size_t)r * 8);
        if (st) return st;
        launch_tall_times_small(s, len, len, U, (int)r, coef, (int)r, 1, 1.0, 0.0, v2, len);
    } else {
        HIP_TRY(c, hipMemsetAsync(v2, 0, (size_t)len * 8, s));
    }
    launch_symmetrize(s, n, n, v2);
    launch_proj_coef(s, len, r, U, nullptr, 0, v2, partial, nblk, coef);
    launch_proj_apply(s, len, r, U, nullptr, 0, v2, coef, 0, 1, 0, v1, nullptr);  // v1 = x0 - U U'x0
    launch_sub_round(s, len, v2, v1, atol, scale, dX0);                           // X0_L = round(x0 - v1)
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}
}  // namespace sdpsr

extern "C" {
// Setup stage for dense problems on the device, src/partitions.jl:117-142:
//   U    orthonormal basis of rowspace(A): modified Gram-Schmidt on the residual rows with
//        pivoting by residual norm and one re-orthogonalisation pass (stands in for qr(A'));
//   C_L  = symmetrize(round(c - U U'c));   X0_L = round(U U' symmetrize(x0)),  x0 = U R^-T b
// All vectors of length n^2 stay in HBM; the host sees m-vectors of dot products only.
int sdpsr_admissible_subspace_dense(sdpsr_ctx* c, int64_t n, int64_t m, const double* C,
                                    const double* A, const double* b, double atol, uint32_t* P_out,
                                    int64_t* dim_out, int32_t* iters_out, double* phase_ms,
                                    int mem_out) {
    CHECK_CTX(c);
    c->hint_symmetric_basis = 0;  // hints describe caller-made CL / X0L / U; here the library makes them itself
    if (!C || !A || !b || !P_out || !dim_out || n < 1 || m < 0 || !(atol > 0)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const int64_t len = n * n;
    int st = check_len(c, len);
    if (st) return st;
    hipStream_t s = c->stream;
    const int64_t mm = std::max<int64_t>(m, 1);
    const int nblk = 2048;
    double* dA = (double*)ctx_buf(c, "set_a", (size_t)len * mm * 8);   // m x len as given
    double* R = (double*)ctx_buf(c, "set_r", (size_t)len * mm * 8);    // residual rows, len x m
    double* U = (double*)ctx_buf(c, "adm_u", (size_t)len * mm * 8);    // basis, len x r
    double* v1 = (double*)ctx_buf(c, "set_v1", (size_t)len * 8);
    double* v2 = (double*)ctx_buf(c, "set_v2", (size_t)len * 8);
    double* dCL = (double*)ctx_buf(c, "adm_cl", (size_t)len * 8);
    double* dX0 = (double*)ctx_buf(c, "adm_x0", (size_t)len * 8);
    double* partial = (double*)ctx_buf(c, "proj_partial", (size_t)mm * nblk * 8);
    double* coef = (double*)ctx_buf(c, "proj_coef", (size_t)mm * 8);
    if (!dA || !R || !U || !v1 || !v2 || !dCL || !dX0 || !partial || !coef) return SDPSR_OUT_OF_MEMORY;
    if (m > 0) HIP_TRY(c, hipMemcpyAsync(dA, A, (size_t)len * m * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(v1, C, (size_t)len * 8, hipMemcpyHostToDevice, s));  // v1 = c
    if (m > 0) launch_transpose_rows(s, len, m, dA, R);  // R[e + i*len] = A[i + e*m]
    std::vector<std::vector<double>> coeffs;
    std::vector<int64_t> piv;
    int64_t r = 0;
    st = setup_mgs(c, len, m, R, U, partial, nblk, coef, coeffs, piv, &r);
    if (st) return st;
    st = setup_tail(c, n, r, U, min_norm_coefficients(r, piv, coeffs, b), atol, v1, v2, dCL, dX0, partial, nblk, coef);
    if (st) return st;
    // the loop, device-resident inputs
    int st_buf = SDPSR_OK;
    uint32_t* dP = labels_out_dev(c, "adm_labels", P_out, (size_t)len, mem_out, &st_buf);
    if (!dP) return SDPSR_OUT_OF_MEMORY;
    st = admissible_subspace_impl(c, n, dCL, dX0, U, r, atol, dP, dim_out, iters_out, phase_ms, SDPSR_MEM_DEVICE, SDPSR_MEM_DEVICE, true, nullptr);  // (dP: uint32 labels)
    if (st && st != SDPSR_NOT_CONVERGED) return st;
    const int st_loop = st;
    if (label_width_overflows(c, (uint64_t)*dim_out)) return label_width_fail(c, "admissible_subspace", (uint64_t)*dim_out);  // (P_out untouched)
    st = labels_out_finish(c, P_out, dP, len, mem_out);
    return st ? st : st_loop;
}
}  // extern "C"
