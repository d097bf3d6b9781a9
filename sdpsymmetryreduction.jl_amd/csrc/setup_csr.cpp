// Setup stage of admissible_subspace from a sparse constraint matrix given as CSR, src/partitions.jl:117-142 with
// projL of src/utils.jl:58-66: the rows of A are validated and canonicalised on the host (O(nnz)), uploaded as CSR,
// densified on the device into the columns of one len x m buffer W that becomes the basis U in place, and
// orthonormalised there -- CholeskyQR2 when the rows are clearly independent, the pivoted MGS of the dense entry
// otherwise (DESIGN.md "Setup from a sparse A").
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "host_internal.h"

using namespace sdpsr;

// Validation + canonical form: sort each row by column (stable: duplicates keep their input order), sum duplicates in
// that order, drop zeros.  Shared with the reduced-SDP assembly (reduce_csr.cpp): one definition of what a CSR input means.
int sdpsr::canonicalize_csr(sdpsr_ctx* c, int64_t len, int64_t m, const int64_t* rowptr, const int64_t* colind, const double* val,
                            int base, CanonCsr& out) {
    if (base != 0 && base != 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "index_base must be 0 or 1");
    if (m == 0) {
        out.rowptr.assign(1, 0);
        return SDPSR_OK;
    }
    if (!rowptr) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowptr is NULL");
    if (rowptr[0] != base) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowptr[0] != index_base");
    for (int64_t i = 0; i < m; ++i)
        if (rowptr[i + 1] < rowptr[i]) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowptr is not monotone at row " + std::to_string(i));
    const int64_t nnz = rowptr[m] - base;
    if (nnz > 0 && (!colind || !val)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "colind / val is NULL");
    for (int64_t p = 0; p < nnz; ++p) {
        const int64_t k = colind[p] - base;
        if (k < 0 || k >= len) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "column index out of [0, n^2) at entry " + std::to_string(p));
        if (!std::isfinite(val[p])) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "non-finite value at entry " + std::to_string(p));
    }
    out.rowptr.assign(m + 1, 0);
    out.col.clear();
    out.val.clear();
    out.col.reserve(nnz);
    out.val.reserve(nnz);
    std::vector<int64_t> order;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t a = rowptr[i] - base, b = rowptr[i + 1] - base;
        bool sorted = true;  // strictly increasing already (the usual input): no sort
        for (int64_t p = a + 1; p < b && sorted; ++p) sorted = colind[p] > colind[p - 1];
        auto push = [&](int64_t k, double v) {
            if (v != 0.0) {
                out.col.push_back((uint32_t)k);
                out.val.push_back(v);
            }
        };
        if (sorted) {
            for (int64_t p = a; p < b; ++p) push(colind[p] - base, val[p]);
        } else {
            order.resize(b - a);
            std::iota(order.begin(), order.end(), a);
            std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return colind[x] < colind[y]; });
            for (size_t q = 0; q < order.size();) {
                const int64_t k = colind[order[q]];
                double s = val[order[q]];
                size_t t = q + 1;
                for (; t < order.size() && colind[order[t]] == k; ++t) s += val[order[t]];
                if (!std::isfinite(s)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "duplicate entries sum to a non-finite value");
                push(k - base, s);
                q = t;
            }
        }
        out.rowptr[i + 1] = (int64_t)out.col.size();
    }
    return SDPSR_OK;
}

namespace {

// every row is a symmetric n x n matrix, bit for bit: the transposed position of every entry is present with the same bits
bool csr_rows_symmetric(const CanonCsr& out, int64_t n) {
    const int64_t m = (int64_t)out.rowptr.size() - 1;
    for (int64_t i = 0; i < m; ++i) {
        const uint32_t* c0 = out.col.data() + out.rowptr[i];
        const uint32_t* c1 = out.col.data() + out.rowptr[i + 1];
        for (const uint32_t* p = c0; p < c1; ++p) {
            const uint64_t k = *p, r = k % (uint64_t)n, q = k / (uint64_t)n;
            if (r == q) continue;
            const uint32_t t = (uint32_t)(q + r * (uint64_t)n);
            const uint32_t* f = std::lower_bound(c0, c1, t);
            if (f == c1 || *f != t ||
                std::memcmp(&out.val[f - out.col.data()], &out.val[p - out.col.data()], sizeof(double)) != 0) {
                return false;
            }
        }
    }
    return true;
}

// Cholesky of a symmetric m x m matrix G (column-major) into an upper-triangular R (row-major, G[perm][:, perm] = R'R).
// pivoting: diagonal pivoting by the largest residual.  Returns false as soon as a pivot's residual norm falls below
// `floor` (the rows are not clearly independent).
bool cholesky_upper(const double* G, int64_t m, bool pivoting, double floor, std::vector<double>& R, std::vector<int64_t>& perm) {
    std::vector<double> S(G, G + (size_t)m * m);  // symmetric: row-major = column-major
    R.assign((size_t)m * m, 0.0);
    perm.resize(m);
    std::iota(perm.begin(), perm.end(), 0);
    for (int64_t k = 0; k < m; ++k) {
        if (pivoting) {
            int64_t p = k;
            for (int64_t i = k + 1; i < m; ++i)
                if (S[i * m + i] > S[p * m + p]) p = i;
            if (p != k) {
                for (int64_t j = 0; j < m; ++j) std::swap(S[k * m + j], S[p * m + j]);
                for (int64_t i = 0; i < m; ++i) std::swap(S[i * m + k], S[i * m + p]);
                for (int64_t j = 0; j < k; ++j) std::swap(R[j * m + k], R[j * m + p]);
                std::swap(perm[k], perm[p]);
            }
        }
        const double d = S[k * m + k];
        if (!(d > 0) || !(std::sqrt(d) >= floor)) return false;
        const double rkk = std::sqrt(d);
        R[k * m + k] = rkk;
        for (int64_t i = k + 1; i < m; ++i) R[k * m + i] = S[k * m + i] / rkk;
        for (int64_t i = k + 1; i < m; ++i) {
            const double ri = R[k * m + i];
            for (int64_t j = k + 1; j < m; ++j) S[i * m + j] -= ri * R[k * m + j];
        }
    }
    return true;
}

// X = R^-1 (upper triangular, row-major like R): back substitution column by column
std::vector<double> upper_inverse(const std::vector<double>& R, int64_t m) {
    std::vector<double> X((size_t)m * m, 0.0);
    for (int64_t j = 0; j < m; ++j) {
        X[j * m + j] = 1.0 / R[j * m + j];
        for (int64_t i = j - 1; i >= 0; --i) {
            double s = 0;
            for (int64_t k = i + 1; k <= j; ++k) s += R[i * m + k] * X[k * m + j];
            X[i * m + j] = -s / R[i * m + i];
        }
    }
    return X;
}

constexpr size_t PINNED_OFF = 8192;  // the refinement's reports live at the start of the pinned area

// the checks every setup entry makes before it looks at A
int setup_check_arguments(sdpsr_ctx* c, int64_t n, int64_t m, const double* b, const double* C, double atol) {
    if (!C || n < 1 || m < 0 || (m > 0 && !b) || !(atol > 0)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = check_len(c, n * n);
    if (st) return st;
    if (m > 0x7FFFFFFF) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "m too large");
    return SDPSR_OK;
}

// the _csr entries: the host pass, the upload of the canonical arrays into the ctx's CSR buffers, then the stage itself
int setup_csr_impl(sdpsr_ctx* c, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* colind, const double* val, int base,
                   const double* b, const double* C, double atol, CsrSetupOut& o) {
    int st = setup_check_arguments(c, n, m, b, C, atol);
    if (st) return st;
    const int64_t len = n * n;
    CanonCsr A;
    st = canonicalize_csr(c, len, m, rowptr, colind, val, base, A);
    if (st) return st;
    const bool symmetric = csr_rows_symmetric(A, n);
    for (int64_t i = 0; i < m; ++i)
        if (!std::isfinite(b[i])) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "non-finite b");
    hipStream_t s = c->stream;
    const int64_t nnz = (int64_t)A.col.size();
    double* W = m > 0 ? (double*)ctx_buf(c, "csr_w", (size_t)len * m * 8) : nullptr;  // (the largest buffer first: its failure costs nothing else)
    if (m > 0 && !W) return SDPSR_OUT_OF_MEMORY;
    int64_t* drp = (int64_t*)ctx_buf(c, "csr_rowptr", (size_t)(m + 1) * 8);
    uint32_t* dcol = (uint32_t*)ctx_buf(c, "csr_col", (size_t)std::max<int64_t>(nnz, 1) * 4);
    double* dval = (double*)ctx_buf(c, "csr_val", (size_t)std::max<int64_t>(nnz, 1) * 8);
    if (!drp || !dcol || !dval) return SDPSR_OUT_OF_MEMORY;
    // (pageable sources: the copies have read them by the stage's first host wait; A lives until the return)
    if (m > 0) {
        HIP_TRY(c, hipMemcpyAsync(drp, A.rowptr.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            HIP_TRY(c, hipMemcpyAsync(dcol, A.col.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(dval, A.val.data(), (size_t)nnz * 8, hipMemcpyHostToDevice, s));
        }
        c->h2d_bytes += (size_t)(m + 1) * 8 + (size_t)nnz * 12;
    }
    st = setup_from_device_csr(c, n, m, drp, dcol, dval, nnz, symmetric, b, C, atol, o);
    if (st && m > 0) (void)ctx_sync_stream(c, s);  // (a failure before the stage's first wait: the copies still read A)
    return st;
}

}  // namespace

// The setup stage from canonical CSR arrays that are on the device already: every kernel sees the same inputs with the same
// launch geometry whether the arrays came from the host pass above or from a handle (sdpsr_admissible_setup_sparse)
int sdpsr::setup_from_device_csr(sdpsr_ctx* c, int64_t n, int64_t m, const int64_t* drp, const uint32_t* dcol, const double* dval, int64_t nnz,
                                 bool symmetric, const double* b, const double* C, double atol, CsrSetupOut& o) {
    (void)nnz;
    const int64_t len = n * n;
    int st = SDPSR_OK;
    hipStream_t s = c->stream;
    const int64_t mm = std::max<int64_t>(m, 1);
    const int nblk = 2048;
    double* W = m > 0 ? (double*)ctx_buf(c, "csr_w", (size_t)len * m * 8) : nullptr;  // A's rows as columns, then U
    if (m > 0 && !W) return SDPSR_OUT_OF_MEMORY;
    double* v1 = (double*)ctx_buf(c, "set_v1", (size_t)len * 8);
    double* v2 = (double*)ctx_buf(c, "set_v2", (size_t)len * 8);
    o.CL = (double*)ctx_buf(c, "adm_cl", (size_t)len * 8);
    o.X0 = (double*)ctx_buf(c, "adm_x0", (size_t)len * 8);
    double* partial = (double*)ctx_buf(c, "proj_partial", (size_t)mm * nblk * 8);
    double* coef = (double*)ctx_buf(c, "proj_coef", (size_t)mm * 8);
    double* gpart = m > 0 ? (double*)ctx_buf(c, "csr_gram_part", gram_tall_partial_doubles(len, m) * 8) : nullptr;
    double* dX = m > 0 ? (double*)ctx_buf(c, "csr_x", (size_t)m * m * 8) : nullptr;
    int32_t* dpiv = m > 0 ? (int32_t*)ctx_buf(c, "csr_piv", (size_t)m * 4) : nullptr;
    if (!v1 || !v2 || !o.CL || !o.X0 || !partial || !coef || (m > 0 && (!gpart || !dX || !dpiv))) return SDPSR_OUT_OF_MEMORY;
    // pinned staging of the small m x m traffic: G (written by the Gram kernel), X and piv (uploaded in stream order)
    char* pin = m > 0 ? (char*)ctx_pinned(c, PINNED_OFF + (size_t)m * m * 16 + (size_t)m * 4) : nullptr;
    if (m > 0 && !pin) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "pinned staging");
    double* hG = m > 0 ? (double*)(pin + PINNED_OFF) : nullptr;
    double* hX = m > 0 ? hG + (size_t)m * m : nullptr;
    int32_t* hpiv = m > 0 ? (int32_t*)(hX + (size_t)m * m) : nullptr;
    // (a pageable source: the copy has read it by the first host wait below)
    HIP_TRY(c, hipMemcpyAsync(v1, C, (size_t)len * 8, hipMemcpyHostToDevice, s));  // v1 = c
    c->h2d_bytes += (size_t)len * 8;
    o.hint = symmetric ? 3 : 0;
    std::vector<std::vector<double>> coeffs;  // coeffs[i][j]: coefficient of U's column j in row i (as setup_mgs has them)
    std::vector<int64_t> piv;
    int64_t r = 0;
    bool fast = false;
    std::vector<double> y;
    if (m > 0) {
        launch_csr_densify(s, len, m, drp, dcol, dval, W);
        launch_gram_tall(s, len, m, W, gpart, hG);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, ctx_sync_stream(c, s));  // host wait 1: G = A A'
        double maxn2 = 0;
        for (int64_t i = 0; i < m; ++i) maxn2 = std::max(maxn2, hG[i * m + i]);
        const double maxnorm = std::sqrt(maxn2);
        std::vector<double> R1;
        // fast path: every pivot's residual norm >= 1e-4 of the largest row norm (a Gram matrix cannot resolve residuals
        // below ~sqrt(eps) of the row norms; the MGS decides rank at 1e-12)
        fast = maxnorm > 0 && cholesky_upper(hG, m, true, 1e-4 * maxnorm, R1, piv);
        if (fast) {
            // pass 1: W <- W[:, piv] R1^-1 (column j of the result in slot piv[j])
            std::vector<double> X1 = upper_inverse(R1, m);
            std::memcpy(hX, X1.data(), (size_t)m * m * 8);
            for (int64_t j = 0; j < m; ++j) hpiv[j] = (int32_t)piv[j];
            HIP_TRY(c, hipMemcpyAsync(dX, hX, (size_t)m * m * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(dpiv, hpiv, (size_t)m * 4, hipMemcpyHostToDevice, s));
            c->h2d_bytes += (size_t)m * m * 8 + (size_t)m * 4;
            launch_apply_upper_inverse(s, len, m, W, dpiv, dX);
            // pass 2: G2 = W'W in pivot order, W <- W R2^-1
            launch_gram_tall(s, len, m, W, gpart, hG);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, ctx_sync_stream(c, s));  // host wait 2
            std::vector<double> G2((size_t)m * m);
            for (int64_t k = 0; k < m; ++k)
                for (int64_t j = 0; j < m; ++j) G2[j + k * m] = hG[piv[j] + piv[k] * m];
            std::vector<double> R2;
            std::vector<int64_t> id;
            if (cholesky_upper(G2.data(), m, false, 0.5, R2, id)) {
                std::vector<double> X2 = upper_inverse(R2, m);
                std::memcpy(hX, X2.data(), (size_t)m * m * 8);
                HIP_TRY(c, hipMemcpyAsync(dX, hX, (size_t)m * m * 8, hipMemcpyHostToDevice, s));
                c->h2d_bytes += (size_t)m * m * 8;
                launch_apply_upper_inverse(s, len, m, W, dpiv, dX);
                // A[piv]' = U R with R = R2 R1; in setup_mgs' terms coeffs[piv[k]][j] = R[j][k]
                coeffs.assign(m, std::vector<double>(m, 0.0));
                for (int64_t j = 0; j < m; ++j)
                    for (int64_t k = j; k < m; ++k) {
                        double sum = 0;
                        for (int64_t t = j; t <= k; ++t) sum += R2[j * m + t] * R1[t * m + k];
                        coeffs[piv[k]][j] = sum;
                    }
                r = m;
                const std::vector<double> yp = min_norm_coefficients(r, piv, coeffs, b);
                y.assign(m, 0.0);
                for (int64_t j = 0; j < m; ++j) y[piv[j]] = yp[j];  // U's column j sits in slot piv[j]
                o.U = W;
                o.info = SDPSR_SETUP_CHOLESKY_QR2;
            } else {  // (not expected after the pivot rule above) start over from A on the MGS path
                fast = false;
                launch_csr_densify(s, len, m, drp, dcol, dval, W);
            }
        }
        if (!fast) {
            double* U = (double*)ctx_buf(c, "adm_u", (size_t)len * m * 8);
            if (!U) return SDPSR_OUT_OF_MEMORY;
            st = setup_mgs(c, len, m, W, U, partial, nblk, coef, coeffs, piv, &r);
            if (st) return st;
            y = min_norm_coefficients(r, piv, coeffs, b);
            o.U = U;
            o.info = SDPSR_SETUP_MGS;
        }
    }
    if (y.empty()) y.assign(1, 0.0);
    o.r = r;
    if (r == 0) o.U = nullptr;
    st = setup_tail(c, n, r, o.U, y, atol, v1, v2, o.CL, o.X0, partial, nblk, coef);
    if (st) return st;
    return SDPSR_OK;
}

namespace {

// what the two setup entries of either kind do with the stage's result
int setup_deliver(sdpsr_ctx* c, int64_t n, const CsrSetupOut& o, double* CL, double* X0L, double* U, int64_t* r_out, int* hint_out,
                  int32_t* info_out, int mem_out) {
    const int64_t len = n * n;
    const hipMemcpyKind kind = mem_out == SDPSR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(CL, o.CL, (size_t)len * 8, kind, s));
    HIP_TRY(c, hipMemcpyAsync(X0L, o.X0, (size_t)len * 8, kind, s));
    if (o.r > 0) HIP_TRY(c, hipMemcpyAsync(U, o.U, (size_t)len * o.r * 8, kind, s));
    if (mem_out != SDPSR_MEM_DEVICE) c->d2h_bytes += (size_t)len * (2 + o.r) * 8;
    HIP_TRY(c, ctx_sync_stream(c, s));
    *r_out = o.r;
    if (hint_out) *hint_out = o.hint;
    if (info_out) *info_out = o.info;
    return SDPSR_OK;
}

int subspace_after_setup(sdpsr_ctx* c, int64_t n, const CsrSetupOut& o, double atol, uint32_t* P_out, int64_t* dim_out, int32_t* iters_out,
                         double* phase_ms, int mem_out) {
    const int64_t len = n * n;
    int st_buf = SDPSR_OK;
    uint32_t* dP = labels_out_dev(c, "adm_labels", P_out, (size_t)len, mem_out, &st_buf);
    if (!dP) return SDPSR_OUT_OF_MEMORY;
    c->hint_symmetric_basis = o.hint;  // proved by the setup: symmetric rows, position-independent arithmetic
    int st = admissible_subspace_impl(c, n, o.CL, o.X0, o.U, o.r, atol, dP, dim_out, iters_out, phase_ms, SDPSR_MEM_DEVICE, SDPSR_MEM_DEVICE, true, nullptr);  // (dP: uint32 labels)
    if (st && st != SDPSR_NOT_CONVERGED) return st;
    const int st_loop = st;
    if (label_width_overflows(c, (uint64_t)*dim_out)) return label_width_fail(c, "admissible_subspace", (uint64_t)*dim_out);  // (P_out untouched)
    st = labels_out_finish(c, P_out, dP, len, mem_out);
    return st ? st : st_loop;
}

// the _sparse entries: the handle's arrays are the stage's inputs as they lie
int setup_sparse_impl(sdpsr_ctx* c, int64_t n, const sdpsr_sparse* A, const double* b, const double* C, double atol, CsrSetupOut& o) {
    if (!A) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "no sparse handle");
    if (A->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "the sparse handle lives on another device");
    int st = setup_check_arguments(c, n, A->m, b, C, atol);
    if (st) return st;
    if (n * n != A->len) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "n^2 != len of the sparse handle");
    for (int64_t i = 0; i < A->m; ++i)
        if (!std::isfinite(b[i])) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "non-finite b");
    return setup_from_device_csr(c, n, A->m, A->rowptr, A->col, A->val, A->nnz, A->rows_symmetric != 0, b, C, atol, o);
}

}  // namespace

extern "C" {

int sdpsr_admissible_setup_csr(sdpsr_ctx* c, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* colind, const double* val,
                               int index_base, const double* b, const double* C, double atol, double* CL, double* X0L, double* U,
                               int64_t* r_out, int* hint_out, int32_t* info_out, int mem_out) {
    CHECK_CTX(c);
    c->hint_symmetric_basis = 0;
    if (!CL || !X0L || !r_out || (m > 0 && !U)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    CsrSetupOut o;
    int st = setup_csr_impl(c, n, m, rowptr, colind, val, index_base, b, C, atol, o);
    if (st) return st;
    return setup_deliver(c, n, o, CL, X0L, U, r_out, hint_out, info_out, mem_out);
}

// the same stage on a handle's arrays (sdpsr_sparse_create): no host pass, no upload of A
int sdpsr_admissible_setup_sparse(sdpsr_ctx* c, int64_t n, const sdpsr_sparse* A, const double* b, const double* C, double atol, double* CL,
                                  double* X0L, double* U, int64_t* r_out, int* hint_out, int32_t* info_out, int mem_out) {
    CHECK_CTX(c);
    c->hint_symmetric_basis = 0;
    if (!A || !CL || !X0L || !r_out || (A->m > 0 && !U)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    CsrSetupOut o;
    int st = setup_sparse_impl(c, n, A, b, C, atol, o);
    if (st) return st;
    return setup_deliver(c, n, o, CL, X0L, U, r_out, hint_out, info_out, mem_out);
}

int sdpsr_admissible_subspace_sparse(sdpsr_ctx* c, int64_t n, const sdpsr_sparse* A, const double* b, const double* C, double atol,
                                     uint32_t* P_out, int64_t* dim_out, int32_t* iters_out, double* phase_ms, int mem_out) {
    CHECK_CTX(c);
    c->hint_symmetric_basis = 0;
    if (!A || !P_out || !dim_out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    CsrSetupOut o;
    int st = setup_sparse_impl(c, n, A, b, C, atol, o);
    if (st) return st;
    return subspace_after_setup(c, n, o, atol, P_out, dim_out, iters_out, phase_ms, mem_out);
}

int sdpsr_admissible_subspace_csr(sdpsr_ctx* c, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* colind, const double* val,
                                  int index_base, const double* b, const double* C, double atol, uint32_t* P_out, int64_t* dim_out,
                                  int32_t* iters_out, double* phase_ms, int mem_out) {
    CHECK_CTX(c);
    c->hint_symmetric_basis = 0;
    if (!P_out || !dim_out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    CsrSetupOut o;
    int st = setup_csr_impl(c, n, m, rowptr, colind, val, index_base, b, C, atol, o);
    if (st) return st;
    return subspace_after_setup(c, n, o, atol, P_out, dim_out, iters_out, phase_ms, mem_out);
}

}  // extern "C"
