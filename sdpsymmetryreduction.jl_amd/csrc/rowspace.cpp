// Removing the linearly dependent reduced constraints: an orthonormal basis of the row space of M = [A * PMat, b] and its rank
// (docs/src/examples/ReduceAndSolveJuMP.jl:44-50: svd(Matrix(M)').U[:, 1:rank(M)]', droptol!; "Removing linearly dependent
// constraints", docs/src/examples/QuadraticAssignmentProblems.jl:116-122).  DESIGN.md "Dependent reduced constraints".
//
// W = M (scaled by a power of two) lives in `out` from the first kernel on.  A pass forms G = W W' on the device
// (kernels_rowspace.hip), reads it back -- the pass's one host wait, m^2 doubles -- lets the host find the Jacobi rotations J
// of G under the relative rule (host_gram_jacobi.cpp), and rotates the rows, W <- J W, in place.  The next G is formed from
// the new W, never updated algebraically: the products of rows that are already nearly orthogonal are accurate relative to
// those rows' own norms, which is what finds singular values down to eps sigma_1 where one eigen-decomposition of G stops
// at sqrt(eps) sigma_1.  The iteration ends with the first pass whose rotations all lie inside the rounding error of G (they
// are still applied) or that makes none; the diagonal of its rotated G holds the squared singular values.
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>

#include "host_internal.h"

using namespace sdpsr;

namespace {
constexpr int64_t COMPRESS_MAX_M = 1024;  // sdpsr.h
constexpr int COMPRESS_MAX_PASSES = 16;
constexpr int COMPRESS_MAX_SWEEPS = 60;
}  // namespace

extern "C" int sdpsr_compress_constraints(sdpsr_ctx* c, int64_t m, int64_t d, const double* newA, const double* b, double rtol,
                                          double droptol, double* out, int64_t* rank_out, double* sv, int64_t* nnz_out,
                                          int32_t* passes_out, int mem) {
    CHECK_CTX(c);
    if (!rank_out || m < 0 || d < 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    if (!(rtol >= 0) || std::isinf(rtol)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "compress_constraints: rtol must be finite and >= 0");
    if (!(droptol >= 0)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "compress_constraints: droptol must be >= 0");
    if (m > COMPRESS_MAX_M) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "compress_constraints: m > 1024 rows");
    const int64_t ncols = d + (b ? 1 : 0);
    if (ncols > (int64_t(1) << 40)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "compress_constraints: too many columns");
    *rank_out = 0;
    if (nnz_out) *nnz_out = 0;
    if (passes_out) *passes_out = 0;
    if (sv) std::fill(sv, sv + m, 0.0);
    if (m == 0 || ncols == 0) return SDPSR_OK;  // no element of out exists
    if ((d > 0 && !newA) || !out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const int64_t md = m * d, total = m * ncols, mm = m * m;
    hipStream_t s = c->stream;
    int st = SDPSR_OK;
    const double* dA = md ? in_dev(c, "cc_a", newA, (size_t)md, mem, &st) : nullptr;
    double* W = out_dev(c, "cc_out", out, (size_t)total, mem, &st);
    double* db = b ? (double*)ctx_buf(c, "cc_b", (size_t)m * 8) : nullptr;
    double* pmax = (double*)ctx_buf(c, "cc_pmax", (size_t)rowspace_absmax_blocks(total) * 8);
    double* pack = (double*)ctx_buf(c, "cc_pack", (size_t)(8 + mm) * 8);  // [max |M|, non-finite verdict, - x 6][G]
    double* P = (double*)ctx_buf(c, "cc_partials", rowspace_gram_partial_doubles(m, ncols) * 8);
    double* dJ = (double*)ctx_buf(c, "cc_j", (size_t)mm * 8);
    double* tab = (double*)ctx_buf(c, "cc_tab", (size_t)m * 24 + 8);  // sigma (m), sig (m), the count of non-zeros, perm (m int32)
    uint32_t* flag = (uint32_t*)ctx_buf(c, "prim_flag", 64);
    if (st || !W || (b && !db) || !pmax || !pack || !P || !dJ || !tab || !flag || !c->pinned_small) return st ? st : SDPSR_OUT_OF_MEMORY;
    if (b && (st = h2d_sync(c, db, b, (size_t)m * 8))) return st;
    HIP_TRY(c, hipMemsetAsync(flag, 0, 4, s));
    launch_rowspace_scale(s, total, md, dA, db, pmax, flag, W, pack);

    const double eps = std::numeric_limits<double>::epsilon();
    const double rt = rtol > 0 ? rtol : (double)std::min(m, ncols) * eps;  // Julia's rank(M): min(size(M)...) * eps
    // the relative rule rotates down to eps; the STOP looks at what a pass rotated away: a computed product of two rows carries a
    // rounding error of about sqrt(ncols) eps |w_p| |w_q|, and once nothing above twice that was left, another G could not tell more
    const double tau = eps, tau_stop = 2.0 * std::sqrt((double)ncols) * eps;
    std::vector<double> h((size_t)(8 + mm)), J((size_t)mm);
    double* G = h.data() + 8;
    int passes = 0;
    bool converged = false;
    double scale = 1.0;
    for (;;) {
        launch_rowspace_gram(s, m, ncols, W, P, pack + 8);
        HIP_TRY(c, hipGetLastError());
        st = d2h_sync(c, h.data(), pack, (size_t)(8 + mm) * 8);
        if (st) return st;
        if (passes == 0) {
            if (h[1] != 0.0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "compress_constraints: non-finite value");  // (W = out is not written)
            scale = rowspace_scale(h[0]);
        }
        if (passes == COMPRESS_MAX_PASSES) break;  // (this G is only read for its diagonal)
        ++passes;
        int sweeps = 0;
        double max_rel = 0.0;
        const int64_t rot = host_gram_jacobi((int)m, G, J.data(), tau, rt * rt, COMPRESS_MAX_SWEEPS, &sweeps, &max_rel);  // (G <- J G J')
        if (dbg_on())
            fprintf(stderr, "[sdpsr] compress_constraints pass %d: %lld rotations in %d sweeps, largest %.3g\n", passes, (long long)rot, sweeps, max_rel);
        if (rot > 0) {
            st = h2d_sync(c, dJ, J.data(), (size_t)mm * 8);
            if (st) return st;
            launch_rowspace_rotate(s, m, ncols, dJ, W);
        }
        if (max_rel <= tau_stop) {  // (rotations this small move the diagonal of G by less than its last bit)
            converged = true;
            break;
        }
    }

    // sigma = the row norms, descending, ties by row index; rank = those above rt sigma_1
    std::vector<double> sigma((size_t)m);
    for (int64_t p = 0; p < m; ++p) sigma[p] = G[p * m + p] > 0 ? std::sqrt(G[p * m + p]) : 0.0;
    std::vector<int32_t> perm((size_t)m);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t bb) { return sigma[a] > sigma[bb]; });
    std::vector<double> sorted((size_t)m);
    for (int64_t k = 0; k < m; ++k) sorted[k] = sigma[perm[k]];
    int64_t r = 0;
    while (r < m && sorted[0] > 0 && sorted[r] > rt * sorted[0]) ++r;
    double* d_sigma = tab;
    double* d_sig = tab + m;
    unsigned long long* d_nnz = (unsigned long long*)(tab + 2 * m);
    int32_t* d_perm = (int32_t*)(tab + 2 * m + 1);
    if ((st = h2d_sync(c, d_sigma, sorted.data(), (size_t)m * 8))) return st;
    if ((st = h2d_sync(c, d_perm, perm.data(), (size_t)m * 4))) return st;
    HIP_TRY(c, hipMemsetAsync(d_nnz, 0, 8, s));
    launch_rowspace_finish(s, m, ncols, r, W, d_perm, d_sigma, d_sig, droptol, W, d_nnz);
    HIP_TRY(c, hipGetLastError());
    uint32_t* hn = c->pinned_small + PINNED_SMALL_ROWSPACE_NNZ.first;
    HIP_TRY(c, hipMemcpyAsync(hn, d_nnz, 8, hipMemcpyDeviceToHost, s));
    st = out_finish(c, out, W, (size_t)total, mem);
    if (st) return st;
    uint64_t nnz;
    memcpy(&nnz, hn, 8);
    *rank_out = r;
    if (nnz_out) *nnz_out = (int64_t)nnz;
    if (passes_out) *passes_out = passes;
    if (sv)
        for (int64_t k = 0; k < m; ++k) sv[k] = sorted[k] / scale;
    if (!converged) return ctx_fail(c, SDPSR_NOT_CONVERGED, "compress_constraints: pass limit reached");
    return SDPSR_OK;
}
