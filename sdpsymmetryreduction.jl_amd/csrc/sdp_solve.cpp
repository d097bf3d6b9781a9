// The last step of the reference's work flow on the device: the reduced SDP
//     max / min c'x   s.t.   A x = b,   x >= 0,   Z_k(x) = sum_i x_i blks[i][k] in PSDCone() for all k
// (reduceAndSolve, docs/src/examples/ReduceAndSolveJuMP.jl:40-91; test/sd_problems.jl:29-55,107-137 of the reference, which
// hands the model to CSDP through JuMP) solved by a first-order method (ADMM) over the operator handle of blockop.cpp, and the
// batched projection onto the PSD cone it is built on (sdpsr_psd_project).  include/sdpsr.h states the iteration and the
// contract; the kernels are kernels_psd.hip (cone step, fused with the dual update) and kernels_sdp.hip (Gram matrix, dense
// setup products, affine step); the pencil and its adjoint are kernels_blockop.hip through their enqueue-only forms.
#include <cmath>

#include "host_internal.h"

using namespace sdpsr;

namespace {

constexpr int64_t SDP_MAX_D = 4096, SDP_MAX_R = 1024;
constexpr int PSD_SMALL_ORDER = 64;  // the reach of the ping-pong core (jacobi64.h); above it, up to the ctx's psd_max_order: the mid kernel

struct PsdPlan {
    // ONE table: the blocks of order 2 .. 64, those of order 1, then the mid blocks (65 .. 128) -- of those, first the nglob
    // whose eigenvectors live in global memory (slice = position among the mid jobs), then the ones that keep them in LDS
    std::vector<PsdJob> jobs;
    int njac = 0, n1 = 0, max_n = 0;
    int nmid = 0, nglob = 0;
    size_t mid_lds = 0;
    int64_t sum_sq = 0;
};

bool psd_plan(sdpsr_ctx* c, const char* who, int32_t nblocks, const int32_t* sizes, PsdPlan& p) {
    const int cap = c->psd_max_order;
    if (nblocks < 1 || !sizes) {
        ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": nblocks < 1 or blk_sizes is NULL");
        return false;
    }
    std::vector<int64_t> off((size_t)nblocks);
    int64_t sum = 0;
    for (int32_t k = 0; k < nblocks; ++k) {
        const int64_t s = sizes[k];
        if (s < 1) {
            ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": a block size is < 1");
            return false;
        }
        if (s > cap) {
            ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": block " + std::to_string(k) + " has order " + std::to_string(s) +
                                                ": orders above " + std::to_string(cap) + " are not supported by the PSD projection");
            return false;
        }
        off[k] = sum;
        sum += s * s;
        if (sum >= (int64_t(1) << 32)) {
            ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": sum s_k^2 >= 2^32: positions are indexed with 32 bits");
            return false;
        }
    }
    p.sum_sq = sum;
    for (int32_t k = 0; k < nblocks; ++k)
        if (sizes[k] >= 2 && sizes[k] <= PSD_SMALL_ORDER) {
            p.jobs.push_back({off[k], sizes[k], k});
            p.max_n = std::max(p.max_n, (int)sizes[k]);
            ++p.njac;
        }
    for (int32_t k = 0; k < nblocks; ++k)
        if (sizes[k] == 1) {
            p.jobs.push_back({off[k], 1, k});
            ++p.n1;
        }
    for (int pass = 0; pass < 2; ++pass)
        for (int32_t k = 0; k < nblocks; ++k)
            if (sizes[k] > PSD_SMALL_ORDER && psd_mid_v_in_global(sizes[k]) == (pass == 0)) {
                p.jobs.push_back({off[k], sizes[k], k});
                p.mid_lds = std::max(p.mid_lds, psd_mid_lds_bytes(sizes[k]));
                ++p.nmid;
                if (pass == 0) ++p.nglob;
            }
    return true;
}

// the eigenvector slices of the mid blocks that do not fit the LDS (nullptr with *st untouched when there is none)
double* psd_mid_scratch(sdpsr_ctx* c, const PsdPlan& p, const char* name, int* st) {
    if (p.nglob == 0) return nullptr;
    double* v = (double*)ctx_buf(c, name, (size_t)p.nglob * PSD_MID_VSLICE * sizeof(double));
    if (!v && !*st) *st = SDPSR_OUT_OF_MEMORY;
    return v;
}

// both launches of a projection over the uploaded table: the blocks of order <= 64, then the mid blocks; either is skipped when empty
void psd_launch_plan(hipStream_t s, const PsdPlan& p, const PsdJob* djobs, const double* Z, double* P, double* lam_min, double* Lam,
                     double* D, double* slots, double* vmid, int* flag) {
    launch_psd_project(s, djobs, p.njac, p.n1, p.max_n, Z, P, lam_min, Lam, D, slots, flag);
    launch_psd_project_mid(s, djobs + p.njac + p.n1, p.nmid, p.mid_lds, Z, P, lam_min, Lam, D, slots, vmid, flag);
}

// the job table on the device (stream-ordered) and the flag word, zeroed
int psd_upload_plan(sdpsr_ctx* c, const PsdPlan& p, const char* jobs_name, const char* flag_name, PsdJob** djobs, int** dflag) {
    *djobs = (PsdJob*)ctx_buf(c, jobs_name, p.jobs.size() * sizeof(PsdJob));
    *dflag = (int*)ctx_buf(c, flag_name, 16);
    if (!*djobs || !*dflag) return SDPSR_OUT_OF_MEMORY;
    const int st = h2d_sync(c, *djobs, p.jobs.data(), p.jobs.size() * sizeof(PsdJob));
    if (st) return st;
    HIP_TRY(c, hipMemsetAsync(*dflag, 0, 16, c->stream));
    return SDPSR_OK;
}

bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// a host copy of `count` doubles that live in `mem` (device arrays cost one wait)
int host_copy(sdpsr_ctx* c, const double* p, size_t count, int mem, std::vector<double>& out) {
    out.resize(count);
    if (count == 0) return SDPSR_OK;
    if (mem != SDPSR_MEM_DEVICE) {
        memcpy(out.data(), p, count * 8);
        return SDPSR_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(out.data(), p, count * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    c->d2h_bytes += count * 8;
    return SDPSR_OK;
}

// G (r x r, column-major, symmetrised in place) -> G^-1 by Cholesky; false: a pivot at rounding level -- dependent rows
bool host_spd_inverse(int64_t r, std::vector<double>& G) {
    for (int64_t j = 0; j < r; ++j)
        for (int64_t i = j + 1; i < r; ++i) G[i + j * r] = G[j + i * r] = 0.5 * (G[i + j * r] + G[j + i * r]);
    std::vector<double> Lm((size_t)r * r, 0.0), Li((size_t)r * r, 0.0);
    for (int64_t j = 0; j < r; ++j) {
        double s = G[j + j * r];
        for (int64_t k = 0; k < j; ++k) s -= Lm[j + k * r] * Lm[j + k * r];
        if (!(s > 1e-12 * G[j + j * r]) || !(G[j + j * r] > 0.0)) return false;
        const double ljj = std::sqrt(s);
        Lm[j + j * r] = ljj;
        for (int64_t i = j + 1; i < r; ++i) {
            double t = G[i + j * r];
            for (int64_t k = 0; k < j; ++k) t -= Lm[i + k * r] * Lm[j + k * r];
            Lm[i + j * r] = t / ljj;
        }
    }
    for (int64_t j = 0; j < r; ++j) {  // Li = L^-1, column by column
        Li[j + j * r] = 1.0 / Lm[j + j * r];
        for (int64_t i = j + 1; i < r; ++i) {
            double t = 0.0;
            for (int64_t k = j; k < i; ++k) t -= Lm[i + k * r] * Li[k + j * r];
            Li[i + j * r] = t / Lm[i + i * r];
        }
    }
    for (int64_t j = 0; j < r; ++j)
        for (int64_t i = j; i < r; ++i) {
            double t = 0.0;
            for (int64_t k = i; k < r; ++k) t += Li[k + i * r] * Li[k + j * r];
            G[i + j * r] = G[j + i * r] = t;
        }
    return true;
}

struct SdpSetup {
    const double* Kt = nullptr;
    double* x0 = nullptr;
};

// M = I + B'B, M^-1 through the library's symmetric eigensolver, G = A M^-1 A' on the host, Kt and x0 (all else on the device)
int sdp_setup(sdpsr_ctx* c, const sdpsr_blockop* op, int64_t r, const double* dA, const double* db, SdpSetup& out) {
    hipStream_t s = c->stream;
    const int64_t d = op->d, nf = op->nnz_full;
    double* M = (double*)ctx_buf(c, "sdp_m", (size_t)d * d * 8);
    double* V = (double*)ctx_buf(c, "sdp_v", (size_t)d * d * 8);
    double* w = (double*)ctx_buf(c, "sdp_w", (size_t)d * 8);
    double* Minv = (double*)ctx_buf(c, "sdp_minv", (size_t)d * d * 8);
    int64_t* cptr = (int64_t*)ctx_buf(c, "sdp_cptr", (size_t)(d + 1) * 8);
    out.x0 = (double*)ctx_buf(c, "sdp_x0", (size_t)d * 8);
    if (!M || !V || !w || !Minv || !cptr || !out.x0) return SDPSR_OUT_OF_MEMORY;
    void* rec = nullptr;
    if (nf > 0) {  // the records in (class, position) order: the position-major list, sorted stably by class
        rec = ctx_buf(c, "sdp_rec", (size_t)nf * 16);
        uint32_t* cls = (uint32_t*)ctx_buf(c, "sdp_cls", (size_t)nf * 4);
        uint32_t *kA = (uint32_t*)ctx_buf(c, "bop_ka", (size_t)nf * 4), *kB = (uint32_t*)ctx_buf(c, "bop_kb", (size_t)nf * 4);
        uint32_t *vA = (uint32_t*)ctx_buf(c, "bop_va", (size_t)nf * 4), *vB = (uint32_t*)ctx_buf(c, "bop_vb", (size_t)nf * 4);
        uint32_t* hist = (uint32_t*)ctx_buf(c, "bop_hist", radix_sort_hist_words(nf) * 4);
        if (!rec || !cls || !kA || !kB || !vA || !vB || !hist) return SDPSR_OUT_OF_MEMORY;
        launch_sdp_record_class(s, nf, op->by_pos, cls);
        launch_radix_sort_pairs(s, nf, std::max(1, ceil_log2((uint64_t)d)), cls, kA, kB, vA, vB, hist);
        launch_blockop_gather(s, nf, vB, op->by_pos, rec);
    }
    launch_sdp_gram(s, d, nf, rec, cptr, M);
    HIP_TRY(c, hipGetLastError());
    int st = sdpsr_syev_f64(c, d, M, w, V, SDPSR_MEM_DEVICE);
    if (st) return st;
    launch_sdp_scale_columns(s, d, w, V);
    launch_sdp_gemm(s, d, d, d, V, 1, d, V, d, 1, 1.0, 0.0, Minv, d);  // M^-1 = (V W^-1/2) (V W^-1/2)'
    HIP_TRY(c, hipGetLastError());
    if (r == 0) {
        out.Kt = Minv;
        HIP_TRY(c, hipMemsetAsync(out.x0, 0, (size_t)d * 8, s));
        return SDPSR_OK;
    }
    double* T = (double*)ctx_buf(c, "sdp_t", (size_t)d * r * 8);
    double* U = (double*)ctx_buf(c, "sdp_u", (size_t)d * r * 8);
    double* G = (double*)ctx_buf(c, "sdp_g", (size_t)(r * r) * 8);
    double* Kt = (double*)ctx_buf(c, "sdp_kt", (size_t)d * d * 8);
    if (!T || !U || !G || !Kt) return SDPSR_OUT_OF_MEMORY;
    launch_sdp_gemm(s, d, r, d, Minv, 1, d, dA, r, 1, 1.0, 0.0, T, d);  // T = M^-1 A'
    launch_sdp_gemm(s, r, r, d, dA, 1, r, T, 1, d, 1.0, 0.0, G, r);     // G = A T
    HIP_TRY(c, hipGetLastError());
    std::vector<double> hG((size_t)r * r);
    st = d2h_sync(c, hG.data(), G, (size_t)r * r * 8);
    if (st) return st;
    if (!all_finite(hG.data(), hG.size())) return ctx_fail(c, SDPSR_SOLVER_ERROR, "sdp_solve: the operator holds a non-finite value");
    if (!host_spd_inverse(r, hG)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: rows of A are dependent: compress_constraints first");
    st = h2d_sync(c, G, hG.data(), (size_t)r * r * 8);
    if (st) return st;
    launch_sdp_gemm(s, d, r, r, T, 1, d, G, 1, r, 1.0, 0.0, U, d);  // U = T G^-1
    HIP_TRY(c, hipMemcpyAsync(Kt, Minv, (size_t)d * d * 8, hipMemcpyDeviceToDevice, s));
    launch_sdp_gemm(s, d, d, r, U, 1, d, T, d, 1, -1.0, 1.0, Kt, d);    // Kt = M^-1 - U T'
    launch_sdp_gemm(s, d, 1, r, U, 1, d, db, 1, r, 1.0, 0.0, out.x0, d);  // x0 = U b
    HIP_TRY(c, hipGetLastError());
    out.Kt = Kt;
    return SDPSR_OK;
}

}  // namespace

extern "C" {

int sdpsr_psd_project(sdpsr_ctx* c, int32_t nblocks, const int32_t* blk_sizes, const double* Z, double* P, double* lambda_min, int mem) {
    CHECK_CTX(c);
    if (!Z || !P) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "psd_project: Z or P is NULL");
    PsdPlan plan;
    if (!psd_plan(c, "psd_project", nblocks, blk_sizes, plan)) return SDPSR_BAD_ARGUMENT;
    hipStream_t s = c->stream;
    const bool host = mem != SDPSR_MEM_DEVICE;
    int st = SDPSR_OK;
    const double* dZ = in_dev(c, "psd_z", Z, (size_t)plan.sum_sq, mem, &st);
    double* dP = out_dev(c, "psd_p", P, (size_t)plan.sum_sq, mem, &st);
    double* dL = lambda_min ? out_dev(c, "psd_lmin", lambda_min, (size_t)nblocks, mem, &st) : nullptr;
    double* vmid = psd_mid_scratch(c, plan, "psd_vmid", &st);
    PsdJob* djobs = nullptr;
    int* dflag = nullptr;
    if (!st) st = psd_upload_plan(c, plan, "psd_jobs", "psd_flag", &djobs, &dflag);
    if (st) {
        (void)ctx_sync_stream(c, s);  // (pageable sources: nothing reads them after the return)
        return st;
    }
    psd_launch_plan(s, plan, djobs, dZ, dP, dL, nullptr, nullptr, nullptr, vmid, dflag);
    HIP_TRY(c, hipGetLastError());
    if (host) {
        HIP_TRY(c, hipMemcpyAsync(P, dP, (size_t)plan.sum_sq * 8, hipMemcpyDeviceToHost, s));
        if (dL) HIP_TRY(c, hipMemcpyAsync(lambda_min, dL, (size_t)nblocks * 8, hipMemcpyDeviceToHost, s));
        c->d2h_bytes += (size_t)plan.sum_sq * 8 + (dL ? (size_t)nblocks * 8 : 0);
    }
    int flag = 0;
    st = d2h_sync(c, &flag, dflag, 4);  // the one host wait: the outputs are complete behind it
    if (st) return st;
    if (flag & 2) return ctx_fail(c, SDPSR_SOLVER_ERROR, "psd_project: a block holds a NaN or an Inf; its outputs are NaN");
    if (flag & 1) return ctx_fail(c, SDPSR_NOT_CONVERGED, "psd_project: the Jacobi sweep limit was reached; outputs are written as they stand");
    return SDPSR_OK;
}

int sdpsr_sdp_solve(sdpsr_ctx* c, const sdpsr_blockop* op, int64_t r, const double* A, const double* b, const double* cvec,
                    const sdpsr_sdp_opts* opts, double* x, double* S, double* Y, sdpsr_sdp_info* info, int mem) {
    CHECK_CTX(c);
    if (!op) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: no handle");
    if (op->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: the handle lives on another device");
    const int64_t d = op->d, n = op->sum_sq;
    const int32_t nb = (int32_t)op->sizes.size();
    if (d < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: the operator has no variable (d < 1)");
    if (d > SDP_MAX_D) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: d > 4096: the dense d x d solve operator is not formed beyond that");
    PsdPlan plan;
    if (!psd_plan(c, "sdp_solve", nb, op->sizes.data(), plan)) return SDPSR_BAD_ARGUMENT;
    if (r < 0 || r > std::min(d, SDP_MAX_R)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: r outside [0, min(d, 1024)]");
    if (!cvec || !x || (r > 0 && (!A || !b))) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: a NULL array");
    sdpsr_sdp_opts o{};
    if (opts) o = *opts;
    if (o.rho == 0.0) o.rho = 1.0;
    if (o.eps == 0.0) o.eps = 1e-9;
    if (o.max_iters == 0) o.max_iters = 20000;
    if (o.check_every == 0) o.check_every = 50;
    if (o.sense == 0) o.sense = 1;
    const bool nonneg = o.nonneg >= 0;  // 0 (the zeroed struct) and 1: x >= 0; -1: x is free
    if (!(o.rho > 0.0) || !std::isfinite(o.rho) || !(o.eps > 0.0) || !std::isfinite(o.eps) || o.max_iters < 1 || o.check_every < 1 ||
        (o.sense != 1 && o.sense != -1))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: rho and eps are positive and finite, max_iters and check_every >= 1, sense is +1 or -1");
    hipStream_t s = c->stream;
    const bool host = mem != SDPSR_MEM_DEVICE;
    // host copies: the finiteness check, chat, and the final report
    std::vector<double> hA, hb, hc;
    int st = host_copy(c, cvec, (size_t)d, mem, hc);
    if (!st) st = host_copy(c, A, (size_t)(r * d), mem, hA);
    if (!st) st = host_copy(c, b, (size_t)r, mem, hb);
    if (st) return st;
    if (!all_finite(hc.data(), hc.size()) || !all_finite(hA.data(), hA.size()) || !all_finite(hb.data(), hb.size()))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdp_solve: a non-finite value in A, b or c");
    double cn = 0.0;
    for (double v : hc) cn += v * v;
    cn = std::sqrt(cn);
    std::vector<double> hchat((size_t)d);
    for (int64_t i = 0; i < d; ++i) hchat[i] = (o.sense > 0 ? -hc[i] : hc[i]) / (cn > 0.0 ? cn : 1.0);
    // ---- setup
    const double* dA = r > 0 ? in_dev(c, "sdp_a", A, (size_t)(r * d), mem, &st) : nullptr;
    const double* db = r > 0 ? in_dev(c, "sdp_b", b, (size_t)r, mem, &st) : nullptr;
    if (st) {
        (void)ctx_sync_stream(c, s);
        return st;
    }
    SdpSetup su;
    st = sdp_setup(c, op, r, dA, db, su);
    if (st) {
        (void)ctx_sync_stream(c, s);
        return st;
    }
    // ---- state: vectors x u lam adj chat, uml twice (d each) and the row slots (2 d); blocks Bx S Lam D (n each) and the block slots (2 nb)
    double* vec = (double*)ctx_buf(c, "sdp_vec", (size_t)(9 * d) * 8);
    double* blk = (double*)ctx_buf(c, "sdp_blk", (size_t)(4 * n + 3 * nb) * 8);
    void* carry = ctx_buf(c, "bop_carry", blockop_carry_bytes(op->nnz_full));
    PsdJob* djobs = nullptr;
    int* dflag = nullptr;
    if (!vec || !blk || !carry) return SDPSR_OUT_OF_MEMORY;
    double* vmid = psd_mid_scratch(c, plan, "sdp_vmid", &st);
    if (st) return st;
    st = psd_upload_plan(c, plan, "sdp_jobs", "sdp_flag", &djobs, &dflag);
    if (st) return st;
    double *dx = vec, *du = vec + d, *dlam = vec + 2 * d, *dadj = vec + 3 * d, *dchat = vec + 4 * d, *dvs = vec + 5 * d;
    double* duml[2] = {vec + 7 * d, vec + 8 * d};  // u - lam: iteration k reads [k & 1] and writes the other (kernels_sdp.hip)
    double *dBx = blk, *dS = blk + n, *dLam = blk + 2 * n, *dD = blk + 3 * n, *dbs = blk + 4 * n, *dlmin = blk + 4 * n + 2 * nb;
    HIP_TRY(c, hipMemsetAsync(vec, 0, (size_t)(9 * d) * 8, s));
    HIP_TRY(c, hipMemsetAsync(blk, 0, (size_t)(4 * n + 3 * nb) * 8, s));
    st = h2d_sync(c, dchat, hchat.data(), (size_t)d * 8);
    if (st) return st;
    volatile double* verdict = (volatile double*)ctx_pinned(c, PINNED_FIXED_BYTES);
    if (!verdict) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "pinned staging");
    // ---- the loop: no host wait between two checks
    double rho = o.rho, rp = INFINITY, rd = INFINITY;
    int32_t iters = 0, changes = 0;
    bool converged = false, nonfinite = false;
    while (iters < o.max_iters) {
        st = blockop_map_enqueue(c, op, true, dD, carry, dadj);  // adj = B'(S - Lam)
        if (st) return st;
        launch_sdp_affine_step(s, d, nonneg ? 1 : 0, rho, su.Kt, su.x0, dadj, dchat, duml[iters & 1], dx, du, dlam, duml[(iters + 1) & 1], dvs);
        st = blockop_map_enqueue(c, op, false, dx, carry, dBx);  // Bx
        if (st) return st;
        psd_launch_plan(s, plan, djobs, dBx, dS, nullptr, dLam, dD, dbs, vmid, dflag);
        ++iters;
        if (iters % o.check_every != 0 && iters != o.max_iters) continue;
        launch_sdp_verdict(s, d, dvs, nb, dbs, (double*)verdict);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, ctx_sync_stream(c, s));  // the one host wait of a check
        c->d2h_bytes += 24;
        if (verdict[2] != 0.0) {
            nonfinite = true;
            break;
        }
        rp = std::sqrt(verdict[0]);
        rd = rho * std::sqrt(verdict[1]);
        if (rp <= o.eps && rd <= o.eps) {
            converged = true;
            break;
        }
        if (o.adapt_rho && iters < o.max_iters) {
            const double nr = rp > 10.0 * rd ? rho * 2.0 : (rd > 10.0 * rp ? rho * 0.5 : rho);
            if (nr != rho) {
                launch_sdp_rescale(s, d, n, rho / nr, du, dlam, duml[iters & 1], dS, dLam, dD);
                rho = nr;
                ++changes;
            }
        }
    }
    // ---- outputs and the report, from the returned x itself: lambda_min through the projection kernel on Bx = B x
    double* scratchP = (double*)ctx_buf(c, "sdp_proj", (size_t)n * 8);
    if (!scratchP) return SDPSR_OUT_OF_MEMORY;
    psd_launch_plan(s, plan, djobs, dBx, scratchP, dlmin, nullptr, nullptr, nullptr, vmid, dflag);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> hx((size_t)d), hl((size_t)nb);
    int flag = 0;
    HIP_TRY(c, hipMemcpyAsync(hx.data(), dx, (size_t)d * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hl.data(), dlmin, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, s));
    c->d2h_bytes += (size_t)(d + nb) * 8 + 4;
    if (host) {
        if (S) HIP_TRY(c, hipMemcpyAsync(S, dS, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        if (Y) {
            launch_sdp_scaled_copy(s, n, rho, dLam, scratchP);
            HIP_TRY(c, hipMemcpyAsync(Y, scratchP, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        }
        c->d2h_bytes += (size_t)n * 8 * ((S ? 1 : 0) + (Y ? 1 : 0));
    } else {
        HIP_TRY(c, hipMemcpyAsync(x, dx, (size_t)d * 8, hipMemcpyDeviceToDevice, s));
        if (S) HIP_TRY(c, hipMemcpyAsync(S, dS, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
        if (Y) launch_sdp_scaled_copy(s, n, rho, dLam, Y);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, ctx_sync_stream(c, s));  // the outputs are complete on return
    if (host) memcpy(x, hx.data(), (size_t)d * 8);
    if (info) {
        sdpsr_sdp_info f{};
        for (int64_t i = 0; i < d; ++i) f.objective += hc[i] * hx[i];
        f.min_x = hx[0];
        for (int64_t i = 1; i < d; ++i) f.min_x = std::min(f.min_x, hx[i]);
        for (int64_t i = 0; i < r; ++i) {
            double t = 0.0;
            for (int64_t k = 0; k < d; ++k) t += hA[i + k * r] * hx[k];
            f.eq_residual = std::max(f.eq_residual, std::fabs(t - hb[i]));
        }
        f.lambda_min = hl[0];
        for (int32_t k = 1; k < nb; ++k) f.lambda_min = std::min(f.lambda_min, hl[k]);
        f.r_primal = rp;
        f.r_dual = rd;
        f.rho = rho;
        f.iters = iters;
        f.rho_changes = changes;
        *info = f;
    }
    if (nonfinite || (flag & 2)) return ctx_fail(c, SDPSR_SOLVER_ERROR, "sdp_solve: the iteration left the finite numbers (a non-finite value in the operator?)");
    if (flag & 1) return ctx_fail(c, SDPSR_SOLVER_ERROR, "sdp_solve: a projection reached the Jacobi sweep limit");
    if (!converged) return ctx_fail(c, SDPSR_NOT_CONVERGED, "sdp_solve: the iteration limit was reached; every output is written as it stands");
    return SDPSR_OK;
}

}  // extern "C"
