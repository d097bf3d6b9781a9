// libsdpsr_prof.so -- measurement entry points (include/sdpsr_prof.h), NOT part of the product
// library: bench.py's roofline leg and the tools/ scripts time single kernels of libsdpsr_hip.so
// through these.  Links against libsdpsr_hip.so (same ctx, same kernels).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <functional>
#include <numeric>

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "../host_internal.h"
#include "../kernel_util.h"
#include "../../../include/sdpsr_prof.h"

using namespace sdpsr;

namespace sdpsr {
void launch_fill_test_sig(hipStream_t s, int64_t len, int64_t nclasses, uint64_t* sig);
void launch_clock_sampler(hipStream_t s, long long* buf, int ns, const unsigned* flag, long long max_ticks, int* count);
void launch_wall_marker(hipStream_t s, long long* out);
bool launch_band_chase(hipStream_t s, int n, int b, double* A, int64_t ld, unsigned* progress, unsigned* abort_flag, double* d, double* e, int max_wgs);
void launch_band_panel_split(hipStream_t s, int64_t m, int b, double* P, int64_t ldp, double* V, int64_t ldv);
}

extern "C" int sdpsr_profile_sytrd_graphs(sdpsr_ctx* c, double* out) {
    CHECK_CTX(c);
    if (!out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    uint64_t h = 0, m = 0;
    double ms = 0;
    sytrd_graph_cache_stats(c->sytrd_graphs, &h, &m, &ms);
    out[0] = (double)h;
    out[1] = (double)m;
    out[2] = ms;
    return SDPSR_OK;
}

// Stage 2 of a two-stage tridiagonalisation, measured: the symmetric band matrix A (n x n dense, column-major, host; entries
// beyond bandwidth b zero) is reduced to tridiagonal form by bulge chasing on the device (prof_kernels.hip); d (n), e (n - 1)
// come back to the host, out[0] = milliseconds of the chase kernel, out[1] = 1 if a workgroup gave up waiting.
extern "C" int sdpsr_profile_band_chase(sdpsr_ctx* c, int64_t n, int b, const double* A_host, double* d_host, double* e_host, double* out) {
    CHECK_CTX(c);
    if (!A_host || !d_host || !e_host || !out || n < 3 || n > 16384) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    hipStream_t s = c->stream;
    double* A = (double*)ctx_buf(c, "prof_band", (size_t)n * n * 8);
    double* de = (double*)ctx_buf(c, "prof_d", (size_t)3 * n * 8);
    unsigned* prog = (unsigned*)ctx_buf(c, "prof_prog", (size_t)(n + 16) * 4);
    if (!A || !de || !prog) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(A, A_host, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(prog, 0, (size_t)(n + 16) * 4, s));
    hipEvent_t e0, e1;
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    HIP_TRY(c, hipEventRecord(e0, s));
    const bool ok = launch_band_chase(s, (int)n, b, A, n, prog, prog + n + 8, de, de + n, c->num_cus);
    HIP_TRY(c, hipEventRecord(e1, s));
    HIP_TRY(c, hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (!ok) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bandwidth must be 16, 32 or 64");
    unsigned ab = 0;
    HIP_TRY(c, hipMemcpy(&ab, prog + n + 8, 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(d_host, de, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(e_host, de + n, (size_t)(n - 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipGetLastError());
    out[0] = ms;
    out[1] = ab;
    return SDPSR_OK;
}

// Stage 1 of a two-stage tridiagonalisation, measured (VERDICT r4 item 5 asks for both stages "whatever they are"): dense
// symmetric A (n x n, column-major, host, lower triangle referenced; n a multiple of b) -> band of width b by blocked
// Householder QR of the sub-diagonal block columns, LIBRARY level-3 updates: per block column k (panel P = A(r0:n, j0:j0+b),
// r0 = j0 + b, m = n - r0 rows): rocsolver_dgeqrf(P) -> V, tau; rocsolver_dlarft -> T;
// Y = A22 V T (rocblas_dsymm + dgemm), M = T'(V'Y) (two dgemm), Z = Y - V M / 2 (dgemm), A22 -= V Z' + Z V' (dsyr2k).
// (Q = I - V T V'; Q' A22 Q = A22 - Y V' - V Y' + V M V' and M is symmetric.)  No back-transformation: eigenvalues only.
// The band matrix comes back in A_host (lower triangle; the reflectors below the panel's R are zeroed).
// out[0] = milliseconds of the whole stage, out[1] = of the panel factorisations (geqrf + larft) alone.
extern "C" int sdpsr_profile_band_reduce(sdpsr_ctx* c, int64_t n, int b, double* A_host, double* out) {
    CHECK_CTX(c);
    if (!A_host || !out || b < 8 || b > 256 || n < 2 * b || n % b != 0 || n > 16384) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    hipStream_t s = c->stream;
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != rocblas_status_success) return ctx_fail(c, SDPSR_SOLVER_ERROR, "rocblas_create_handle failed");
    rocblas_set_stream(h, s);
    double* A = (double*)ctx_buf(c, "prof_band", (size_t)n * n * 8);
    double* V = (double*)ctx_buf(c, "prof_br_v", (size_t)n * b * 8);
    double* Y = (double*)ctx_buf(c, "prof_br_y", (size_t)n * b * 8);
    double* Z = (double*)ctx_buf(c, "prof_br_z", (size_t)n * b * 8);
    double* sm = (double*)ctx_buf(c, "prof_br_small", (size_t)(4 * b * b + b) * 8);
    if (!A || !V || !Y || !Z || !sm) {
        rocblas_destroy_handle(h);
        return SDPSR_OUT_OF_MEMORY;
    }
    double *T = sm, *S = sm + (size_t)b * b, *M = sm + (size_t)2 * b * b, *tau = sm + (size_t)4 * b * b;
    HIP_TRY(c, hipMemcpyAsync(A, A_host, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
    hipEvent_t e0, e1, p0, p1;
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    HIP_TRY(c, hipEventCreate(&p0));
    HIP_TRY(c, hipEventCreate(&p1));
    const double one = 1.0, zero = 0.0, mhalf = -0.5, mone = -1.0;
    float panel_ms = 0;
    bool ok = true;
    // one untimed pass over a copy would warm the library's kernels; the first panel's launches are the warm-up here:
    // the stage is timed twice and the second time is reported (the matrix is uploaded again in between)
    float ms = 0;
    for (int rep = 0; rep < 2 && ok; ++rep) {
        HIP_TRY(c, hipMemcpyAsync(A, A_host, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
        panel_ms = 0;
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int64_t j0 = 0; j0 + b < n && ok; j0 += b) {
            const int64_t r0 = j0 + b, m = n - r0;
            double* P = A + r0 + j0 * n;
            double* A22 = A + r0 + r0 * n;
            HIP_TRY(c, hipEventRecord(p0, s));
            ok = ok && rocsolver_dgeqrf(h, (rocblas_int)m, b, P, (rocblas_int)n, tau) == rocblas_status_success;
            ok = ok && rocsolver_dlarft(h, rocblas_forward_direction, rocblas_column_wise, (rocblas_int)m, b, P, (rocblas_int)n, tau, T, b) == rocblas_status_success;
            HIP_TRY(c, hipEventRecord(p1, s));
            launch_band_panel_split(s, m, b, P, n, V, m);  // V explicit (unit diagonal, zeros above), P keeps R
            ok = ok && rocblas_dsymm(h, rocblas_side_left, rocblas_fill_lower, (rocblas_int)m, b, &one, A22, (rocblas_int)n, V, (rocblas_int)m, &zero, Z, (rocblas_int)m) == rocblas_status_success;  // Z = A22 V
            ok = ok && rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, (rocblas_int)m, b, b, &one, Z, (rocblas_int)m, T, b, &zero, Y, (rocblas_int)m) == rocblas_status_success;  // Y = A22 V T
            ok = ok && rocblas_dgemm(h, rocblas_operation_transpose, rocblas_operation_none, b, b, (rocblas_int)m, &one, V, (rocblas_int)m, Y, (rocblas_int)m, &zero, S, b) == rocblas_status_success;  // S = V'Y
            ok = ok && rocblas_dgemm(h, rocblas_operation_transpose, rocblas_operation_none, b, b, b, &one, T, b, S, b, &zero, M, b) == rocblas_status_success;  // M = T'S
            HIP_TRY(c, hipMemcpyAsync(Z, Y, (size_t)m * b * 8, hipMemcpyDeviceToDevice, s));
            ok = ok && rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, (rocblas_int)m, b, b, &mhalf, V, (rocblas_int)m, M, b, &one, Z, (rocblas_int)m) == rocblas_status_success;  // Z = Y - V M / 2
            ok = ok && rocblas_dsyr2k(h, rocblas_fill_lower, rocblas_operation_none, (rocblas_int)m, b, &mone, V, (rocblas_int)m, Z, (rocblas_int)m, &one, A22, (rocblas_int)n) == rocblas_status_success;
            if (rep == 1) {
                HIP_TRY(c, hipEventSynchronize(p1));
                float pm = 0;
                HIP_TRY(c, hipEventElapsedTime(&pm, p0, p1));
                panel_ms += pm;
            }
        }
        HIP_TRY(c, hipEventRecord(e1, s));
        HIP_TRY(c, hipEventSynchronize(e1));
        HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipEventDestroy(p0);
    hipEventDestroy(p1);
    rocblas_destroy_handle(h);
    if (!ok) return ctx_fail(c, SDPSR_SOLVER_ERROR, "a rocSOLVER / rocBLAS call of the band reduction failed");
    HIP_TRY(c, hipMemcpy(A_host, A, (size_t)n * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipGetLastError());
    out[0] = ms;
    out[1] = panel_ms;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_host_waits(sdpsr_ctx* c, uint64_t* out) {
    CHECK_CTX(c);
    if (!out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    *out = c->host_waits;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_loop_counts(sdpsr_ctx* c, int32_t restart, uint64_t* out) {
    CHECK_CTX(c);
    if (!out || restart < 0 || restart > (int32_t)c->batch_children.size()) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const sdpsr_ctx* ci = restart == 0 ? c : c->batch_children[restart - 1];
    out[0] = ci->stream_counter;
    out[1] = ci->squares_launched;
    out[2] = ci->squares_speculative;
    out[3] = (uint64_t)ci->hint_used;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_initial_guess(sdpsr_ctx* c, int32_t restart, uint64_t* out) {
    CHECK_CTX(c);
    if (!out || restart < 0 || restart > (int32_t)c->batch_children.size()) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const sdpsr_ctx* ci = restart == 0 ? c : c->batch_children[restart - 1];
    out[0] = ci->initial_guesses;
    out[1] = ci->initial_guesses_violated;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_narrow_labels(sdpsr_ctx* c, int32_t restart, uint64_t* out) {
    CHECK_CTX(c);
    if (!out || restart < 0 || restart > (int32_t)c->batch_children.size()) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    out[0] = (restart == 0 ? c : c->batch_children[restart - 1])->label_narrowings;
    return SDPSR_OK;
}

// ---- the consumers of the loop's packed labels on caller-made inputs, at either label width (tests/test_gpu_label_passes.py,
// test_gpu_verify_pair.py, test_gpu_narrow_loop_labels.py) ----
namespace {
// width 8: *Lp8 = the byte copy of the np packed labels Lp (device), made by the library's own narrowing pass; width 32: nullptr.  d: the
// labels' bound (the byte forms take <= 255 classes)
int prof_label_shadow(sdpsr_ctx* c, const uint32_t* Lp, int64_t np, int64_t d, int width, const uint8_t** Lp8) {
    *Lp8 = nullptr;
    if (width == 32) return SDPSR_OK;
    if (width != 8 || d > 255) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label width: 32, or 8 with at most 255 classes");
    uint8_t* p = (uint8_t*)ctx_buf(c, "prof_lp8", (size_t)np);
    if (!p || !c->pinned_small) return SDPSR_OUT_OF_MEMORY;
    uint32_t* over = c->pinned_small + PINNED_SMALL_NARROW.first;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the labels' upload; nothing in flight on the word)
    *(volatile uint32_t*)over = 0u;
    launch_labels_narrow(c->stream, np, Lp, p, 8, over, c->num_cus);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (*(volatile uint32_t*)over != 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a label does not fit 8 bits");
    *Lp8 = p;
    return SDPSR_OK;
}
// What the three checks of the class-compare kernel share.  Up: the packed labels, their d representatives (each inside the triangle: the
// step and basis checks index with them unguarded) and the labels' shadow on the device, the stream idle, the verdict word holding 0xDEAD (the
// pass has to clear it).  Down: out[0] = the verdict word, out[1] = the class count up to which a check is one launch.
struct ProfClasses {
    uint32_t *Lp, *first, *flag;
    const uint8_t* Lp8;
};
int prof_classes_up(sdpsr_ctx* c, int64_t n, int64_t d, int width, const uint32_t* Lp_host, const uint32_t* first_idx_host, ProfClasses* p) {
    const int64_t np = n * (n + 1) / 2;
    for (int64_t k = 0; k < d; ++k)
        if ((int64_t)first_idx_host[k] >= np) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a representative outside the packed triangle");
    p->Lp = (uint32_t*)ctx_buf(c, "prof_lp", (size_t)np * 4);
    p->first = (uint32_t*)ctx_buf(c, "prof_first", (size_t)d * 4);
    p->flag = pinned_report(c, PINNED_VERIFY);
    if (!p->Lp || !p->first || !p->flag) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(p->Lp, Lp_host, (size_t)np * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(p->first, first_idx_host, (size_t)d * 4, hipMemcpyHostToDevice, c->stream));
    const int st = prof_label_shadow(c, p->Lp, np, d, width, &p->Lp8);
    if (st) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (nothing may be in flight on the verdict word)
    p->flag[0] = 0xDEADu;
    return SDPSR_OK;
}
int prof_verdict_down(sdpsr_ctx* c, bool ran, const ProfClasses& p, uint32_t* out) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (!ran) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "no check for this shape");
    out[0] = ((const volatile uint32_t*)p.flag)[0];
    out[1] = (uint32_t)verify_lds_cap();
    return SDPSR_OK;
}

// Gather: the packed triangle Lp (order n, labels <= d) through the plain and the label-writing form of the packed channel gather and, where
// Lfull_host / X_full are given, the mirrored full labels through the full-matrix gather; the X (T channels of ld x ld, ld = n rounded up to
// 128; every buffer filled with 0x5A first, so padding nobody wrote shows) come back with the full matrix the writing form made.  L_inout:
// n * n + guard words, uploaded as they are (the test's fill) and downloaded after the kernel.
int prof_gather_packed(sdpsr_ctx* c, int64_t n, int T, int64_t d, uint64_t key, int width, const uint32_t* Lp_host, const uint32_t* Lfull_host,
                       int8_t* X_plain, int8_t* X_writing, int8_t* X_full, uint32_t* L_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!Lp_host || !X_plain || !X_writing || !L_inout || !Lfull_host != !X_full || n < 1 || n > 8192 || d < 0 || guard < 0 ||
        (T != 1 && T != 2 && T != 4))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    hipStream_t s = c->stream;
    const int64_t ld = round_up(n, 128), np = n * (n + 1) / 2;
    const size_t xb = (size_t)T * ld * ld;
    uint32_t* Lp = (uint32_t*)ctx_buf(c, "prof_lp", (size_t)np * 4);
    uint32_t* Lf = (uint32_t*)ctx_buf(c, "prof_lfull", (size_t)n * n * 4);
    uint32_t* Lw = (uint32_t*)ctx_buf(c, "prof_lwritten", (size_t)(n * n + guard) * 4);
    int8_t* X = (int8_t*)ctx_buf(c, "prof_gx", 3 * xb);
    if (!Lp || !Lf || !Lw || !X) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Lp, Lp_host, (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Lw, L_inout, (size_t)(n * n + guard) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(X, 0x5A, 3 * xb, s));
    const uint8_t* Lp8 = nullptr;
    const int st = prof_label_shadow(c, Lp, np, d, width, &Lp8);
    if (st) return st;
    launch_gather_i8_sym_packed(s, n, ld, T, Lp, key, X, d, nullptr, Lp8);
    launch_gather_i8_sym_packed(s, n, ld, T, Lp, key, X + xb, d, Lw, Lp8);
    if (X_full) {
        HIP_TRY(c, hipMemcpyAsync(Lf, Lfull_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s));
        launch_gather_i8(s, n, ld, T, Lf, key, X + 2 * xb, d);
        HIP_TRY(c, hipMemcpyAsync(X_full, X + 2 * xb, xb, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipMemcpyAsync(X_plain, X, xb, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(X_writing, X + xb, xb, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(L_inout, Lw, (size_t)(n * n + guard) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

// The step check "does any entry of the packed triangle differ from the representative of its class?" on caller-made inputs.  Lp: packed
// labels <= d, first_idx: the d packed indices of the representatives, C_host: T (2 or 4) int32 channels of ld x ld.  r = -1: the channels
// alone; r = 0 .. 4: joint with the r basis matrices U_host (r * n * n) and coefficients coef_host (r); the class draws come from key.
int prof_verify(sdpsr_ctx* c, int64_t n, int T, int64_t d, int r, int width, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                const int32_t* C_host, const double* U_host, const double* coef_host, uint64_t key, double atol, uint32_t* out) {
    CHECK_CTX(c);
    if (!Lp_host || !first_idx_host || !C_host || !out || n < 1 || n > 8192 || d < 1 || d > (int64_t)refine_first_cap() || r < -1 || r > 4 ||
        (T != 2 && T != 4) || (r > 0 && (!U_host || !coef_host)) || !(atol > 0))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    hipStream_t s = c->stream;
    const int64_t ld = round_up(n, 128), rr = r > 0 ? r : 0;
    const size_t cb = (size_t)T * ld * ld * 4;
    int32_t* Cd = (int32_t*)ctx_buf(c, "prof_vc", cb);
    double* Ud = (double*)ctx_buf(c, "prof_vu", (size_t)(n * n + 1) * 4 * 8);  // + the coefficients
    void* ref = ctx_buf(c, "prof_vref", verify_ref_bytes(d));
    if (!Cd || !Ud || !ref) return SDPSR_OUT_OF_MEMORY;
    double* coef = Ud + 4 * n * n;
    ProfClasses p;
    const int st = prof_classes_up(c, n, d, width, Lp_host, first_idx_host, &p);
    if (st) return st;
    // (after the last early return: coef_host may be a caller's stack variable, and prof_verdict_down waits for the stream)
    HIP_TRY(c, hipMemcpyAsync(Cd, C_host, cb, hipMemcpyHostToDevice, s));
    if (rr > 0) {
        HIP_TRY(c, hipMemcpyAsync(Ud, U_host, (size_t)rr * n * n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(coef, coef_host, (size_t)rr * 8, hipMemcpyHostToDevice, s));
    }
    SigSource q;
    q.kind = r >= 0 ? SIG_JOINT_I32 : SIG_CHAN_I32, q.U = Ud, q.coef = coef, q.r = (int)rr, q.key = key, q.atol = atol, q.scale = round_scale(c, atol);
    q.n = n, q.ld = ld, q.T = T, q.C = Cd, q.L = p.Lp, q.L8 = p.Lp8, q.packed = 1, q.lab_packed = 1;
    return prof_verdict_down(c, launch_verify_no_split(s, q, d, p.first, ref, p.flag), p, out);
}

// The basis check "is every one of the r (1 .. 4) basis matrices U_host (r * n * n) constant on the classes, and 0 on label 0?"; wide labels.
int prof_basis_constant(sdpsr_ctx* c, int64_t n, int r, int64_t d, const uint32_t* Lp_host, const uint32_t* first_idx_host, const double* U_host,
                        double atol, uint32_t* out) {
    CHECK_CTX(c);
    if (!Lp_host || !first_idx_host || !U_host || !out || n < 1 || n > 8192 || d < 1 || d > (int64_t)refine_first_cap() || r < 1 || r > 4 ||
        !(atol > 0))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    double* Ud = (double*)ctx_buf(c, "prof_vu", (size_t)(n * n + 1) * 4 * 8);
    void* ref = ctx_buf(c, "prof_vref", uconst_ref_bytes(d, r));
    if (!Ud || !ref) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Ud, U_host, (size_t)r * n * n * 8, hipMemcpyHostToDevice, c->stream));
    ProfClasses p;
    const int st = prof_classes_up(c, n, d, 32, Lp_host, first_idx_host, &p);
    if (st) return st;
    const bool ran = launch_basis_constant_on_classes(c->stream, n, r, Ud, p.Lp, d, p.first, atol, round_scale(c, atol), ref, p.flag);
    return prof_verdict_down(c, ran, p, out);
}

// The pair check "would the initial refinement of (a, b) write these labels and representatives again?" on caller-made inputs
// (tests/test_gpu_verify_pair.py).  a_host, b_host: n x n column-major (the lower triangle is read).  More classes than one launch takes
// (out[1]) are refused.
int prof_verify_pair(sdpsr_ctx* c, int64_t n, int64_t d, int width, const uint32_t* Lp_host, const uint32_t* first_idx_host, const double* a_host,
                     const double* b_host, uint32_t* out) {
    CHECK_CTX(c);
    if (!Lp_host || !first_idx_host || !a_host || !b_host || !out || n < 1 || n > 8192 || d < 1 || d > (int64_t)verify_lds_cap())
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    double* ab = (double*)ctx_buf(c, "prof_pair_ab", (size_t)2 * n * n * 8);
    if (!ab) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(ab, a_host, (size_t)n * n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ab + n * n, b_host, (size_t)n * n * 8, hipMemcpyHostToDevice, c->stream));
    ProfClasses p;
    const int st = prof_classes_up(c, n, d, width, Lp_host, first_idx_host, &p);
    if (st) return st;
    return prof_verdict_down(c, launch_verify_pair(c->stream, n, ab, ab + n * n, p.Lp, d, p.first, p.flag, p.Lp8), p, out);
}
}  // namespace

// The entries (include/sdpsr_prof.h): each pass has ONE body above; the entries without a width argument are its width-32 form.
extern "C" int sdpsr_profile_gather_packed(sdpsr_ctx* c, int64_t n, int T, int64_t d, uint64_t key, const uint32_t* Lp_host, const uint32_t* Lfull_host,
                                           int8_t* X_plain, int8_t* X_writing, int8_t* X_full, uint32_t* L_inout, int64_t guard) {
    if (!Lfull_host || !X_full) return c ? ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments") : SDPSR_BAD_ARGUMENT;
    return prof_gather_packed(c, n, T, d, key, 32, Lp_host, Lfull_host, X_plain, X_writing, X_full, L_inout, guard);
}
extern "C" int sdpsr_profile_gather_packed_w(sdpsr_ctx* c, int64_t n, int T, int64_t d, uint64_t key, int width, const uint32_t* Lp_host,
                                             int8_t* X_plain, int8_t* X_writing, uint32_t* L_inout, int64_t guard) {
    return prof_gather_packed(c, n, T, d, key, width, Lp_host, nullptr, X_plain, X_writing, nullptr, L_inout, guard);
}
// mode 0: the channels alone; 1: joint with the one basis matrix U_host and coefficient coef; 2: the basis check of U_host (C_host unused)
extern "C" int sdpsr_profile_verify(sdpsr_ctx* c, int64_t n, int T, int64_t d, int mode, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                                    const int32_t* C_host, const double* U_host, double coef, uint64_t key, double atol, uint32_t* out) {
    if (mode == 2) return prof_basis_constant(c, n, 1, d, Lp_host, first_idx_host, U_host, atol, out);
    if (mode != 0 && mode != 1) return c ? ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments") : SDPSR_BAD_ARGUMENT;
    return prof_verify(c, n, T, d, mode == 1 ? 1 : -1, 32, Lp_host, first_idx_host, C_host, U_host, &coef, key, atol, out);
}
extern "C" int sdpsr_profile_verify_w(sdpsr_ctx* c, int64_t n, int T, int64_t d, int r, int width, const uint32_t* Lp_host,
                                      const uint32_t* first_idx_host, const int32_t* C_host, const double* U_host, const double* coef_host,
                                      uint64_t key, double atol, uint32_t* out) {
    return prof_verify(c, n, T, d, r, width, Lp_host, first_idx_host, C_host, U_host, coef_host, key, atol, out);
}
extern "C" int sdpsr_profile_basis_constant(sdpsr_ctx* c, int64_t n, int r, int64_t d, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                                            const double* U_host, double atol, uint32_t* out) {
    return prof_basis_constant(c, n, r, d, Lp_host, first_idx_host, U_host, atol, out);
}
extern "C" int sdpsr_profile_verify_pair(sdpsr_ctx* c, int64_t n, int64_t d, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                                         const double* a_host, const double* b_host, uint32_t* out) {
    return prof_verify_pair(c, n, d, 32, Lp_host, first_idx_host, a_host, b_host, out);
}
extern "C" int sdpsr_profile_verify_pair_w(sdpsr_ctx* c, int64_t n, int64_t d, int width, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                                           const double* a_host, const double* b_host, uint32_t* out) {
    return prof_verify_pair(c, n, d, width, Lp_host, first_idx_host, a_host, b_host, out);
}

extern "C" int sdpsr_profile_square_checks(sdpsr_ctx* c, int32_t restart, uint64_t* out) {
    CHECK_CTX(c);
    if (!out || restart < 0 || restart > (int32_t)c->batch_children.size()) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const sdpsr_ctx* ci = restart == 0 ? c : c->batch_children[restart - 1];
    out[0] = ci->square_checks;
    out[1] = ci->square_check_fallbacks;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_deferred_checks(sdpsr_ctx* c, int32_t restart, uint64_t* out) {
    CHECK_CTX(c);
    if (!out || restart < 0 || restart > (int32_t)c->batch_children.size()) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const DeferredCheckStats& t = (restart == 0 ? c : c->batch_children[restart - 1])->check_stats;
    out[0] = t.registered, out[1] = t.in_ride, out[2] = t.outside_ride;
    out[3] = t.window_ns[0], out[4] = t.window_count[0], out[5] = t.window_ns[1], out[6] = t.window_count[1];
    out[7] = t.voided[0], out[8] = t.voided[1], out[9] = t.voided[2];
    return SDPSR_OK;
}
extern "C" int sdpsr_profile_recorded_labels(sdpsr_ctx* c, int32_t restart, uint64_t* out) {
    const int st = sdpsr_profile_deferred_checks(c, restart, out);
    if (st) return st;
    out[10] = (restart == 0 ? c : c->batch_children[restart - 1])->check_stats.on_record;
    return SDPSR_OK;
}

// The square check on caller-made inputs (tests/test_gpu_square_check.py).  ws_inout == nullptr: only layout[] is filled.
extern "C" int sdpsr_profile_square_check(sdpsr_ctx* c, int64_t n, int64_t d, int G, int T, const uint64_t* keys, int width, int write_full,
                                          const uint32_t* Lp_host, const uint32_t* first_idx_host, uint8_t* ws_inout, uint64_t* layout,
                                          uint32_t* verdicts_out, uint32_t* L_inout, int64_t guard) {
    CHECK_CTX(c);
    constexpr size_t gap = 64;
    if (!layout || !square_check_supports(n, d, G, T) || n > 8192 || (width != 8 && width != 32) || guard < 0 || guard > (int64_t(1) << 20))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    SquareCheck q;
    q.n = n, q.d = d, q.G = G, q.T = T;
    const size_t bytes = square_check_ws_carve(q, nullptr, gap);
    void* ws = ctx_buf(c, "prof_sqcheck", bytes);
    if (!ws) return SDPSR_OUT_OF_MEMORY;
    square_check_ws_carve(q, ws, gap);
    const void* parts[7] = {q.c, q.part_x, q.part_c, q.y, q.w, q.esum, q.bits};
    for (int k = 0; k < 7; ++k) layout[k] = (uint64_t)((const char*)parts[k] - (const char*)ws);
    layout[7] = bytes;
    if (!ws_inout) return SDPSR_OK;
    if (!keys || !Lp_host || !first_idx_host || !verdicts_out || (write_full && !L_inout)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    hipStream_t s = c->stream;
    uint32_t* Lw = write_full ? (uint32_t*)ctx_buf(c, "prof_lwritten", (size_t)(n * n + guard) * 4) : nullptr;
    uint32_t* flag1 = pinned_report(c, PINNED_SPECULATIVE);
    if ((write_full && !Lw) || !flag1) return SDPSR_OUT_OF_MEMORY;
    ProfClasses p;
    const int st = prof_classes_up(c, n, d, width, Lp_host, first_idx_host, &p);  // (p.flag: PINNED_VERIFY)
    if (st) return st;
    HIP_TRY(c, hipMemcpyAsync(ws, ws_inout, bytes, hipMemcpyHostToDevice, s));
    if (write_full) HIP_TRY(c, hipMemcpyAsync(Lw, L_inout, (size_t)(n * n + guard) * 4, hipMemcpyHostToDevice, s));
    for (int g = 0; g < G; ++g) q.key[g] = keys[g];
    q.Lp = p.Lp, q.Lp8 = p.Lp8, q.first_idx = p.first, q.Lfull = Lw;
    q.flag[0] = p.flag, q.flag[1] = flag1;
    *(volatile uint32_t*)q.flag[0] = 0u;  // (the stream is idle: prof_classes_up waited)
    *(volatile uint32_t*)q.flag[1] = 0u;
    launch_square_check_ref_and_pass(s, q);
    launch_square_check_verdict(s, q);
    HIP_TRY(c, hipMemcpyAsync(ws_inout, ws, bytes, hipMemcpyDeviceToHost, s));
    if (write_full) HIP_TRY(c, hipMemcpyAsync(L_inout, Lw, (size_t)(n * n + guard) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    verdicts_out[0] = ((const volatile uint32_t*)q.flag[0])[0];
    verdicts_out[1] = ((const volatile uint32_t*)q.flag[1])[0];
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_proj_coef_lower(sdpsr_ctx* c, int64_t n, int64_t r, uint64_t key, int width, const uint32_t* Lp_host,
                                             const double* U_host, double* partial_out, double* coef_out) {
    CHECK_CTX(c);
    if (!Lp_host || !U_host || !partial_out || !coef_out || n < 1 || n > 8192 || r < 1 || r > 4) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    constexpr int nblk = 2048;  // the loop's (loop.cpp)
    hipStream_t s = c->stream;
    const int64_t np = n * (n + 1) / 2;
    uint32_t* Lp = (uint32_t*)ctx_buf(c, "prof_lp", (size_t)np * 4);
    double* Ud = (double*)ctx_buf(c, "prof_vu", (size_t)(n * n + 1) * 4 * 8);
    double* partial = (double*)ctx_buf(c, "prof_partial", (size_t)(r * nblk + r) * 8);
    if (!Lp || !Ud || !partial) return SDPSR_OUT_OF_MEMORY;
    double* coef = partial + r * nblk;
    HIP_TRY(c, hipMemcpyAsync(Lp, Lp_host, (size_t)np * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Ud, U_host, (size_t)r * n * n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(partial, 0xFF, (size_t)(r * nblk + r) * 8, s));
    const uint8_t* Lp8 = nullptr;
    const int st = prof_label_shadow(c, Lp, np, 0, width, &Lp8);  // (the narrowing pass itself refuses a label above 255)
    if (st) return st;
    launch_proj_coef_lower(s, n, r, Ud, Lp, 1, key, partial, nblk, coef, Lp8);
    HIP_TRY(c, hipMemcpyAsync(partial_out, partial, (size_t)r * nblk * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(coef_out, coef, (size_t)r * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

// The full-matrix channel gathers of the square step on caller-made labels (tests/test_gpu_primitives.py).  kind 0 / 1 / 2: launch_gather_i8
// / launch_gather_f32 / launch_gather_f64_padded (one channel).  L_host: ANY n x n labels; X_inout: T * ld * ld + guard elements of the kind's
// type (ld = n rounded up to 128), uploaded as they are (the test's fill) and downloaded after the kernel.  out[0] = the kernel's work items
// (one per 16 / 4 / 2 rows of a column), out[1] = the threads of its launch.
extern "C" int sdpsr_profile_gather_full(sdpsr_ctx* c, int kind, int64_t n, int T, int vmax, int64_t dmax, uint64_t key, const uint32_t* L_host,
                                         void* X_inout, int64_t guard, uint64_t* out) {
    CHECK_CTX(c);
    if (!L_host || !X_inout || !out || kind < 0 || kind > 2 || n < 1 || n > 8192 || T < 1 || T > 8 || (kind == 2 && T != 1) || dmax < 0 ||
        guard < 0 || guard > (int64_t(1) << 20) || (kind == 1 && (vmax < 1 || vmax > 127)))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    if (dmax > 0)  // (the int8 form indexes its LDS table with the labels)
        for (int64_t e = 0; e < n * n; ++e)
            if ((int64_t)L_host[e] > dmax) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a label above dmax");
    hipStream_t s = c->stream;
    const int64_t ld = round_up(n, 128);
    const int elem = kind == 0 ? 1 : (kind == 1 ? 4 : 8), per_thread = kind == 0 ? 16 : (kind == 1 ? 4 : 2);
    const size_t xb = ((size_t)T * ld * ld + (size_t)guard) * elem;
    uint32_t* L = (uint32_t*)ctx_buf(c, "prof_lfull", (size_t)n * n * 4);
    void* X = ctx_buf(c, "prof_gx", xb);
    if (!L || !X) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(L, L_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(X, X_inout, xb, hipMemcpyHostToDevice, s));
    if (kind == 0) launch_gather_i8(s, n, ld, T, L, key, (int8_t*)X, dmax);
    else if (kind == 1) launch_gather_f32(s, n, ld, T, vmax, L, key, (float*)X);
    else launch_gather_f64_padded(s, n, ld, L, key, (double*)X);
    HIP_TRY(c, hipMemcpyAsync(X_inout, X, xb, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    const int64_t work = ld / per_thread * ld;
    out[0] = (uint64_t)work;
    out[1] = (uint64_t)grid_for(work, 256) * 256u;
    return SDPSR_OK;
}

// The dot products of the projection on labels (tests/test_gpu_primitives.py): form 0 = launch_proj_coef with x drawn from L_host and key,
// coef_out[0 .. r); form 1 = launch_proj_coef_probe (len == n * n), coef_out[0 .. 2r): the dot products, then the symmetry probes.
// U_host: r * len, 1 <= r <= 4; 2048 workgroups as in primitives.cpp and loop.cpp.
extern "C" int sdpsr_profile_proj_coef(sdpsr_ctx* c, int form, int64_t len, int64_t n, int64_t r, uint64_t key, const uint32_t* L_host,
                                       const double* U_host, double* coef_out) {
    CHECK_CTX(c);
    if (!L_host || !U_host || !coef_out || (form != 0 && form != 1) || len < 1 || len > (int64_t(1) << 26) || r < 1 || r > 4 ||
        (form == 1 && (n < 1 || n > 8192 || n * n != len)))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    constexpr int nblk = 2048;
    hipStream_t s = c->stream;
    const int64_t rows = form == 1 ? 2 * r : r;
    uint32_t* L = (uint32_t*)ctx_buf(c, "prof_lfull", (size_t)len * 4);
    double* Ud = (double*)ctx_buf(c, "prof_vu", (size_t)r * len * 8);
    double* partial = (double*)ctx_buf(c, "prof_partial", (size_t)(rows * nblk + rows) * 8);
    if (!L || !Ud || !partial) return SDPSR_OUT_OF_MEMORY;
    double* coef = partial + rows * nblk;
    HIP_TRY(c, hipMemcpyAsync(L, L_host, (size_t)len * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Ud, U_host, (size_t)r * len * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(partial, 0xFF, (size_t)(rows * nblk + rows) * 8, s));
    if (form == 0) launch_proj_coef(s, len, r, Ud, L, key, nullptr, partial, nblk, coef);
    else launch_proj_coef_probe(s, len, n, r, Ud, L, key, partial, nblk, coef);
    HIP_TRY(c, hipMemcpyAsync(coef_out, coef, (size_t)rows * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

// One refinement over a computed signature source on caller-made inputs (tests/test_gpu_refine_sources.py): the SigSource is put together
// the way loop.cpp does it (proj_source, chan_source, joint_source, initial_partition) and handed to the product's refine_signatures, the
// labels in place wherever the loop refines in place.  Conventions of the module-kernel entries below.
extern "C" int sdpsr_profile_refine_source(sdpsr_ctx* c, int kind, int what, int64_t n, int64_t ld, int T, int r, int packed, int lab_packed,
                                           uint64_t key, double atol, const double* a_host, const double* b_host, const double* U_host,
                                           const double* coef_host, const void* C_host, uint32_t* L_inout, uint32_t* Lnew_inout, int64_t guard,
                                           int64_t prev_classes, int sym, uint64_t* sig_out, int64_t* nparts, uint32_t* first_out, int32_t* report) {
    CHECK_CTX(c);
    enum { RS_PAIR = 0, RS_PROJ = 1, RS_CHAN_I32 = 2, RS_CHAN_F32 = 3, RS_JOINT = 4 };
    const bool pair = kind == RS_PAIR, proj = kind == RS_PROJ || kind == RS_JOINT, chan = kind == RS_CHAN_I32 || kind == RS_CHAN_F32 || kind == RS_JOINT;
    if (kind < RS_PAIR || kind > RS_JOINT || (what != 0 && what != 1) || n < 1 || n > 2048 || guard < 0 || guard > (int64_t(1) << 20) ||
        prev_classes < 0 || prev_classes > (int64_t(1) << 32) || !L_inout || !nparts || !report || (packed != 0 && packed != 1) ||
        (lab_packed != 0 && lab_packed != 1) || (lab_packed && !packed) || (sym && packed))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "refine_source: bad arguments");
    if (pair && (!a_host || !b_host || lab_packed != packed)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "refine_source: bad pair source");
    if (proj && (r < 0 || r > 8 || (r > 0 && (!U_host || !coef_host)) || !(atol > 0))) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "refine_source: bad projection");
    if (chan && (!C_host || T < 1 || T > 8 || ld < n || ld > 2048 || ld % 128)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "refine_source: bad channels");
    // the loop refines the packed triangle from full labels into ANOTHER array (LoopLabels::refine_packed: reads L, writes Lp)
    const bool apart = !pair && packed && !lab_packed;
    if (apart != (Lnew_inout != nullptr)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "refine_source: Lnew_inout goes with packed and not lab_packed");
    hipStream_t s = c->stream;
    const int64_t np = n * (n + 1) / 2, len = packed ? np : n * n, lablen = lab_packed ? np : n * n;
    const int64_t rr = proj ? r : 0;
    const size_t cb = chan ? (size_t)T * ld * ld * 4 : 0;
    double* ab = pair ? (double*)ctx_buf(c, "prof_rs_ab", (size_t)2 * n * n * 8) : nullptr;
    double* Ud = proj ? (double*)ctx_buf(c, "prof_rs_u", (size_t)(rr * n * n + rr + 1) * 8) : nullptr;  // + the coefficients
    void* Cd = chan ? ctx_buf(c, "prof_rs_c", cb) : nullptr;
    uint32_t* Ld = (uint32_t*)ctx_buf(c, "prof_rs_l", (size_t)(lablen + guard) * 4);
    uint32_t* Lnew = apart ? (uint32_t*)ctx_buf(c, "prof_rs_lnew", (size_t)(np + guard) * 4) : nullptr;
    uint64_t* sig = (uint64_t*)ctx_buf(c, "prof_rs_sig", (size_t)len * 8);
    uint64_t* sig2 = (sig_out && what == 0) ? (uint64_t*)ctx_buf(c, "prof_rs_sig2", (size_t)len * 8) : nullptr;
    uint32_t* symflag = sym ? (uint32_t*)ctx_buf(c, "prof_rs_symflag", 64) : nullptr;
    if ((pair && !ab) || (proj && !Ud) || (chan && !Cd) || !Ld || (apart && !Lnew) || !sig || (sig_out && what == 0 && !sig2) || (sym && !symflag))
        return SDPSR_OUT_OF_MEMORY;
    double* coef = proj ? Ud + rr * n * n : nullptr;
    SigSource q;
    q.sig = sig;
    if (pair) {
        q.kind = SIG_PAIR, q.a = ab, q.b = ab + n * n;
        if (packed) q.n = n, q.packed = 1;
    } else {
        if (proj) q.kind = SIG_PROJ, q.U = Ud, q.coef = coef, q.r = (int)rr, q.key = key, q.atol = atol, q.scale = round_scale(c, atol), q.n = n;
        if (chan) q.kind = kind == RS_JOINT ? SIG_JOINT_I32 : (kind == RS_CHAN_F32 ? SIG_CHAN_F32 : SIG_CHAN_I32), q.n = n, q.ld = ld, q.T = T, q.C = Cd;
        q.L = Ld, q.packed = packed, q.lab_packed = lab_packed;
    }
    // who writes this source's signatures: its functor (insert and materialise kernels), or the stand-alone kernel of its run-time shape
    const bool standalone = (chan && kind != RS_JOINT) || (kind == RS_PROJ && !packed);
    if (what == 0 ? !(sig_source_fusable(q) || standalone) : !standalone)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "refine_source: no kernel for this source's shape");
    if (pair) {
        HIP_TRY(c, hipMemcpyAsync(ab, a_host, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(ab + n * n, b_host, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
    }
    if (rr > 0) {
        HIP_TRY(c, hipMemcpyAsync(Ud, U_host, (size_t)rr * n * n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(coef, coef_host, (size_t)rr * 8, hipMemcpyHostToDevice, s));
    }
    if (chan) HIP_TRY(c, hipMemcpyAsync(Cd, C_host, cb, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Ld, L_inout, (size_t)(lablen + guard) * 4, hipMemcpyHostToDevice, s));
    if (apart) HIP_TRY(c, hipMemcpyAsync(Lnew, Lnew_inout, (size_t)(np + guard) * 4, hipMemcpyHostToDevice, s));
    uint32_t* labels = apart ? Lnew : Ld;
    c->table_log2_hint = refine_table_hint(len, (uint64_t)prev_classes);
    const uint64_t passes0 = c->refine_passes;
    int64_t d = 0;
    int symv = -1, st;
    if (what == 0) {
        if (sig_out) {
            if (!launch_sig_materialize(s, len, q, sig2)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "refine_source: nothing writes this source out");
            HIP_TRY(c, hipMemcpyAsync(sig_out, sig2, (size_t)len * 8, hipMemcpyDeviceToHost, s));
        }
        st = sym ? refine_signatures(c, len, q, labels, &d, n, symflag, &symv) : refine_signatures(c, len, q, labels, &d);
    } else {
        if (kind == RS_PROJ) launch_proj_apply(s, len, rr, Ud, Ld, key, nullptr, coef, atol, q.scale, 1, nullptr, sig);
        else if (kind == RS_CHAN_I32) launch_sig_i32(s, n, ld, T, Ld, (const int32_t*)Cd, sig, packed, lab_packed);
        else launch_sig_f32(s, n, ld, T, Ld, (const float*)Cd, sig, packed, lab_packed);
        if (sig_out) HIP_TRY(c, hipMemcpyAsync(sig_out, sig, (size_t)len * 8, hipMemcpyDeviceToHost, s));
        st = sym ? refine_signatures(c, len, sig, labels, &d, n, symflag, &symv) : refine_signatures(c, len, sig, labels, &d);
    }
    if (st) return st;
    HIP_TRY(c, hipMemcpyAsync(L_inout, Ld, (size_t)(lablen + guard) * 4, hipMemcpyDeviceToHost, s));
    if (apart) HIP_TRY(c, hipMemcpyAsync(Lnew_inout, Lnew, (size_t)(np + guard) * 4, hipMemcpyDeviceToHost, s));
    const uint32_t* first = (const uint32_t*)ctx_buf(c, "ref_first", (size_t)refine_first_cap() * 4);
    if (first_out && first && d > 0)
        HIP_TRY(c, hipMemcpyAsync(first_out, first, (size_t)std::min<int64_t>(d, refine_first_cap()) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    *nparts = d;
    report[0] = (int32_t)(c->refine_passes - passes0);
    report[1] = symv;
    report[2] = c->first_idx_labels == labels ? 1 : 0;
    return SDPSR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The kernels of the module-compression driver on caller-made inputs (tests/test_gpu_module_kernels.py): host arrays in, the
// product's own launcher called the way compress.cpp calls it, everything back.  Every output array is in/out: uploaded as the
// caller filled it and downloaded whole (padding and `guard` elements behind it included), so what no kernel wrote is visible.
// Every argument that could index outside a buffer is refused before anything is uploaded or launched.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t MK_MAX_N = 8192, MK_MAX_LD = 16384, MK_MAX_GUARD = 1 << 20;
bool mk_labels_ok(const uint32_t* L, size_t len, int64_t d) {
    for (size_t e = 0; e < len; ++e)
        if ((int64_t)L[e] > d) return false;
    return true;
}
}  // namespace

extern "C" int sdpsr_profile_gram(sdpsr_ctx* c, int mode, int64_t k, int64_t ma, int64_t nb, int64_t lda, int64_t ldb, int64_t mp, int64_t np,
                                  const double* A_host, const double* B_host, double* C_inout, double* pinned_inout, int64_t guard, int32_t* report) {
    CHECK_CTX(c);
    if (!A_host || !B_host || !C_inout || !report || (mode != 0 && mode != 1) || k < 1 || k > MK_MAX_N || ma < 1 || nb < 1 || mp < ma || np < nb ||
        mp > 256 || np > 256 || lda < k || ldb < k || lda > MK_MAX_LD || ldb > MK_MAX_LD || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "gram: bad arguments");
    const bool skinny = gram_tn_is_skinny(ma, nb);
    if (mode == 1 && !skinny) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "gram: the exact-shape kernel does not take this shape");
    // the split-K route is the tiled MFMA product over all mp x np columns: whole tiles, K in tiles, aligned columns
    if (mode == 0 && !skinny && (mp % 128 || np % 128 || k % 128 || lda % 128 || ldb % 128))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "gram: the split-K route needs mp, np, k, lda, ldb in multiples of 128");
    hipStream_t s = c->stream;
    const size_t cn = (size_t)(mp * np + guard);
    double* A = (double*)ctx_buf(c, "prof_mk_a", (size_t)lda * mp * 8);
    double* B = (double*)ctx_buf(c, "prof_mk_b", (size_t)ldb * np * 8);
    double* Cd = (double*)ctx_buf(c, "prof_mk_c", cn * 8);
    double* gp = mode == 1 ? (double*)ctx_buf(c, "gram_partials", gram_small_partial_doubles(k, (int)ma, (int)nb) * 8) : nullptr;
    double* pin = pinned_inout ? (double*)ctx_pinned(c, cn * 8) : nullptr;
    if (!A || !B || !Cd || (mode == 1 && !gp) || (pinned_inout && !pin)) return SDPSR_OUT_OF_MEMORY;
    if (pin) memcpy(pin, pinned_inout, cn * 8);
    HIP_TRY(c, hipMemcpyAsync(A, A_host, (size_t)lda * mp * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B, B_host, (size_t)ldb * np * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Cd, C_inout, cn * 8, hipMemcpyHostToDevice, s));
    bool host_filled = false;
    if (mode == 0) {
        const int st = gram_tn(c, ma, nb, k, A, lda, B, ldb, Cd, mp, np, pin, &host_filled);
        if (st) return st;
    } else {
        launch_gram_small(s, k, (int)ma, (int)nb, A, lda, B, ldb, gp, Cd, mp, (int)mp, (int)np, pin);
        host_filled = pin != nullptr;
    }
    HIP_TRY(c, hipMemcpyAsync(C_inout, Cd, cn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    if (pin) memcpy(pinned_inout, pin, cn * 8);
    report[0] = skinny ? 1 : 0;
    report[1] = host_filled ? 1 : 0;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_tall_times_small(sdpsr_ctx* c, int64_t n, int64_t ldi, int64_t kk, int64_t lds, int64_t ncols, double alpha, double beta,
                                              int64_t ldo, const double* In_host, const double* S_host, double* out_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!In_host || !S_host || !out_inout || n < 1 || n > MK_MAX_N || ldi < n || ldo < n || ldi > MK_MAX_LD || ldo > MK_MAX_LD || kk < 1 || kk > 512 ||
        lds < kk || lds > 1024 || ncols < 1 || ncols > 512 || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "tall_times_small: bad arguments");
    hipStream_t s = c->stream;
    const size_t on = (size_t)(ldo * ncols + guard);
    double* In = (double*)ctx_buf(c, "prof_mk_a", (size_t)ldi * kk * 8);
    double* S = (double*)ctx_buf(c, "prof_mk_b", (size_t)lds * ncols * 8);
    double* out = (double*)ctx_buf(c, "prof_mk_c", on * 8);
    if (!In || !S || !out) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(In, In_host, (size_t)ldi * kk * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(S, S_host, (size_t)lds * ncols * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(out, out_inout, on * 8, hipMemcpyHostToDevice, s));
    launch_tall_times_small(s, n, ldi, In, (int)kk, S, (int)lds, (int)ncols, alpha, beta, out, ldo);
    HIP_TRY(c, hipMemcpyAsync(out_inout, out, on * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_label_product(sdpsr_ctx* c, int64_t n, int64_t d, int G, int64_t w, int64_t ldw, int64_t ldy, const uint64_t* keys,
                                           const uint32_t* L_host, const double* W_host, double* Y_inout, int64_t guard, int32_t* report) {
    CHECK_CTX(c);
    if (!keys || !L_host || !W_host || !Y_inout || !report || n < 1 || n > MK_MAX_N || d < 0 || ldw < n || ldy < n || ldw > MK_MAX_LD ||
        ldy > MK_MAX_LD || w < 1 || w > 64 || G < 1 || G > 4 || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product: bad arguments");
    LabelSpmmForm f;
    if (!label_spmm_select(n, d, G, (int)w, &f)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product: shape not supported by the label product");
    if (!mk_labels_ok(L_host, (size_t)n * n, d)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product: a label exceeds d");
    hipStream_t s = c->stream;
    const size_t yn = (size_t)(ldy * G * w + guard);
    uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)n * n * 4);
    const size_t wn = (size_t)ldw * 64;  // all 64 columns the launcher could take: those >= w are the caller's poison
    double* W = (double*)ctx_buf(c, "prof_mk_a", wn * 8);
    double* Y = (double*)ctx_buf(c, "prof_mk_c", yn * 8);
    double* part = (double*)ctx_buf(c, "cm_part", label_spmm_partial_doubles(n, 64) * 8);
    if (!Lb || !W || !Y || !part) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Lb, L_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(W, W_host, wn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Y, Y_inout, yn * 8, hipMemcpyHostToDevice, s));
    const bool ran = G == 1 ? launch_label_spmm(s, n, Lb, keys[0], d, W, ldw, (int)w, part, Y, ldy)
                            : launch_label_spmm_multi(s, n, Lb, keys, G, d, W, ldw, (int)w, part, Y, ldy);
    HIP_TRY(c, hipMemcpyAsync(Y_inout, Y, yn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    if (!ran) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product: shape not supported by the label product");
    report[0] = f.mfma, report[1] = f.tile, report[2] = f.z, report[3] = f.cols_per_block;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_label_product_pair(sdpsr_ctx* c, int64_t n, int64_t d, int64_t w, int64_t ldw, int64_t ldy, const uint64_t* keys,
                                                const uint32_t* L_host, const double* W_host, double* Y0_inout, double* Y1_inout, int64_t guard,
                                                int32_t* report) {
    CHECK_CTX(c);
    if (!keys || !L_host || !W_host || !Y0_inout || !Y1_inout || !report || n < 1 || n > MK_MAX_N || d < 0 || ldw < n || ldy < n || ldw > MK_MAX_LD ||
        ldy > MK_MAX_LD || w < 1 || w > 64 || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product_pair: bad arguments");
    LabelSpmmForm f;
    if (!label_spmm_pair_select(n, d, (int)w, &f)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product_pair: shape not supported by the pair launch");
    if (!mk_labels_ok(L_host, (size_t)n * n, d)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product_pair: a label exceeds d");
    hipStream_t s = c->stream;
    const size_t yn = (size_t)(ldy * w + guard);
    uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)n * n * 4);
    const size_t wn = (size_t)ldw * 64;  // all 64 columns the launcher could take: those >= w are the caller's poison
    double* W = (double*)ctx_buf(c, "prof_mk_a", wn * 8);
    double* Y0 = (double*)ctx_buf(c, "prof_mk_c", yn * 8);
    double* Y1 = (double*)ctx_buf(c, "prof_mk_b", yn * 8);
    double* part = (double*)ctx_buf(c, "cm_part", label_spmm_pair_partial_doubles(n) * 8);
    if (!Lb || !W || !Y0 || !Y1 || !part) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Lb, L_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(W, W_host, wn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Y0, Y0_inout, yn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Y1, Y1_inout, yn * 8, hipMemcpyHostToDevice, s));
    const bool ran = launch_label_spmm_pair(s, n, Lb, keys, d, W, ldw, (int)w, part, Y0, ldy, Y1, ldy);
    HIP_TRY(c, hipMemcpyAsync(Y0_inout, Y0, yn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(Y1_inout, Y1, yn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    if (!ran) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label_product_pair: shape not supported by the pair launch");
    report[0] = f.mfma, report[1] = f.tile, report[2] = f.z, report[3] = f.cols_per_block;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_class_sums2(sdpsr_ctx* c, int64_t n, int64_t d, uint32_t first, int plain, const uint32_t* L_host, const double* X_host,
                                         double* Y_inout, int64_t guard, int32_t* report) {
    CHECK_CTX(c);
    if (!L_host || !X_host || !Y_inout || !report || n < 1 || n > MK_MAX_N || d < 1 || d > 4000 || first < 1 || (plain != 0 && plain != 1) ||
        (plain && first != 1) || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_sums2: bad arguments");
    // (the launcher's own rule, asked before anything is uploaded: one wave's tables, 64 lanes x (d + 1, made odd) pairs, within 150 KiB)
    if ((size_t)64 * ((d + 1) | 1) * 16 > 150 * 1024) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_sums2: no instance for this many classes");
    // plain: the kernel indexes its tables with the labels as they are
    if (plain && !mk_labels_ok(L_host, (size_t)n * n, d)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_sums2: a label exceeds d");
    hipStream_t s = c->stream;
    const size_t yn = (size_t)(2 * n * d + guard);
    uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)n * n * 4);
    double* X = (double*)ctx_buf(c, "prof_mk_a", (size_t)2 * n * 8);
    double* Y = (double*)ctx_buf(c, "prof_mk_c", yn * 8);
    if (!Lb || !X || !Y) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Lb, L_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(X, X_host, (size_t)2 * n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Y, Y_inout, yn * 8, hipMemcpyHostToDevice, s));
    const int W = launch_class_sums_pair(s, n, d, first, plain != 0, Lb, X, Y);
    HIP_TRY(c, hipMemcpyAsync(Y_inout, Y, yn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    if (!W) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_sums2: no instance for this many classes");
    report[0] = W;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_class_sums(sdpsr_ctx* c, int64_t n, int64_t d, int64_t ldo, const uint32_t* L_host, const double* x_host,
                                        double* out_inout, int64_t guard, int32_t* report) {
    CHECK_CTX(c);
    if (!L_host || !x_host || !out_inout || !report || n < 1 || n > MK_MAX_N || d < 1 || d > 4000 || ldo < n || ldo > MK_MAX_LD || guard < 0 ||
        guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_sums: bad arguments");
    if (!mk_labels_ok(L_host, (size_t)n * n, d)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_sums: a label exceeds d");
    // the per-lane tables in LDS take any ldo (class_sums_supports says so for an ldo != n); the fallback writes with ldo == n only
    const bool table = class_sums_supports(n, d, n + 1);
    report[0] = class_sums_supports(n, d, ldo) ? 1 : 0;
    report[1] = table ? 1 : 0;
    if (!report[0]) return SDPSR_OK;  // nothing ran: the caller (compress.cpp) does not call launch_class_sums either
    if (!table && !basis_image_two_stage_fits(n, d, 1)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_sums: the fallback does not take this shape");
    hipStream_t s = c->stream;
    const size_t on = (size_t)(ldo * d + guard);
    uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)n * n * 4);
    double* x = (double*)ctx_buf(c, "prof_mk_a", (size_t)n * 8);
    double* out = (double*)ctx_buf(c, "prof_mk_c", on * 8);
    if (!Lb || !x || !out) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Lb, L_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(x, x_host, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(out, out_inout, on * 8, hipMemcpyHostToDevice, s));
    launch_class_sums(s, n, d, Lb, x, out, ldo, 1);
    HIP_TRY(c, hipMemcpyAsync(out_inout, out, on * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_symmetrize(sdpsr_ctx* c, int64_t m, int64_t ld, double* B_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!B_inout || m < 1 || m > 1024 || ld < m || ld > 2048 || guard < 0 || guard > MK_MAX_GUARD) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "symmetrize: bad arguments");
    hipStream_t s = c->stream;
    const size_t bn = (size_t)(ld * m + guard);
    double* B = (double*)ctx_buf(c, "prof_mk_c", bn * 8);
    if (!B) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(B, B_inout, bn * 8, hipMemcpyHostToDevice, s));
    launch_symmetrize(s, m, ld, B);
    HIP_TRY(c, hipMemcpyAsync(B_inout, B, bn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_extract_symmetric(sdpsr_ctx* c, int64_t m, int64_t mp, int64_t lds, const double* src_host, double* dst_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!src_host || !dst_inout || m < 1 || mp < m || mp > 1024 || lds < m || lds > 2048 || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "extract_symmetric: bad arguments");
    hipStream_t s = c->stream;
    const size_t dn = (size_t)(mp * mp + guard);
    double* src = (double*)ctx_buf(c, "prof_mk_a", (size_t)lds * m * 8);
    double* dst = (double*)ctx_buf(c, "prof_mk_c", dn * 8);
    if (!src || !dst) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(src, src_host, (size_t)lds * m * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(dst, dst_inout, dn * 8, hipMemcpyHostToDevice, s));
    launch_extract_symmetric(s, m, mp, src, lds, dst);
    HIP_TRY(c, hipMemcpyAsync(dst_inout, dst, dn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_normalize_columns(sdpsr_ctx* c, int64_t n, int64_t ldx, int64_t hstride, int64_t nruns, const double* X_host,
                                               double* H_inout, double* norm_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!X_host || !H_inout || !norm_inout || n < 1 || n > MK_MAX_N || ldx < n || ldx > MK_MAX_LD || nruns < 1 || nruns > 64 ||
        (nruns > 1 && hstride < n) || hstride < 0 || hstride > 4 * MK_MAX_LD || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "normalize_columns: bad arguments");
    hipStream_t s = c->stream;
    const size_t hn = (size_t)(hstride * (nruns - 1) + n + guard), nn = (size_t)(nruns + guard);
    double* X = (double*)ctx_buf(c, "prof_mk_a", (size_t)ldx * nruns * 8);
    double* H = (double*)ctx_buf(c, "prof_mk_c", hn * 8);
    double* nrm = (double*)ctx_buf(c, "prof_mk_b", nn * 8);
    if (!X || !H || !nrm) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(X, X_host, (size_t)ldx * nruns * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(H, H_inout, hn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(nrm, norm_inout, nn * 8, hipMemcpyHostToDevice, s));
    launch_normalize_columns(s, n, ldx, H, hstride, X, ldx, (int)nruns, nrm);
    HIP_TRY(c, hipMemcpyAsync(H_inout, H, hn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(norm_inout, nrm, nn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_random_vector(sdpsr_ctx* c, int64_t n, uint64_t key, double* x_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!x_inout || n < 1 || n > MK_MAX_N || guard < 0 || guard > MK_MAX_GUARD) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "random_vector: bad arguments");
    hipStream_t s = c->stream;
    const size_t xn = (size_t)(n + guard);
    double* x = (double*)ctx_buf(c, "prof_mk_c", xn * 8);
    if (!x) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(x, x_inout, xn * 8, hipMemcpyHostToDevice, s));
    launch_random_vector(s, n, key, x);
    HIP_TRY(c, hipMemcpyAsync(x_inout, x, xn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The module growth's scratch discipline (tests/test_gpu_module_scratch.py): the form each entry runs is the one the ctx's
// flags choose, as in compress.cpp.
// ---------------------------------------------------------------------------------------------------------------------------
static bool mk_parent_form(const sdpsr_ctx* c) { return (c->opts.flags & SDPSR_FLAG_MODULE_SCRATCH_FILLS) != 0; }

extern "C" int sdpsr_profile_poison_scratch(sdpsr_ctx* c) {
    CHECK_CTX(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<uint64_t> pat;
    for (auto& kv : c->bufs) {
        if (!kv.second.p || !(kv.first.rfind("cm_", 0) == 0 || kv.first == "bd_qrm")) continue;
        const size_t words = kv.second.bytes / 8;
        if (pat.size() < words) pat.assign(words, 0x7FF85A5ADEADBEEFull);
        HIP_TRY(c, hipMemcpy(kv.second.p, pat.data(), words * 8, hipMemcpyHostToDevice));
    }
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_stacked_in_place(sdpsr_ctx* c, int64_t n, int64_t ldi, int64_t kk, int64_t lds, int64_t ncols, int64_t w, int64_t mcols,
                                              double* M_inout, const double* S_host, int64_t guard, int32_t* report) {
    CHECK_CTX(c);
    if (!M_inout || !S_host || !report || n < 1 || n > MK_MAX_N || ldi < n || ldi > MK_MAX_LD || kk < 1 || kk > 512 || lds < kk || lds > 1024 ||
        ncols < 1 || ncols > 512 || w < 1 || w > 512 || mcols < kk || mcols < w + ncols || mcols > 1024 || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "stacked_in_place: bad arguments");
    hipStream_t s = c->stream;
    const size_t mn = (size_t)(ldi * mcols + guard);
    double* M = (double*)ctx_buf(c, "prof_mk_a", mn * 8);
    double* S = (double*)ctx_buf(c, "prof_mk_b", (size_t)lds * ncols * 8);
    double* Q1 = (double*)ctx_buf(c, "prof_mk_c", (size_t)ldi * ncols * 8);
    if (!M || !S || !Q1) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(M, M_inout, mn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(S, S_host, (size_t)lds * ncols * 8, hipMemcpyHostToDevice, s));
    double* V = M + (size_t)w * ldi;
    const bool in_place = !mk_parent_form(c) && launch_tall_times_small_rows(s, n, ldi, M, (int)kk, S, (int)lds, (int)ncols, 1.0, 0.0, V, ldi);
    if (!in_place) {
        launch_tall_times_small(s, n, ldi, M, (int)kk, S, (int)lds, (int)ncols, 1.0, 0.0, Q1, ldi);
        HIP_TRY(c, hipMemcpy2DAsync(V, (size_t)ldi * 8, Q1, (size_t)ldi * 8, (size_t)n * 8, (size_t)ncols, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(c, hipMemcpyAsync(M_inout, M, mn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    report[0] = in_place ? 1 : 0;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_lift(sdpsr_ctx* c, int64_t n, int64_t ldi, int64_t kk, int64_t lds, int64_t S1, double atol, const double* In_host,
                                  const double* S_host, double* Qcm_inout, double* Qrm_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!In_host || !S_host || !Qcm_inout || !Qrm_inout || n < 1 || n > MK_MAX_N || ldi < n || ldi > MK_MAX_LD || kk < 1 || kk > 512 || lds < kk ||
        lds > 1024 || S1 < 1 || S1 > 512 || guard < 0 || guard > MK_MAX_GUARD || !(atol >= 0) ||
        (!mk_parent_form(c) && !tall_times_small_rows_supports((int)S1)))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "lift: bad arguments");
    hipStream_t s = c->stream;
    const size_t qn = (size_t)(n * S1 + guard);
    double* In = (double*)ctx_buf(c, "prof_mk_a", (size_t)ldi * kk * 8);
    double* S = (double*)ctx_buf(c, "prof_mk_b", (size_t)lds * S1 * 8);
    double* Qcm = (double*)ctx_buf(c, "prof_mk_c", qn * 8);
    double* Qrm = (double*)ctx_buf(c, "prof_mk_d", qn * 8);
    if (!In || !S || !Qcm || !Qrm) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(In, In_host, (size_t)ldi * kk * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(S, S_host, (size_t)lds * S1 * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Qcm, Qcm_inout, qn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Qrm, Qrm_inout, qn * 8, hipMemcpyHostToDevice, s));
    if (mk_parent_form(c)) {
        launch_tall_times_small(s, n, ldi, In, (int)kk, S, (int)lds, (int)S1, 1.0, 0.0, Qcm, n);
        launch_clamptol(s, n * S1, Qcm, atol);
        launch_transpose_to_rowmajor(s, n, S1, Qcm, Qrm);
    } else {
        launch_lift_clamped(s, n, ldi, In, (int)kk, S, (int)lds, (int)S1, atol, Qcm, Qrm);
    }
    HIP_TRY(c, hipMemcpyAsync(Qcm_inout, Qcm, qn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(Qrm_inout, Qrm, qn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_seed_vector(sdpsr_ctx* c, int64_t n, uint64_t key, double* x_inout, double* h_inout, double* norm_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!x_inout || !h_inout || !norm_inout || n < 1 || n > MK_MAX_N || guard < 0 || guard > MK_MAX_GUARD)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "seed_vector: bad arguments");
    hipStream_t s = c->stream;
    const size_t xn = (size_t)(n + guard), nn = (size_t)(1 + guard);
    double* x = (double*)ctx_buf(c, "prof_mk_a", xn * 8);
    double* h = (double*)ctx_buf(c, "prof_mk_c", xn * 8);
    double* nrm = (double*)ctx_buf(c, "prof_mk_b", nn * 8);
    if (!x || !h || !nrm) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(x, x_inout, xn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(h, h_inout, xn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(nrm, norm_inout, nn * 8, hipMemcpyHostToDevice, s));
    if (mk_parent_form(c)) {
        launch_random_vector(s, n, key, x);
        launch_normalize_columns(s, n, n, h, 0, x, n, 1, nrm);
    } else {
        launch_seed_vector(s, n, key, x, h, nrm);
    }
    HIP_TRY(c, hipMemcpyAsync(x_inout, x, xn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(h_inout, h, xn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(norm_inout, nrm, nn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_qrm_current(sdpsr_ctx* c, int32_t* current) {
    CHECK_CTX(c);
    if (!current) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    *current = c->bd_qrm_current ? 1 : 0;
    return SDPSR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The steps of blockDiagonalize(P; complex = true) on caller-made inputs (tests/test_gpu_complex_steps.py), by the conventions
// of the module-kernel entries above: host arrays in (column-major, real / imaginary planes with ld = n), every *_inout array
// uploaded as the caller filled it and downloaded whole, the product's own launcher or host function called the way
// complex.cpp calls it, nothing measured, every argument that could index outside a buffer refused before any upload.
// route 0: the one-workgroup kernels of n <= 64; route 1: the route through the real embedding (the driver's for n > 64).
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
bool cx_common_ok(int route, int64_t n, int64_t guard) {
    return (route == 0 || route == 1) && n >= 1 && n <= SDPSR_CX_MAX_N && (route == 1 || n <= 64) && guard >= 0 && guard <= MK_MAX_GUARD;
}
// the planes of H (n x n) and of V (n x vcols) on the device
int cx_upload_planes(sdpsr_ctx* c, int64_t n, int64_t vcols, const double* Hr_host, const double* Hi_host, const double* Vr_host,
                     const double* Vi_host, double** Hr, double** Hi, double** Vr, double** Vi) {
    hipStream_t s = c->stream;
    const size_t hb = (size_t)n * n * 8, vb = (size_t)n * vcols * 8;
    *Hr = (double*)ctx_buf(c, "prof_cx_hr", hb);
    *Hi = (double*)ctx_buf(c, "prof_cx_hi", hb);
    *Vr = (double*)ctx_buf(c, "prof_cx_vr", vb);
    *Vi = (double*)ctx_buf(c, "prof_cx_vi", vb);
    if (!*Hr || !*Hi || !*Vr || !*Vi) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(*Hr, Hr_host, hb, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(*Hi, Hi_host, hb, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(*Vr, Vr_host, vb, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(*Vi, Vi_host, vb, hipMemcpyHostToDevice, s));
    return SDPSR_OK;
}
}  // namespace

extern "C" int sdpsr_profile_cx_gather_herm(sdpsr_ctx* c, int64_t n, const uint32_t* L_host, uint64_t key, double* Hr_inout, double* Hi_inout,
                                            int64_t guard) {
    CHECK_CTX(c);
    if (!L_host || !Hr_inout || !Hi_inout || !cx_common_ok(1, n, guard)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "cx_gather_herm: bad arguments");
    hipStream_t s = c->stream;
    const size_t hn = (size_t)(n * n + guard);
    uint32_t* L = (uint32_t*)ctx_buf(c, "prof_l", (size_t)n * n * 4);
    double* Hr = (double*)ctx_buf(c, "prof_cx_hr", hn * 8);
    double* Hi = (double*)ctx_buf(c, "prof_cx_hi", hn * 8);
    if (!L || !Hr || !Hi) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(L, L_host, (size_t)n * n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Hr, Hr_inout, hn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Hi, Hi_inout, hn * 8, hipMemcpyHostToDevice, s));
    launch_cx_gather_herm(s, n, L, key, Hr, Hi);
    HIP_TRY(c, hipMemcpyAsync(Hr_inout, Hr, hn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(Hi_inout, Hi, hn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_cx_heev(sdpsr_ctx* c, int route, int64_t n, const double* Hr_host, const double* Hi_host, double atol, double* w_inout,
                                     double* Vr_inout, double* Vi_inout, int64_t guard, int32_t* info_out) {
    CHECK_CTX(c);
    if (!Hr_host || !Hi_host || !w_inout || !Vr_inout || !Vi_inout || !info_out || !cx_common_ok(route, n, guard) || !(atol >= 0))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, route == 0 && n > 64 ? "cx_heev: route 0 takes n <= 64" : "cx_heev: bad arguments");
    hipStream_t s = c->stream;
    const size_t hb = (size_t)n * n * 8, wn = (size_t)(n + guard), vn = (size_t)(n * n + guard);
    double* Hr = (double*)ctx_buf(c, "prof_cx_hr", hb);
    double* Hi = (double*)ctx_buf(c, "prof_cx_hi", hb);
    double* Vr = (double*)ctx_buf(c, "prof_cx_vr", vn * 8);
    double* Vi = (double*)ctx_buf(c, "prof_cx_vi", vn * 8);
    double* w = (double*)ctx_buf(c, "prof_cx_w", wn * 8);
    int* info = (int*)ctx_buf(c, "prof_cx_info", 64);
    if (!Hr || !Hi || !Vr || !Vi || !w || !info) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Hr, Hr_host, hb, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Hi, Hi_host, hb, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Vr, Vr_inout, vn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Vi, Vi_inout, vn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(w, w_inout, wn * 8, hipMemcpyHostToDevice, s));
    info_out[0] = info_out[1] = 0;
    if (route == 0) {
        launch_cx_heev(s, n, Hr, Hi, w, Vr, Vi, info);
        HIP_TRY(c, hipMemcpyAsync(w_inout, w, wn * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(info_out, info, 8, hipMemcpyDeviceToHost, s));
    } else {
        std::vector<double> vals;  // the general route hands its eigenvalues back on the host: the guard of w stays the caller's
        const int st = cx_heev_general(c, n, Hr, Hi, atol, Vr, Vi, vals);
        if (st) return st;
        memcpy(w_inout, vals.data(), (size_t)n * 8);
    }
    HIP_TRY(c, hipMemcpyAsync(Vr_inout, Vr, vn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(Vi_inout, Vi, vn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_cx_block_norms(sdpsr_ctx* c, int route, int64_t n, const double* Hr_host, const double* Hi_host, const double* Vr_host,
                                            const double* Vi_host, const int32_t* space_of, int32_t neig, double* norms_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!Hr_host || !Hi_host || !Vr_host || !Vi_host || !space_of || !norms_inout || !cx_common_ok(route, n, guard) || neig < 1 || neig > n)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "cx_block_norms: bad arguments");
    for (int64_t a = 0; a < n; ++a)
        if (space_of[a] < 0 || space_of[a] >= neig) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "cx_block_norms: space_of points outside the norms");
    hipStream_t s = c->stream;
    const size_t nn = (size_t)((int64_t)neig * neig + guard);
    double *Hr, *Hi, *Vr, *Vi;
    int st = cx_upload_planes(c, n, n, Hr_host, Hi_host, Vr_host, Vi_host, &Hr, &Hi, &Vr, &Vi);
    if (st) return st;
    int32_t* dspace = (int32_t*)ctx_buf(c, "prof_cx_space", (size_t)n * 4);
    unsigned long long* dnorms = (unsigned long long*)ctx_buf(c, "prof_cx_norms", nn * 8);
    if (!dspace || !dnorms) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(dspace, space_of, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(dnorms, norms_inout, nn * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(dnorms, 0, (size_t)neig * neig * 8, s));  // the maxima start from the driver's zero fill
    if (route == 0) launch_cx_block_norms(s, n, Hr, Hi, Vr, Vi, dspace, neig, dnorms);
    else if ((st = cx_block_norms_general(c, n, Hr, Hi, Vr, Vi, dspace, neig, dnorms)) != SDPSR_OK) return st;
    HIP_TRY(c, hipMemcpyAsync(norms_inout, dnorms, nn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_cx_irreducible(sdpsr_ctx* c, int route, int64_t n, int64_t vcols, const double* Hr_host, const double* Hi_host,
                                            const double* Vr_host, const double* Vi_host, const int32_t* desc, int32_t ncols, double atol,
                                            double* Qhat_inout, int64_t guard) {
    CHECK_CTX(c);
    if (!Hr_host || !Hi_host || !Vr_host || !Vi_host || !desc || !Qhat_inout || !cx_common_ok(route, n, guard) || vcols < 1 ||
        vcols > SDPSR_CX_MAX_N || ncols < 1 || ncols > SDPSR_CX_MAX_N || !(atol >= 0))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "cx_irreducible: bad arguments");
    for (int32_t j = 0; j < ncols; ++j) {
        const int32_t* d = desc + 6 * (size_t)j;
        const bool col_ok = d[5] >= 0 && d[5] < ncols;
        const bool k0 = d[0] == 0 && d[1] >= 0 && d[1] < vcols;
        const bool k1 = d[0] == 1 && d[1] >= 0 && d[2] >= 1 && d[2] <= n && (int64_t)d[1] + d[2] <= vcols && d[3] >= 0 && d[4] >= 1 && d[4] <= n &&
                        (int64_t)d[3] + d[4] <= vcols;
        if (!col_ok || !(k0 || k1)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "cx_irreducible: a descriptor points outside V or Qhat");
    }
    if (route == 1 && !cx_irreducible_general_lds_bytes(n)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "cx_irreducible: order not supported by the general kernel");
    hipStream_t s = c->stream;
    const size_t qn = (size_t)(2 * n * ncols + guard);
    double *Hr, *Hi, *Vr, *Vi;
    const int st = cx_upload_planes(c, n, vcols, Hr_host, Hi_host, Vr_host, Vi_host, &Hr, &Hi, &Vr, &Vi);
    if (st) return st;
    int32_t* ddesc = (int32_t*)ctx_buf(c, "prof_cx_desc", (size_t)6 * ncols * 4);
    double* Qhat = (double*)ctx_buf(c, "prof_cx_qhat", qn * 8);
    if (!ddesc || !Qhat) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(ddesc, desc, (size_t)6 * ncols * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(Qhat, Qhat_inout, qn * 8, hipMemcpyHostToDevice, s));
    if (route == 0) launch_cx_irreducible(s, n, Hr, Hi, Vr, Vi, ddesc, ncols, atol, Qhat);
    else if (!launch_cx_irreducible_general(s, n, Hr, Hi, Vr, Vi, ddesc, ncols, atol, Qhat))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "cx_irreducible: order not supported by the general kernel");
    HIP_TRY(c, hipMemcpyAsync(Qhat_inout, Qhat, qn * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The steps of the real dense blockDiagonalize (eigdec.cpp; the kernels at the head of kernels_blockdiag.hip) on caller-made
// inputs (tests/test_gpu_dense_steps.py), by the conventions of the entries above: column-major host arrays in, every *_inout
// array uploaded as the caller filled it and downloaded whole, the launcher or step eigdec.cpp itself calls, nothing measured,
// every argument that could index outside a buffer refused before any upload.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t DS_MAX_N = 4096;
bool ds_guard_ok(int64_t guard) { return guard >= 0 && guard <= MK_MAX_GUARD; }
// upload / download of one in/out array of `count` 8-byte elements
int ds_up(sdpsr_ctx* c, void* dev, const void* host, size_t count) {
    HIP_TRY(c, hipMemcpyAsync(dev, host, count * 8, hipMemcpyHostToDevice, c->stream));
    return SDPSR_OK;
}
int ds_down(sdpsr_ctx* c, void* host, const void* dev, size_t count) {
    HIP_TRY(c, hipMemcpyAsync(host, dev, count * 8, hipMemcpyDeviceToHost, c->stream));
    return SDPSR_OK;
}
int ds_finish(sdpsr_ctx* c) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}
}  // namespace

extern "C" int sdpsr_profile_dense_block_norms(sdpsr_ctx* c, int route, int64_t n, int64_t ld, const double* A_host, const double* Q_host,
                                               const int32_t* space_of, int32_t neig, double* norms_inout, double* M_inout, double* T_inout,
                                               int64_t guard) {
    CHECK_CTX(c);
    if (route < 0 || route > 2 || n < 1 || n > DS_MAX_N || ld < n || ld > DS_MAX_N || !space_of || !norms_inout || neig < 1 || neig > n ||
        !ds_guard_ok(guard))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_block_norms: bad arguments");
    if (route != 2 && (!A_host || !Q_host)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_block_norms: bad arguments");
    if (route == 0 && n > 64) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_block_norms: route 0 takes n <= 64");
    if (route == 1 && (ld % 128 || !M_inout || !T_inout))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_block_norms: route 1 works on padded ld x ld buffers, ld a multiple of 128");
    if (route == 2 && !M_inout) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_block_norms: route 2 reads M_inout");
    for (int64_t a = 0; a < n; ++a)
        if (space_of[a] < 0 || space_of[a] >= neig) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_block_norms: space_of points outside the norms");
    hipStream_t s = c->stream;
    const int64_t cols = route == 1 ? ld : n;  // route 1: the padded squares of the driver
    const size_t in = (size_t)ld * cols, mn = in + (size_t)guard, nn = (size_t)neig * neig + (size_t)guard;
    double* A = route == 0 ? (double*)ctx_buf(c, "prof_ds_a", in * 8) : nullptr;
    double* Q = route != 2 ? (double*)ctx_buf(c, "prof_ds_q", in * 8) : nullptr;
    double* M = M_inout ? (double*)ctx_buf(c, "prof_ds_m", mn * 8) : nullptr;
    double* T = T_inout ? (double*)ctx_buf(c, "prof_ds_t", mn * 8) : nullptr;
    int32_t* dspace = (int32_t*)ctx_buf(c, "prof_ds_space", (size_t)n * 4);
    unsigned long long* dnorms = (unsigned long long*)ctx_buf(c, "prof_ds_norms", nn * 8);
    if ((route == 0 && !A) || (route != 2 && !Q) || (M_inout && !M) || (T_inout && !T) || !dspace || !dnorms) return SDPSR_OUT_OF_MEMORY;
    int st = SDPSR_OK;
    if (M) st = ds_up(c, M, M_inout, mn);
    if (!st && T) st = ds_up(c, T, T_inout, mn);
    if (!st && route == 0) st = ds_up(c, A, A_host, in);
    if (!st && route == 1) st = ds_up(c, M, A_host, in);  // the driver's Ap: the element goes in, M = Q'AQ comes out
    if (!st && route != 2) st = ds_up(c, Q, Q_host, in);
    if (!st) st = ds_up(c, dnorms, norms_inout, nn);
    if (st) return st;
    HIP_TRY(c, hipMemcpyAsync(dspace, space_of, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (route == 0) launch_small_qtaq_block_norms(s, n, ld, A, Q, dspace, neig, dnorms, M, T);
    else if (route == 1) couple_block_norms(s, n, ld, M, Q, T, dspace, neig, dnorms);
    else launch_block_norms(s, n, ld, M, dspace, neig, dnorms);
    if (M) st = ds_down(c, M_inout, M, mn);
    if (!st && T) st = ds_down(c, T_inout, T, mn);
    if (!st) st = ds_down(c, norms_inout, dnorms, nn);
    return st ? st : ds_finish(c);
}

extern "C" int sdpsr_profile_dense_cluster_norms(sdpsr_ctx* c, int64_t n, int64_t ld, const double* A_host, const double* Q_host,
                                                 const double* evals_host, double atol, const int32_t* einfo, void* pack_inout, double* T_inout,
                                                 int64_t guard) {
    CHECK_CTX(c);
    if (!A_host || !Q_host || !evals_host || !einfo || !pack_inout || n < 1 || n > 64 || ld < n || ld > DS_MAX_N || !ds_guard_ok(guard))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_cluster_norms: bad arguments");
    hipStream_t s = c->stream;
    const size_t in = (size_t)ld * n, tn = in + (size_t)guard, pn = small_cluster_pack_bytes(n) / 8 + (size_t)guard;
    double* A = (double*)ctx_buf(c, "prof_ds_a", in * 8);
    double* Q = (double*)ctx_buf(c, "prof_ds_q", in * 8);
    double* T = T_inout ? (double*)ctx_buf(c, "prof_ds_t", tn * 8) : nullptr;
    double* w = (double*)ctx_buf(c, "prof_ds_w", (size_t)n * 8);
    int* dinfo = (int*)ctx_buf(c, "prof_ds_info", 64);
    char* pack = (char*)ctx_buf(c, "prof_ds_pack", pn * 8);
    if (!A || !Q || (T_inout && !T) || !w || !dinfo || !pack) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, A, A_host, in);
    if (!st) st = ds_up(c, Q, Q_host, in);
    if (!st) st = ds_up(c, w, evals_host, (size_t)n);
    if (!st) st = ds_up(c, dinfo, einfo, 1);
    if (!st) st = ds_up(c, pack, pack_inout, pn);
    if (!st && T) st = ds_up(c, T, T_inout, tn);
    if (st) return st;
    launch_small_cluster_qtaq_block_norms(s, n, ld, A, Q, w, atol, dinfo, pack, T);
    st = ds_down(c, pack_inout, pack, pn);
    if (!st && T) st = ds_down(c, T_inout, T, tn);
    return st ? st : ds_finish(c);
}

extern "C" int sdpsr_profile_dense_classes(sdpsr_ctx* c, int32_t neig, double* norms_inout, const int32_t* dims_host, double atol,
                                           uint64_t* stat_out, double* edges_out, double* thr_out, uint64_t* bits_inout, int32_t* kpart_out,
                                           int64_t guard) {
    CHECK_CTX(c);
    if (!norms_inout || !dims_host || !stat_out || !edges_out || !thr_out || !bits_inout || !kpart_out || neig < 1 || neig > DS_MAX_N ||
        !(atol > 0) || !ds_guard_ok(guard))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_classes: bad arguments");
    for (int32_t i = 0; i < neig; ++i)
        if (dims_host[i] < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_classes: a dimension < 1");
    const int W = (neig + 63) / 64;
    const size_t nn = (size_t)neig * neig + (size_t)guard, bn = (size_t)neig * W + (size_t)guard;
    unsigned long long* dnorms = (unsigned long long*)ctx_buf(c, "prof_ds_norms", nn * 8);
    // the step's own buffers, sized with the guard: it asks for them by name and gets these
    unsigned long long* dbits = (unsigned long long*)ctx_buf(c, "bd_cbits", bn * 8);
    unsigned long long* stat = (unsigned long long*)ctx_buf(c, "bd_cstat", 32 * 8);
    if (!dnorms || !dbits || !stat) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, dnorms, norms_inout, nn);
    if (!st) st = ds_up(c, dbits, bits_inout, bn);
    if (st) return st;
    const std::vector<int32_t> dims(dims_host, dims_host + neig);
    std::vector<int> kpart;
    CouplingTrace tr;
    const int verdict = isomorphism_classes_device(c, dnorms, neig, dims, atol, kpart, &tr);
    if (verdict != SDPSR_OK && verdict != SDPSR_NUMERICAL_INCONSISTENCY) return verdict;
    st = ds_down(c, norms_inout, dnorms, nn);
    if (!st) st = ds_down(c, bits_inout, dbits, bn);
    if (!st) st = ds_down(c, stat_out, stat, 20);
    if (!st) st = ds_finish(c);
    if (st) return st;
    memcpy(edges_out, tr.edges, sizeof(tr.edges));
    *thr_out = tr.thr;
    for (int32_t i = 0; i < neig; ++i) kpart_out[i] = kpart[i];
    return verdict;
}

extern "C" int sdpsr_profile_dense_irreducible(sdpsr_ctx* c, int route, int64_t n, int64_t ldq, int64_t vcols, const double* Q_host,
                                               const double* Bf_host, int64_t nf, const int32_t* desc, int32_t npairs, double* Qhat_inout,
                                               int64_t ncols, int64_t guard, int32_t* report) {
    CHECK_CTX(c);
    if (!Q_host || !Bf_host || !desc || !Qhat_inout || !report || route < -1 || route > 1 || n < 1 || n > DS_MAX_N || ldq < n || ldq > DS_MAX_N ||
        vcols < 1 || vcols > DS_MAX_N || nf < 1 || nf > DS_MAX_N || npairs < 1 || npairs > DS_MAX_N || ncols < 1 || ncols > DS_MAX_N ||
        !ds_guard_ok(guard))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_irreducible: bad arguments");
    int64_t max_m2 = 0;
    for (int32_t p = 0; p < npairs; ++p) {
        const int32_t* d = desc + 7 * (size_t)p;
        // (m_i, m_j <= n as for eigenspaces: the one-by-one route keeps Q_j' b_i and Q_i' b_j in n doubles each)
        const bool ok = d[0] >= 0 && d[1] >= 1 && d[1] <= n && (int64_t)d[0] + d[1] <= vcols && d[2] >= 0 && d[3] >= 1 && d[3] <= n &&
                        (int64_t)d[2] + d[3] <= vcols &&
                        d[4] >= 0 && d[4] < nf && d[5] >= 0 && d[5] < nf && d[6] >= 0 && d[6] < ncols;
        if (!ok) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_irreducible: a descriptor points outside Q, B or Qhat");
        max_m2 = std::max<int64_t>(max_m2, (int64_t)d[1] + d[3]);
    }
    if (route == 0 && !irreducible_pairs_fit_lds(max_m2))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dense_irreducible: eigenspaces too large for the pair kernel");
    const size_t qn = (size_t)ldq * vcols, bn = (size_t)ldq * nf, hn = (size_t)n * ncols + (size_t)guard;
    double* Q = (double*)ctx_buf(c, "prof_ds_q", qn * 8);
    double* Bf = (double*)ctx_buf(c, "prof_ds_a", bn * 8);
    double* Qhat = (double*)ctx_buf(c, "prof_ds_m", hn * 8);
    if (!Q || !Bf || !Qhat) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, Q, Q_host, qn);
    if (!st) st = ds_up(c, Bf, Bf_host, bn);
    if (!st) st = ds_up(c, Qhat, Qhat_inout, hn);
    if (st) return st;
    const std::vector<int32_t> pairs(desc, desc + 7 * (size_t)npairs);
    int ran = -1;
    st = irreducible_pairs(c, n, ldq, Q, Bf, pairs, max_m2, Qhat, route, &ran);
    if (st) return st;
    st = ds_down(c, Qhat_inout, Qhat, hn);
    if (!st) st = ds_finish(c);
    if (!st) report[0] = ran;
    return st;
}

extern "C" int sdpsr_profile_copy_cols(sdpsr_ctx* c, int64_t n, int64_t count, const int32_t* src_cols, const int32_t* dst_cols,
                                       const double* src_host, int64_t ld_src, int64_t scols, double* dst_inout, int64_t ld_dst, int64_t dcols,
                                       int64_t guard) {
    CHECK_CTX(c);
    if (!src_cols || !dst_cols || !src_host || !dst_inout || n < 1 || n > DS_MAX_N || count < 1 || count > DS_MAX_N || ld_src < n ||
        ld_src > DS_MAX_N || ld_dst < n || ld_dst > DS_MAX_N || scols < 1 || scols > DS_MAX_N || dcols < 1 || dcols > DS_MAX_N || !ds_guard_ok(guard))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "copy_cols: bad arguments");
    for (int64_t k = 0; k < count; ++k)
        if (src_cols[k] < 0 || src_cols[k] >= scols || dst_cols[k] < 0 || dst_cols[k] >= dcols)
            return ctx_fail(c, SDPSR_BAD_ARGUMENT, "copy_cols: a column outside its matrix");
    const size_t sn = (size_t)ld_src * scols, dn = (size_t)ld_dst * dcols + (size_t)guard;
    double* src = (double*)ctx_buf(c, "prof_ds_q", sn * 8);
    double* dst = (double*)ctx_buf(c, "prof_ds_m", dn * 8);
    if (!src || !dst) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, src, src_host, sn);
    if (!st) st = ds_up(c, dst, dst_inout, dn);
    if (st) return st;
    launch_copy_cols(c->stream, n, count, src_cols, dst_cols, src, ld_src, dst, ld_dst);
    st = ds_down(c, dst_inout, dst, dn);
    return st ? st : ds_finish(c);
}

extern "C" int sdpsr_profile_clamptol(sdpsr_ctx* c, int64_t len, double* a_inout, double atol, int64_t guard) {
    CHECK_CTX(c);
    if (!a_inout || len < 1 || len > DS_MAX_N * DS_MAX_N || !(atol >= 0) || !ds_guard_ok(guard))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "clamptol: bad arguments");
    const size_t an = (size_t)len + (size_t)guard;
    double* a = (double*)ctx_buf(c, "prof_ds_m", an * 8);
    if (!a) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, a, a_inout, an);
    if (st) return st;
    launch_clamptol(c->stream, len, a, atol);
    st = ds_down(c, a_inout, a, an);
    return st ? st : ds_finish(c);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The stages of the dense symmetric eigensolver (eigen.cpp: syev_device) on caller-made inputs (tests/test_gpu_eigen_stages.py), by
// the conventions of the entries above.  Orders 2 <= n <= ld <= 4096, ld a multiple of 128 (the padded square sdpsr_syev_f64 makes).
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
bool es_shape_ok(int64_t n, int64_t ld, int64_t guard) { return n >= 2 && ld >= n && ld <= DS_MAX_N && ld % 128 == 0 && ds_guard_ok(guard); }
}  // namespace

// launch_sytrd on the buffers syev_device itself hands it ("ev_pad", "ev_val", "eig_E", "eig_tau", "eig_sytrd_ws"), so that a second
// call of the same shape in one ctx replays the cached graph.  May write: the leading n x n of A (the row form mirrors the lower
// triangle into the upper one first; d, e stay in the arrays, the reflectors go below the subdiagonal), d[0 .. n), e[0 .. n-1),
// tau[0 .. n-1).  Never: rows / columns n .. ld-1 of A, e[n-1], tau[n-1], the guards.
extern "C" int sdpsr_profile_sytrd(sdpsr_ctx* c, int64_t n, int64_t ld, double* A_inout, double* d_inout, double* e_inout, double* tau_inout,
                                   int64_t guard) {
    CHECK_CTX(c);
    if (!A_inout || !d_inout || !e_inout || !tau_inout || !es_shape_ok(n, ld, guard)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sytrd: bad arguments");
    const size_t an = (size_t)ld * ld + (size_t)guard, vn = (size_t)n + (size_t)guard;
    double* A = (double*)ctx_buf(c, "ev_pad", an * 8);
    double* d = (double*)ctx_buf(c, "ev_val", vn * 8);
    double* e = (double*)ctx_buf(c, "eig_E", vn * 8);
    double* tau = (double*)ctx_buf(c, "eig_tau", vn * 8);
    double* ws = (double*)ctx_buf(c, "eig_sytrd_ws", sytrd_workspace_doubles(n, ld) * sizeof(double));
    if (!A || !d || !e || !tau || !ws) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, A, A_inout, an);
    if (!st) st = ds_up(c, d, d_inout, vn);
    if (!st) st = ds_up(c, e, e_inout, vn);
    if (!st) st = ds_up(c, tau, tau_inout, vn);
    if (st) return st;
    launch_sytrd(c, n, A, ld, d, e, tau, ws);
    st = ds_down(c, A_inout, A, an);
    if (!st) st = ds_down(c, d_inout, d, vn);
    if (!st) st = ds_down(c, e_inout, e, vn);
    if (!st) st = ds_down(c, tau_inout, tau, vn);
    return st ? st : ds_finish(c);
}

// backtransform_prepare, then backtransform_apply, both on the main stream (the branch syev_device takes when the side stream cannot
// be forked): Z <- H_0 ... H_{n-2} Z, reflectors below the subdiagonal of A_host (ld x ld; nothing else of it is read), tau_host: n - 1.
// Z_inout: ld x ld + guard, uploaded as the caller filled it (the driver's padding rows and columns are zero).  The products run over
// all ld x ld of Z; what can CHANGE is rows 1 .. n-1 of it -- row 0, rows n .. ld-1 and, with zero padding columns, those columns
// come back with the values they had -- and never the guards.
extern "C" int sdpsr_profile_backtransform(sdpsr_ctx* c, int64_t n, int64_t ld, const double* A_host, const double* tau_host, double* Z_inout,
                                           int64_t guard) {
    CHECK_CTX(c);
    if (!A_host || !tau_host || !Z_inout || !es_shape_ok(n, ld, guard)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "backtransform: bad arguments");
    const size_t in = (size_t)ld * ld, zn = in + (size_t)guard;
    double* A = (double*)ctx_buf(c, "prof_es_a", in * 8);
    double* tau = (double*)ctx_buf(c, "prof_es_tau", (size_t)n * 8);
    double* Z = (double*)ctx_buf(c, "prof_es_z", zn * 8);
    if (!A || !tau || !Z) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, A, A_host, in);
    if (!st) st = ds_up(c, tau, tau_host, (size_t)n - 1);
    if (!st) st = ds_up(c, Z, Z_inout, zn);
    if (!st) st = backtransform_prepare(c, n, A, ld, tau);
    if (!st) st = backtransform_apply(c, n, ld, Z);
    if (!st) st = ds_down(c, Z_inout, Z, zn);
    return st ? st : ds_finish(c);
}

// The tridiagonal problem T = tridiag(e_host (n - 1), d_host (n), e_host) as syev_device issues it: zero fill of Z, upload of the merge
// descriptors, launch_stedc_check, launch_stedc, launch_stedc_check.  w_inout (n + guard): w[0 .. n) written, ascending.  Z_inout
// (ld x ld + guard): all ld x ld written -- the eigenvectors in the leading n x n, exact zeros in rows and columns n .. ld-1.
// SDPSR_SOLVER_ERROR (outputs filled) when a check raises the flag.
extern "C" int sdpsr_profile_stedc(sdpsr_ctx* c, int64_t n, int64_t ld, const double* d_host, const double* e_host, double* w_inout, double* Z_inout,
                                   int64_t guard) {
    CHECK_CTX(c);
    if (!d_host || !e_host || !w_inout || !Z_inout || !es_shape_ok(n, ld, guard)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "stedc: bad arguments");
    hipStream_t s = c->stream;
    const size_t in = (size_t)ld * ld, zn = in + (size_t)guard, wn = (size_t)n + (size_t)guard;
    double* d = (double*)ctx_buf(c, "prof_es_d", (size_t)n * 8);
    double* e = (double*)ctx_buf(c, "eig_E", (size_t)n * 8);
    double* w = (double*)ctx_buf(c, "prof_es_w", wn * 8);
    double* Z = (double*)ctx_buf(c, "prof_es_z", zn * 8);
    int* info = (int*)ctx_buf(c, "eig_info", 64);
    void* dws = ctx_buf(c, "eig_dc_ws", stedc_workspace_bytes(ld));
    double* W1 = (double*)ctx_buf(c, "eig_dc_w1", in * 8);
    double* W2 = (double*)ctx_buf(c, "eig_dc_w2", in * 8);
    if (!d || !e || !w || !Z || !info || !dws || !W1 || !W2) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, d, d_host, (size_t)n);
    if (!st) st = ds_up(c, e, e_host, (size_t)n - 1);
    if (!st) st = ds_up(c, w, w_inout, wn);
    if (!st) st = ds_up(c, Z, Z_inout, zn);
    if (st) return st;
    HIP_TRY(c, hipMemsetAsync(Z, 0, in * 8, s));
    std::vector<int> desc;
    const size_t db = stedc_descriptors(ld, desc);
    st = h2d_sync(c, stedc_descriptor_slot(dws, ld), desc.data(), db);
    if (st) return st;
    launch_stedc_check(s, n, d, e, 1, info);
    if (!launch_stedc(s, n, ld, d, e, w, Z, W1, W2, dws)) return ctx_fail(c, SDPSR_HIP_ERROR, "stedc: launch failed");
    launch_stedc_check(s, n, w, nullptr, 0, info);
    int hinfo[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(hinfo, info, 8, hipMemcpyDeviceToHost, s));
    st = ds_down(c, w_inout, w, wn);
    if (!st) st = ds_down(c, Z_inout, Z, zn);
    if (!st) st = ds_finish(c);
    if (st) return st;
    return hinfo[0] ? ctx_fail(c, SDPSR_SOLVER_ERROR, "stedc: the checks raised info = " + std::to_string(hinfo[0])) : SDPSR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The row-space kernels of sdpsr_compress_constraints (kernels_rowspace.hip) on caller-made inputs (tests/test_gpu_rowspace_kernels.py),
// by the conventions of the module-kernel entries: each calls the launcher rowspace.cpp calls, the way it calls it.  M and W are
// m x ncols, column-major with leading dimension m, 1 <= m <= 1024, 1 <= ncols, m * ncols <= 2^26.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t RS_MAX_M = 1024, RS_MAX_TOTAL = int64_t(1) << 26;
bool rs_shape_ok(int64_t m, int64_t ncols, int64_t guard) {
    return m >= 1 && m <= RS_MAX_M && ncols >= 1 && ncols <= RS_MAX_TOTAL && m * ncols <= RS_MAX_TOTAL && ds_guard_ok(guard);
}
}  // namespace

extern "C" int sdpsr_profile_rowspace_scale(sdpsr_ctx* c, int64_t m, int64_t d, const double* A_host, const double* b_host, double* W_inout,
                                            double* info_out, int64_t guard) {
    CHECK_CTX(c);
    if (d < 0 || d > RS_MAX_TOTAL) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowspace_scale: bad arguments");
    const int64_t ncols = d + (b_host ? 1 : 0);
    if ((d > 0 && !A_host) || !W_inout || !info_out || !rs_shape_ok(m, ncols, guard)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowspace_scale: bad arguments");
    const int64_t md = m * d, total = m * ncols;
    const size_t wn = (size_t)total + (size_t)guard;
    hipStream_t s = c->stream;
    double* A = md ? (double*)ctx_buf(c, "prof_rs_a", (size_t)md * 8) : nullptr;
    double* b = b_host ? (double*)ctx_buf(c, "prof_rs_b", (size_t)m * 8) : nullptr;
    double* W = (double*)ctx_buf(c, "prof_rs_w", wn * 8);
    double* pmax = (double*)ctx_buf(c, "cc_pmax", (size_t)rowspace_absmax_blocks(total) * 8);
    double* info = (double*)ctx_buf(c, "prof_rs_info", 64);
    uint32_t* flag = (uint32_t*)ctx_buf(c, "prim_flag", 64);
    if ((md && !A) || (b_host && !b) || !W || !pmax || !info || !flag) return SDPSR_OUT_OF_MEMORY;
    int st = md ? ds_up(c, A, A_host, (size_t)md) : SDPSR_OK;
    if (!st && b) st = ds_up(c, b, b_host, (size_t)m);
    if (!st) st = ds_up(c, W, W_inout, wn);
    if (st) return st;
    HIP_TRY(c, hipMemsetAsync(flag, 0, 4, s));
    launch_rowspace_scale(s, total, md, A, b, pmax, flag, W, info);
    st = ds_down(c, W_inout, W, wn);
    if (!st) st = ds_down(c, info_out, info, 2);
    return st ? st : ds_finish(c);
}

// (the partial sums are filled with NaN bytes first: a partial the Gram kernel did not write shows in G)
extern "C" int sdpsr_profile_rowspace_gram(sdpsr_ctx* c, int64_t m, int64_t ncols, const double* W_host, double* G_inout, int64_t guard,
                                           int32_t* report) {
    CHECK_CTX(c);
    if (!W_host || !G_inout || !report || !rs_shape_ok(m, ncols, guard)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowspace_gram: bad arguments");
    const size_t wn = (size_t)(m * ncols), gn = (size_t)(m * m) + (size_t)guard, pn = rowspace_gram_partial_doubles(m, ncols);
    hipStream_t s = c->stream;
    double* W = (double*)ctx_buf(c, "prof_rs_w", wn * 8);
    double* G = (double*)ctx_buf(c, "prof_rs_g", gn * 8);
    double* P = (double*)ctx_buf(c, "cc_partials", pn * 8);
    if (!W || !G || !P) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, W, W_host, wn);
    if (!st) st = ds_up(c, G, G_inout, gn);
    if (st) return st;
    HIP_TRY(c, hipMemsetAsync(P, 0xFF, pn * 8, s));
    launch_rowspace_gram(s, m, ncols, W, P, G);
    st = ds_down(c, G_inout, G, gn);
    if (!st) st = ds_finish(c);
    if (st) return st;
    int npairs, Z;
    int64_t cps;
    rowspace_gram_shape(m, ncols, &npairs, &Z, &cps);
    report[0] = npairs, report[1] = Z, report[2] = (int32_t)cps;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_rowspace_rotate(sdpsr_ctx* c, int64_t m, int64_t ncols, const double* J_host, double* W_inout, int64_t guard,
                                             int32_t* report) {
    CHECK_CTX(c);
    if (!J_host || !W_inout || !report || !rs_shape_ok(m, ncols, guard)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowspace_rotate: bad arguments");
    const size_t wn = (size_t)(m * ncols) + (size_t)guard;
    double* J = (double*)ctx_buf(c, "cc_j", (size_t)(m * m) * 8);
    double* W = (double*)ctx_buf(c, "prof_rs_w", wn * 8);
    if (!J || !W) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, J, J_host, (size_t)(m * m));
    if (!st) st = ds_up(c, W, W_inout, wn);
    if (st) return st;
    launch_rowspace_rotate(c->stream, m, ncols, J, W);
    st = ds_down(c, W_inout, W, wn);
    if (!st) st = ds_finish(c);
    if (st) return st;
    bool j_lds;
    report[0] = rowspace_chunk(m, &j_lds);
    report[1] = j_lds ? 1 : 0;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_rowspace_finish(sdpsr_ctx* c, int64_t m, int64_t ncols, int64_t r, const int32_t* perm_host, const double* sigma_host,
                                             double droptol, int in_place, double* W_inout, double* out_inout, double* sig_inout, int64_t* nnz_out,
                                             int64_t guard) {
    CHECK_CTX(c);
    if (!perm_host || !sigma_host || !W_inout || (!in_place && !out_inout) || !sig_inout || !nnz_out || !rs_shape_ok(m, ncols, guard) || r < 0 || r > m ||
        !(droptol >= 0))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowspace_finish: bad arguments");
    for (int64_t k = 0; k < m; ++k)
        if (perm_host[k] < 0 || perm_host[k] >= m) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowspace_finish: a perm entry outside [0, m)");
    const size_t wn = (size_t)(m * ncols) + (size_t)guard, sn = (size_t)m + (size_t)guard;
    hipStream_t s = c->stream;
    double* W = (double*)ctx_buf(c, "prof_rs_w", wn * 8);
    double* out = in_place ? W : (double*)ctx_buf(c, "prof_rs_out", wn * 8);
    double* sigma = (double*)ctx_buf(c, "prof_rs_sigma", (size_t)m * 8);
    double* sig = (double*)ctx_buf(c, "prof_rs_sig", sn * 8);
    int32_t* perm = (int32_t*)ctx_buf(c, "prof_rs_perm", (size_t)m * 4);
    unsigned long long* nnz = (unsigned long long*)ctx_buf(c, "prof_rs_nnz", 64);
    if (!W || !out || !sigma || !sig || !perm || !nnz) return SDPSR_OUT_OF_MEMORY;
    int st = ds_up(c, W, W_inout, wn);
    if (!st && !in_place) st = ds_up(c, out, out_inout, wn);
    if (!st) st = ds_up(c, sigma, sigma_host, (size_t)m);
    if (!st) st = ds_up(c, sig, sig_inout, sn);
    if (st) return st;
    HIP_TRY(c, hipMemcpyAsync(perm, perm_host, (size_t)m * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(nnz, 0, 8, s));
    launch_rowspace_finish(s, m, ncols, r, W, perm, sigma, sig, droptol, out, nnz);
    unsigned long long hn = 0;
    HIP_TRY(c, hipMemcpyAsync(&hn, nnz, 8, hipMemcpyDeviceToHost, s));
    st = ds_down(c, W_inout, W, wn);
    if (!st && !in_place) st = ds_down(c, out_inout, out, wn);
    if (!st) st = ds_down(c, sig_inout, sig, sn);
    if (!st) st = ds_finish(c);
    if (st) return st;
    *nnz_out = (int64_t)hn;
    return SDPSR_OK;
}

extern "C" int sdpsr_profile_kernel(sdpsr_ctx* c, int kind, int64_t n, int64_t aux, int reps,
                                    double* ms_per_launch) {
    CHECK_CTX(c);
    if (!ms_per_launch || n < 1 || reps < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    if (kind == 11) n = n * n;  // (kind 11 takes the array length below)
    hipStream_t s = c->stream;
    const int64_t ld = round_up(n, 128);
    hipEvent_t e0, e1;
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    int st = SDPSR_OK;
    if (kind >= 0 && kind <= 2) {
        const size_t es = kind == 0 ? 1 : (kind == 1 ? 4 : 8);
        const size_t os = kind == 0 ? 4 : es;
        // aux = batch (channels of one launch, as the product path launches them); operands of
        // all channels are distinct memory
        // aux >= 100: the lower-triangle launch of the product path (symmetric labels), batch aux - 100
        // aux 100..: the default kernel of that launch (int8: the persistent 256 x 256 launch of kernels_gemm_sym.hip);
        // 200..: int8 with 128 x 128 tiles (round 3's launch); 300..: the persistent launch with two 128-byte stages
        const bool tri = aux >= 100 && kind <= 1;
        // 1000 * d + 100..: diagnostic build d of the persistent launch (1 no MFMAs, 2 no DMA after the prologue, 4 no stores);
        // 400..: the operand's leading dimension padded by 128 bytes (row stride not a power of two)
        int sq_variant = aux >= 1000 ? 1000 + (int)(aux / 1000) : (aux >= 300 && aux < 400 ? 128 : (aux >= 200 && aux < 300 ? 1 : 0));
        const int64_t ldx_pad = (aux % 1000) >= 400 && (aux % 1000) < 500 ? 128 : 0;
        if (tri) aux %= 100;
        const int bt = (int)std::min<int64_t>(std::max<int64_t>(aux, 1), 8);
        uint32_t* zflag = (uint32_t*)ctx_buf(c, "prof_zero", 64);
        if (!zflag) return SDPSR_OUT_OF_MEMORY;
        HIP_TRY(c, hipMemsetAsync(zflag, 0, 64, s));
        void* X = ctx_buf(c, "prof_x", (size_t)(ld + 128) * ld * es * bt);
        void* Cc = ctx_buf(c, "prof_c", (size_t)ld * ld * os * bt);
        uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)ld * ld * 4);
        if (!X || !Cc || !Lb) return SDPSR_OUT_OF_MEMORY;
        // random symmetric operand with full-range values (not zeros: clocks differ on zeros)
        HIP_TRY(c, hipMemsetAsync(Lb, 0, (size_t)ld * ld * 4, s));
        launch_fill_test_sig(s, ld * ld / 2, 1 << 20, (uint64_t*)Lb);  // pseudo-random labels
        for (int b = 0; b < bt; ++b) {
            if (kind == 0) launch_gather_i8(s, ld, ld, 1, Lb, 12345 + b, (int8_t*)X + (size_t)b * ld * ld);
            else if (kind == 1) launch_gather_f32(s, ld, ld, 1, 45, Lb, 12345 + b, (float*)X + (size_t)b * ld * ld);
            else launch_gather_f64_padded(s, ld, ld, Lb, 12345 + b, (double*)X + (size_t)b * ld * ld);
        }
        const int64_t sb = ld * ld;
        auto run = [&]() {
            if (tri && kind == 0) launch_gemm_tn_i8_sym(s, ld, ld, (int8_t*)X, ld + ldx_pad, (int32_t*)Cc, ld, bt, sb + ldx_pad * ld, sb, zflag, c->num_cus, sq_variant);
            else if (tri && kind == 1) launch_gemm_tn_f32_sym(s, ld, ld, (float*)X, ld, (float*)Cc, ld, bt, sb, sb, zflag);
            else if (kind == 0) launch_gemm_tn_i8(s, ld, ld, ld, (int8_t*)X, ld, (int8_t*)X, ld, (int32_t*)Cc, ld, bt, sb, sb, sb);
            else if (kind == 1) launch_gemm_tn_f32(s, ld, ld, ld, (float*)X, ld, (float*)X, ld, (float*)Cc, ld, bt, sb, sb, sb);
            else launch_gemm_tn_f64(s, ld, ld, ld, (double*)X, ld, (double*)X, ld, (double*)Cc, ld, bt, sb, sb, sb);
        };
        run();
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) run();
        HIP_TRY(c, hipEventRecord(e1, s));
    } else if (kind == 3) {
        const int64_t len = n * n;
        uint64_t* sig = (uint64_t*)ctx_buf(c, "sig", len * 8);
        uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)len * 4);
        if (!sig || !Lb) return SDPSR_OUT_OF_MEMORY;
        launch_fill_test_sig(s, len, std::max<int64_t>(aux, 1), sig);
        int64_t np = 0;
        st = refine_signatures(c, len, sig, Lb, &np);  // warm-up + table sizing
        if (st) return st;
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) {
            st = refine_signatures(c, len, sig, Lb, &np);
            if (st) return st;
        }
        HIP_TRY(c, hipEventRecord(e1, s));
    } else if (kind == 11) {
        // the refinement as the FIRST one of a call meets it: no class-count prediction (the loop resets the hint at the
        // start of every admissible_subspace), so a many-classes input pays the overflowing first pass, the sample and
        // the materialised path every time.  n < 0: a len = -n array instead of n x n
        const int64_t len = n;
        uint64_t* sig = (uint64_t*)ctx_buf(c, "sig", len * 8);
        uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)len * 4);
        if (!sig || !Lb) return SDPSR_OUT_OF_MEMORY;
        launch_fill_test_sig(s, len, std::max<int64_t>(aux, 1), sig);
        int64_t np = 0;
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) {
            c->table_log2_hint = 12;
            st = refine_signatures(c, len, sig, Lb, &np);
            if (st) return st;
        }
        HIP_TRY(c, hipEventRecord(e1, s));
    } else if (kind == 4) {
        const int64_t len = n * n, r = std::max<int64_t>(aux, 0);
        uint64_t* sig = (uint64_t*)ctx_buf(c, "sig", len * 8);
        uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)len * 4);
        double* U = (double*)ctx_buf(c, "prof_u", (size_t)len * std::max<int64_t>(r, 1) * 8);
        double* partial = (double*)ctx_buf(c, "proj_partial", (size_t)std::max<int64_t>(r, 1) * 2048 * 8);
        double* coef = (double*)ctx_buf(c, "proj_coef", (size_t)std::max<int64_t>(r, 1) * 8);
        if (!sig || !Lb || !U || !partial || !coef) return SDPSR_OUT_OF_MEMORY;
        HIP_TRY(c, hipMemsetAsync(Lb, 0, (size_t)len * 4, s));
        launch_fill_test_sig(s, len / 2, 1000, (uint64_t*)Lb);
        HIP_TRY(c, hipMemsetAsync(U, 0, (size_t)len * std::max<int64_t>(r, 1) * 8, s));
        auto run = [&]() {
            launch_proj_coef(s, len, r, U, Lb, 777, nullptr, partial, 2048, coef);
            launch_proj_apply(s, len, r, U, Lb, 777, nullptr, coef, 1.5e-8, 1e7, 1, nullptr, sig);
        };
        run();
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) run();
        HIP_TRY(c, hipEventRecord(e1, s));
    } else if (kind == 5 || kind == 6) {
        // 5: the symv kernel of the tridiagonalisation alone, one launch per column j = 0..n-2
        //    (ms_per_launch = total / (n-1));  6: the whole tridiagonalisation (ms per sytrd)
        double* A = (double*)ctx_buf(c, "prof_x", (size_t)ld * ld * 8);
        uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)ld * ld * 4);
        double* ws = (double*)ctx_buf(c, "eig_sytrd_ws", sytrd_workspace_doubles(n, ld) * 8);
        double* dd = (double*)ctx_buf(c, "prof_d", (size_t)3 * n * 8);
        if (!A || !Lb || !ws || !dd) return SDPSR_OUT_OF_MEMORY;
        // symmetric pseudo-random matrix: labels symmetric in (i,j)
        std::vector<uint32_t> hl((size_t)n * n);
        for (int64_t j2 = 0; j2 < n; ++j2)
            for (int64_t i2 = 0; i2 < n; ++i2) {
                const int64_t lo = std::min(i2, j2), hi = std::max(i2, j2);
                hl[(size_t)i2 + j2 * n] = (uint32_t)(sdpsr_fmix64((uint64_t)(lo * 1315423911ll + hi)) | 1u);
            }
        HIP_TRY(c, hipMemcpyAsync(Lb, hl.data(), (size_t)n * n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        const int runs = (kind == 5) ? 1 : reps;
        launch_gather_f64_padded(s, n, ld, Lb, 999, A);
        if (kind == 6) launch_sytrd(c, n, A, ld, dd, dd + n, dd + 2 * n, ws);  // warm-up
        launch_gather_f64_padded(s, n, ld, Lb, 999, A);
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int i = 0; i < runs; ++i) {
            if (kind == 5) launch_sytrd_symv_sweep(s, n, A, ld, dd, dd + n, dd + 2 * n, ws);
            else launch_sytrd(c, n, A, ld, dd, dd + n, dd + 2 * n, ws);
        }
        HIP_TRY(c, hipEventRecord(e1, s));
        HIP_TRY(c, hipEventSynchronize(e1));
        float ms5 = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms5, e0, e1));
        ms_per_launch[0] = (kind == 5) ? (double)ms5 / (double)std::max<int64_t>(n - 1, 1) : (double)ms5 / runs;
        hipEventDestroy(e0);
        hipEventDestroy(e1);
        HIP_TRY(c, hipGetLastError());
        return SDPSR_OK;
    } else if (kind == 8) {
        // one-workgroup Jacobi eigensolver (n <= 128) on a device-resident random symmetric matrix
        if (n > 128) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "kind 8: n <= 128");
        double* A = (double*)ctx_buf(c, "prof_x", (size_t)(reps + 1) * n * n * 8);
        double* wv = (double*)ctx_buf(c, "prof_d", (size_t)n * 8 + 64);
        double* Vt = (double*)ctx_buf(c, "prof_c", (size_t)n * n * 8);
        int* info = (int*)ctx_buf(c, "eig_info", 64);
        if (!A || !wv || !Vt || !info) return SDPSR_OUT_OF_MEMORY;
        std::vector<double> h((size_t)(reps + 1) * n * n);
        for (int rp = 0; rp <= reps; ++rp)
            for (int64_t j2 = 0; j2 < n; ++j2)
                for (int64_t i2 = 0; i2 <= j2; ++i2) {
                    const double v = (double)(sdpsr_fmix64((uint64_t)(rp * 7919 + i2 * 131 + j2 * 1000003)) >> 11) * (1.0 / 9007199254740992.0);
                    h[(size_t)rp * n * n + i2 + j2 * n] = h[(size_t)rp * n * n + j2 + i2 * n] = v;
                }
        HIP_TRY(c, hipMemcpyAsync(A, h.data(), h.size() * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        launch_small_syev(s, n, A + (size_t)reps * n * n, n, wv, Vt, info);  // warm-up
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) launch_small_syev(s, n, A + (size_t)i * n * n, n, wv, Vt, info);
        HIP_TRY(c, hipEventRecord(e1, s));
    } else if (kind == 9) {
        // label product Y = A(v) W of the module-compression driver: aux = w | G << 8 | d << 12 (| 1 << 30:
        // report the largest deviation from a host evaluation of sampled rows instead of the time)
        const int w = (int)(aux & 0xff), G = ((aux >> 8) & 0xf) ? (int)((aux >> 8) & 0xf) : 1;
        const int64_t d = ((aux >> 12) & 0xffff) ? ((aux >> 12) & 0xffff) : 34;
        const bool verify = (aux >> 30) & 1;
        if (w < 1 || G * w > 64) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "kind 9: 1 <= G w <= 64");
        uint32_t* Lb = (uint32_t*)ctx_buf(c, "prof_l", (size_t)n * n * 4);
        double* W = (double*)ctx_buf(c, "prof_x", (size_t)n * w * 8);
        double* Y = (double*)ctx_buf(c, "prof_c", (size_t)n * G * w * 8);
        double* part = (double*)ctx_buf(c, "cm_part", label_spmm_partial_doubles(n, 64) * 8);
        if (!Lb || !W || !Y || !part) return SDPSR_OUT_OF_MEMORY;
        std::vector<uint32_t> hl((size_t)n * n);
        std::vector<double> hw((size_t)n * w);
        for (size_t e = 0; e < hl.size(); ++e) hl[e] = (uint32_t)(sdpsr_fmix64(e * 2654435761ull + 17) % (uint64_t)(d + 1));
        for (size_t e = 0; e < hw.size(); ++e) hw[e] = 2.0 * ((double)(sdpsr_fmix64(e + 99991) >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
        const uint64_t keys[4] = {0x1234567ull, 0x89abcdefull, 0x13579bdfull, 0x2468aceull};
        HIP_TRY(c, hipMemcpyAsync(Lb, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(W, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (!launch_label_spmm_multi(s, n, Lb, keys, G, d, W, n, w, part, Y, n))
            return ctx_fail(c, SDPSR_BAD_ARGUMENT, "kind 9: shape not supported by the label product");
        HIP_TRY(c, hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) launch_label_spmm_multi(s, n, Lb, keys, G, d, W, n, w, part, Y, n);
        HIP_TRY(c, hipEventRecord(e1, s));
        if (verify) {
            std::vector<double> hy((size_t)n * G * w);
            HIP_TRY(c, hipMemcpyAsync(hy.data(), Y, hy.size() * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            double worst = 0;
            const int64_t rows[12] = {0, 1, 15, 16, 17, 63, 64, n / 3, n / 2, n - 17, n - 2, n - 1};
            for (int64_t r : rows) {
                if (r < 0 || r >= n) continue;
                for (int g = 0; g < G; ++g)
                    for (int j = 0; j < w; ++j) {
                        long double acc = 0;
                        for (int64_t cc = 0; cc < n; ++cc) {
                            const uint32_t lab = hl[(size_t)r + (size_t)cc * n];
                            if (lab) acc += (long double)sdpsr_class_uniform(keys[g], lab) * hw[(size_t)cc + (size_t)j * n];
                        }
                        worst = std::max(worst, std::fabs((double)acc - hy[(size_t)r + (size_t)(g * w + j) * n]));
                    }
            }
            ms_per_launch[0] = worst;
            hipEventDestroy(e0);
            hipEventDestroy(e1);
            return SDPSR_OK;
        }
    } else if (kind == 10) {
        // the host eigensolver of the compressed problem (host_syev.cpp: Householder + implicit QL, order n <= 512) on a
        // random symmetric matrix: wall-clock milliseconds per solve on ONE host core (no device work)
        if (n > 512) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "kind 10: n <= 512");
        std::vector<double> h((size_t)n * n), w((size_t)n), z((size_t)n * n);
        for (int64_t j2 = 0; j2 < n; ++j2)
            for (int64_t i2 = 0; i2 <= j2; ++i2) {
                const double v = (double)(sdpsr_fmix64((uint64_t)(i2 * 131 + j2 * 1000003 + 17)) >> 11) * (1.0 / 9007199254740992.0);
                h[(size_t)i2 + j2 * n] = h[(size_t)j2 + i2 * n] = v;
            }
        host_syev((int)n, h.data(), (int)n, w.data(), z.data(), (int)n);  // warm-up
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) host_syev((int)n, h.data(), (int)n, w.data(), z.data(), (int)n);
        ms_per_launch[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
        hipEventDestroy(e0);
        hipEventDestroy(e1);
        return SDPSR_OK;
    } else {
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "unknown kernel kind");
    }
    HIP_TRY(c, hipEventSynchronize(e1));
    HIP_TRY(c, hipGetLastError());
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    ms_per_launch[0] = (double)ms / reps;
    if (kind == 8 && aux == 1) {  // diagnostic: sweeps of the last run instead of the time
        int h[2] = {0, 0};
        HIP_TRY(c, hipMemcpy(h, ctx_buf(c, "eig_info", 64), 8, hipMemcpyDeviceToHost));
        ms_per_launch[0] = (double)h[1];
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return SDPSR_OK;
}

// Diagnostic: sdpsr_profile_kernel(kind, n, aux, reps) with the shader clock sampled meanwhile.
// out[0] = ms per launch, out[1] = median shader clock (MHz) over the ~20 us intervals of the run,
// out[2] = number of intervals used.
extern "C" int sdpsr_profile_clock(sdpsr_ctx* c, int kind, int64_t n, int64_t aux, int reps, double* out) {
    CHECK_CTX(c);
    if (!out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    double ms = 0;
    int st = sdpsr_profile_kernel(c, kind, n, aux, 1, &ms);  // buffers, tables, clocks: warm
    if (st) return st;
    const int NS = 8192;
    long long* buf = (long long*)ctx_buf(c, "clk_buf", (size_t)(2 * NS + 8) * 8);
    unsigned* flag = (unsigned*)ctx_buf(c, "clk_flag", 64);
    if (!buf || !flag) return SDPSR_OUT_OF_MEMORY;
    long long* marks = buf + 2 * NS;
    int* count = (int*)(flag + 8);
    hipStream_t side = nullptr;
    HIP_TRY(c, hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    HIP_TRY(c, hipMemsetAsync(flag, 0, 64, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    launch_clock_sampler(side, buf, NS, flag, 200000000ll /* 2 s */, count);
    launch_wall_marker(c->stream, marks);
    st = sdpsr_profile_kernel(c, kind, n, aux, reps, &ms);
    launch_wall_marker(c->stream, marks + 1);
    hipMemsetAsync(flag, 1, 4, c->stream);  // releases the sampler whatever happened above
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(side);
    hipStreamDestroy(side);
    if (st) return st;
    std::vector<long long> h((size_t)2 * NS + 8);
    int hc = 0;
    HIP_TRY(c, hipMemcpy(h.data(), buf, h.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&hc, count, 4, hipMemcpyDeviceToHost));
    std::vector<double> mhz;
    // the timed launches are the tail of the marked window (set-up and warm-up come first): use its second half
    const long long t0 = h[2 * NS] + (h[2 * NS + 1] - h[2 * NS]) / 2, t1 = h[2 * NS + 1];
    for (int i = 1; i < hc; ++i) {
        const long long w0 = h[2 * (i - 1) + 1], w1 = h[2 * i + 1];
        if (w0 >= t0 && w1 <= t1 && w1 > w0) mhz.push_back((double)(h[2 * i] - h[2 * (i - 1)]) / (double)(w1 - w0) * 100.0);
    }
    std::sort(mhz.begin(), mhz.end());
    out[0] = ms;
    out[1] = mhz.empty() ? 0.0 : mhz[mhz.size() / 2];
    out[2] = (double)mhz.size();
    return SDPSR_OK;
}

