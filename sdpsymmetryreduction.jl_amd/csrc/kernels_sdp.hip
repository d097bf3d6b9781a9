// The vector side of sdpsr_sdp_solve (sdp_solve.cpp): the setup's Gram matrix M = I + B'B and its dense products, and the
// loop's affine step x = Kt g + x0 fused with the update of the non-negative split.  The cone side is kernels_psd.hip, the
// pencil B and its adjoint are kernels_blockop.hip.  Every sum here has an order fixed by the sizes alone; no floating-point
// atomics.
#include "host_internal.h"

namespace sdpsr {

namespace {

constexpr int SDP_T = 256;

// ---- setup -------------------------------------------------------------------------------------------------------------
// cls[p] = class of the position-major record p (the key of the stable sort that brings the records into (class, position) order)
__global__ void __launch_bounds__(SDP_T)
sdp_record_class_kernel(int64_t n, const uint4* __restrict__ rec, uint32_t* __restrict__ cls) {
    for (int64_t p = (int64_t)blockIdx.x * SDP_T + threadIdx.x; p < n; p += (int64_t)gridDim.x * SDP_T) cls[p] = rec[p].y;
}

// cptr[i] = first record of class i in the records sorted by (class, position): the lower bound of i, i <= d
__global__ void __launch_bounds__(SDP_T)
sdp_class_offsets_kernel(int64_t n, int64_t d, const uint4* __restrict__ rec, long long* __restrict__ cptr) {
    const int64_t i = (int64_t)blockIdx.x * SDP_T + threadIdx.x;
    if (i > d) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)rec[mid].x < i) lo = mid + 1; else hi = mid;
    }
    cptr[i] = lo;
}

__device__ __forceinline__ double sdp_rec_val(const uint4 r) { return __hiloint2double((int)r.w, (int)r.z); }

// M[i, j] = [i == j] + sum over the positions p that classes i and j share of (sum of i's values at p) * (sum of j's values at p),
// p ascending: a merge of the two classes' record runs, both sorted by position.  One thread per element of the lower
// triangle, mirrored: M is symmetric bit for bit.  (Setup, run once per solve: the runs are read at random.)
__global__ void __launch_bounds__(SDP_T)
sdp_gram_kernel(int64_t d, const uint4* __restrict__ rec, const long long* __restrict__ cptr, double* __restrict__ M) {
    const int64_t i = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4), j = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= d || j > i) return;
    int64_t a = cptr[i], b = cptr[j];
    const int64_t ae = cptr[i + 1], be = cptr[j + 1];
    double acc = 0.0;
    while (a < ae && b < be) {
        const uint32_t pa = rec[a].y, pb = rec[b].y;
        if (pa < pb) {
            ++a;
        } else if (pb < pa) {
            ++b;
        } else {
            double sa = 0.0, sb = 0.0;
            for (; a < ae && rec[a].y == pa; ++a) sa += sdp_rec_val(rec[a]);
            for (; b < be && rec[b].y == pa; ++b) sb += sdp_rec_val(rec[b]);
            acc = fma(sa, sb, acc);
        }
    }
    if (i == j) acc += 1.0;
    M[i + j * d] = acc;
    M[j + i * d] = acc;
}

// V[:, k] *= 1 / sqrt(w[k]).  M = I + B'B has w >= 1; a w[k] that is not a positive finite number (a NaN in the operator) makes
// the column NaN, which the loop's first verdict reports.
__global__ void __launch_bounds__(SDP_T)
sdp_scale_columns_kernel(int64_t d, const double* __restrict__ w, double* __restrict__ V) {
    const int64_t total = d * d;
    for (int64_t e = (int64_t)blockIdx.x * SDP_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * SDP_T) {
        const double wk = w[e / d];
        V[e] *= (wk > 0.0 && wk < INFINITY) ? 1.0 / sqrt(wk) : __longlong_as_double(0x7FF8000000000000ll);
    }
}

// C (m x n, ld ldc) = alpha * A B + beta * C with A[i, k] at A[i * ar + k * ac], B[k, j] at B[k * br + j * bc]: 16 x 16 tiles
// through LDS, every element summed over k ascending by its own thread.  The dense products of the setup (at most d <= 4096).
__global__ void __launch_bounds__(SDP_T)
sdp_gemm_kernel(int64_t m, int64_t n, int64_t k, const double* __restrict__ A, int64_t ar, int64_t ac, const double* __restrict__ B,
                int64_t br, int64_t bc, double alpha, double beta, double* __restrict__ C, int64_t ldc) {
    __shared__ double sa[16][17], sb[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * 16, j0 = (int64_t)blockIdx.y * 16;
    double acc = 0.0;
    for (int64_t k0 = 0; k0 < k; k0 += 16) {
        // sa[kk][ii] = A[i0 + ii, k0 + kk], sb[kk][jj] = B[k0 + kk, j0 + jj]
        sa[ty][tx] = (i0 + tx < m && k0 + ty < k) ? A[(i0 + tx) * ar + (k0 + ty) * ac] : 0.0;
        sb[ty][tx] = (k0 + ty < k && j0 + tx < n) ? B[(k0 + ty) * br + (j0 + tx) * bc] : 0.0;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = fma(sa[kk][tx], sb[kk][ty], acc);
        __syncthreads();
    }
    const int64_t i = i0 + tx, j = j0 + ty;
    if (i < m && j < n) C[i + j * ldc] = beta == 0.0 ? alpha * acc : fma(alpha, acc, beta * C[i + j * ldc]);
}

// ---- the loop ----------------------------------------------------------------------------------------------------------
// One wave per row i:  g_j = uml_j + adj_j - chat_j / rho  (staged in LDS by the workgroup),
//   x_i = x0_i + sum_j Kt[j + i d] g_j   (column i of the stored Kt, lane l takes j = l, l + 64, .. ascending, then the
//                                         shuffle tree over the lanes: an order fixed by d alone)
// and lane 0 makes the split's update for its row:  t = x_i + lam_i,  u+ = max(0, t) (t itself without the sign constraint),
// lam+ = t - u+,  uml_out = u+ - lam+  (what the next g needs),  and the row's residual terms vs[2 i] = (x_i - u+)^2,
// vs[2 i + 1] = (u+ - u_i)^2.  uml_in and uml_out are two buffers: every workgroup reads all of uml_in for its g while others
// already store their rows.
struct SdpStepArgs {
    int d, nonneg;
    double rho;
    const double *Kt, *x0, *adj, *chat, *uml_in;
    double *x, *u, *lam, *uml_out, *vs;
};

__global__ void __launch_bounds__(1024)
sdp_affine_step_kernel(SdpStepArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sg[];
    const int d = a.d;
    for (int j = threadIdx.x; j < d; j += blockDim.x) sg[j] = (a.uml_in[j] + a.adj[j]) - a.chat[j] / a.rho;
    __syncthreads();
    const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const int i = blockIdx.x * waves + (threadIdx.x >> 6);
    if (i >= d) return;
    const double* __restrict__ col = a.Kt + (int64_t)i * d;
    double acc = 0.0;
    for (int j = lane; j < d; j += 64) acc = fma(col[j], sg[j], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane != 0) return;
    const double x = acc + a.x0[i];
    const double t = x + a.lam[i];
    const double un = (a.nonneg && !(t > 0.0)) ? (t != t ? t : 0.0) : t;
    const double ln = t - un;
    const double ep = x - un, ed = un - a.u[i];
    a.x[i] = x;
    a.u[i] = un;
    a.lam[i] = ln;
    a.uml_out[i] = un - ln;
    a.vs[2 * i] = ep * ep;
    a.vs[2 * i + 1] = ed * ed;
}

// The verdict of a check: out[0] = r_p^2 = sum of the even slots, out[1] = r_d^2 / rho^2 = sum of the odd ones, out[2] = 1.0 when
// either is not finite -- vector slots first, then the block slots, thread t takes slots t, t + 256, .., lanes by shuffle,
// waves left to right.  out: pinned host memory the host reads behind its one wait.
__global__ void __launch_bounds__(SDP_T)
sdp_verdict_kernel(int64_t nv, const double* __restrict__ vs, int64_t nb, const double* __restrict__ bs, double* __restrict__ out) {
    __shared__ double sp[SDP_T / 64], sd[SDP_T / 64];
    double rp = 0.0, rd = 0.0;
    for (int64_t e = threadIdx.x; e < nv; e += SDP_T) {
        rp += vs[2 * e];
        rd += vs[2 * e + 1];
    }
    for (int64_t e = threadIdx.x; e < nb; e += SDP_T) {
        rp += bs[2 * e];
        rd += bs[2 * e + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rp += __shfl_down(rp, o, 64);
        rd += __shfl_down(rd, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sp[threadIdx.x >> 6] = rp;
        sd[threadIdx.x >> 6] = rd;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tp = ((sp[0] + sp[1]) + sp[2]) + sp[3], td = ((sd[0] + sd[1]) + sd[2]) + sd[3];
        out[0] = tp;
        out[1] = td;
        out[2] = (fabs(tp) < INFINITY && fabs(td) < INFINITY) ? 0.0 : 1.0;
        __threadfence_system();
    }
}

// a change of rho: the scaled duals times f = rho_old / rho_new, and what the next iteration reads of them
__global__ void __launch_bounds__(SDP_T)
sdp_rescale_kernel(int64_t d, int64_t n, double f, const double* __restrict__ u, double* __restrict__ lam, double* __restrict__ uml,
                   const double* __restrict__ S, double* __restrict__ Lam, double* __restrict__ D) {
    for (int64_t e = (int64_t)blockIdx.x * SDP_T + threadIdx.x; e < d + n; e += (int64_t)gridDim.x * SDP_T) {
        if (e < d) {
            const double l = lam[e] * f;
            lam[e] = l;
            uml[e] = u[e] - l;
        } else {
            const int64_t p = e - d;
            const double l = Lam[p] * f;
            Lam[p] = l;
            D[p] = S[p] - l;
        }
    }
}

// out[e] = f * in[e]  (Y = rho Lam)
__global__ void __launch_bounds__(SDP_T)
sdp_scaled_copy_kernel(int64_t n, double f, const double* __restrict__ in, double* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * SDP_T + threadIdx.x; e < n; e += (int64_t)gridDim.x * SDP_T) out[e] = f * in[e];
}

inline unsigned sdp_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + SDP_T - 1) / SDP_T, 4096)); }

}  // namespace

void launch_sdp_record_class(hipStream_t s, int64_t n, const void* rec, uint32_t* cls) {
    if (n > 0) sdp_record_class_kernel<<<sdp_grid(n), SDP_T, 0, s>>>(n, (const uint4*)rec, cls);
}

void launch_sdp_gram(hipStream_t s, int64_t d, int64_t n, const void* rec_by_class_pos, int64_t* cptr, double* M) {
    if (d <= 0) return;
    sdp_class_offsets_kernel<<<(unsigned)((d + 1 + SDP_T - 1) / SDP_T), SDP_T, 0, s>>>(n, d, (const uint4*)rec_by_class_pos, (long long*)cptr);
    const unsigned t = (unsigned)((d + 15) / 16);
    sdp_gram_kernel<<<dim3(t, t), SDP_T, 0, s>>>(d, (const uint4*)rec_by_class_pos, (const long long*)cptr, M);
}

void launch_sdp_scale_columns(hipStream_t s, int64_t d, const double* w, double* V) {
    if (d > 0) sdp_scale_columns_kernel<<<sdp_grid(d * d), SDP_T, 0, s>>>(d, w, V);
}

void launch_sdp_gemm(hipStream_t s, int64_t m, int64_t n, int64_t k, const double* A, int64_t ar, int64_t ac, const double* B, int64_t br,
                     int64_t bc, double alpha, double beta, double* C, int64_t ldc) {
    if (m <= 0 || n <= 0) return;
    sdp_gemm_kernel<<<dim3((unsigned)((m + 15) / 16), (unsigned)((n + 15) / 16)), SDP_T, 0, s>>>(m, n, k, A, ar, ac, B, br, bc, alpha, beta, C, ldc);
}

void launch_sdp_affine_step(hipStream_t s, int64_t d, int nonneg, double rho, const double* Kt, const double* x0, const double* adj,
                            const double* chat, const double* uml_in, double* x, double* u, double* lam, double* uml_out, double* vs) {
    if (d <= 0) return;
    const int threads = d > 64 ? 1024 : 256, waves = threads / 64;
    const SdpStepArgs a{(int)d, nonneg, rho, Kt, x0, adj, chat, uml_in, x, u, lam, uml_out, vs};
    sdp_affine_step_kernel<<<(unsigned)((d + waves - 1) / waves), threads, (size_t)d * 8, s>>>(a);
}

void launch_sdp_verdict(hipStream_t s, int64_t d, const double* vs, int64_t nblocks, const double* bs, double* pinned_out) {
    sdp_verdict_kernel<<<1, SDP_T, 0, s>>>(d, vs, nblocks, bs, pinned_out);
}

void launch_sdp_rescale(hipStream_t s, int64_t d, int64_t n, double f, const double* u, double* lam, double* uml, const double* S, double* Lam,
                        double* D) {
    if (d + n > 0) sdp_rescale_kernel<<<sdp_grid(d + n), SDP_T, 0, s>>>(d, n, f, u, lam, uml, S, Lam, D);
}

void launch_sdp_scaled_copy(hipStream_t s, int64_t n, double f, const double* in, double* out) {
    if (n > 0) sdp_scaled_copy_kernel<<<sdp_grid(n), SDP_T, 0, s>>>(n, f, in, out);
}

}  // namespace sdpsr
