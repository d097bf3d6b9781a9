// The small dense algebra of the set-up stage for gfx950 (setup_dense.cpp, reduce_csr.cpp): the class sums of the columns
// of A, and the vector kernels of the device setup.
#include "sdpsr_internal.h"
#include "kernel_util.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// Reduced-SDP assembly (README.md:57-60, test/sd_problems.jl:32-37): out = A * PMat with
// PMat[e, i] = 1[L[e] == i], i.e. the columns of A (m x n^2, column-major) summed per class.
// One wave per chunk of entries: lanes own the rows of A (m <= 64 per pass), the per-class
// accumulators sit in LDS, entries are walked in order (fixed summation order); chunk partials
// are added in chunk order by the second kernel.  A label beyond d has no accumulator: its entry
// is skipped (counted like label 0) and the flag raised, as fill_f64_kernel does.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
reduce_columns_kernel(int64_t len, int64_t chunk, int m, int d, const uint32_t* __restrict__ L,
                      const double* __restrict__ A, double* __restrict__ partial, uint32_t* __restrict__ bad_flag) {
    extern __shared__ __attribute__((aligned(16))) double s_bins[];  // [(d + 1)][mw]
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * chunk;
    int64_t e1 = e0 + chunk;
    if (e1 > len) e1 = len;
    bool bad = false;
    for (int r0 = 0; r0 < m; r0 += 64) {
        const int mw = (m - r0 < 64) ? m - r0 : 64;
        for (int t = lane; t < (d + 1) * mw; t += 64) s_bins[t] = 0.0;
        __syncthreads();
        for (int64_t eb = e0; eb < e1; eb += 64) {
            uint32_t mylab = (eb + lane < e1) ? L[eb + lane] : 0u;
            if (mylab > (uint32_t)d) {  // never index s_bins past its (d + 1) rows
                bad = true;
                mylab = 0u;
            }
            const int lim = (int)((e1 - eb < 64) ? e1 - eb : 64);
            for (int u = 0; u < lim; ++u) {
                const uint32_t lb = __shfl(mylab, u, 64);
                if (lane < mw) s_bins[lb * mw + lane] += A[(int64_t)(eb + u) * m + r0 + lane];
            }
        }
        __syncthreads();
        for (int t = lane; t < d * mw; t += 64) {
            const int i = t / mw, r = t - i * mw;
            partial[((int64_t)blockIdx.x * d + i) * m + r0 + r] = s_bins[(i + 1) * mw + r];
        }
        __syncthreads();
    }
    if (bad) *bad_flag = 1u;
}
__global__ void reduce_columns_final_kernel(int64_t nchunks, int m, int d, const double* __restrict__ partial,
                                            double* __restrict__ out) {
    const int64_t total = (int64_t)m * d;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t i = t / m, r = t - i * m;
    double acc = 0;
    for (int64_t ch = 0; ch < nchunks; ++ch) acc += partial[(ch * d + i) * m + r];
    out[r + i * m] = acc;  // m x d column-major
}
// per-device kernel attributes, set by sdpsr_create() (see gemm_set_device_attributes)
bool dense_setup_set_device_attributes() {
    bool ok = true;
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&reduce_columns_kernel),
                        hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    return ok;
}

int64_t reduce_columns_chunk(int64_t len, int64_t m, int64_t d) {
    int64_t chunk = 4096;
    while ((len + chunk - 1) / chunk * d * m * 8 > ((int64_t)64 << 20)) chunk *= 2;
    return chunk;
}
bool launch_reduce_columns(hipStream_t s, int64_t len, int64_t m, int64_t d, const uint32_t* L, const double* A,
                           double* partial, double* out, uint32_t* bad_flag) {
    const int mw = (int)(m < 64 ? m : 64);
    const size_t lds = (size_t)(d + 1) * mw * 8;
    if (lds > 60 * 1024) return false;
    const int64_t chunk = reduce_columns_chunk(len, m, d);
    const int64_t nch = (len + chunk - 1) / chunk;
    reduce_columns_kernel<<<(unsigned)nch, 64, lds, s>>>(len, chunk, (int)m, (int)d, L, A, partial, bad_flag);
    reduce_columns_final_kernel<<<(unsigned)((m * d + 255) / 256), 256, 0, s>>>(nch, (int)m, (int)d, partial, out);
    return true;
}

// ---------------------------------------------------------------------------
// small vector kernels of the device setup stage (src/partitions.jl:117-142)
// ---------------------------------------------------------------------------
// R[e + i*len] = A[i + e*m]
__global__ void transpose_rows_kernel(int64_t len, int m, const double* __restrict__ A, double* __restrict__ R) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride)
        for (int i = 0; i < m; ++i) R[e + (int64_t)i * len] = A[i + e * m];
}
void launch_transpose_rows(hipStream_t s, int64_t len, int64_t m, const double* A, double* R) {
    transpose_rows_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, (int)m, A, R);
}
// out[k] = |V[:,k]|^2 ; grid (nblk, k)
__global__ void col_norms2_kernel(int64_t len, const double* __restrict__ V, double* __restrict__ partial) {
    __shared__ double sh[8];
    const double* v = V + (int64_t)blockIdx.y * len;
    double acc = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) acc = fma(v[e], v[e], acc);
    double r = block_reduce_sum(acc, sh);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
}
void launch_col_norms2(hipStream_t s, int64_t len, int64_t k, const double* V, double* partial, int nblk, double* out) {
    if (k <= 0) return;
    dim3 g(nblk, (unsigned)k);
    col_norms2_kernel<<<g, 256, 0, s>>>(len, V, partial);
    proj_coef_final_kernel<<<(unsigned)k, 256, 0, s>>>(nblk, partial, out);
}
__global__ void scale_copy_kernel(int64_t len, const double* __restrict__ v, double alpha, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) out[e] = v[e] * alpha;
}
void launch_scale_copy(hipStream_t s, int64_t len, const double* v, double alpha, double* out) {
    scale_copy_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, v, alpha, out);
}
// R[:, i] -= dots[i] * u   for every i (dots[i] = 0 leaves the row alone)
__global__ void rank1_update_kernel(int64_t len, int m, double* __restrict__ R, const double* __restrict__ u,
                                    const double* __restrict__ dots) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        const double ue = u[e];
        for (int i = 0; i < m; ++i) {
            const double dd = dots[i];
            if (dd != 0.0) R[e + (int64_t)i * len] = fma(-dd, ue, R[e + (int64_t)i * len]);
        }
    }
}
void launch_rank1_update(hipStream_t s, int64_t len, int64_t m, double* R, const double* u, const double* dots) {
    rank1_update_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, (int)m, R, u, dots);
}
// out = clamp_round(a - b)
__global__ void sub_round_kernel(int64_t len, const double* __restrict__ a, const double* __restrict__ b, double atol,
                                 double scale, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride)
        out[e] = sdpsr_clamp_round(a[e] - b[e], atol, scale);
}
void launch_sub_round(hipStream_t s, int64_t len, const double* a, const double* b, double atol, double scale, double* out) {
    sub_round_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, a, b, atol, scale, out);
}

}  // namespace sdpsr
