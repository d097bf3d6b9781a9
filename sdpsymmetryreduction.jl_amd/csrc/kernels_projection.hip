// Projection onto L for gfx950: the dot products U'x and the projected, rounded, signed element.
//
// Reference semantics restated here:
//   x .-= projL(x)        src/partitions.jl:161, src/utils.jl:62-66
//
// HBM-bound: one pass over the entries each, grid sized to a few blocks per CU with grid-stride loops.
#include "sdpsr_internal.h"
#include "kernel_util.h"
#include "sig_sources.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// projection  y = x - U (U' x)
// ---------------------------------------------------------------------------
// grid = (nblk, r).  partial[k * nblk + b]
__global__ void proj_coef_kernel(int64_t len, const double* __restrict__ U,
                                 const uint32_t* __restrict__ L, uint64_t key,
                                 const double* __restrict__ xin, double* __restrict__ partial) {
    __shared__ double sh[8];
    const int k = blockIdx.y;
    const double* Uk = U + (int64_t)k * len;
    // four independent strided streams per thread: the loads of one round are all in flight
    // before the first FMA (the kernel is bound by memory latency, not by the hash)
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    auto value = [&](int64_t e) -> double {
        if (xin) return xin[e];
        const uint32_t l = L[e];
        return l ? sdpsr_class_uniform(key, l) : 0.0;
    };
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; e + 3 * stride < len; e += 4 * stride) {
        const double u0 = Uk[e], u1 = Uk[e + stride], u2 = Uk[e + 2 * stride], u3 = Uk[e + 3 * stride];
        const double x0 = value(e), x1 = value(e + stride), x2 = value(e + 2 * stride), x3 = value(e + 3 * stride);
        a0 = fma(u0, x0, a0);
        a1 = fma(u1, x1, a1);
        a2 = fma(u2, x2, a2);
        a3 = fma(u3, x3, a3);
    }
    for (; e < len; e += stride) a0 = fma(Uk[e], value(e), a0);
    const double acc = (a0 + a1) + (a2 + a3);
    double r = block_reduce_sum(acc, sh);
    if (threadIdx.x == 0) partial[(int64_t)k * gridDim.x + blockIdx.x] = r;
}

// (declared in kernel_util.h: also the second stage of the column norms, kernels_dense_setup.hip launches it)
__global__ void proj_coef_final_kernel(int nblk, const double* __restrict__ partial,
                                       double* __restrict__ coef) {
    __shared__ double sh[8];
    const int k = blockIdx.x;
    double acc = 0;
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) acc += partial[(int64_t)k * nblk + b];
    double r = block_reduce_sum(acc, sh);
    if (threadIdx.x == 0) coef[k] = r;
}

void launch_proj_coef(hipStream_t s, int64_t len, int64_t r, const double* U, const uint32_t* L,
                      uint64_t key, const double* xin, double* partial, int nblk, double* coef) {
    if (r <= 0) return;
    dim3 g(nblk, (unsigned)r);
    proj_coef_kernel<<<g, 256, 0, s>>>(len, U, L, key, xin, partial);
    proj_coef_final_kernel<<<(unsigned)r, 256, 0, s>>>(nblk, partial, coef);
}

__global__ void proj_apply_kernel(int64_t len, int r, const double* __restrict__ U,
                                  const uint32_t* __restrict__ L, uint64_t key,
                                  const double* __restrict__ xin, const double* __restrict__ coef,
                                  double atol, double scale, int do_round,
                                  double* __restrict__ yout, uint64_t* __restrict__ sig) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
#pragma unroll 4
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        uint32_t l = L ? L[e] : 0u;
        double x;
        if (xin)
            x = xin[e];
        else
            x = l ? sdpsr_class_uniform(key, l) : 0.0;
        double p = 0;
        for (int k = 0; k < r; ++k) p = fma(U[(int64_t)k * len + e], coef[k], p);
        double y = x - p;
        // signature: the injective code of the rounded value (sdpsr_hash.h) -- no division / ldexp; raw bits when not rounding
        const uint64_t kcode = do_round ? sdpsr_round_key(y, atol, scale) : (uint64_t)__double_as_longlong(y);
        if (yout) yout[e] = do_round ? sdpsr_clamp_round(y, atol, scale) : y;
        if (sig) sig[e] = sig_label_key(l, kcode);
    }
}

void launch_proj_apply(hipStream_t s, int64_t len, int64_t r, const double* U, const uint32_t* L,
                       uint64_t key, const double* xin, const double* coef, double atol,
                       double scale, int do_round, double* yout, uint64_t* sig) {
    proj_apply_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, (int)r, U, L, key, xin, coef, atol,
                                                         scale, do_round, yout, sig);
}

// ---------------------------------------------------------------------------
// Projection on the lower triangle.  With symmetric labels (x symmetric) and symmetric basis
// matrices U_k the products U_k'x and the projected element need the entries i >= j only
// (off-diagonal ones count twice in the dot products): half the bytes and half the hashes of the
// projection step; the refinement then runs on the packed lower triangle like the one of the squares.
// ---------------------------------------------------------------------------
// grid = (nblk, r): workgroups stride over the columns, threads over the rows i >= j of a column
// LT: the labels' element type (uint8_t: the loop's 8-bit shadow of packed labels <= 255).  Only the loads differ: every thread adds the same
// entries in the same order whatever the width, so partial and coef are bit for bit the same.
template <typename LT>
__global__ void proj_coef_lower_kernel(int n, const double* __restrict__ U, const LT* __restrict__ L, int lab_packed,
                                       uint64_t key, double* __restrict__ partial) {
    __shared__ double sh[8];
    const int k = blockIdx.y;
    const double* Uk = U + (int64_t)k * n * n;
    double a0 = 0, a1 = 0;
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const double* Uj = Uk + (int64_t)j * n;
        // labels: the full matrix, or its packed lower triangle (column j at offset j n - j (j - 1) / 2, rows j ..)
        const LT* Lj = lab_packed ? L + ((int64_t)j * n - (int64_t)j * (j - 1) / 2 - j) : L + (int64_t)j * n;
        int i = j + threadIdx.x;
        for (; i + (int)blockDim.x < n; i += 2 * blockDim.x) {
            const double u0 = Uj[i], u1 = Uj[i + blockDim.x];
            const uint32_t l0 = (uint32_t)Lj[i], l1 = (uint32_t)Lj[i + blockDim.x];
            const double x0 = l0 ? sdpsr_class_uniform(key, l0) : 0.0, x1 = l1 ? sdpsr_class_uniform(key, l1) : 0.0;
            a0 = fma(i == j ? u0 : 2.0 * u0, x0, a0);
            a1 = fma(2.0 * u1, x1, a1);
        }
        if (i < n) {
            const uint32_t l0 = (uint32_t)Lj[i];
            const double u0 = Uj[i], x0 = l0 ? sdpsr_class_uniform(key, l0) : 0.0;
            a0 = fma(i == j ? u0 : 2.0 * u0, x0, a0);
        }
    }
    const double r = block_reduce_sum(a0 + a1, sh);
    if (threadIdx.x == 0) partial[(int64_t)k * gridDim.x + blockIdx.x] = r;
}
// Lp8 (packed labels only): see sdpsr_internal.h
void launch_proj_coef_lower(hipStream_t s, int64_t n, int64_t r, const double* U, const uint32_t* L, int lab_packed,
                            uint64_t key, double* partial, int nblk, double* coef, const uint8_t* Lp8) {
    if (r <= 0) return;
    dim3 g(nblk, (unsigned)r);
    if (Lp8 && lab_packed) proj_coef_lower_kernel<uint8_t><<<g, 256, 0, s>>>((int)n, U, Lp8, 1, key, partial);
    else proj_coef_lower_kernel<uint32_t><<<g, 256, 0, s>>>((int)n, U, L, lab_packed, key, partial);
    proj_coef_final_kernel<<<(unsigned)r, 256, 0, s>>>(nblk, partial, coef);
}

// Symmetry probe of the basis matrices, riding on the full dot-product pass of the first
// iteration: with W[i,j] = w(i + j n) pseudo-random, <U_k, W - W'> = 0 for a symmetric U_k and a
// random number of size ~|U_k - U_k'| otherwise.  partial rows r .. 2r-1.
__global__ void proj_coef_probe_kernel(int64_t len, int n, const double* __restrict__ U, const uint32_t* __restrict__ L,
                                       uint64_t key, double* __restrict__ partial, int r) {
    __shared__ double sh[8];
    const int k = blockIdx.y;
    const double* Uk = U + (int64_t)k * len;
    double acc = 0, pa = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t wkey = key ^ 0x5DEECE66D1CE4E5BULL;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        const double u = Uk[e];
        const uint32_t l = L[e];
        acc = fma(u, l ? sdpsr_class_uniform(key, l) : 0.0, acc);
        const uint32_t j = (uint32_t)e / (uint32_t)n, i = (uint32_t)e - j * (uint32_t)n;
        const uint64_t et = (uint64_t)j + (uint64_t)i * (uint32_t)n;
        const double w = (double)(sdpsr_fmix64(wkey + (uint64_t)e) >> 11) - (double)(sdpsr_fmix64(wkey + et) >> 11);
        pa = fma(u, w * (1.0 / 9007199254740992.0), pa);
    }
    double t = block_reduce_sum(acc, sh);
    if (threadIdx.x == 0) partial[(int64_t)k * gridDim.x + blockIdx.x] = t;
    __syncthreads();
    t = block_reduce_sum(pa, sh);
    if (threadIdx.x == 0) partial[(int64_t)(r + k) * gridDim.x + blockIdx.x] = t;
}
// coef[0..r) = U'x, coef[r..2r) = the symmetry probes
void launch_proj_coef_probe(hipStream_t s, int64_t len, int64_t n, int64_t r, const double* U, const uint32_t* L, uint64_t key,
                            double* partial, int nblk, double* coef) {
    if (r <= 0) return;
    dim3 g(nblk, (unsigned)r);
    proj_coef_probe_kernel<<<g, 256, 0, s>>>(len, (int)n, U, L, key, partial, (int)r);
    proj_coef_final_kernel<<<(unsigned)(2 * r), 256, 0, s>>>(nblk, partial, coef);
}

}  // namespace sdpsr
