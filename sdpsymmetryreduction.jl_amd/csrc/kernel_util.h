// Small helpers shared by the kernel translation units: grid sizing, the workgroup sum, the inversion of the packed
// lower-triangle numbering, and the dispatch of a run-time integer to a compile-time one.  Device code and launch
// arithmetic only; everything has internal linkage or is inline, so every translation unit carries its own copy.
#pragma once
#include <type_traits>
#include "sdpsr_internal.h"

namespace sdpsr {

static inline int grid_for(int64_t work_items, int block, int max_blocks = 256 * 8) {
    int64_t g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

static inline dim3 column_grid(int64_t n) {
    int64_t gx = (n + 1023) / 1024;  // ~4 rows per thread
    if (gx < 1) gx = 1;
    if (gx > 64) gx = 64;
    // one round of resident workgroups (8 per CU): the kernel strides over the columns
    int64_t gy = (256 * 8) / gx;
    if (gy < 1) gy = 1;
    if (gy > n) gy = n;
    return dim3((unsigned)gx, (unsigned)gy);
}

// f(std::integral_constant<int, v>) for the v of the list that equals x; false when none does
template <int... Vs, class F>
static bool with_constant(int x, F&& f) {
    return ((x == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

__device__ __forceinline__ double block_reduce_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
    return r;  // valid in thread 0
}

// coef[k] = the sum of the nblk partials of row k, one workgroup per row: the second stage of the block_reduce_sum passes.
// Defined in kernels_projection.hip; the column norms of kernels_dense_setup.hip launch it too (a launch from another
// translation unit calls the kernel's host stub, so this one declaration serves both files).
__global__ void proj_coef_final_kernel(int nblk, const double* __restrict__ partial, double* __restrict__ coef);

// (i, j), i >= j, of packed index e: column j starts at off(j) = j n - j (j - 1) / 2
__device__ __forceinline__ void packed_lower_ij(int n, int64_t e, uint32_t& i, uint32_t& j) {
    const float t = (float)(2 * n + 1);
    int jj = (int)((t - sqrtf(fmaxf(t * t - 8.0f * (float)e, 0.0f))) * 0.5f);
    jj = jj < 0 ? 0 : (jj > n - 1 ? n - 1 : jj);
    while ((int64_t)jj * n - (int64_t)jj * (jj - 1) / 2 > e) --jj;
    while (jj + 1 < n && (int64_t)(jj + 1) * n - (int64_t)(jj + 1) * jj / 2 <= e) ++jj;
    j = (uint32_t)jj;
    i = j + (uint32_t)(e - ((int64_t)jj * n - (int64_t)jj * (jj - 1) / 2));
}

}  // namespace sdpsr
