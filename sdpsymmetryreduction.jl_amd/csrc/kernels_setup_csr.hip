// Kernels of the setup stage from a sparse (CSR) constraint matrix (setup_csr.cpp, src/partitions.jl:117-142):
// the densification of A's rows into the columns of one len x m work buffer W, the tall-skinny Gram W'W for any m,
// and the in-place right multiplication W <- W[:, piv] X by an upper-triangular X (CholeskyQR2).
// Every kernel does the same arithmetic for every row e of W (nothing depends on e's position): rows e and e' of W
// that hold the same bits give rows of the result that hold the same bits, which is what makes the basis of a
// symmetric A bitwise symmetric (the hint bits of sdpsr_admissible_setup_csr).
#include <algorithm>
#include "sdpsr_internal.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// W[:, i] = row i of A (dense, len entries).  Workgroup = DZ_CHUNK consecutive entries of one column: the chunk is
// zeroed, then the row's entries that fall into it (found by two binary searches over the sorted column indices)
// are written; the barrier between the two orders the stores of the workgroup.
// ---------------------------------------------------------------------------
constexpr int DZ_THREADS = 256;
constexpr int DZ_CHUNK = 4096;

__device__ inline int64_t lower_bound_u32(const uint32_t* __restrict__ a, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(DZ_THREADS)
csr_densify_kernel(int64_t len, int64_t m, const int64_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                   const double* __restrict__ val, double* __restrict__ W) {
    __shared__ int64_t range[2];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * DZ_CHUNK;
    const int64_t c1 = c0 + DZ_CHUNK < len ? c0 + DZ_CHUNK : len;
    for (int64_t i = blockIdx.y; i < m; i += gridDim.y) {
        double* w = W + (size_t)i * len;
        for (int64_t e = c0 + tid; e < c1; e += DZ_THREADS) w[e] = 0.0;
        if (tid < 2) range[tid] = lower_bound_u32(col, rowptr[i], rowptr[i + 1], (uint64_t)(tid == 0 ? c0 : c1));
        __syncthreads();
        const int64_t lo = range[0], hi = range[1];
        for (int64_t p = lo + tid; p < hi; p += DZ_THREADS) w[col[p]] = val[p];
        __syncthreads();  // (range[] is rewritten for the next column)
    }
}

void launch_csr_densify(hipStream_t s, int64_t len, int64_t m, const int64_t* rowptr, const uint32_t* col, const double* val, double* W) {
    if (m <= 0) return;
    dim3 g((unsigned)((len + DZ_CHUNK - 1) / DZ_CHUNK), (unsigned)std::min<int64_t>(m, 65535));
    csr_densify_kernel<<<g, DZ_THREADS, 0, s>>>(len, m, rowptr, col, val, W);
}

// ---------------------------------------------------------------------------
// G = W'W for any m.  The m x m result is cut into 64 x 64 tiles; only the tiles (I, J) with I <= J are computed.
// Workgroup = one tile pair x one chunk of rows: GT_ROWS rows of both column blocks go through LDS (transposed,
// pitch 65), every thread accumulates a 4 x 4 register tile with FMA.  The partial tiles of the chunks are added in
// chunk order by gram_tall_reduce_kernel, which writes the full symmetric matrix (the lower triangle read from the
// same sums) straight into pinned host memory: the host reads it after its next wait.  The chunking depends on
// (len, m) only, so the result is the same bits on every run.
// ---------------------------------------------------------------------------
constexpr int GT_TILE = 64;
constexpr int GT_ROWS = 32;
constexpr int GT_PITCH = GT_TILE + 1;
constexpr int GT_TARGET_WGS = 2048;

struct GramTallShape {
    int64_t nt, npairs, Z, rows_per_chunk;
};
static GramTallShape gram_tall_shape(int64_t len, int64_t m) {
    GramTallShape g;
    g.nt = (m + GT_TILE - 1) / GT_TILE;
    g.npairs = g.nt * (g.nt + 1) / 2;
    const int64_t row_blocks = (len + GT_ROWS - 1) / GT_ROWS;
    int64_t Z = std::max<int64_t>(1, std::min<int64_t>(row_blocks, GT_TARGET_WGS / std::max<int64_t>(g.npairs, 1)));
    const int64_t blocks_per_chunk = (row_blocks + Z - 1) / Z;
    g.rows_per_chunk = blocks_per_chunk * GT_ROWS;
    g.Z = (len + g.rows_per_chunk - 1) / g.rows_per_chunk;
    return g;
}
size_t gram_tall_partial_doubles(int64_t len, int64_t m) {
    const GramTallShape g = gram_tall_shape(len, m);
    return (size_t)g.Z * g.npairs * GT_TILE * GT_TILE;
}

__device__ inline void gram_pair(int64_t p, int64_t nt, int64_t* I, int64_t* J) {
    int64_t i = 0;
    while (p >= nt - i) {
        p -= nt - i;
        ++i;
    }
    *I = i;
    *J = i + p;
}

__global__ void __launch_bounds__(256)
gram_tall_partial_kernel(int64_t len, int64_t m, const double* __restrict__ W, int64_t nt, int64_t npairs, int64_t rows_per_chunk,
                         double* __restrict__ P) {
    __shared__ double sA[GT_ROWS * GT_PITCH];
    __shared__ double sB[GT_ROWS * GT_PITCH];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x % npairs, z = blockIdx.x / npairs;
    int64_t I, J;
    gram_pair(pair, nt, &I, &J);
    const int64_t i0 = I * GT_TILE, j0 = J * GT_TILE;
    const int64_t ca = std::min<int64_t>(GT_TILE, m - i0), cb = std::min<int64_t>(GT_TILE, m - j0);
    const int64_t r_begin = z * rows_per_chunk;
    const int64_t r_end = std::min<int64_t>(len, r_begin + rows_per_chunk);
    const int ti = tid & 15, tj = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += GT_ROWS) {
        // 32 rows x 64 columns of each block: 8 elements per thread and block, 32 consecutive rows of a column per
        // half wave (coalesced); columns past m and rows past the chunk are zero
        double va[8], vb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q;
            const int r = e & (GT_ROWS - 1), cidx = e >> 5;
            const int64_t row = r0 + r;
            const bool rok = row < r_end;
            va[q] = (rok && cidx < ca) ? W[row + (size_t)(i0 + cidx) * len] : 0.0;
            vb[q] = (rok && cidx < cb) ? W[row + (size_t)(j0 + cidx) * len] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q;
            const int r = e & (GT_ROWS - 1), cidx = e >> 5;
            sA[r * GT_PITCH + cidx] = va[q];
            sB[r * GT_PITCH + cidx] = vb[q];
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < GT_ROWS; ++r) {
            double xa[4], yb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) xa[a] = sA[r * GT_PITCH + ti + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) yb[b] = sB[r * GT_PITCH + tj + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(xa[a], yb[b], acc[a][b]);
        }
        __syncthreads();
    }
    double* out = P + ((size_t)z * npairs + pair) * (GT_TILE * GT_TILE);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) out[(ti + 16 * a) + (tj + 16 * b) * GT_TILE] = acc[a][b];
}

// host_G[i + j m] = sum_z P[z][pair(I, J)][li + lj 64] in chunk order; (i, j) below the diagonal reads the sums of (j, i)
__global__ void __launch_bounds__(256)
gram_tall_reduce_kernel(int64_t m, int64_t nt, int64_t npairs, int64_t Z, const double* __restrict__ P, double* __restrict__ host_G) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m * m) return;
    const int64_t j = e / m, i = e - j * m;
    const int64_t a = i <= j ? i : j, b = i <= j ? j : i;  // upper-triangle position
    const int64_t I = a / GT_TILE, J = b / GT_TILE;
    const int64_t pair = I * nt - I * (I - 1) / 2 + (J - I);
    int64_t li = a - I * GT_TILE, lj = b - J * GT_TILE;
    const double* p = P + (size_t)pair * (GT_TILE * GT_TILE) + li + lj * GT_TILE;
    const size_t stride = (size_t)npairs * GT_TILE * GT_TILE;
    double acc = 0.0;
    for (int64_t z = 0; z < Z; ++z) acc += p[z * stride];
    host_G[e] = acc;
}

void launch_gram_tall(hipStream_t s, int64_t len, int64_t m, const double* W, double* partials, double* host_G) {
    if (m <= 0) return;
    const GramTallShape g = gram_tall_shape(len, m);
    gram_tall_partial_kernel<<<(unsigned)(g.Z * g.npairs), 256, 0, s>>>(len, m, W, g.nt, g.npairs, g.rows_per_chunk, partials);
    gram_tall_reduce_kernel<<<(unsigned)((m * m + 255) / 256), 256, 0, s>>>(m, g.nt, g.npairs, g.Z, partials, host_G);
}

// ---------------------------------------------------------------------------
// W <- W[:, piv] X in place, X upper triangular (m x m, given ROW-major: Xrow[k m + j] = X[k][j]); column j of the
// result is stored in slot piv[j].  Row-local: thread = one row e of W.  Output columns go in blocks of AU_COLS from
// the last block down: block [j0, j1) reads the old slots piv[0 .. j1) only, and the slots written so far are piv[j1
// ..), so no second len x m buffer is needed.  X's entries are wave-uniform (scalar loads).
// ---------------------------------------------------------------------------
constexpr int AU_COLS = 32;

__global__ void __launch_bounds__(256)
apply_upper_inverse_kernel(int64_t len, int64_t m, double* __restrict__ W, const int32_t* __restrict__ piv,
                           const double* __restrict__ Xrow) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= len) return;
    const int64_t nb = (m + AU_COLS - 1) / AU_COLS;
    for (int64_t bj = nb - 1; bj >= 0; --bj) {
        const int64_t j0 = bj * AU_COLS;
        const int64_t j1 = std::min<int64_t>(m, j0 + AU_COLS);
        const int w = (int)(j1 - j0);
        double acc[AU_COLS];
#pragma unroll
        for (int q = 0; q < AU_COLS; ++q) acc[q] = 0.0;
        if (w == AU_COLS) {
            for (int64_t k = 0; k < j1; ++k) {
                const double x = W[e + (size_t)piv[k] * len];
                const double* xr = Xrow + k * m + j0;
#pragma unroll
                for (int q = 0; q < AU_COLS; ++q) acc[q] = fma(x, xr[q], acc[q]);
            }
        } else {
            for (int64_t k = 0; k < j1; ++k) {
                const double x = W[e + (size_t)piv[k] * len];
                const double* xr = Xrow + k * m + j0;
#pragma unroll
                for (int q = 0; q < AU_COLS; ++q)
                    if (q < w) acc[q] = fma(x, xr[q], acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < AU_COLS; ++q)
            if (q < w) W[e + (size_t)piv[j0 + q] * len] = acc[q];
    }
}

void launch_apply_upper_inverse(hipStream_t s, int64_t len, int64_t m, double* W, const int32_t* piv, const double* Xrow) {
    if (m <= 0) return;
    apply_upper_inverse_kernel<<<(unsigned)((len + 255) / 256), 256, 0, s>>>(len, m, W, piv, Xrow);
}

}  // namespace sdpsr
