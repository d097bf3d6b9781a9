// Label utilities for gfx950: the largest pair code, the checksum of a label array, the symmetry checks (alone, or folded
// into a copy), and the unpack / transpose of label matrices.  One pass over the labels each.
#include "sdpsr_internal.h"
#include "kernel_util.h"
#include "sym_tile_pass.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// largest pair code l1 + l2 (d1 + 1) of refine!(P1, P2) (src/partitions.jl:63): what the reference
// stores into its label type T before renumbering -- InexactError when it exceeds typemax(T)
// (sdpsr_opts.label_bits).  out[0] must be zero.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
max_pair_code_kernel(int64_t len, const uint32_t* __restrict__ p1, const uint32_t* __restrict__ p2, unsigned long long d1p1,
                     unsigned long long* __restrict__ out) {
    unsigned long long m = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        const unsigned long long v = (unsigned long long)p1[e] + (unsigned long long)p2[e] * d1p1;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_down(m, o, 64);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
void launch_max_pair_code(hipStream_t s, int64_t len, const uint32_t* p1, const uint32_t* p2, uint64_t d1, uint64_t* out) {
    max_pair_code_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, p1, p2, (unsigned long long)d1 + 1ull, (unsigned long long*)out);
}

// ---------------------------------------------------------------------------
// checksum of a label array: two position-weighted sums mod 2^64 (order of summation irrelevant)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
labels_checksum_kernel(int64_t len, const uint32_t* __restrict__ L, unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long sh[2][4];
    unsigned long long h1 = 0, h2 = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        const unsigned long long l = (unsigned long long)L[e] + 1ull;
        const unsigned long long ee = (unsigned long long)e;
        h1 += l * (ee * 0x9E3779B97F4A7C15ull + 0xD1342543DE82EF95ull);
        h2 += (l * l + 0x27D4EB2F165667C5ull) * ((ee ^ (ee >> 13)) * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        h1 += __shfl_down(h1, o, 64);
        h2 += __shfl_down(h2, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        sh[0][w] = h1;
        sh[1][w] = h2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        partial[gridDim.x + blockIdx.x] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    }
}
__global__ void __launch_bounds__(256)
labels_checksum_final_kernel(int nblk, const unsigned long long* __restrict__ partial, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sh[4];
    for (int which = 0; which < 2; ++which) {
        unsigned long long h = 0;
        for (int b = threadIdx.x; b < nblk; b += 256) h += partial[which * nblk + b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) h += __shfl_down(h, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = h;
        __syncthreads();
        if (threadIdx.x == 0) out[which] = sh[0] + sh[1] + sh[2] + sh[3];
        __syncthreads();
    }
}
// partial: 2 * 2048 words of scratch, out: 2 words (device)
void launch_labels_checksum(hipStream_t s, int64_t len, const uint32_t* L, uint64_t* partial, uint64_t* out) {
    const int nblk = grid_for(len, 256);
    labels_checksum_kernel<<<nblk, 256, 0, s>>>(len, L, (unsigned long long*)partial);
    labels_checksum_final_kernel<<<1, 256, 0, s>>>(nblk, (const unsigned long long*)partial, (unsigned long long*)out);
}

// ---------------------------------------------------------------------------
// symmetric label check
// ---------------------------------------------------------------------------
// 64 x 64 tiles through LDS: both the tile and its mirror image are read along columns
__global__ void __launch_bounds__(256)
check_symmetric_kernel(int64_t n, const uint32_t* __restrict__ L, uint32_t* flag) {
    __shared__ uint32_t tile[64][65];
    const int64_t i0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;
    if (i0 < j0) return;  // lower triangle of tiles only
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
    for (int c = ty; c < 64; c += 4) {  // mirror tile: rows j0.., columns i0..
        const int64_t r = j0 + tx, cc = i0 + c;
        tile[c][tx] = (r < n && cc < n) ? L[r + cc * n] : 0u;
    }
    __syncthreads();
    bool bad = false;
    for (int c = ty; c < 64; c += 4) {  // tile: rows i0.., columns j0..
        const int64_t r = i0 + tx, cc = j0 + c;
        if (r < n && cc < n && L[r + cc * n] != tile[tx][c]) bad = true;  // L[r,cc] vs L[cc,r]
    }
    if (bad) flag[0] = 1u;
}
// dst = src (n x n labels) with the symmetry check of the same tiles: one pass instead of a copy
// and a check.  flag[0] = epoch if NOT symmetric (no zeroing pass: the host compares with the
// epoch of this call).
template <bool VEC4>
__global__ void __launch_bounds__(256)
copy_check_symmetric_kernel(int64_t n, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t* flag,
                            uint32_t epoch) {
    __shared__ uint32_t tile[64][65];
    if (blockIdx.x < blockIdx.y) return;
    if (sym_tile_pass<VEC4>(n, src, dst, MapIdentity{}, tile)) flag[0] = epoch;
}
void launch_copy_check_symmetric(hipStream_t s, int64_t n, const uint32_t* src, uint32_t* dst, uint32_t* flag, uint32_t epoch) {
    const unsigned t = (unsigned)((n + 63) / 64);
    const bool v4 = n % 4 == 0 && (reinterpret_cast<uintptr_t>(src) % 16) == 0 && (reinterpret_cast<uintptr_t>(dst) % 16) == 0;
    if (v4) copy_check_symmetric_kernel<true><<<dim3(t, t), 256, 0, s>>>(n, src, dst, flag, epoch);
    else copy_check_symmetric_kernel<false><<<dim3(t, t), 256, 0, s>>>(n, src, dst, flag, epoch);
}
// The same pass for a caller's labels of unknown quality (sdpsr_basis_image): symmetry, and "a label exceeds dmax" from the
// words that pass through the registers anyway (MapNoteExceeds).  src == dst (labels already in place) is allowed: the values
// written are the values read.  Plain stores of 1 into words the caller cleared.
template <bool VEC4>
__global__ void __launch_bounds__(256)
copy_check_labels_kernel(int64_t n, const uint32_t* src, uint32_t* dst, uint32_t dmax, uint32_t* flag) {
    __shared__ uint32_t tile[64][65];
    if (blockIdx.x < blockIdx.y) return;
    bool over = false;
    if (sym_tile_pass<VEC4>(n, src, dst, MapNoteExceeds{dmax, &over}, tile)) flag[0] = 1u;
    if (over) flag[1] = 1u;
}
void launch_copy_check_labels(hipStream_t s, int64_t n, const uint32_t* src, uint32_t* dst, uint32_t dmax, uint32_t* flag) {
    const unsigned t = (unsigned)((n + 63) / 64);
    const bool v4 = n % 4 == 0 && (reinterpret_cast<uintptr_t>(src) % 16) == 0 && (reinterpret_cast<uintptr_t>(dst) % 16) == 0;
    if (v4) copy_check_labels_kernel<true><<<dim3(t, t), 256, 0, s>>>(n, src, dst, dmax, flag);
    else copy_check_labels_kernel<false><<<dim3(t, t), 256, 0, s>>>(n, src, dst, dmax, flag);
}
void launch_check_symmetric(hipStream_t s, int64_t n, const uint32_t* L, uint32_t* flag) {
    hipMemsetAsync(flag, 0, sizeof(uint32_t), s);
    const unsigned t = (unsigned)((n + 63) / 64);
    check_symmetric_kernel<<<dim3(t, t), 256, 0, s>>>(n, L, flag);
}

// Full symmetric label matrix from the packed lower triangle (column j at offset
// j n - j (j - 1) / 2, rows j .. n-1): both triangles are written along columns, the mirrored
// one through a 64 x 64 LDS tile.
__global__ void __launch_bounds__(256)
unpack_symmetric_labels_kernel(int64_t n, const uint32_t* __restrict__ Lp, uint32_t* __restrict__ L) {
    __shared__ uint32_t tile[64][65];
    const int64_t i0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;  // lower tile: rows i0.., cols j0..
    if (i0 < j0) return;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c = ty; c < 64; c += 4) {
        const int64_t r = i0 + tx, cc = j0 + c;
        uint32_t v = 0u;
        if (r < n && cc < n && r >= cc) {
            v = Lp[cc * n - cc * (cc - 1) / 2 + (r - cc)];
            L[r + cc * n] = v;
        }
        tile[c][tx] = v;
    }
    __syncthreads();
    for (int c = ty; c < 64; c += 4) {  // destination: row j0 + tx, column i0 + c  (= entry (i0 + c, j0 + tx))
        const int64_t r = j0 + tx, cc = i0 + c;
        if (r < n && cc < n && r < cc) L[r + cc * n] = tile[tx][c];
    }
}
void launch_unpack_symmetric_labels(hipStream_t s, int64_t n, const uint32_t* Lp, uint32_t* L) {
    const unsigned t = (unsigned)((n + 63) / 64);
    unpack_symmetric_labels_kernel<<<dim3(t, t), 256, 0, s>>>(n, Lp, L);
}

// Lt[k + i*n] = L[i + k*n]: 64 x 64 label tiles through LDS (both sides coalesced)
__global__ void __launch_bounds__(256)
transpose_labels_kernel(int n, const uint32_t* __restrict__ L, uint32_t* __restrict__ Lt) {
    __shared__ uint32_t tile[64][65];
    const int bi = blockIdx.x * 64, bk = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 4 rows of the tile per pass
    for (int q = ty; q < 64; q += 4) {
        const int i = bi + tx, kk = bk + q;
        tile[q][tx] = (i < n && kk < n) ? L[i + (int64_t)kk * n] : 0u;
    }
    __syncthreads();
    for (int q = ty; q < 64; q += 4) {
        const int kk = bk + tx, i = bi + q;
        if (kk < n && i < n) Lt[kk + (int64_t)i * n] = tile[tx][q];
    }
}
void launch_transpose_labels(hipStream_t s, int64_t n, const uint32_t* L, uint32_t* Lt) {
    dim3 g((unsigned)((n + 63) / 64), (unsigned)((n + 63) / 64));
    transpose_labels_kernel<<<g, 256, 0, s>>>((int)n, L, Lt);
}

}  // namespace sdpsr
