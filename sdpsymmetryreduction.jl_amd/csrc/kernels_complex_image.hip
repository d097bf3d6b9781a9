// basis_image over C for a caller's Q_hat and a window of classes (sdpsr_basis_image_complex; src/diagonalize.jl:64-89 with
// T = ComplexF64, called by src/compat.jl:54-57 with the desymmetrized partition):
//   blks[i][k][a,b] = sum over the entries (r,c) of class i of conj(Q_k[r,a]) * Q_k[c,b]
// Complex forms of the two entry-based routes of the real path (kernels_blockdiag.hip: basis_image_kernel +
// basis_image_reduce_kernel, basis_image_outer_kernel), over the same grouped entries (sort_entries_by_label), the same chunk
// cutting and the same descriptors.  Neither route assumes a symmetric partition.  Q_hat is re-laid once per call into
// row-major interleaved form (one 16-byte (re, im) per element), so the values of one row a workgroup needs are contiguous.
// No atomics, every sum in a fixed order: equal inputs give equal bits, and a class's sum depends on that class alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sdpsr_internal.h"
#include "kernel_util.h"

namespace sdpsr {

// acc += conj(x) * y: four real FMAs
__device__ __forceinline__ void cfma_conj(double2& acc, const double2 x, const double2 y) {
    acc.x = fma(x.x, y.x, acc.x);
    acc.x = fma(x.y, y.y, acc.x);
    acc.y = fma(x.x, y.y, acc.y);
    acc.y = fma(-x.y, y.x, acc.y);
}
// clamptol over C (src/utils.jl:14-16): by magnitude, strict <
__device__ __forceinline__ double2 clamp_magnitude(double2 v, double atol) {
    return (sqrt(v.x * v.x + v.y * v.y) < atol) ? make_double2(0.0, 0.0) : v;
}

// ---------------------------------------------------------------------------
// Q_hat (n x S1 complex, column-major, (re, im) pairs) -> row-major: 32 x 32 tiles through LDS, reads along columns,
// writes along rows
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cx_rowmajor_kernel(int64_t n, int64_t S1, const double* __restrict__ Qcm, double2* __restrict__ Qrm) {  // Qcm: the caller's, 8-byte aligned
    __shared__ double2 tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int64_t r0 = (int64_t)blockIdx.x * 32, j0 = (int64_t)blockIdx.y * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = r0 + tx, j = j0 + ty + 8 * q;
        if (r < n && j < S1) tile[ty + 8 * q][tx] = make_double2(Qcm[2 * (r + j * n)], Qcm[2 * (r + j * n) + 1]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = r0 + ty + 8 * q, j = j0 + tx;
        if (r < n && j < S1) Qrm[r * S1 + j] = tile[tx][ty + 8 * q];
    }
}
void launch_cx_rowmajor(hipStream_t s, int64_t n, int64_t S1, const double* Qcm, double* Qrm) {
    dim3 g((unsigned)((n + 31) / 32), (unsigned)((S1 + 31) / 32));  // S1 <= n < 65536: both within the grid limits
    cx_rowmajor_kernel<<<g, 256, 0, s>>>(n, S1, Qcm, reinterpret_cast<double2*>(Qrm));
}

// ---------------------------------------------------------------------------
// `chunk`: a workgroup = (chunk of at most 4096 entries of one class, tile of CI_OT outputs); threads walk the entries with
// CI_OT complex accumulators in registers, then wave and workgroup reduction.  The second kernel sums a class's partials in
// chunk order, clamps by magnitude and writes the (re, im) pairs.  A class of any size is spread over its chunks' workgroups.
// ---------------------------------------------------------------------------
constexpr int CI_THREADS = 256;
constexpr int CI_OT = 8;  // complex outputs per tile: 16 doubles of accumulators, as the real kernel's BI_OT = 16

__global__ void __launch_bounds__(CI_THREADS)
cx_image_chunk_kernel(uint32_t n, int64_t S1, int64_t S, const double2* __restrict__ Qrm, const uint32_t* __restrict__ ent,
                      const int64_t* __restrict__ chunk_begin, const int64_t* __restrict__ chunk_end,
                      const int32_t* __restrict__ descA, const int32_t* __restrict__ descB, double2* __restrict__ partial) {
    __shared__ int sA[CI_OT], sB[CI_OT];
    __shared__ double2 red[CI_THREADS / 64][CI_OT];
    const int64_t chunk = blockIdx.x;
    const int64_t b = chunk_begin[chunk], e_end = chunk_end[chunk];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tiles = (S + CI_OT - 1) / CI_OT;
    for (int64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {  // (one round unless S > 65535 * CI_OT)
        const int64_t o0 = tile * CI_OT;
        __syncthreads();  // the previous tile's sA / sB / red have been read
        if (threadIdx.x < CI_OT) {
            const int64_t o = o0 + threadIdx.x;
            sA[threadIdx.x] = (o < S) ? descA[o] : 0;
            sB[threadIdx.x] = (o < S) ? descB[o] : 0;
        }
        __syncthreads();
        double2 acc[CI_OT];
#pragma unroll
        for (int o = 0; o < CI_OT; ++o) acc[o] = make_double2(0.0, 0.0);
        for (int64_t p = b + threadIdx.x; p < e_end; p += CI_THREADS) {
            const uint32_t lin = ent[p];
            const uint32_t c = lin / n, r = lin - c * n;
            const double2* qr = Qrm + (int64_t)r * S1;
            const double2* qc = Qrm + (int64_t)c * S1;
#pragma unroll
            for (int o = 0; o < CI_OT; ++o) cfma_conj(acc[o], qr[sA[o]], qc[sB[o]]);
        }
#pragma unroll
        for (int o = 0; o < CI_OT; ++o) {
            double vr = acc[o].x, vi = acc[o].y;
#pragma unroll
            for (int sft = 32; sft > 0; sft >>= 1) {
                vr += __shfl_down(vr, sft, 64);
                vi += __shfl_down(vi, sft, 64);
            }
            if (lane == 0) red[w][o] = make_double2(vr, vi);
        }
        __syncthreads();
        if (threadIdx.x < CI_OT) {
            const int64_t o = o0 + threadIdx.x;
            if (o < S) {
                double2 v = make_double2(0.0, 0.0);
                for (int k = 0; k < CI_THREADS / 64; ++k) v.x += red[k][threadIdx.x].x, v.y += red[k][threadIdx.x].y;
                partial[chunk * S + o] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
cx_image_reduce_kernel(int64_t d, int64_t S, const int64_t* __restrict__ chunk_ptr, const double2* __restrict__ partial,
                       double atol, double* __restrict__ out) {  // out: the caller's, 8-byte aligned
    const int64_t total = d * S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t cls = t / S, o = t - cls * S;
        double2 v = make_double2(0.0, 0.0);
        for (int64_t ch = chunk_ptr[cls]; ch < chunk_ptr[cls + 1]; ++ch) {
            const double2 p = partial[ch * S + o];
            v.x += p.x;
            v.y += p.y;
        }
        v = clamp_magnitude(v, atol);
        out[2 * t] = v.x;
        out[2 * t + 1] = v.y;
    }
}

// out: d * S complex (the window's classes); partial: nchunks * S complex
void launch_cx_image_chunk(hipStream_t s, int64_t n, int64_t d, int64_t S1, int64_t S, const double* Qrm, const uint32_t* ent,
                           const int32_t* descA, const int32_t* descB, const int64_t* chunk_ptr, int64_t nchunks,
                           const int64_t* chunk_begin, const int64_t* chunk_end, double* partial, double* out, double atol) {
    if (d < 1 || S < 1) return;
    if (nchunks > 0) {
        const int64_t tiles = (S + CI_OT - 1) / CI_OT;
        dim3 g((unsigned)nchunks, (unsigned)(tiles < 65535 ? tiles : 65535));
        cx_image_chunk_kernel<<<g, CI_THREADS, 0, s>>>((uint32_t)n, S1, S, reinterpret_cast<const double2*>(Qrm), ent, chunk_begin,
                                                       chunk_end, descA, descB, reinterpret_cast<double2*>(partial));
    }
    cx_image_reduce_kernel<<<grid_for(d * S, 256), 256, 0, s>>>(d, S, chunk_ptr, reinterpret_cast<const double2*>(partial), atol,
                                                                out);
}

// ---------------------------------------------------------------------------
// `outer`: one workgroup per (class i, block k).  The two row segments of a batch of CO_EB entries are staged in LDS, a
// thread owns one row index a of the s_k x s_k output and every G-th column b (CO_MAXACC complex accumulators per pass), one
// 16-byte LDS read per complex FMA; every output is written exactly once, with the clamp on the write.  Blocks up to
// CO_MAX_BLOCK (2 * CO_EB * s * 16 bytes of LDS: 32 KiB at 128).
// ---------------------------------------------------------------------------
constexpr int CO_THREADS = 256;
constexpr int CO_EB = 8;
constexpr int CO_MAXACC = 16;
constexpr int CO_MAX_BLOCK = 128;

__global__ void __launch_bounds__(CO_THREADS)
cx_image_outer_kernel(uint32_t n, int64_t S1, int64_t S, const double2* __restrict__ Qrm, const uint32_t* __restrict__ ent,
                      const int64_t* __restrict__ cls_ptr, const int32_t* __restrict__ blk_col,
                      const int32_t* __restrict__ blk_size, const int64_t* __restrict__ blk_off, double atol,
                      double* __restrict__ out) {  // out: the caller's, 8-byte aligned
    extern __shared__ __attribute__((aligned(16))) double2 co_smem[];  // qr[EB][s], qc[EB][s]
    const int i = blockIdx.x, k = blockIdx.y;
    const int s = blk_size[k], cb = blk_col[k];
    const int64_t p_begin = cls_ptr[i + 1], p_end = cls_ptr[i + 2];  // window-relative label i + 1
    double2* qr = co_smem;
    double2* qc = co_smem + CO_EB * s;
    const int G = CO_THREADS / s;  // >= 2 (s <= 128)
    const int tid = threadIdx.x;
    const bool active = tid < G * s;
    const int a = active ? tid % s : 0, g = active ? tid / s : 0;
    double* o = out + 2 * ((int64_t)i * S + blk_off[k]);
    for (int b0 = 0; b0 < s; b0 += G * CO_MAXACC) {  // passes over the columns b (one pass if s <= G * 16, i.e. s <= 64)
        double2 acc[CO_MAXACC];
#pragma unroll
        for (int j = 0; j < CO_MAXACC; ++j) acc[j] = make_double2(0.0, 0.0);
        for (int64_t p0 = p_begin; p0 < p_end; p0 += CO_EB) {
            const int ne = (int)((p_end - p0 < CO_EB) ? (p_end - p0) : CO_EB);
            __syncthreads();
            for (int t = tid; t < ne * s; t += CO_THREADS) {
                const int e = t / s, j = t - e * s;
                const uint32_t lin = ent[p0 + e];
                const uint32_t c = lin / n, r = lin - c * n;
                qr[e * s + j] = Qrm[(int64_t)r * S1 + cb + j];
                qc[e * s + j] = Qrm[(int64_t)c * S1 + cb + j];
            }
            __syncthreads();
            if (active)
                for (int e = 0; e < ne; ++e) {
                    const double2 x = qr[e * s + a];
                    const double2* qce = qc + e * s + b0 + g;
#pragma unroll
                    for (int j = 0; j < CO_MAXACC; ++j)
                        if (b0 + g + j * G < s) cfma_conj(acc[j], x, qce[j * G]);
                }
        }
        if (active)
#pragma unroll
            for (int j = 0; j < CO_MAXACC; ++j) {
                const int b = b0 + g + j * G;
                if (b < s) {
                    const double2 v = clamp_magnitude(acc[j], atol);
                    o[2 * (a + (int64_t)b * s)] = v.x;
                    o[2 * (a + (int64_t)b * s) + 1] = v.y;
                }
            }
    }
}

bool cx_image_outer_supports(int max_s, int nblocks, int64_t d) { return max_s >= 1 && max_s <= CO_MAX_BLOCK && nblocks <= 65535 && d <= 0x7FFFFFFF; }

void launch_cx_image_outer(hipStream_t s, int64_t n, int64_t d, int64_t S1, int64_t S, int nblocks, int max_s, const double* Qrm,
                           const uint32_t* ent, const int64_t* cls_ptr, const int32_t* blk_col, const int32_t* blk_size,
                           const int64_t* blk_off, double atol, double* out) {
    if (d < 1) return;
    dim3 g((unsigned)d, (unsigned)nblocks);
    const size_t lds = (size_t)2 * CO_EB * max_s * sizeof(double2);
    cx_image_outer_kernel<<<g, CO_THREADS, lds, s>>>((uint32_t)n, S1, S, reinterpret_cast<const double2*>(Qrm), ent, cls_ptr, blk_col,
                                                     blk_size, blk_off, atol, out);
}

}  // namespace sdpsr
