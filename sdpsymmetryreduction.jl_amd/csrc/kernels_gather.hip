// Fills, channel gathers and padded copies for gfx950: label gather (fill!/randomize!), the int8 / f32 / f64 channel
// matrices of the square step, and the copies into and out of padded matrices.
//
// Reference semantics restated here:
//   fill!/randomize!      src/partitions.jl:68-75, src/abstract_part.jl:107-110
//   _clamp_round!         src/utils.jl:34-53
//
// All of these are HBM-bound: one pass over n^2 entries each, 16-byte accesses per lane,
// grid sized to a few blocks per CU with grid-stride loops.
#include "sdpsr_internal.h"
#include "kernel_util.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// fill / randomize / clamp_round
// ---------------------------------------------------------------------------
__global__ void fill_f64_kernel(int64_t len, const uint32_t* __restrict__ L,
                                const double* __restrict__ values, uint32_t d, double* __restrict__ M,
                                uint32_t* __restrict__ bad_flag) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        uint32_t l = L[e];
        if (l > d) {  // @assert length(values) == dim(P), src/partitions.jl:69: never read past `values`
            bad = true;
            l = 0;
        }
        M[e] = l ? values[l - 1] : 0.0;
    }
    if (bad) *bad_flag = 1u;
}

__global__ void randomize_f64_kernel(int64_t len, const uint32_t* __restrict__ L, uint64_t key,
                                     double* __restrict__ M) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        uint32_t l = L[e];
        M[e] = l ? sdpsr_class_uniform(key, l) : 0.0;
    }
}

__global__ void clamp_round_kernel(int64_t len, double* __restrict__ a, double atol,
                                   double scale) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride)
        a[e] = sdpsr_clamp_round(a[e], atol, scale);
}

void launch_fill_f64(hipStream_t s, int64_t len, const uint32_t* L, const double* values, int64_t d,
                     double* M, uint32_t* bad_flag) {
    fill_f64_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, L, values, (uint32_t)d, M, bad_flag);
}
void launch_randomize_f64(hipStream_t s, int64_t len, const uint32_t* L, uint64_t key,
                          double* M) {
    randomize_f64_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, L, key, M);
}
void launch_clamp_round(hipStream_t s, int64_t len, double* a, double atol, double scale) {
    clamp_round_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, a, atol, scale);
}

// ---------------------------------------------------------------------------
// channel gathers for the square step.  One thread = 16 consecutive rows of one
// column of the padded ld x ld matrix; each channel gets one 16-byte store (int8) or
// four (f32).  Padding rows/columns are zero.
// ---------------------------------------------------------------------------
constexpr int GATHER_LUT = 2048;  // classes whose random bits are tabulated in LDS

template <int T>
__global__ void gather_i8_kernel(int64_t n, int64_t ld, const uint32_t* __restrict__ L,
                                 uint64_t key, int8_t* __restrict__ X, int dlut) {
    // dlut > 0: the labels are <= dlut <= GATHER_LUT and their 64 random bits come from an LDS
    // table (the per-entry hash costs three quarter-rate 64-bit multiplies, more than the
    // memory traffic of this kernel); the labels of a thread's 16 rows are read as four 16-byte
    // loads when the row count allows it
    __shared__ uint64_t lut[GATHER_LUT + 1];
    if (dlut > 0) {
        for (int i = threadIdx.x; i <= dlut; i += blockDim.x) lut[i] = i ? sdpsr_class_bits(key, (uint32_t)i) : 0ull;
        __syncthreads();
    }
    const bool vec = (n & 3) == 0;
    const int64_t chunks_per_col = ld / 16;
    const int64_t total = chunks_per_col * ld;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += stride) {
        const int64_t j = c / chunks_per_col;
        const int64_t i0 = (c - j * chunks_per_col) * 16;
        uint32_t out[T][4];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int w = 0; w < 4; ++w) out[t][w] = 0;
        if (j < n) {
            uint32_t lab[16];
            if (vec && i0 + 16 <= n) {
                const uint4* p = reinterpret_cast<const uint4*>(L + i0 + j * n);
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const uint4 v = p[q4];
                    lab[4 * q4] = v.x;
                    lab[4 * q4 + 1] = v.y;
                    lab[4 * q4 + 2] = v.z;
                    lab[4 * q4 + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 16; ++q) lab[q] = (i0 + q < n) ? L[i0 + q + j * n] : 0u;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint32_t l = lab[q];
                const uint64_t bits = dlut > 0 ? lut[l] : (l ? sdpsr_class_bits(key, l) : 0ull);
#pragma unroll
                for (int t = 0; t < T; ++t)
                    out[t][q >> 2] |= (uint32_t)((bits >> (8 * t)) & 0xFFull) << (8 * (q & 3));
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            uint4 v = make_uint4(out[t][0], out[t][1], out[t][2], out[t][3]);
            *reinterpret_cast<uint4*>(X + (int64_t)t * ld * ld + i0 + j * ld) = v;
        }
    }
}

void launch_gather_i8(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* L,
                      uint64_t key, int8_t* X, int64_t dmax) {
    // dmax: upper bound of the labels (0 = unknown): enables the LDS table of class bits
    const int dlut = (dmax > 0 && dmax <= GATHER_LUT) ? (int)dmax : 0;
    int g = grid_for(ld / 16 * ld, 256);
    switch (T) {
        case 1: gather_i8_kernel<1><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
        case 2: gather_i8_kernel<2><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
        case 3: gather_i8_kernel<3><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
        case 4: gather_i8_kernel<4><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
        case 5: gather_i8_kernel<5><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
        case 6: gather_i8_kernel<6><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
        case 7: gather_i8_kernel<7><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
        default: gather_i8_kernel<8><<<g, 256, 0, s>>>(n, ld, L, key, X, dlut); break;
    }
}

// Channel gather from the PACKED lower triangle of symmetric labels (column j at offset
// j n - j (j - 1) / 2, rows j .. n-1): 64 x 64 tile pairs (I >= J).  The tile's entries are gathered
// once (coalesced along the packed columns) as 32-bit words holding the <= 4 channel bytes of the
// class, staged in LDS, and written twice: to X[I, J] and, transposed, to X[J, I], 16 rows per
// thread and channel (one 16-byte store each, bytes regrouped by v_perm).  Replaces
// unpack_symmetric_labels + gather_i8 inside the loop (the labels stay packed between the
// refinements of an iteration).  Padding rows / columns (>= n) are written as zero.
__device__ __forceinline__ void bytes_4x4_transpose(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t o[4]) {
    // o[t] = byte t of a, b, c, d (a lowest)
    const uint32_t ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u);  // a0 b0 a1 b1
    const uint32_t ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u);  // a2 b2 a3 b3
    const uint32_t cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u);
    const uint32_t cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);  // a0 b0 c0 d0
    o[1] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
}

// WRITE_L: the kernel also forms the full label matrix Lfull (n x n, leading dimension n) from the labels it has just read -- the work of
// unpack_symmetric_labels_kernel without its pass over Lp.  The lower tile is stored as read, the mirrored one through the SAME LDS tile in a phase
// of its own before the channel bytes are staged (a second tile would halve the resident workgroups); diagonal tiles hold every entry of the tile
// by symmetry and are stored whole.  Nothing is stored at or beyond row / column n.
// LT: the element type of Lp -- uint32_t, or uint8_t for the loop's 8-bit shadow of labels <= 255 (a quarter of the label bytes; the
// sentinel and Lfull stay 32-bit words).
template <int T, bool WRITE_L, typename LT>
__global__ void __launch_bounds__(256)
gather_i8_sym_packed_kernel(int n, int64_t ld, const LT* __restrict__ Lp, uint64_t key, int8_t* __restrict__ X, int dlut,
                            uint32_t* __restrict__ Lfull) {
    __shared__ uint32_t lut[GATHER_LUT + 1];
    __shared__ uint32_t tile[64][65];  // [column][row]: channel bytes of element (i0 + row, j0 + column) (WRITE_L: its label first)
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi < bj) return;
    if (dlut > 0) {
        for (int i = threadIdx.x; i <= dlut; i += blockDim.x) lut[i] = i ? (uint32_t)sdpsr_class_bits(key, (uint32_t)i) : 0u;
        __syncthreads();
    }
    const int i0 = bi * 64, j0 = bj * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    uint32_t lab[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = i0 + tx, j = j0 + ty + 4 * q;
        lab[q] = 0xFFFFFFFFu;
        if (i < n && j < n) {
            const int hi = i > j ? i : j, lo = i > j ? j : i;  // (diagonal tiles: the upper half by symmetry)
            lab[q] = (uint32_t)Lp[(int64_t)lo * n - (int64_t)lo * (lo - 1) / 2 + (hi - lo)];
        }
    }
    if (WRITE_L) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = i0 + tx, j = j0 + ty + 4 * q;
            if (i < n && j < n) Lfull[(int64_t)i + (int64_t)j * n] = lab[q];
            if (bi != bj) tile[ty + 4 * q][tx] = lab[q];
        }
        if (bi != bj) {  // (uniform in the workgroup)
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 16; ++q) {  // destination: row j0 + tx, column i0 + c  (= entry (i0 + c, j0 + tx))
                const int c = ty + 4 * q, rr = j0 + tx, cc = i0 + c;
                if (rr < n && cc < n) Lfull[(int64_t)rr + (int64_t)cc * n] = tile[tx][c];
            }
            __syncthreads();  // the tile is staged again below
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint32_t l = lab[q];
        uint32_t v = 0u;
        if (l != 0xFFFFFFFFu) v = dlut > 0 ? lut[l] : (l ? (uint32_t)sdpsr_class_bits(key, l) : 0u);
        tile[ty + 4 * q][tx] = v;
    }
    __syncthreads();
    // 64 columns x 4 sixteen-row groups = 256 (column, group) pairs per orientation: one per thread
    const int col = threadIdx.x >> 2, seg = threadIdx.x & 3;
#pragma unroll
    for (int orient = 0; orient < 2; ++orient) {
        if (orient == 1 && bi == bj) break;
        uint32_t w[T][4];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            uint32_t e[4], o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = seg * 16 + g4 * 4 + k;
                e[k] = orient == 0 ? tile[col][r] : tile[r][col];  // straight: column `col`, rows r; transposed: row `col` of the tile
            }
            bytes_4x4_transpose(e[0], e[1], e[2], e[3], o);
#pragma unroll
            for (int t = 0; t < T; ++t) w[t][g4] = o[t];
        }
        // straight: X[i0 + seg*16 .., j0 + col]; transposed: X[j0 + seg*16 .., i0 + col]
        const int64_t r0 = (orient == 0 ? i0 : j0) + seg * 16, c0 = (orient == 0 ? j0 : i0) + col;
#pragma unroll
        for (int t = 0; t < T; ++t)
            *reinterpret_cast<uint4*>(X + (int64_t)t * ld * ld + r0 + c0 * ld) = make_uint4(w[t][0], w[t][1], w[t][2], w[t][3]);
    }
}
// Lfull != nullptr: the full n x n label matrix is written as well (leading dimension n)
void launch_gather_i8_sym_packed(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* Lp, uint64_t key, int8_t* X,
                                 int64_t dmax, uint32_t* Lfull, const uint8_t* Lp8) {
    const int dlut = (dmax > 0 && dmax <= GATHER_LUT) ? (int)dmax : 0;
    const unsigned t = (unsigned)(ld / 64);  // ld is a multiple of 128
    dim3 g(t, t);
    if (T == 1) Lp8 = nullptr;  // (one channel: the plain byte form has occupancy 6 against the wide form's 8; no guess runs with one channel)
#define SDPSR_GATHER_PACKED_CASE(TT)                                                                                            \
    case TT:                                                                                                                       \
        if (Lp8 && Lfull) gather_i8_sym_packed_kernel<TT, true, uint8_t><<<g, 256, 0, s>>>((int)n, ld, Lp8, key, X, dlut, Lfull);  \
        else if (Lp8) gather_i8_sym_packed_kernel<TT, false, uint8_t><<<g, 256, 0, s>>>((int)n, ld, Lp8, key, X, dlut, nullptr);   \
        else if (Lfull) gather_i8_sym_packed_kernel<TT, true, uint32_t><<<g, 256, 0, s>>>((int)n, ld, Lp, key, X, dlut, Lfull);    \
        else gather_i8_sym_packed_kernel<TT, false, uint32_t><<<g, 256, 0, s>>>((int)n, ld, Lp, key, X, dlut, nullptr);            \
        break;
    switch (T) {
        SDPSR_GATHER_PACKED_CASE(1)
        SDPSR_GATHER_PACKED_CASE(2)
        SDPSR_GATHER_PACKED_CASE(4)
        default: break;
    }
#undef SDPSR_GATHER_PACKED_CASE
}

__global__ void gather_f32_kernel(int64_t n, int64_t ld, int T, int vmax,
                                  const uint32_t* __restrict__ L, uint64_t key,
                                  float* __restrict__ X) {
    const int64_t chunks_per_col = ld / 4;
    const int64_t total = chunks_per_col * ld;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += stride) {
        const int64_t j = c / chunks_per_col;
        const int64_t i0 = (c - j * chunks_per_col) * 4;
        uint64_t bits[4];
        bool nz[4];  // "non-zero class", kept apart from the 64 bits: channel t draws from byte t of ALL of them, t = 7 included
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + q;
            uint32_t l = (i < n && j < n) ? L[i + j * n] : 0u;
            nz[q] = l != 0u;
            bits[q] = l ? sdpsr_class_bits(key, l) : 0ull;
        }
        for (int t = 0; t < T; ++t) {
            float4 v;
            v.x = nz[0] ? (float)sdpsr_class_small(bits[0], t, vmax) : 0.f;
            v.y = nz[1] ? (float)sdpsr_class_small(bits[1], t, vmax) : 0.f;
            v.z = nz[2] ? (float)sdpsr_class_small(bits[2], t, vmax) : 0.f;
            v.w = nz[3] ? (float)sdpsr_class_small(bits[3], t, vmax) : 0.f;
            *reinterpret_cast<float4*>(X + (int64_t)t * ld * ld + i0 + j * ld) = v;
        }
    }
}

void launch_gather_f32(hipStream_t s, int64_t n, int64_t ld, int T, int vmax, const uint32_t* L,
                       uint64_t key, float* X) {
    gather_f32_kernel<<<grid_for(ld / 4 * ld, 256), 256, 0, s>>>(n, ld, T, vmax, L, key, X);
}

__global__ void gather_f64_padded_kernel(int64_t n, int64_t ld, const uint32_t* __restrict__ L,
                                         uint64_t key, double* __restrict__ X) {
    const int64_t chunks_per_col = ld / 2;
    const int64_t total = chunks_per_col * ld;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += stride) {
        const int64_t j = c / chunks_per_col;
        const int64_t i0 = (c - j * chunks_per_col) * 2;
        double2 v;
        uint32_t l0 = (i0 < n && j < n) ? L[i0 + j * n] : 0u;
        uint32_t l1 = (i0 + 1 < n && j < n) ? L[i0 + 1 + j * n] : 0u;
        v.x = l0 ? sdpsr_class_uniform(key, l0) : 0.0;
        v.y = l1 ? sdpsr_class_uniform(key, l1) : 0.0;
        *reinterpret_cast<double2*>(X + i0 + j * ld) = v;
    }
}

void launch_gather_f64_padded(hipStream_t s, int64_t n, int64_t ld, const uint32_t* L,
                              uint64_t key, double* X) {
    gather_f64_padded_kernel<<<grid_for(ld / 2 * ld, 256), 256, 0, s>>>(n, ld, L, key, X);
}

template <typename T>
__global__ void pad_copy_kernel(int64_t n, int64_t ld, const T* __restrict__ src,
                                T* __restrict__ dst) {
    const int64_t total = ld * ld;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += stride) {
        const int64_t j = c / ld, i = c - j * ld;
        dst[c] = (i < n && j < n) ? src[i + j * n] : T(0);
    }
}
template <typename T>
__global__ void unpad_copy_kernel(int64_t n, int64_t ld, const T* __restrict__ src,
                                  T* __restrict__ dst) {
    const int64_t total = n * n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += stride) {
        const int64_t j = c / n, i = c - j * n;
        dst[c] = src[i + j * ld];
    }
}
void launch_pad_copy(hipStream_t s, int64_t n, int64_t ld, const void* src, void* dst,
                     int elem_bytes) {
    int g = grid_for(ld * ld, 256);
    if (elem_bytes == 1)
        pad_copy_kernel<int8_t><<<g, 256, 0, s>>>(n, ld, (const int8_t*)src, (int8_t*)dst);
    else if (elem_bytes == 4)
        pad_copy_kernel<float><<<g, 256, 0, s>>>(n, ld, (const float*)src, (float*)dst);
    else
        pad_copy_kernel<double><<<g, 256, 0, s>>>(n, ld, (const double*)src, (double*)dst);
}
// dst (n x n) from the LOWER triangle of the padded src (ld x ld), mirrored: dst[i, j] = src[max(i, j), min(i, j)]
__global__ void unpad_mirror_lower_i32_kernel(int64_t n, int64_t ld, const int32_t* __restrict__ src, int32_t* __restrict__ dst) {
    const int64_t total = n * n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += stride) {
        const int64_t j = c / n, i = c - j * n;
        dst[c] = i >= j ? src[i + j * ld] : src[j + i * ld];
    }
}
void launch_unpad_mirror_lower_i32(hipStream_t s, int64_t n, int64_t ld, const int32_t* src, int32_t* dst) {
    unpad_mirror_lower_i32_kernel<<<grid_for(n * n, 256), 256, 0, s>>>(n, ld, src, dst);
}
void launch_unpad_copy(hipStream_t s, int64_t n, int64_t ld, const void* src, void* dst,
                       int elem_bytes) {
    int g = grid_for(n * n, 256);
    if (elem_bytes == 4)
        unpad_copy_kernel<float><<<g, 256, 0, s>>>(n, ld, (const float*)src, (float*)dst);
    else
        unpad_copy_kernel<double><<<g, 256, 0, s>>>(n, ld, (const double*)src, (double*)dst);
}

}  // namespace sdpsr
