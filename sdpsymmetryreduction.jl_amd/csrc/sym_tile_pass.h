// The symmetric tile pass and its per-entry maps.  Two users: the label pass of the refinement with the symmetry check folded
// in (refine_label_sym_kernel, kernels_refine.hip) and the symmetric copy checks (kernels_label_util.hip).  Device code only.
#pragma once
#include "sdpsr_internal.h"
#include "refine_table.h"

namespace sdpsr {

// Tile pass shared by refine_label_sym_kernel and copy_check_symmetric_kernel: out = map(in) over an
// n x n column-major matrix, 64 x 64 tile pairs (I, J), I >= J, with the mirror tile compared
// through LDS.  16-byte accesses (4 rows per lane) when n % 4 == 0.  Returns true if some
// out[r, c] != out[c, r] in this workgroup's tiles.
template <bool VEC4, class MAP>
__device__ __forceinline__ bool sym_tile_pass(int64_t n, const uint32_t* in, uint32_t* out, const MAP& map,
                                              uint32_t (*tile)[65]) {
    const int64_t i0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;
    bool bad = false;
    if (VEC4) {
        const int vr = threadIdx.x & 15, cb = threadIdx.x >> 4;  // 16 row groups x 16 columns per round
        uint4 m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // mirror tile: rows j0.., columns i0..
            const int64_t r = j0 + 4 * vr, cc = i0 + cb + 16 * q;
            m[q] = make_uint4(0u, 0u, 0u, 0u);
            if (r < n && cc < n) m[q] = *reinterpret_cast<const uint4*>(in + r + cc * n);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = j0 + 4 * vr, cc = i0 + cb + 16 * q;
            uint4 l = make_uint4(map(m[q].x), map(m[q].y), map(m[q].z), map(m[q].w));
            if (r < n && cc < n && i0 != j0) *reinterpret_cast<uint4*>(out + r + cc * n) = l;
            const int c = cb + 16 * q;
            tile[4 * vr + 0][c] = l.x;
            tile[4 * vr + 1][c] = l.y;
            tile[4 * vr + 2][c] = l.z;
            tile[4 * vr + 3][c] = l.w;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // tile: rows i0.., columns j0..
            const int64_t r = i0 + 4 * vr, cc = j0 + cb + 16 * q;
            if (r < n && cc < n) m[q] = *reinterpret_cast<const uint4*>(in + r + cc * n);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = i0 + 4 * vr, cc = j0 + cb + 16 * q;
            if (r < n && cc < n) {
                const uint4 l = make_uint4(map(m[q].x), map(m[q].y), map(m[q].z), map(m[q].w));
                *reinterpret_cast<uint4*>(out + r + cc * n) = l;
                const int c = cb + 16 * q;  // out[r + k, cc] against out[cc, r + k] = mirror tile (row c, column 4 vr + k)
                bad = bad || l.x != tile[c][4 * vr + 0] || l.y != tile[c][4 * vr + 1] || l.z != tile[c][4 * vr + 2] ||
                      l.w != tile[c][4 * vr + 3];
            }
        }
    } else {
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
#pragma unroll 4
        for (int q = 0; q < 16; ++q) {
            const int64_t r = j0 + tx, cc = i0 + ty + 4 * q;
            uint32_t l = 0u;
            if (r < n && cc < n) {
                l = map(in[r + cc * n]);
                if (i0 != j0) out[r + cc * n] = l;
            }
            tile[tx][ty + 4 * q] = l;
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < 16; ++q) {
            const int64_t r = i0 + tx, cc = j0 + ty + 4 * q;
            if (r < n && cc < n) {
                const uint32_t l = map(in[r + cc * n]);
                out[r + cc * n] = l;
                if (l != tile[ty + 4 * q][tx]) bad = true;
            }
        }
    }
    return bad;
}

struct MapSlotLabel {
    const uint32_t* __restrict__ tab_lab;
    __device__ __forceinline__ uint32_t operator()(uint32_t sl) const { return (sl == NO_SLOT) ? 0u : tab_lab[sl]; }
};
struct MapIdentity {
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return v; }
};
// notes "a label exceeds dmax" from the words that pass through the registers anyway (copy_check_labels_kernel)
struct MapNoteExceeds {
    uint32_t dmax;
    bool* over;
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const {
        if (v > dmax) *over = true;
        return v;
    }
};

}  // namespace sdpsr
