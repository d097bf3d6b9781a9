// The pieces every streaming pass over label arrays shares (kernels_labels.hip: the width conversions; kernels_agree.hip: the
// key pass of the restarts' agreement): 16 bytes per lane and step, a head that brings the OUTPUT to a 16-byte boundary, inputs
// aligned to their element only, a grid sized by the CU count.  HIP device code; include behind host_internal.h.
#pragma once
#include <cstdint>

namespace sdpsr {

template <int ALIGN>
__device__ __forceinline__ uint4 load16(const void* p) {
    uint4 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, ALIGN), 16);
    return v;
}

// the K labels of one 16-byte piece of a narrow array, lowest address first (little endian)
template <typename TN>
__device__ __forceinline__ uint32_t narrow_piece_get(const uint4& v, int i) {
    constexpr int PER = 4 / (int)sizeof(TN);  // labels per 32-bit word
    constexpr int BITS = 8 * (int)sizeof(TN);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    return (w[i / PER] >> ((i % PER) * BITS)) & (uint32_t)(TN)~(TN)0;
}

// elements in front of the first 16-byte boundary of `out`
__device__ __forceinline__ int64_t head_elements(const void* out, int elem_bytes, int64_t len) {
    const int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)out & 15u)) & 15u) / (uint32_t)elem_bytes);
    return head < len ? head : len;
}

// a grid-stride pass over `pieces` 16-byte pieces: at most 8 workgroups of 256 per CU
inline int stream_grid(int64_t pieces, int num_cus) {
    int64_t g = (pieces + 255) / 256;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace sdpsr
