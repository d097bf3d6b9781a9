// The key pass of the restarts' agreement (agree.cpp): keys[e] = sum_i labels_i[e] * m_i mod 2^64 over up to 64 label
// arrays -- the universal hash whose canonical relabel is the meet of the partitions (refine!, src/partitions.jl:62-66, folded
// over the restarts).  One streaming pass, (R * B / 8 + 8) bytes per entry: the arrays are read at the interface's label width
// B = 8 / 16 / 32 as they lie, no widened copy.
// Shape: that of kernels_labels.hip.  A lane reads 16 bytes of EVERY array per step -- K = 4 / 8 / 16 labels -- and writes its K
// keys with K / 2 adjacent 16-byte stores.  The head (at most one key: keys are 8-byte aligned) brings `keys` to a 16-byte
// boundary; the arrays behind the head are read with 16-byte loads when all of them are aligned too, else with whatever the
// compiler makes of a 16-byte read at element alignment (sub-arrays).  The tail finishes the last (len - head) % K entries one by
// one.  No LDS, nothing shared between workgroups; grid-stride, sized by the CU count.
// The R pointers and multipliers travel as kernel arguments (1 KiB): wave-uniform, read through the scalar cache, no pointer
// table in device memory to upload.
#include "host_internal.h"
#include "label_stream.h"

namespace sdpsr {

namespace {

struct MeetArgs {
    const void* p[AGREE_MAX_RESTARTS];
    uint64_t m[AGREE_MAX_RESTARTS];
};

template <typename T>
__device__ __forceinline__ uint64_t meet_key_at(const MeetArgs& a, int R, int64_t e) {
    uint64_t s = 0;
    for (int i = 0; i < R; ++i) s += (uint64_t)static_cast<const T*>(a.p[i])[e] * a.m[i];
    return s;
}

template <typename T, int ALIGN>
__global__ void __launch_bounds__(256)
meet_keys_kernel(int64_t len, int R, const MeetArgs a, uint64_t* __restrict__ keys) {
    constexpr int K = 16 / (int)sizeof(T);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t head = head_elements(keys, 8, len);
    const int64_t nvec = (len - head) / K;
    if (t < head) keys[t] = meet_key_at<T>(a, R, t);
    uint4* dst = reinterpret_cast<uint4*>(keys + head);  // 16-byte aligned by the choice of head
    for (int64_t g = t; g < nvec; g += stride) {
        uint64_t acc[K];
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = 0;
#pragma unroll 4
        for (int i = 0; i < R; ++i) {
            const uint4 v = load16<ALIGN>(static_cast<const T*>(a.p[i]) + head + g * K);
            const uint64_t m = a.m[i];
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j] += (uint64_t)narrow_piece_get<T>(v, j) * m;
        }
#pragma unroll
        for (int q = 0; q < K / 2; ++q)
            dst[g * (K / 2) + q] = make_uint4((uint32_t)acc[2 * q], (uint32_t)(acc[2 * q] >> 32), (uint32_t)acc[2 * q + 1], (uint32_t)(acc[2 * q + 1] >> 32));
    }
    for (int64_t e = head + nvec * K + t; e < len; e += stride) keys[e] = meet_key_at<T>(a, R, e);
}

template <typename T>
void meet_keys_at_width(hipStream_t s, int64_t len, int R, const MeetArgs& a, uint64_t* keys, int num_cus) {
    constexpr int K = 16 / (int)sizeof(T);
    const int64_t head = std::min<int64_t>((int64_t)(((16u - (uint32_t)((uintptr_t)keys & 15u)) & 15u) / 8u), len);
    const int grid = stream_grid((len - head) / K + 1, num_cus);
    bool aligned = true;
    for (int i = 0; i < R; ++i) aligned = aligned && (((uintptr_t)(static_cast<const T*>(a.p[i]) + head) & 15u) == 0);
    if (aligned) hipLaunchKernelGGL((meet_keys_kernel<T, 16>), dim3(grid), dim3(256), 0, s, len, R, a, keys);
    else hipLaunchKernelGGL((meet_keys_kernel<T, (int)sizeof(T)>), dim3(grid), dim3(256), 0, s, len, R, a, keys);
}

}  // namespace

// arrays[R] (device, `bits` = 8 / 16 / 32 wide, aligned to their element), mult[R]; keys: len words, 8-byte aligned.  0 <= R <= 64
// (R = 0: zeros)
void launch_meet_keys(hipStream_t s, int64_t len, int R, const void* const* arrays, const uint64_t* mult, int bits, uint64_t* keys, int num_cus) {
    if (len <= 0 || R < 0 || R > AGREE_MAX_RESTARTS) return;
    MeetArgs a;
    for (int i = 0; i < AGREE_MAX_RESTARTS; ++i) {
        a.p[i] = i < R ? arrays[i] : nullptr;
        a.m[i] = i < R ? mult[i] : 0;
    }
    if (bits == 32) meet_keys_at_width<uint32_t>(s, len, R, a, keys, num_cus);
    else if (bits == 16) meet_keys_at_width<uint16_t>(s, len, R, a, keys, num_cus);
    else meet_keys_at_width<uint8_t>(s, len, R, a, keys, num_cus);
}

}  // namespace sdpsr
