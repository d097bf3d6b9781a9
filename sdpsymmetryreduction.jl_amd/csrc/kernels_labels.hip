// Label arrays in the reference's own widths: Partition{T} with T = UInt8 / UInt16 (src/partitions.jl:6-11, :84) against the
// uint32 labels every kernel of this library works on.  Two streaming passes, element-wise:
//   narrow  out[e] = (TN)in[e]   uint32 -> uint16 / uint8, flag[0] = 1 if some value does not fit (InexactError, :29)
//   widen   out[e] = in[e]       uint16 / uint8 -> uint32
// A lane moves 16 bytes of the narrow type per step: K = 8 (uint16) or 16 (uint8) labels, against K / 4 16-byte accesses on
// the uint32 side -- narrow stores are the expensive form on this part (a short store costs ~12.5 x a dwordx4 store per byte),
// so a narrow array is only ever written 16 bytes at a time outside the head and the tail.
// Alignment: a caller's device pointer is aligned to its element only (a sub-array).  The head (one element per lane) brings
// the OUTPUT to a 16-byte boundary, so every store of the body is an aligned 16-byte store; the input behind the head is read
// with 16-byte loads when it is aligned too, else with whatever the compiler makes of a 16-byte read at element alignment.
// The tail finishes the last len % K elements one by one.  No LDS, nothing shared between workgroups; grid-stride, sized by
// the CU count.  (load16, narrow_piece_get, head_elements and stream_grid live in label_stream.h: the key pass of
// kernels_agree.hip streams label arrays the same way.)
// Access shape: a lane's 2 / 4 uint32 pieces are ADJACENT, so a wave instruction on that side covers a 2 / 4 KiB span at 50 % /
// 25 % density.  The form with every wave instruction dense (uint32 piece q * 64 + lane, the chunks of four labels changing
// lanes inside groups of 2 / 4 by shuffles) was built and measured: the same 3.3 TB/s at 16 bits, 1.7 TB/s instead of 3.1 / 2.2
// at 8 bits (profiles/r08_label_width.txt) -- the shuffles and selects cost more than the density gains.
#include "host_internal.h"
#include "label_stream.h"

namespace sdpsr {

namespace {

// uint32 -> TN.  `over` collects the OR of everything read: a value above typemax(TN) = 2^B - 1 sets a bit above B, and values
// that fit never do
template <typename TN, int ALIGN_IN>
__global__ void __launch_bounds__(256)
labels_narrow_kernel(int64_t len, const uint32_t* __restrict__ in, TN* __restrict__ out, uint32_t* __restrict__ flag) {
    constexpr int K = 16 / (int)sizeof(TN), PER = 4 / (int)sizeof(TN), BITS = 8 * (int)sizeof(TN);
    constexpr uint32_t TMAX = (uint32_t)(TN)~(TN)0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t head = head_elements(out, (int)sizeof(TN), len);
    const int64_t nvec = (len - head) / K;
    uint32_t over = 0;
    if (t < head) {
        const uint32_t v = in[t];
        over |= v;
        out[t] = (TN)v;
    }
    const uint32_t* src = in + head;
    uint4* dst = reinterpret_cast<uint4*>(out + head);  // 16-byte aligned by the choice of head
    for (int64_t g = t; g < nvec; g += stride) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const uint4 v = load16<ALIGN_IN>(src + g * K + 4 * q);
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * q + j;
                over |= e[j];
                w[i / PER] |= (e[j] & TMAX) << ((i % PER) * BITS);
            }
        }
        dst[g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int64_t e = head + nvec * K + t; e < len; e += stride) {
        const uint32_t v = in[e];
        over |= v;
        out[e] = (TN)v;
    }
    if (over > TMAX) flag[0] = 1u;  // (a word of pinned host memory the host cleared before the launch; every writer stores the same value)
}

// TN -> uint32
template <typename TN, int ALIGN_IN>
__global__ void __launch_bounds__(256)
labels_widen_kernel(int64_t len, const TN* __restrict__ in, uint32_t* __restrict__ out) {
    constexpr int K = 16 / (int)sizeof(TN);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t head = head_elements(out, 4, len);
    const int64_t nvec = (len - head) / K;
    if (t < head) out[t] = (uint32_t)in[t];
    const TN* src = in + head;
    uint4* dst = reinterpret_cast<uint4*>(out + head);  // 16-byte aligned by the choice of head
    for (int64_t g = t; g < nvec; g += stride) {
        const uint4 v = load16<ALIGN_IN>(src + g * K);
#pragma unroll
        for (int q = 0; q < K / 4; ++q)
            dst[g * (K / 4) + q] = make_uint4(narrow_piece_get<TN>(v, 4 * q), narrow_piece_get<TN>(v, 4 * q + 1),
                                              narrow_piece_get<TN>(v, 4 * q + 2), narrow_piece_get<TN>(v, 4 * q + 3));
    }
    for (int64_t e = head + nvec * K + t; e < len; e += stride) out[e] = (uint32_t)in[e];
}

template <typename TN>
void narrow_to(hipStream_t s, int64_t len, const uint32_t* in, TN* out, uint32_t* flag, int num_cus) {
    constexpr int K = 16 / (int)sizeof(TN);
    const int64_t head = std::min<int64_t>((int64_t)(((16u - (uint32_t)((uintptr_t)out & 15u)) & 15u) / sizeof(TN)), len);
    const int grid = stream_grid((len - head) / K + 1, num_cus);
    if (((uintptr_t)(in + head) & 15u) == 0) hipLaunchKernelGGL((labels_narrow_kernel<TN, 16>), dim3(grid), dim3(256), 0, s, len, in, out, flag);
    else hipLaunchKernelGGL((labels_narrow_kernel<TN, 4>), dim3(grid), dim3(256), 0, s, len, in, out, flag);
}

template <typename TN>
void widen_from(hipStream_t s, int64_t len, const TN* in, uint32_t* out, int num_cus) {
    constexpr int K = 16 / (int)sizeof(TN);
    const int64_t head = std::min<int64_t>((int64_t)(((16u - (uint32_t)((uintptr_t)out & 15u)) & 15u) / 4u), len);
    const int grid = stream_grid((len - head) / K + 1, num_cus);
    if (((uintptr_t)(in + head) & 15u) == 0) hipLaunchKernelGGL((labels_widen_kernel<TN, 16>), dim3(grid), dim3(256), 0, s, len, in, out);
    else hipLaunchKernelGGL((labels_widen_kernel<TN, (int)sizeof(TN)>), dim3(grid), dim3(256), 0, s, len, in, out);
}

}  // namespace

// bits = 16 / 8; in / out aligned to their element; flag: see labels_narrow_kernel
void launch_labels_narrow(hipStream_t s, int64_t len, const uint32_t* in, void* out, int bits, uint32_t* flag, int num_cus) {
    if (len <= 0) return;
    if (bits == 16) narrow_to<uint16_t>(s, len, in, (uint16_t*)out, flag, num_cus);
    else narrow_to<uint8_t>(s, len, in, (uint8_t*)out, flag, num_cus);
}

void launch_labels_widen(hipStream_t s, int64_t len, const void* in, int bits, uint32_t* out, int num_cus) {
    if (len <= 0) return;
    if (bits == 16) widen_from<uint16_t>(s, len, (const uint16_t*)in, out, num_cus);
    else widen_from<uint8_t>(s, len, (const uint8_t*)in, out, num_cus);
}

}  // namespace sdpsr
