// Signature arrays for gfx950: the stand-alone signature kernels of a run-time shape, and the materialise kernel that
// writes a computed source (sig_sources.h) out as an array.
//
// Reference semantics restated here:
//   Partition(M), refine! src/partitions.jl:24-35,44-66
//
// HBM-bound: one pass over the entries each, grid sized to a few blocks per CU with grid-stride loops.
#include <type_traits>
#include "sdpsr_internal.h"
#include "kernel_util.h"
#include "sig_sources.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// signatures
// ---------------------------------------------------------------------------
__global__ void sig_f64_kernel(int64_t len, const uint32_t* __restrict__ L,
                               const double* __restrict__ v, uint64_t* __restrict__ sig) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        uint32_t l = L ? L[e] : 0u;
        uint64_t kb = (uint64_t)__double_as_longlong(v[e]);
        sig[e] = finish_sig(l, kb == 0, sdpsr_sig_mix(sdpsr_sig_start(l), kb));
    }
}
void launch_sig_f64(hipStream_t s, int64_t len, const uint32_t* L, const double* v,
                    uint64_t* sig) {
    sig_f64_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, L, v, sig);
}

// v is a padded ld x ld matrix; output sig is dense n x n
__global__ void sig_f64_rounded_kernel(int64_t n, int64_t ld, const uint32_t* __restrict__ L,
                                       const double* __restrict__ v, double atol, double scale,
                                       uint64_t* __restrict__ sig) {
    const int64_t len = n * n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        const int64_t j = e / n, i = e - j * n;
        uint32_t l = L[e];
        const uint64_t kb = sdpsr_round_key(v[i + j * ld], atol, scale);
        sig[e] = finish_sig(l, kb == 0, sdpsr_sig_mix(sdpsr_sig_start(l), kb));
    }
}
void launch_sig_f64_rounded(hipStream_t s, int64_t n, int64_t ld, const uint32_t* L,
                            const double* v, double atol, double scale, uint64_t* sig) {
    sig_f64_rounded_kernel<<<grid_for(n * n, 256), 256, 0, s>>>(n, ld, L, v, atol, scale, sig);
}

__global__ void sig_u32_kernel(int64_t len, const uint32_t* __restrict__ L,
                               const uint32_t* __restrict__ k, uint64_t* __restrict__ sig) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        uint32_t l = L ? L[e] : 0u;
        uint32_t kk = k[e];
        sig[e] = finish_sig(l, kk == 0, sdpsr_sig_mix(sdpsr_sig_start(l), (uint64_t)kk));
    }
}
void launch_sig_u32(hipStream_t s, int64_t len, const uint32_t* L, const uint32_t* k,
                    uint64_t* sig) {
    sig_u32_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, L, k, sig);
}

// 64-bit integer keys (labels of an Int64 partition, or the hash-combined labels of several
// restarts): key 0 -> signature 0 (the zero class), any other key -> its mixed value
__global__ void sig_u64_kernel(int64_t len, const uint64_t* __restrict__ k, uint64_t* __restrict__ sig) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) {
        const uint64_t kk = k[e];
        sig[e] = finish_sig(0u, kk == 0, sdpsr_sig_mix(sdpsr_sig_start(0u), kk));
    }
}
void launch_sig_u64(hipStream_t s, int64_t len, const uint64_t* k, uint64_t* sig) {
    sig_u64_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, k, sig);
}

// The channel signatures for a run-time channel count T (SrcChan<CT, T> has instances for T = 1, 2, 4, 8 only).
// grid (row chunks, columns): no 64-bit division per entry.
// packed: labels and products are symmetric, only the entries i >= j get a signature, written densely -- column j at
// offset j n - j (j - 1) / 2, rows j .. n-1 (the refinement runs on n (n + 1) / 2 entries; first occurrences in
// column-major order always sit in the lower triangle, so the canonical numbering is that of the full matrix);
// lab_packed: the labels come packed the same way
template <typename CT>
__global__ void sig_channels_kernel(int64_t n, int64_t ld, int T, const uint32_t* __restrict__ L,
                                    const CT* __restrict__ C, uint64_t* __restrict__ sig, int packed, int lab_packed) {
    const int64_t istride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = blockIdx.y; j < n; j += gridDim.y) {
        const int64_t poff = j * n - j * (j - 1) / 2 - j;
        const uint32_t* Lj = (packed && lab_packed) ? L + poff : L + j * n;
        uint64_t* sj = packed ? sig + poff : sig + j * n;
        const CT* Cj = C + j * ld;
#pragma unroll 2
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += istride) {
            if (packed && i < j) continue;
            const uint32_t l = Lj[i];
            uint64_t h = sdpsr_sig_start(l);
            bool allz = true;
            for (int t = 0; t < T; t += 2) {
                const int32_t c0 = (int32_t)Cj[(int64_t)t * ld * ld + i];  // exact: f32 channels hold integers < 2^24
                const int32_t c1 = (t + 1 < T) ? (int32_t)Cj[(int64_t)(t + 1) * ld * ld + i] : 0;
                allz = allz && (c0 == 0) && (c1 == 0);
                h = sig_mix_channels(h, c0, c1);
            }
            sj[i] = finish_sig(l, allz, h);
        }
    }
}
void launch_sig_i32(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* L,
                    const int32_t* C, uint64_t* sig, int packed, int lab_packed) {
    sig_channels_kernel<int32_t><<<column_grid(n), 256, 0, s>>>(n, ld, T, L, C, sig, packed, lab_packed);
}
void launch_sig_f32(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* L,
                    const float* C, uint64_t* sig, int packed, int lab_packed) {
    sig_channels_kernel<float><<<column_grid(n), 256, 0, s>>>(n, ld, T, L, C, sig, packed, lab_packed);
}

bool sig_source_fusable(const SigSource& q) {
    return with_source(q, [](const auto&) {});
}

// A computed source written out as an array, by the source's own fetch / sig.  A source that walks the matrix: columns
// over workgroups, the rows of a column -- i >= j on the packed lower triangle -- over threads; entry (i, j) is number
// off(j) + i of the source's numbering (packed: column j starts at j n - j (j - 1) / 2).  A flat one: a grid-stride loop.
template <class SRC>
__global__ void __launch_bounds__(256)
sig_materialize_kernel(int64_t len, const SRC src, uint64_t* __restrict__ sig) {
    if (!src.walks()) {  // uniform
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += stride) sig[e] = src(e);
        return;
    }
    const int n = src.order();
    const bool low = src.lower();
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const int64_t off = (int64_t)j * n - (low ? (int64_t)j * (j - 1) / 2 + j : 0);
        for (int i = (low ? j : 0) + threadIdx.x; i < n; i += blockDim.x)
            sig[off + i] = src.sig(src.fetch((uint32_t)i, (uint32_t)j, off + i));
    }
}

// The signature array of a computed source: sort / bucket paths, a table that overflowed, SDPSR_FLAG_REFINE_NO_FUSE, or
// a shape without a functor instance -- those have a stand-alone kernel: proj_apply_kernel (any r, full matrix) and
// sig_channels_kernel (any T).  false: nothing can write this source out.
bool launch_sig_materialize(hipStream_t s, int64_t len, const SigSource& q, uint64_t* sig) {
    if (q.kind == SIG_ARRAY) return false;
    const bool done = with_source(q, [&](const auto& src) {
        using SRC = std::decay_t<decltype(src)>;
        if constexpr (SRC::kIJ) {
            const int g = src.walks() ? (int)(q.n < 2048 ? q.n : 2048) : grid_for(len, 256);
            sig_materialize_kernel<SRC><<<g, 256, 0, s>>>(len, src, sig);
        }
    });
    if (done) return true;
    switch (q.kind) {
        case SIG_PROJ:
            if (q.packed) return false;  // (the loop runs the packed projection for r <= 4 only)
            launch_proj_apply(s, len, q.r, q.U, q.L, q.key, nullptr, q.coef, q.atol, q.scale, 1, nullptr, sig);
            return true;
        case SIG_CHAN_I32: launch_sig_i32(s, q.n, q.ld, q.T, q.L, (const int32_t*)q.C, sig, q.packed, q.lab_packed); return true;
        case SIG_CHAN_F32: launch_sig_f32(s, q.n, q.ld, q.T, q.L, (const float*)q.C, sig, q.packed, q.lab_packed); return true;
        default: return false;
    }
}

}  // namespace sdpsr
