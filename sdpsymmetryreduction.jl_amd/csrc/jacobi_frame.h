// The frame the workgroup Jacobi kernels put around a sweep core: load the lower triangle of a symmetric block into LDS with
// V = I (and the workgroup's max |a|), scale it by a power of two, run the sweeps, then either rank the eigenvalues and store
// w and V in ascending order (the solvers) or reconstruct from the unsorted columns (the PSD projection, kernels_psd.hip).
// Every step is written once, over a core policy:
//   JacobiPP  order <= 64  : the ping-pong core of jacobi64.h, padded to an even order, four LDS buffers;
//   JacobiWG  order <= 128 : the one-workgroup core of jacobi128.h, unpadded, V in LDS while it fits, else in global memory.
// A policy gives the frame n, ext (the extent of the load loop), sA / ldl, V / ldv, MAXN and sweeps().  The host-side launch
// shapes of the two cores stand next to them.  Included by kernels_psd.hip (psd_project_kernel on JacobiPP,
// psd_project_mid_kernel on JacobiWG), kernels_batched.hip (blocks_syev64_kernel on JacobiPP) and kernels_sytrd.hip
// (small_syev_jacobi64_kernel on JacobiPP, small_syev_jacobi_kernel on JacobiWG).
#pragma once
#include "jacobi64.h"
#include "jacobi128.h"

namespace sdpsr {

// ---- launch shapes
constexpr int JAC64_MAXN = 64;
constexpr size_t JAC64_MAX_LDS = 136 * 1024;  // the dynamic LDS the kernels on the ping-pong core opt into (order 64: 133 184 bytes)

// one thread per 2 x 2 block of a tournament step, whole waves; max_n: the largest order of the launch (1 .. 64)
inline int jacobi64_pp_threads(int max_n) {
    const int half = (max_n + 1) / 2;
    return (half * half + 63) / 64 * 64;
}
// A, V and their ping-pong twins at the padded order (ld odd)
inline size_t jacobi64_pp_lds_bytes(int max_n) {
    const int mm = (max_n + 1) & ~1;
    return 4 * (size_t)(mm | 1) * mm * sizeof(double) + 64;
}
// one thread per element of the n/2 rotated column pairs, whole waves, at most JAC_MAXTHREADS
inline int jacobi128_threads(int n) {
    const int t = ((n + 1) / 2 * n + 63) / 64 * 64;
    return t > JAC_MAXTHREADS ? JAC_MAXTHREADS : t;
}
// A, and V behind it while both fit
inline size_t jacobi128_frame_lds_bytes(int n) { return jacobi128_lds_bytes(n) * (jacobi128_v_in_lds(n) ? 2 : 1); }

// ---- the two cores
struct JacobiPP {
    static constexpr int MAXN = JAC64_MAXN;
    const int n, ext, ldl, ldv;
    double *const sA, *const V, *const s_red;
    // smem: jacobi64_pp_lds_bytes(n) or more; red: 2 * blockDim / 64 doubles, the caller's again outside sweeps()
    __device__ __forceinline__ JacobiPP(int n_, double* smem, double* red)
        : n(n_), ext((n_ + 1) & ~1), ldl(ext | 1), ldv(ldl), sA(smem), V(smem + (size_t)ldl * ext), s_red(red) {}
    __device__ __forceinline__ int sweeps() const {
        return jacobi64_sweeps_pp(n, ext, ldl, sA, V, V + (size_t)ldl * ext, V + 2 * (size_t)ldl * ext, s_red);
    }
};

struct JacobiWG {
    static constexpr int MAXN = JAC_MAXN;
    const int n, ext, ldl, ldv;
    double *const sA, *const V;
    Jacobi128Shared& sh;
    // smem: jacobi128_frame_lds_bytes(n) or more; vglob + voff: n * n doubles of the workgroup's own, read only when
    // !jacobi128_v_in_lds(n)
    __device__ __forceinline__ JacobiWG(int n_, double* smem, double* vglob, size_t voff, Jacobi128Shared& sh_)
        : n(n_), ext(n_), ldl(n_ | 1), ldv(jacobi128_v_in_lds(n_) ? ldl : n_), sA(smem),
          V(jacobi128_v_in_lds(n_) ? smem + (size_t)ldl * n_ + 8 : vglob + voff), sh(sh_) {}
    __device__ __forceinline__ int sweeps() const { return jacobi128_sweeps(n, ldl, sA, V, ldv, sh); }
};

// ---- the frame's steps: every thread of the workgroup calls them
//
// sA <- the symmetric matrix whose lower triangle is elem(i, j), i >= j (zero in the padding), V <- I, behind a barrier.
// AMAX: returns the workgroup's max |a| over what it loaded, as bits (s_max: blockDim / 64 words); otherwise 0, s_max unused.
template <bool AMAX, class Core, class Elem>
__device__ __forceinline__ unsigned long long jacobi_frame_load(const Core& c, Elem elem, unsigned long long* s_max) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    unsigned long long amax = 0;
    for (int e = tid; e < c.ext * c.ext; e += nthr) {
        const int j = e / c.ext, i = e - j * c.ext;
        const int ii = i > j ? i : j, jj = i > j ? j : i;
        const double v = (ii < c.n) ? elem(ii, jj) : 0.0;
        if (AMAX) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;
            amax = b > amax ? b : amax;  // non-negative doubles order like their bit patterns (NaN above Inf)
        }
        c.sA[i + j * c.ldl] = v;
        c.V[i + j * c.ldv] = (i == j) ? 1.0 : 0.0;
    }
    if (AMAX) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long x = __shfl_down(amax, o, 64);
            amax = x > amax ? x : amax;
        }
        if ((tid & 63) == 0) s_max[tid >> 6] = amax;
    }
    __syncthreads();
    if (AMAX) {
        amax = 0;
        for (int k = 0; k < (nthr >> 6); ++k) amax = s_max[k] > amax ? s_max[k] : amax;
    }
    return amax;
}

// sA *= f (a power of two: exact), behind a barrier
template <class Core>
__device__ __forceinline__ void jacobi_frame_scale(const Core& c, double f) {
    for (int e = threadIdx.x; e < c.ext * c.ext; e += blockDim.x) {
        const int j = e / c.ext, i = e - j * c.ext;
        c.sA[i + j * c.ldl] *= f;
    }
    __syncthreads();
}

// After sweeps(): w <- the diagonal of sA times back in ascending order (ties by index), and, unless Vg == nullptr,
// Vg (leading dimension ldg) <- the columns of V in that order.
template <class Core>
__device__ __forceinline__ void jacobi_frame_store_sorted(const Core& c, double back, double* __restrict__ w, double* __restrict__ Vg,
                                                          int64_t ldg) {
    __shared__ int s_rank[Core::MAXN];
    const int tid = threadIdx.x, nthr = blockDim.x, n = c.n;
    for (int i = tid; i < n; i += nthr) {
        const double li = c.sA[i + i * c.ldl];
        int rk = 0;
        for (int j = 0; j < n; ++j) {
            const double lj = c.sA[j + j * c.ldl];
            rk += (lj < li) || (lj == li && j < i);
        }
        s_rank[i] = rk;
        w[rk] = li * back;
    }
    __syncthreads();
    if (Vg) {
        for (int e = tid; e < n * n; e += nthr) {
            const int j = e / n, i = e - j * n;
            Vg[i + (int64_t)s_rank[j] * ldg] = c.V[i + j * c.ldv];
        }
    }
}

// The workgroup's sums of a and of b, lanes by shuffle, waves left to right: an order fixed by blockDim alone.  The sums
// are thread 0's a and b on return; s_red: 2 * blockDim / 64 doubles.
__device__ __forceinline__ void jacobi_frame_sum2(double& a, double& b, double* s_red) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6] = a;
        s_red[nw + (tid >> 6)] = b;
    }
    __syncthreads();
    if (tid == 0) {
        a = b = 0.0;
        for (int k = 0; k < nw; ++k) {
            a += s_red[k];
            b += s_red[nw + k];
        }
    }
}

}  // namespace sdpsr
