// Workgroup-level parallel cyclic Jacobi for symmetric matrices of order 65 <= n <= 128 (any n <= 128 works): A resident in
// LDS, the eigenvector accumulator next to it while both fit the 150 KB opt-in, else in global memory.  Device code only;
// included through jacobi_frame.h, whose one-workgroup policy wraps it, by kernels_sytrd.hip (one problem per launch,
// sdpsr_syev_f64's small path) and kernels_psd.hip (one problem per workgroup: the PSD projection of the blocks of order
// 65 .. 128); kernels_batched.hip gets it the same way and does not use it.
//
// Round-robin ordering: n/2 disjoint rotations per step, n-1 steps per sweep; every step is
// (angles) -> barrier -> (two-sided 2 x 2 block updates of A, column rotations of V) -> barrier.
#pragma once
#include <hip/hip_runtime.h>
#include "jacobi64.h"  // jacobi_angle_newton

namespace sdpsr {

constexpr int JAC_MAXTHREADS = 1024;
constexpr int JAC_MAXN = 128;
constexpr size_t JAC_MAX_LDS = 150 * 1024;  // the dynamic LDS the kernels on this core opt into

// dynamic LDS of A alone (n x n, odd leading dimension n | 1, 8 doubles of padding)
__host__ __device__ inline size_t jacobi128_lds_bytes(int n) { return (size_t)((n | 1) * n + 8) * sizeof(double); }
// V sits in LDS behind A when two such buffers fit (n <= 97)
__host__ __device__ inline bool jacobi128_v_in_lds(int n) { return 2 * jacobi128_lds_bytes(n) <= JAC_MAX_LDS; }

// the core's static LDS: the step's rotations and the norms of the stopping rule
struct Jacobi128Shared {
    double c[JAC_MAXN / 2], s[JAC_MAXN / 2];
    int p[JAC_MAXN / 2], q[JAC_MAXN / 2];
    double red[JAC_MAXTHREADS / 64];
    double off, diag;
};

// Sweeps until ||off(A)||_F <= n eps ||A||_F or 40 sweeps.  sA: n x n symmetric in LDS (leading dimension ldl = n | 1),
// Vtmp: accumulates the rotations (identity on entry; LDS or global, leading dimension ldv).  All threads of the workgroup
// call it behind a barrier that follows the writes of sA and Vtmp; returns the number of sweeps done (40 = not converged).
// On return the eigenvalues are the diagonal of sA (unsorted), the eigenvectors the columns of Vtmp, visible to every thread.
__device__ __forceinline__ int jacobi128_sweeps(int n, int ldl, double* __restrict__ sA, double* __restrict__ Vtmp, int ldv,
                                                Jacobi128Shared& sh) {
    const int tid = threadIdx.x;
    const int JAC_THREADS = blockDim.x;
    const int m = (n + 1) & ~1;  // players of the tournament (a dummy one when n is odd)
    const int half = m >> 1;
    int sweep = 0;
    for (; sweep < 40; ++sweep) {
        // off-diagonal and diagonal norms
        double off = 0, dg = 0;
        for (int e = tid; e < n * n; e += JAC_THREADS) {
            const int j = e / n, i = e - j * n;
            const double v = sA[i + j * ldl];
            if (i == j) dg = fma(v, v, dg);
            else off = fma(v, v, off);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            off += __shfl_down(off, o, 64);
            dg += __shfl_down(dg, o, 64);
        }
        if ((tid & 63) == 0) sh.red[tid >> 6] = off;
        __syncthreads();
        if (tid == 0) {
            double t = 0;
            for (int k = 0; k < JAC_THREADS / 64; ++k) t += sh.red[k];
            sh.off = t;
        }
        __syncthreads();
        if ((tid & 63) == 0) sh.red[tid >> 6] = dg;
        __syncthreads();
        if (tid == 0) {
            double t = 0;
            for (int k = 0; k < JAC_THREADS / 64; ++k) t += sh.red[k];
            sh.diag = t;
        }
        __syncthreads();
        // stop at the backward-error level of a LAPACK solver: ||off(A)||_F <= n eps ||A||_F (the
        // rounding floor of the sweeps themselves is ~ sqrt(n) eps, a tighter bound only spins)
        const double tolr = (double)n * 2.220446049250313e-16;
        if (sh.off <= tolr * tolr * (sh.diag + sh.off) || sh.off == 0.0) break;
        for (int step = 0; step < m - 1; ++step) {
            if (tid < half) {
                int p, q;
                if (tid == 0) {
                    p = m - 1;
                    q = step;
                } else {
                    p = (step + tid) % (m - 1);
                    q = (step - tid + (m - 1)) % (m - 1);
                }
                if (p > q) {
                    const int t = p;
                    p = q;
                    q = t;
                }
                double c = 1.0, s = 0.0;
                if (q < n) {
                    const double apq = sA[p + q * ldl];
                    if (apq != 0.0) jacobi_angle_newton(sA[p + p * ldl], sA[q + q * ldl], apq, c, s);
                }
                sh.c[tid] = c;
                sh.s[tid] = s;
                sh.p[tid] = p;
                sh.q[tid] = (q < n) ? q : -1;
            }
            __syncthreads();
            // A <- J' A J on the 2 x 2 blocks (row pair k1, column pair k2): one thread owns a block,
            // so the two-sided update needs no barrier in between; V <- V J alongside
            for (int e = tid; e < half * half; e += JAC_THREADS) {
                const int k1 = e / half, k2 = e - k1 * half;
                const int r0 = sh.p[k1], r1 = sh.q[k1], c0 = sh.p[k2], c1 = sh.q[k2];
                const double cr = sh.c[k1], sr = sh.s[k1], cc = sh.c[k2], sc = sh.s[k2];
                if (sr == 0.0 && sc == 0.0) continue;
                const bool vr = r1 >= 0, vc = c1 >= 0;
                const double x00 = sA[r0 + c0 * ldl];
                const double x01 = vc ? sA[r0 + c1 * ldl] : 0.0;
                const double x10 = vr ? sA[r1 + c0 * ldl] : 0.0;
                const double x11 = (vr && vc) ? sA[r1 + c1 * ldl] : 0.0;
                const double y00 = cr * x00 - sr * x10, y10 = sr * x00 + cr * x10;
                const double y01 = cr * x01 - sr * x11, y11 = sr * x01 + cr * x11;
                sA[r0 + c0 * ldl] = cc * y00 - sc * y01;
                if (vc) sA[r0 + c1 * ldl] = sc * y00 + cc * y01;
                if (vr) sA[r1 + c0 * ldl] = cc * y10 - sc * y11;
                if (vr && vc) sA[r1 + c1 * ldl] = sc * y10 + cc * y11;
            }
            for (int e = tid; e < half * n; e += JAC_THREADS) {
                const int k = e / n, i = e - k * n;
                const int q = sh.q[k];
                if (q < 0) continue;
                const int p = sh.p[k];
                const double c = sh.c[k], s = sh.s[k];
                if (s == 0.0) continue;
                const double vx = Vtmp[i + p * ldv], vy = Vtmp[i + q * ldv];
                Vtmp[i + p * ldv] = c * vx - s * vy;
                Vtmp[i + q * ldv] = s * vx + c * vy;
            }
            __syncthreads();
        }
    }
    return sweep;
}

}  // namespace sdpsr
