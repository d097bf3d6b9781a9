// sdpsr_psd_project: the projection of many symmetric blocks of order <= 64 onto the PSD cone in ONE launch,
// P_k = V max(w, 0) V' -- the cone step of a first-order method over the reduced SDP (Z_k(x) in PSDCone(),
// docs/src/examples/ReduceAndSolveJuMP.jl:79-83, test/sd_problems.jl:50-52,132-134 of the reference).  sdp_solve.cpp has the
// entry points; the solver's loop runs the FUSED form, which also makes the dual update and the block's residual terms.
//
// One workgroup per block of order 2 .. 64 on the ping-pong Jacobi core of jacobi64.h (what sdpsr_blocks_syev runs); the
// workgroup size follows the largest order of the call, (ceil(s / 2))^2 threads rounded up to waves -- ONE wave per block
// while every order is <= 16, the reduced theta' problems' case.  Blocks of order 1 are clamps, one per thread, in the
// workgroups behind those.  jobs: first the njac blocks of order >= 2, then the n1 of order 1.
//
// A block: load the lower triangle into LDS (the fused form adds Lam on the way), scale by a power of two when max |a| lies
// outside [2^-400, 2^400] (syev_scale_exponent), Jacobi sweeps, then one thread per lower-triangle element forms
//   P_ij = sum over the eigenvalues w_k > 0 of w_k V_ik V_jk              when at most half of them are positive, else
//   P_ij = Z_ij - sum over the w_k < 0 of w_k V_ik V_jk                   (the complement: fewer columns),
// k ascending in the Jacobi's own (unsorted) order, and stores it at (i, j) and (j, i): P is symmetric bit for bit.  The
// complement re-reads Z_ij from global memory (the Jacobi has overwritten its LDS copy; four buffers of order 64 fill the LDS):
// the element's own thread reads it before it writes there, and the upper triangle is never read, so P may alias Z.
// No positive eigenvalue: every sum is empty and P is exactly +0.0.  A NaN or Inf in the lower triangle: the block's outputs are
// NaN and bit 2 of the flag is set; the sweep limit sets bit 1.
//
// Blocks of order 65 .. 128 (opt-in per ctx, sdpsr_set_psd_max_order) go through psd_project_mid_kernel, in a launch of its own
// behind this one: the same contract on the one-workgroup Jacobi of jacobi128.h (what sdpsr_syev_f64 runs at these orders).
#include "sdpsr_internal.h"
#include "jacobi64.h"
#include "jacobi128.h"

namespace sdpsr {

namespace {

constexpr int PSD_MAX_THREADS = 1024;

// In the plain form W = Z and only P / lam_min are written.  In the fused form W = Bx + Lam, P is S (read: the previous
// iterate, written: the new one), and Lam, D = S+ - Lam+ and the block's two residual terms are written as well.
struct PsdArgs {
    const PsdJob* jobs;
    int njac, n1;
    const double* Z;   // plain: the input; fused: Bx
    double* P;         // plain: the projection; fused: S
    double* lam_min;   // one per block, or nullptr
    double* Lam;       // fused only
    double* D;         // fused only
    double* slots;     // fused only: slots[2 blk] = |Bx - S+|^2, slots[2 blk + 1] = |S+ - S|^2 over the block
    int* flag;
};

template <bool FUSED>
__device__ __forceinline__ double psd_input(const PsdArgs& a, int64_t p) {
    return FUSED ? a.Z[p] + a.Lam[p] : a.Z[p];
}

// the element at flat position p of a block gets the projected value v (plain), or the whole dual update (fused)
template <bool FUSED>
__device__ __forceinline__ void psd_store(const PsdArgs& a, int64_t p, double v, double& rp, double& rd) {
    if (!FUSED) {
        a.P[p] = v;
        return;
    }
    const double bx = a.Z[p], lam = a.Lam[p], sold = a.P[p];
    const double lnew = (bx + lam) - v;
    const double ep = bx - v, ed = v - sold;
    rp = fma(ep, ep, rp);
    rd = fma(ed, ed, rd);
    a.P[p] = v;
    a.Lam[p] = lnew;
    a.D[p] = v - lnew;
}

template <bool FUSED>
__global__ void __launch_bounds__(PSD_MAX_THREADS)
psd_project_kernel(PsdArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];  // A, V and their ping-pong twins (m x m, ld ldl)
    __shared__ double s_red[2 * PSD_MAX_THREADS / 64];
    __shared__ unsigned long long s_max[PSD_MAX_THREADS / 64];
    __shared__ double s_w[64];
    __shared__ int s_sel[64];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    if ((int)blockIdx.x >= a.njac) {  // the blocks of order 1: a clamp each
        const int64_t t = (int64_t)(blockIdx.x - a.njac) * nthr + tid;
        if (t >= a.n1) return;
        const PsdJob jb = a.jobs[a.njac + t];
        const double z = psd_input<FUSED>(a, jb.zoff);
        const bool bad = !(fabs(z) < INFINITY);
        double rp = 0.0, rd = 0.0;
        psd_store<FUSED>(a, jb.zoff, bad ? qnan : (z > 0.0 ? z : 0.0), rp, rd);
        if (a.lam_min) a.lam_min[jb.blk] = bad ? qnan : z;
        if (FUSED) {
            a.slots[2 * (int64_t)jb.blk] = rp;
            a.slots[2 * (int64_t)jb.blk + 1] = rd;
        }
        if (bad) atomicOr(a.flag, 2);
        return;
    }
    const PsdJob jb = a.jobs[blockIdx.x];
    const int n = jb.n;
    const int m = (n + 1) & ~1;
    const int ldl = m | 1;
    double* sA = smem;
    double* sV = sA + (size_t)ldl * m;
    unsigned long long amax = 0;
    for (int e = tid; e < m * m; e += nthr) {
        const int j = e / m, i = e - j * m;
        const int ii = i > j ? i : j, jj = i > j ? j : i;
        const double v = (ii < n) ? psd_input<FUSED>(a, jb.zoff + ii + (int64_t)jj * n) : 0.0;
        const unsigned long long b = (unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;
        amax = b > amax ? b : amax;  // non-negative doubles order like their bit patterns (NaN above Inf)
        sA[i + j * ldl] = v;
        sV[i + j * ldl] = (i == j) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_down(amax, o, 64);
        amax = x > amax ? x : amax;
    }
    if ((tid & 63) == 0) s_max[tid >> 6] = amax;
    __syncthreads();
    amax = 0;
    for (int k = 0; k < nw; ++k) amax = s_max[k] > amax ? s_max[k] : amax;
    double rp = 0.0, rd = 0.0;
    if (amax >= 0x7FF0000000000000ull) {  // uniform: an Inf or a NaN in the lower triangle
        for (int e = tid; e < n * n; e += nthr) psd_store<FUSED>(a, jb.zoff + e, qnan, rp, rd);
        if (tid == 0) {
            if (a.lam_min) a.lam_min[jb.blk] = qnan;
            if (FUSED) a.slots[2 * (int64_t)jb.blk] = a.slots[2 * (int64_t)jb.blk + 1] = qnan;
            atomicOr(a.flag, 2);
        }
        return;
    }
    const int ex = syev_scale_exponent(amax);
    const double fwd = __longlong_as_double((long long)(1023 - ex) << 52), back = __longlong_as_double((long long)(1023 + ex) << 52);
    if (ex != 0) {  // uniform
        for (int e = tid; e < m * m; e += nthr) {
            const int j = e / m, i = e - j * m;
            sA[i + j * ldl] *= fwd;
        }
        __syncthreads();
    }
    const int sweep = jacobi64_sweeps_pp(n, m, ldl, sA, sV, sV + (size_t)ldl * m, sV + 2 * (size_t)ldl * m, s_red);
    // the eigenvalues (scaled), how many are positive, and the columns the reconstruction sums over
    if (tid < 64) {
        const double w = tid < n ? sA[tid + tid * ldl] : 0.0;
        s_w[tid] = w;
        const unsigned long long pos = __ballot(tid < n && w > 0.0);
        const bool use_pos = 2 * __popcll(pos) <= n;
        const unsigned long long sel = use_pos ? pos : __ballot(tid < n && w < 0.0);
        if ((sel >> tid) & 1ull) s_sel[__popcll(sel & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) {
            s_cnt[0] = __popcll(sel);
            s_cnt[1] = use_pos ? 1 : 0;
        }
        if (a.lam_min) {
            double mn = tid < n ? w : INFINITY;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_down(mn, o, 64));
            if (tid == 0) a.lam_min[jb.blk] = mn * back;
        }
    }
    __syncthreads();
    const int nsel = s_cnt[0];
    const bool use_pos = s_cnt[1] != 0;
    for (int e = tid; e < n * n; e += nthr) {
        const int j = e / n, i = e - j * n;
        if (i < j) continue;
        double acc = 0.0;
        for (int q = 0; q < nsel; ++q) {
            const int k = s_sel[q];
            acc = fma(s_w[k] * sV[i + k * ldl], sV[j + k * ldl], acc);
        }
        if (!use_pos) acc = psd_input<FUSED>(a, jb.zoff + i + (int64_t)j * n) * fwd - acc;
        const double v = acc * back;
        psd_store<FUSED>(a, jb.zoff + i + (int64_t)j * n, v, rp, rd);
        if (i != j) psd_store<FUSED>(a, jb.zoff + j + (int64_t)i * n, v, rp, rd);
    }
    if (FUSED) {  // the block's two residual terms: lanes by shuffle, waves left to right -- an order fixed by the block's order alone
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            rp += __shfl_down(rp, o, 64);
            rd += __shfl_down(rd, o, 64);
        }
        if ((tid & 63) == 0) {
            s_red[tid >> 6] = rp;
            s_red[nw + (tid >> 6)] = rd;
        }
        __syncthreads();
        if (tid == 0) {
            double tp = 0.0, td = 0.0;
            for (int k = 0; k < nw; ++k) {
                tp += s_red[k];
                td += s_red[nw + k];
            }
            a.slots[2 * (int64_t)jb.blk] = tp;
            a.slots[2 * (int64_t)jb.blk + 1] = td;
        }
    }
    if (tid == 0 && sweep >= 40) atomicOr(a.flag, 1);  // (an integer flag: order does not matter)
}

// The blocks of order 65 .. 128 (a ctx with sdpsr_set_psd_max_order(128)): one workgroup of 1024 threads per block on the
// Jacobi core of jacobi128.h -- A in LDS (n x n, ld n | 1), V behind it while both fit (n <= 97), else in the block's slice
// of a scratch in global memory: the jobs with V in global memory come FIRST, so slice = blockIdx.x.  The contract is that of
// psd_project_kernel above, line by line: lower triangle (+ Lam), power-of-two scaling, the same stopping rule and sweep
// limit, the positive columns or the complement with Z re-read by the element's own thread, (i, j) and (j, i) from one value,
// flag bits 1 and 2, the block's residual terms summed lanes by shuffle and waves left to right.  The columns are selected by
// two 64-lane ballots (waves 0 and 1), wave 1's columns behind wave 0's: k ascends.
template <bool FUSED>
__global__ void __launch_bounds__(JAC_MAXTHREADS)
psd_project_mid_kernel(PsdArgs a, double* __restrict__ vglob) {
    extern __shared__ __attribute__((aligned(16))) double smem[];  // A, and V while n <= 97
    __shared__ Jacobi128Shared s_jac;
    __shared__ double s_red[2 * JAC_MAXTHREADS / 64];
    __shared__ unsigned long long s_max[JAC_MAXTHREADS / 64];
    __shared__ double s_w[JAC_MAXN];
    __shared__ int s_sel[JAC_MAXN];
    __shared__ unsigned long long s_bal[4];
    const int tid = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const PsdJob jb = a.jobs[blockIdx.x];
    const int n = jb.n;
    const int ldl = n | 1;
    const bool v_in_lds = jacobi128_v_in_lds(n);
    double* sA = smem;
    double* V = v_in_lds ? sA + (size_t)ldl * n + 8 : vglob + (size_t)blockIdx.x * PSD_MID_VSLICE;
    const int ldv = v_in_lds ? ldl : n;
    unsigned long long amax = 0;
    for (int e = tid; e < n * n; e += nthr) {
        const int j = e / n, i = e - j * n;
        const int ii = i > j ? i : j, jj = i > j ? j : i;
        const double v = psd_input<FUSED>(a, jb.zoff + ii + (int64_t)jj * n);
        const unsigned long long b = (unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;
        amax = b > amax ? b : amax;  // non-negative doubles order like their bit patterns (NaN above Inf)
        sA[i + j * ldl] = v;
        V[i + j * ldv] = (i == j) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_down(amax, o, 64);
        amax = x > amax ? x : amax;
    }
    if ((tid & 63) == 0) s_max[tid >> 6] = amax;
    __syncthreads();
    amax = 0;
    for (int k = 0; k < nw; ++k) amax = s_max[k] > amax ? s_max[k] : amax;
    double rp = 0.0, rd = 0.0;
    if (amax >= 0x7FF0000000000000ull) {  // uniform: an Inf or a NaN in the lower triangle
        for (int e = tid; e < n * n; e += nthr) psd_store<FUSED>(a, jb.zoff + e, qnan, rp, rd);
        if (tid == 0) {
            if (a.lam_min) a.lam_min[jb.blk] = qnan;
            if (FUSED) a.slots[2 * (int64_t)jb.blk] = a.slots[2 * (int64_t)jb.blk + 1] = qnan;
            atomicOr(a.flag, 2);
        }
        return;
    }
    const int ex = syev_scale_exponent(amax);
    const double fwd = __longlong_as_double((long long)(1023 - ex) << 52), back = __longlong_as_double((long long)(1023 + ex) << 52);
    if (ex != 0) {  // uniform
        for (int e = tid; e < n * n; e += nthr) {
            const int j = e / n, i = e - j * n;
            sA[i + j * ldl] *= fwd;
        }
        __syncthreads();
    }
    const int sweep = jacobi128_sweeps(n, ldl, sA, V, ldv, s_jac);
    // the eigenvalues (scaled), how many are positive, and the columns the reconstruction sums over: one ballot per wave
    if (tid < JAC_MAXN) {
        const double w = tid < n ? sA[tid + tid * ldl] : 0.0;
        s_w[tid] = w;
        const unsigned long long pos = __ballot(tid < n && w > 0.0), neg = __ballot(tid < n && w < 0.0);
        if ((tid & 63) == 0) {
            s_bal[tid >> 6] = pos;
            s_bal[2 + (tid >> 6)] = neg;
        }
    }
    __syncthreads();
    const bool use_pos = 2 * (__popcll(s_bal[0]) + __popcll(s_bal[1])) <= n;
    const unsigned long long sel0 = use_pos ? s_bal[0] : s_bal[2], sel1 = use_pos ? s_bal[1] : s_bal[3];
    const int nsel0 = __popcll(sel0), nsel = nsel0 + __popcll(sel1);
    if (tid < JAC_MAXN) {
        const int lane = tid & 63;
        const unsigned long long mine = tid < 64 ? sel0 : sel1;
        if ((mine >> lane) & 1ull) s_sel[(tid < 64 ? 0 : nsel0) + __popcll(mine & ((1ull << lane) - 1ull))] = tid;
    }
    if (a.lam_min && tid < 64) {
        double mn = fmin(tid < n ? s_w[tid] : INFINITY, tid + 64 < n ? s_w[tid + 64] : INFINITY);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_down(mn, o, 64));
        if (tid == 0) a.lam_min[jb.blk] = mn * back;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += nthr) {
        const int j = e / n, i = e - j * n;
        if (i < j) continue;
        double acc = 0.0;
        for (int q = 0; q < nsel; ++q) {
            const int k = s_sel[q];
            acc = fma(s_w[k] * V[i + k * ldv], V[j + k * ldv], acc);
        }
        if (!use_pos) acc = psd_input<FUSED>(a, jb.zoff + i + (int64_t)j * n) * fwd - acc;
        const double v = acc * back;
        psd_store<FUSED>(a, jb.zoff + i + (int64_t)j * n, v, rp, rd);
        if (i != j) psd_store<FUSED>(a, jb.zoff + j + (int64_t)i * n, v, rp, rd);
    }
    if (FUSED) {  // the block's two residual terms: lanes by shuffle, waves left to right -- an order fixed by the block's order alone
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            rp += __shfl_down(rp, o, 64);
            rd += __shfl_down(rd, o, 64);
        }
        if ((tid & 63) == 0) {
            s_red[tid >> 6] = rp;
            s_red[nw + (tid >> 6)] = rd;
        }
        __syncthreads();
        if (tid == 0) {
            double tp = 0.0, td = 0.0;
            for (int k = 0; k < nw; ++k) {
                tp += s_red[k];
                td += s_red[nw + k];
            }
            a.slots[2 * (int64_t)jb.blk] = tp;
            a.slots[2 * (int64_t)jb.blk + 1] = td;
        }
    }
    if (tid == 0 && sweep >= 40) atomicOr(a.flag, 1);  // (an integer flag: order does not matter)
}

}  // namespace

bool psd_set_device_attributes() {
    bool ok = true;
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_kernel<false>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_kernel<true>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_mid_kernel<false>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)JAC_MAX_LDS);
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_mid_kernel<true>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)JAC_MAX_LDS);
    return ok;
}

bool psd_mid_v_in_global(int n) { return !jacobi128_v_in_lds(n); }

size_t psd_mid_lds_bytes(int n) { return jacobi128_lds_bytes(n) * (jacobi128_v_in_lds(n) ? 2 : 1); }

// The nmid blocks of order 65 .. 128 in a launch of their own (jobs: those with psd_mid_v_in_global first -- block b of the
// grid owns slice b of vscratch, PSD_MID_VSLICE doubles each; lds: the largest psd_mid_lds_bytes of the jobs).  The other
// arguments and the two forms are launch_psd_project's.
void launch_psd_project_mid(hipStream_t s, const PsdJob* jobs, int nmid, size_t lds, const double* Z, double* P, double* lam_min,
                            double* Lam, double* D, double* slots, double* vscratch, int* flag) {
    if (nmid <= 0) return;
    const PsdArgs a{jobs, nmid, 0, Z, P, lam_min, Lam, D, slots, flag};
    if (Lam) psd_project_mid_kernel<true><<<nmid, JAC_MAXTHREADS, lds, s>>>(a, vscratch);
    else psd_project_mid_kernel<false><<<nmid, JAC_MAXTHREADS, lds, s>>>(a, vscratch);
}

// max_n: the largest order among the njac Jacobi jobs (2 .. 64; ignored when njac == 0); flag: one int, zeroed by the caller.
// Lam == nullptr: the plain form (Z -> P, lam_min optional).  Otherwise the fused form of the solver's loop: Z = Bx, P = S.
void launch_psd_project(hipStream_t s, const PsdJob* jobs, int njac, int n1, int max_n, const double* Z, double* P, double* lam_min,
                        double* Lam, double* D, double* slots, int* flag) {
    if (njac + n1 <= 0) return;
    int threads = 64;
    size_t lds = 0;
    if (njac > 0) {
        const int half = (max_n + 1) / 2, mm = 2 * half;
        threads = (half * half + 63) / 64 * 64;
        lds = 4 * (size_t)(mm | 1) * mm * sizeof(double) + 64;
    } else if (n1 > 64) {
        threads = 256;
    }
    const int grid = njac + (n1 + threads - 1) / threads;
    const PsdArgs a{jobs, njac, n1, Z, P, lam_min, Lam, D, slots, flag};
    if (Lam) psd_project_kernel<true><<<grid, threads, lds, s>>>(a);
    else psd_project_kernel<false><<<grid, threads, lds, s>>>(a);
}

}  // namespace sdpsr
