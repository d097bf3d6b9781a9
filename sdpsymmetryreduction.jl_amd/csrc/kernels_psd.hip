// sdpsr_psd_project: the projection of many symmetric blocks onto the PSD cone, P_k = V max(w, 0) V' -- the cone step of a
// first-order method over the reduced SDP (Z_k(x) in PSDCone(), docs/src/examples/ReduceAndSolveJuMP.jl:79-83,
// test/sd_problems.jl:50-52,132-134 of the reference).  sdp_solve.cpp has the entry points; the solver's loop runs the FUSED
// form, which also makes the dual update and the block's residual terms.
//
// One workgroup per block, and ONE body for every order, psd_block, over a Jacobi core of jacobi_frame.h:
//   psd_project_kernel      orders 2 .. 64 on the ping-pong core (what sdpsr_blocks_syev runs); the workgroup size follows the
//                           largest order of the call, (ceil(s / 2))^2 threads rounded up to waves -- ONE wave per block while
//                           every order is <= 16, the reduced theta' problems' case.  Blocks of order 1 are clamps, one per
//                           thread, in the workgroups behind those.  jobs: first the njac blocks of order >= 2, then the n1
//                           of order 1.
//   psd_project_mid_kernel  orders 65 .. 128 (opt-in per ctx, sdpsr_set_psd_max_order), in a launch of its own behind that
//                           one, on the one-workgroup core (what sdpsr_syev_f64 runs at these orders): 1024 threads, V in LDS
//                           up to order 97, else in the block's slice of a scratch in global memory.
//
// A block: load the lower triangle into LDS (the fused form adds Lam on the way), scale by a power of two when max |a| lies
// outside [2^-400, 2^400] (syev_scale_exponent), Jacobi sweeps, then one thread per lower-triangle element forms
//   P_ij = sum over the eigenvalues w_k > 0 of w_k V_ik V_jk              when at most half of them are positive, else
//   P_ij = Z_ij - sum over the w_k < 0 of w_k V_ik V_jk                   (the complement: fewer columns),
// k ascending in the Jacobi's own (unsorted) order, and stores it at (i, j) and (j, i): P is symmetric bit for bit.  The
// complement re-reads Z_ij from global memory (the Jacobi has overwritten its LDS copy, and the LDS is full):
// the element's own thread reads it before it writes there, and the upper triangle is never read, so P may alias Z.
// No positive eigenvalue: every sum is empty and P is exactly +0.0.  A NaN or Inf in the lower triangle: the block's outputs are
// NaN and bit 2 of the flag is set; the sweep limit sets bit 1.
#include "sdpsr_internal.h"
#include "jacobi_frame.h"

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

// One block of order >= 2 on the workgroup's Jacobi core.  s_red: 2 * blockDim / 64 doubles (the ping-pong core's own will do).
template <bool FUSED, class Core>
__device__ __forceinline__ void psd_block(const PsdArgs& a, const PsdJob& jb, const Core& core, double* s_red) {
    constexpr int NWORD = Core::MAXN / 64;  // the ballot words of the eigenvalues' signs, one per wave
    __shared__ unsigned long long s_word[PSD_MAX_THREADS / 64];  // the waves' maxima of the load; then the ballots, > 0 before < 0
    __shared__ double s_w[Core::MAXN];
    __shared__ int s_sel[Core::MAXN];
    __shared__ int s_cnt[2];  // how many columns are selected; whether they are the positive ones
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int n = jb.n;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const unsigned long long amax =
        jacobi_frame_load<true>(core, [&](int i, int j) { return psd_input<FUSED>(a, jb.zoff + i + (int64_t)j * n); }, s_word);
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
    const int ex = __builtin_amdgcn_readfirstlane(syev_scale_exponent(amax));  // uniform: fwd and back in scalar registers
    const double fwd = __longlong_as_double((long long)(1023 - ex) << 52), back = __longlong_as_double((long long)(1023 + ex) << 52);
    if (ex != 0) jacobi_frame_scale(core, fwd);  // uniform
    const int sweep = core.sweeps();
    const double* V = core.V;
    const int ldv = core.ldv;
    // the eigenvalues (scaled), how many are positive, and the columns the reconstruction sums over: one ballot per wave that
    // holds eigenvalues, wave w's columns behind wave w - 1's, so k ascends.  One word: the wave has it all in registers and
    // the words never go through LDS; more: they do, behind a barrier.
    unsigned long long pos = 0, neg = 0;
    if (tid < Core::MAXN) {
        const double w = tid < n ? core.sA[tid + tid * core.ldl] : 0.0;
        s_w[tid] = w;
        pos = __ballot(tid < n && w > 0.0);
        neg = __ballot(tid < n && w < 0.0);
        if (NWORD > 1 && (tid & 63) == 0) {
            s_word[tid >> 6] = pos;
            s_word[NWORD + (tid >> 6)] = neg;
        }
    }
    if (NWORD > 1) __syncthreads();
    if (tid < Core::MAXN) {
        const auto word = [&](int k, bool positive) { return NWORD > 1 ? s_word[(positive ? 0 : NWORD) + k] : (positive ? pos : neg); };
        int npos = 0;
#pragma unroll
        for (int k = 0; k < NWORD; ++k) npos += __popcll(word(k, true));
        const bool use_pos = 2 * npos <= n;
        const int lane = tid & 63;
        int nsel = 0, before = 0;  // before: the selected columns of the waves in front of this thread's
#pragma unroll
        for (int k = 0; k < NWORD; ++k) {
            const int cnt = __popcll(word(k, use_pos));
            if (k < (tid >> 6)) before += cnt;
            nsel += cnt;
        }
        const unsigned long long mine = word(tid >> 6, use_pos);
        if ((mine >> lane) & 1ull) s_sel[before + __popcll(mine & ((1ull << lane) - 1ull))] = tid;
        if (tid == 0) {
            s_cnt[0] = nsel;
            s_cnt[1] = use_pos ? 1 : 0;
        }
        if (a.lam_min && tid < 64) {
            double mn = tid < n ? s_w[tid] : INFINITY;
#pragma unroll
            for (int k = 1; k < NWORD; ++k) mn = fmin(mn, tid + 64 * k < n ? s_w[tid + 64 * k] : INFINITY);
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
            acc = fma(s_w[k] * V[i + k * ldv], V[j + k * ldv], acc);
        }
        if (!use_pos) acc = psd_input<FUSED>(a, jb.zoff + i + (int64_t)j * n) * fwd - acc;
        const double v = acc * back;
        psd_store<FUSED>(a, jb.zoff + i + (int64_t)j * n, v, rp, rd);
        if (i != j) psd_store<FUSED>(a, jb.zoff + j + (int64_t)i * n, v, rp, rd);
    }
    if (FUSED) {  // the block's two residual terms, in an order fixed by the block's order alone
        jacobi_frame_sum2(rp, rd, s_red);
        if (tid == 0) {
            a.slots[2 * (int64_t)jb.blk] = rp;
            a.slots[2 * (int64_t)jb.blk + 1] = rd;
        }
    }
    if (tid == 0 && sweep >= 40) atomicOr(a.flag, 1);  // (an integer flag: order does not matter)
}

template <bool FUSED>
__global__ void __launch_bounds__(PSD_MAX_THREADS)
psd_project_kernel(PsdArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];  // A, V and their ping-pong twins (m x m, ld ldl)
    __shared__ double s_red[2 * PSD_MAX_THREADS / 64];
    if ((int)blockIdx.x >= a.njac) {  // the blocks of order 1: a clamp each
        const int64_t t = (int64_t)(blockIdx.x - a.njac) * blockDim.x + threadIdx.x;
        if (t >= a.n1) return;
        const PsdJob jb = a.jobs[a.njac + t];
        const double qnan = __longlong_as_double(0x7FF8000000000000ll);
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
    psd_block<FUSED>(a, jb, JacobiPP(jb.n, smem, s_red), s_red);
}

// vglob: the slices of the blocks whose V does not fit the LDS, PSD_MID_VSLICE doubles each.  Those jobs come FIRST, so
// slice = blockIdx.x.
template <bool FUSED>
__global__ void __launch_bounds__(JAC_MAXTHREADS)
psd_project_mid_kernel(PsdArgs a, double* __restrict__ vglob) {
    extern __shared__ __attribute__((aligned(16))) double smem[];  // A, and V while n <= 97
    __shared__ Jacobi128Shared s_jac;
    __shared__ double s_red[2 * JAC_MAXTHREADS / 64];
    const PsdJob jb = a.jobs[blockIdx.x];
    psd_block<FUSED>(a, jb, JacobiWG(jb.n, smem, vglob, (size_t)blockIdx.x * PSD_MID_VSLICE, s_jac), s_red);
}

}  // namespace

bool psd_set_device_attributes() {
    bool ok = true;
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_kernel<false>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)JAC64_MAX_LDS);
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_kernel<true>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)JAC64_MAX_LDS);
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_mid_kernel<false>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)JAC_MAX_LDS);
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&psd_project_mid_kernel<true>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)JAC_MAX_LDS);
    return ok;
}

bool psd_mid_v_in_global(int n) { return !jacobi128_v_in_lds(n); }

size_t psd_mid_lds_bytes(int n) { return jacobi128_frame_lds_bytes(n); }

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
        threads = jacobi64_pp_threads(max_n);
        lds = jacobi64_pp_lds_bytes(max_n);
    } else if (n1 > 64) {
        threads = 256;
    }
    const int grid = njac + (n1 + threads - 1) / threads;
    const PsdArgs a{jobs, njac, n1, Z, P, lam_min, Lam, D, slots, flag};
    if (Lam) psd_project_kernel<true><<<grid, threads, lds, s>>>(a);
    else psd_project_kernel<false><<<grid, threads, lds, s>>>(a);
}

}  // namespace sdpsr
