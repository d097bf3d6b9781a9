// Signature arithmetic and the signature sources (Src*) of the refinement.  Users: the insert kernels (refine_insert.h), the
// materialise kernel and the stand-alone signature kernels (kernels_signature.hip), proj_apply_kernel (kernels_projection.hip)
// and the pair check (ChkPair, kernels_class_compare.hip).  Device code only.
#pragma once
#include <type_traits>
#include "sdpsr_internal.h"
#include "kernel_util.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// Signature arithmetic shared by the sources below (Src*), whose signatures the insert pass of the refinement computes
// itself, and the stand-alone kernels that keep a run-time shape (proj_apply_kernel: any r; sig_channels_kernel: any T).
// A refinement may switch from one to the other in the middle of a call, so both must give the same bits: each
// piece is written once, here or in the source's sig().
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t finish_sig(uint32_t l, bool all_zero, uint64_t h) {
    if (l == 0 && all_zero) return 0;
    return h ? h : 1;
}
// (old label, code of the rounded projected value); the zero class: label 0 with code 0
__device__ __forceinline__ uint64_t sig_label_key(uint32_t l, uint64_t kb) {
    uint64_t h = 0;
    if (l != 0 || kb != 0) {
        h = sdpsr_sig_mix(sdpsr_sig_start(l), kb);
        if (h == 0) h = 1;
    }
    return h;
}
// one mixing step of the channel values of a square: two 32-bit values per 64-bit word
__device__ __forceinline__ uint64_t sig_mix_channels(uint64_t h, int32_t c0, int32_t c1) {
    return sdpsr_sig_mix(h, (uint64_t)(uint32_t)c0 | ((uint64_t)(uint32_t)c1 << 32));
}

// ---------------------------------------------------------------------------
// Signature sources of the insert pass: the refinement either reads a signature array or computes
// each signature itself, and the 8 bytes per entry never travel through HBM.  A computed source is a
// functor: fetch(i, j, e) loads what entry (i, j) -- number e of the source's numbering -- needs, sig(Raw)
// is THE definition of its signature.  Everybody goes through that pair: the insert kernels, the
// materialise kernel that writes the source out as an array (sort / bucket paths, a table that
// overflowed, SDPSR_FLAG_REFINE_NO_FUSE: a refinement may go on with the array where it began with
// the source), so both see the same bits.  with_source() maps a SigSource to its functor.
// Beside the fetch batch every source names the shape of its insert kernel: kInsertPer entries per
// thread and chunk, kLdsSlots entries of the workgroup's LDS table, and kMid: the source also has
// the one-workgroup-per-CU kernel (refine_insert_mid_kernel).
// ---------------------------------------------------------------------------
// A source is either FLAT (signature of the linear index e) or walks the matrix by (row i, column j):
// the insert kernel locates the first entry of a thread's chunk once (a division, or the inversion
// of the packed lower-triangle numbering: a square root and two correction loops) and STEPS from
// one of its entries to the next (+256 rows, wrapping into the following columns) -- the per-entry
// inversion cost as much as the hash (packed passes took 100-118 us for half the entries of a
// 130 us full pass).
struct IjWalk {
    // lower: rows j .. n-1 of column j, column-major (packed lower triangle); else the full n x n square
    __device__ __forceinline__ static void locate(int n, bool lower, int64_t e, uint32_t& i, uint32_t& j) {
        if (lower) {
            packed_lower_ij(n, e, i, j);
        } else {
            j = (uint32_t)e / (uint32_t)n;
            i = (uint32_t)e - j * (uint32_t)n;
        }
    }
    __device__ __forceinline__ static void step(int n, bool lower, uint32_t& i, uint32_t& j, uint32_t by) {
        i += by;
        while (i >= (uint32_t)n && j < (uint32_t)n) {
            ++j;
            i = i - (uint32_t)n + (lower ? j : 0u);
        }
    }
};
struct SrcArray {
    static constexpr bool kIJ = false;
    static constexpr int kFetchBatch = 1;
    static constexpr int kInsertPer = 16, kLdsSlots = 2048;
    static constexpr bool kMid = true;
    const uint64_t* __restrict__ sig;
    __device__ __forceinline__ bool walks() const { return false; }
    __device__ __forceinline__ bool lower() const { return false; }
    __device__ __forceinline__ int order() const { return 1; }
    __device__ __forceinline__ uint64_t at(uint32_t, uint32_t, int64_t) const { return 0; }
    __device__ __forceinline__ uint64_t operator()(int64_t e) const { return __builtin_nontemporal_load(&sig[e]); }
};
// S = Part(a); S = refine!(S, Part(b)) in one pass: the canonical relabel of the value pairs
// (src/partitions.jl:145-146); label 0 only where both values are +0.0.
// packed: the lower triangle column by column (a, b symmetric); else flat, entry e of both
struct SrcPair {
    static constexpr bool kIJ = true;
    static constexpr int kFetchBatch = 8;  // refine_insert_kernel: entries loaded before their signatures are formed
    static constexpr int kInsertPer = 8, kLdsSlots = 1024;
    static constexpr bool kMid = true;
    const double* __restrict__ a;
    const double* __restrict__ b;
    int n, packed;
    __host__ __device__ __forceinline__ bool walks() const { return packed != 0; }
    __host__ __device__ __forceinline__ bool lower() const { return true; }
    __host__ __device__ __forceinline__ int order() const { return n; }
    // fetch / sig: the loads of an entry and the signature of what was loaded
    struct Raw {
        double a, b;
    };
    __device__ __forceinline__ Raw fetch(uint32_t i, uint32_t j, int64_t) const {
        const int64_t e = (int64_t)i + (int64_t)j * n;
        return Raw{__builtin_nontemporal_load(&a[e]), __builtin_nontemporal_load(&b[e])};
    }
    __device__ __forceinline__ uint64_t sig(const Raw& r) const {
        const uint64_t ka = (uint64_t)__double_as_longlong(r.a), kb = (uint64_t)__double_as_longlong(r.b);
        return finish_sig(0u, ka == 0 && kb == 0, sdpsr_sig_mix(sdpsr_sig_mix(sdpsr_sig_start(0u), ka), kb));
    }
    __device__ __forceinline__ uint64_t at(uint32_t i, uint32_t j, int64_t e) const { return sig(fetch(i, j, e)); }
    __device__ __forceinline__ uint64_t operator()(int64_t e) const {
        if (packed) {
            uint32_t i, j;
            packed_lower_ij(n, e, i, j);
            return at(i, j, e);
        }
        return at((uint32_t)e, 0u, e);  // flat: entry e of every operand
    }
};
template <int R>
struct SrcProj {  // what proj_apply_kernel signs with xin = nullptr, do_round = 1, for r = R
    static constexpr bool kIJ = true;
    static constexpr int kFetchBatch = 1;
    static constexpr int kInsertPer = 8, kLdsSlots = 1024;
    static constexpr bool kMid = false;
    const double* __restrict__ U;
    const uint32_t* L;  // may alias the label output of the refinement (read before the entry's own write)
    const double* __restrict__ coef;
    int64_t len;
    uint64_t key;
    double atol, scale;
    int n, packed;  // packed: the lower triangle column by column (symmetric labels and basis)
    int lab_packed;  // L is the packed lower triangle itself (label of packed entry e = L[e])
    __host__ __device__ __forceinline__ bool walks() const { return packed != 0; }
    __host__ __device__ __forceinline__ bool lower() const { return true; }
    __host__ __device__ __forceinline__ int order() const { return n; }
    struct Raw {
        uint32_t l;
        double u[R > 0 ? R : 1];
    };
    __device__ __forceinline__ Raw fetch(uint32_t i, uint32_t j, int64_t e) const {
        const int64_t ef = (int64_t)i + (int64_t)j * n;
        Raw r;
        r.l = L[lab_packed ? e : ef];
#pragma unroll
        for (int k = 0; k < R; ++k) r.u[k] = __builtin_nontemporal_load(&U[(int64_t)k * len + ef]);
        return r;
    }
    __device__ __forceinline__ uint64_t sig(const Raw& r) const {
        const double x = r.l ? sdpsr_class_uniform(key, r.l) : 0.0;
        double p = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) p = fma(r.u[k], coef[k], p);
        return sig_label_key(r.l, sdpsr_round_key(x - p, atol, scale));
    }
    __device__ __forceinline__ uint64_t at(uint32_t i, uint32_t j, int64_t e) const { return sig(fetch(i, j, e)); }
    __device__ __forceinline__ uint64_t operator()(int64_t e) const {
        if (packed) {
            uint32_t i, j;
            packed_lower_ij(n, e, i, j);
            return at(i, j, e);
        }
        return at((uint32_t)e, 0u, e);  // flat: entry e of every operand
    }
};
template <typename CT, int T>
struct SrcChan {  // (old label, T channel values of the square); packed: the lower triangle column by column
    static constexpr bool kIJ = true;
    static constexpr int kFetchBatch = T <= 2 ? 4 : 1;  // (measured at T = 2: 65 -> 58 us; all 8 with three workgroups per CU: 64 us; wider entries not measured)
    static constexpr int kInsertPer = T <= 4 ? 8 : 4, kLdsSlots = 1024;
    static constexpr bool kMid = std::is_same<CT, int32_t>::value && T == 2;
    int n;
    int64_t ld;
    const uint32_t* L;
    const CT* __restrict__ C;
    int packed;
    int lab_packed;  // (with packed) L is the packed lower triangle itself
    __host__ __device__ __forceinline__ bool walks() const { return true; }  // C is ld-strided: (i, j) needed either way
    __host__ __device__ __forceinline__ bool lower() const { return packed != 0; }
    __host__ __device__ __forceinline__ int order() const { return n; }
    struct Raw {
        uint32_t l;
        CT c[T];
    };
    __device__ __forceinline__ Raw fetch(uint32_t i, uint32_t j, int64_t e) const {
        Raw r;
        r.l = lab_packed ? L[e] : L[(int64_t)j * n + i];
        const CT* Cij = C + (int64_t)j * ld + i;
#pragma unroll
        for (int t = 0; t < T; ++t) r.c[t] = __builtin_nontemporal_load(&Cij[(int64_t)t * ld * ld]);
        return r;
    }
    __device__ __forceinline__ uint64_t sig(const Raw& r) const {
        int32_t c[T + (T & 1)];
#pragma unroll
        for (int t = 0; t < T; ++t) c[t] = (int32_t)r.c[t];  // exact: f32 channels hold integers < 2^24
        if constexpr ((T & 1) != 0) c[T] = 0;
        uint64_t h = sdpsr_sig_start(r.l);
        bool allz = true;
#pragma unroll
        for (int t = 0; t < T; t += 2) {
            allz = allz && (c[t] == 0) && (c[t + 1] == 0);
            h = sig_mix_channels(h, c[t], c[t + 1]);
        }
        return finish_sig(r.l, allz, h);
    }
    __device__ __forceinline__ uint64_t at(uint32_t i, uint32_t j, int64_t e) const { return sig(fetch(i, j, e)); }
    __device__ __forceinline__ uint64_t operator()(int64_t e) const {
        uint32_t i, j;
        IjWalk::locate(n, packed != 0, e, i, j);
        return at(i, j, e);
    }
};

// Projection and square of ONE iteration refined together: signature of (old label, rounded
// projected value, channel values of the square) on the packed lower triangle.  Both random
// elements are drawn from the same partition S; the loop reaches the same fixed point as the
// reference's two refinements per iteration (a class is only ever split when it has to be), with
// one insert pass per iteration instead of two.
template <int R, int T>  // T = 2 or 4 channels
struct SrcJoint {
    static constexpr bool kIJ = true;
    static constexpr int kFetchBatch = 1;  // (2: 79 -> 99 us, 8: 114 us for SrcJoint<2, 2>)
    static constexpr int kInsertPer = 8, kLdsSlots = 1024;
    static constexpr bool kMid = false;
    const double* __restrict__ U;
    const uint32_t* L;
    const double* __restrict__ coef;
    uint64_t key;
    double atol, scale;
    const int32_t* __restrict__ C;  // T channels, ld x ld each
    int64_t ld;
    int n, lab_packed;
    __host__ __device__ __forceinline__ bool walks() const { return true; }
    __host__ __device__ __forceinline__ bool lower() const { return true; }
    __host__ __device__ __forceinline__ int order() const { return n; }
    struct Raw {
        uint32_t l;
        double u[R > 0 ? R : 1];
        int32_t c[T];
    };
    __device__ __forceinline__ Raw fetch(uint32_t i, uint32_t j, int64_t e) const {
        static_assert(T == 2 || T == 4, "joint signatures: 2 or 4 channels");
        const int64_t ef = (int64_t)i + (int64_t)j * n;
        Raw r;
        r.l = lab_packed ? L[e] : L[ef];
#pragma unroll
        for (int k = 0; k < R; ++k) r.u[k] = __builtin_nontemporal_load(&U[(int64_t)k * n * n + ef]);
        const int32_t* Cij = C + (int64_t)j * ld + i;
#pragma unroll
        for (int t = 0; t < T; ++t) r.c[t] = __builtin_nontemporal_load(&Cij[(int64_t)t * ld * ld]);
        return r;
    }
    __device__ __forceinline__ uint64_t sig(const Raw& r) const {
        const double x = r.l ? sdpsr_class_uniform(key, r.l) : 0.0;
        double p = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) p = fma(r.u[k], coef[k], p);
        const uint64_t kb = sdpsr_round_key(x - p, atol, scale);
        uint64_t h = sdpsr_sig_mix(sdpsr_sig_start(r.l), kb);
        bool allz = kb == 0;
#pragma unroll
        for (int t = 0; t < T; t += 2) {
            h = sig_mix_channels(h, r.c[t], r.c[t + 1]);
            allz = allz && r.c[t] == 0 && r.c[t + 1] == 0;
        }
        return finish_sig(r.l, allz, h);
    }
    __device__ __forceinline__ uint64_t at(uint32_t i, uint32_t j, int64_t e) const { return sig(fetch(i, j, e)); }
    __device__ __forceinline__ uint64_t operator()(int64_t e) const {
        uint32_t i, j;
        packed_lower_ij(n, e, i, j);
        return at(i, j, e);
    }
};

// THE map from a SigSource to its functor: f(src) with the Src* instance of q.  false (f not called) when q's shape has
// no instance -- a projection onto more than four basis matrices, a channel count other than 1, 2, 4, 8, a joint source
// that is not packed: such a source is not fusable and is written out by the stand-alone kernel of its run-time shape
// (launch_sig_materialize).  Every instance named here gets an insert kernel and a materialise kernel.
template <class F>
static bool with_source(const SigSource& q, F&& f) {
    const int n = (int)q.n;
    switch (q.kind) {
        case SIG_ARRAY: f(SrcArray{q.sig}); return true;
        case SIG_PAIR: f(SrcPair{q.a, q.b, n, q.packed}); return true;
        case SIG_PROJ:
            return with_constant<0, 1, 2, 3, 4>(q.r, [&](auto R) {
                f(SrcProj<decltype(R)::value>{q.U, q.L, q.coef, q.n * q.n, q.key, q.atol, q.scale, n, q.packed, q.lab_packed});
            });
        case SIG_CHAN_I32:
            return with_constant<1, 2, 4, 8>(q.T, [&](auto T) {
                f(SrcChan<int32_t, decltype(T)::value>{n, q.ld, q.L, (const int32_t*)q.C, q.packed, q.lab_packed});
            });
        case SIG_CHAN_F32:
            return with_constant<1, 2, 4, 8>(q.T, [&](auto T) {
                f(SrcChan<float, decltype(T)::value>{n, q.ld, q.L, (const float*)q.C, q.packed, q.lab_packed});
            });
        case SIG_JOINT_I32: {
            bool found = false;
            if (q.packed)
                with_constant<0, 1, 2, 3, 4>(q.r, [&](auto R) {
                    found = with_constant<2, 4>(q.T, [&](auto T) {
                        f(SrcJoint<decltype(R)::value, decltype(T)::value>{q.U, q.L, q.coef, q.key, q.atol, q.scale, (const int32_t*)q.C,
                                                                           q.ld, n, q.lab_packed});
                    });
                });
            return found;
        }
        default: return false;
    }
}

}  // namespace sdpsr
