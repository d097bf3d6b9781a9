// The pieces the matrix-core products (kernels_gemm.hip, kernels_gemm_sym.hip) are built from, each defined once:
// the MFMA step and accumulator layout per dtype, the global -> LDS DMA and its source swizzle, the tile numbering.
//
// Fragment rule used throughout: a lane reads 16 contiguous bytes of "its" operand row and uses them for 1 (i8),
// 4 (f32) or 2 (f64) consecutive MFMAs.  Both operands are cut the same way, so each MFMA multiplies matching k
// indices; the order in which k is consumed differs from the natural one, which only permutes an exact sum (integers)
// or the fp rounding order (f32 / f64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdpsr {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));

enum { KIND_I8 = 0, KIND_F32 = 1, KIND_F64 = 2 };

// An EDGE x EDGE block of C on one wave.  Lane = grp * EDGE + row: `row` is the lane's row of the operand block,
// `grp` which 16 bytes of a K-group it holds (r32, h for the 32 x 32 blocks of int8 / f32; r16, g for 16 x 16 f64).
// The MFMA "A" operand is taken from the B side (columns j of C) and the MFMA "B" operand from the A side (rows i),
// so the result is D[jj][ii] and the lanes run along i, contiguous in C.
template <int EDGE_> struct MfmaLayout {
    static constexpr int EDGE = EDGE_;
    static constexpr int LG = 64 / EDGE;          // lane groups
    static constexpr int NR = EDGE * EDGE / 64;   // accumulator registers per lane
    static constexpr int QB = 16 * LG;            // bytes of K per operand row and K-group
    static __device__ __forceinline__ int row(int lane) { return lane & (EDGE - 1); }
    static __device__ __forceinline__ int grp(int lane) { return lane / EDGE; }
    // 16-byte chunk of an operand row that K-group q hands to this lane group: 2 q + h / 4 q + g
    static __device__ __forceinline__ int chunk(int q, int grp) { return LG * q + grp; }
    // accumulator register r of a lane holds D[jj][ii] with ii = row(lane) and jj = lane_col(grp) + reg_col(r): a part
    // that varies with the lane and a part that is uniform
    static __device__ __forceinline__ int lane_col(int grp) { return EDGE == 32 ? 4 * grp : grp; }
    static __device__ __forceinline__ int reg_col(int r) { return EDGE == 32 ? (r & 3) + 8 * (r >> 2) : 4 * r; }
};

template <int KIND> struct MfmaTile;
template <> struct MfmaTile<KIND_I8> : MfmaLayout<32> {
    typedef int8_t in_t;
    typedef int32_t out_t;
    typedef v4i frag_t;
    typedef v16i acc_t;
    static __device__ __forceinline__ void step(const frag_t& fj, const frag_t& fi, acc_t& acc) {
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fj, fi, acc, 0, 0, 0);
    }
};
template <> struct MfmaTile<KIND_F32> : MfmaLayout<32> {  // v_mfma_f32_32x32x2_f32: an exact f32 fma chain
    typedef float in_t;
    typedef float out_t;
    typedef v4f frag_t;
    typedef v16f acc_t;
    static __device__ __forceinline__ void step(const frag_t& fj, const frag_t& fi, acc_t& acc) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fj[e], fi[e], acc, 0, 0, 0);
    }
};
template <> struct MfmaTile<KIND_F64> : MfmaLayout<16> {
    typedef double in_t;
    typedef double out_t;
    typedef v2d frag_t;
    typedef v4d acc_t;
    static __device__ __forceinline__ void step(const frag_t& fj, const frag_t& fi, acc_t& acc) {
#pragma unroll
        for (int e = 0; e < 2; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fj[e], fi[e], acc, 0, 0, 0);
    }
};

// Where a lane's registers of the block that starts at C[i, j] go: register r at the returned pointer + reg_col(r) * ldc.
template <class MT>
__device__ __forceinline__ typename MT::out_t* mfma_lane_ptr(typename MT::out_t* C, int64_t ldc, int64_t i, int64_t j, int lane) {
    return C + (i + MT::row(lane)) + (j + MT::lane_col(MT::grp(lane))) * ldc;
}

// One block, whose first element is C[i, j], into C.
template <int KIND>
__device__ __forceinline__ void mfma_store(const typename MfmaTile<KIND>::acc_t& acc, typename MfmaTile<KIND>::out_t* C, int64_t ldc,
                                           int64_t i, int64_t j, int lane) {
    typedef MfmaTile<KIND> MT;
    typename MT::out_t* Cl = mfma_lane_ptr<MT>(C, ldc, i, j, lane);
#pragma unroll
    for (int r = 0; r < MT::NR; ++r) Cl[(int64_t)MT::reg_col(r) * ldc] = acc[r];
}

// The NJ x NI blocks of a wave, acc[tj][ti] at C[i + ti * EDGE, j + tj * EDGE].  CMODE 0: C = acc; CMODE 1: C -= acc, one
// block column at a time as a batch of independent loads followed by the stores (16 loads for the 4 x 4 f64 blocks of a
// wave in the back-transformation's update, kernels_backtransform.hip).
template <int KIND, int CMODE, int NJ, int NI>
__device__ __forceinline__ void mfma_store_blocks(const typename MfmaTile<KIND>::acc_t (&acc)[NJ][NI], typename MfmaTile<KIND>::out_t* C,
                                                  int64_t ldc, int64_t i, int64_t j, int lane) {
    typedef MfmaTile<KIND> MT;
    constexpr int E = MT::EDGE;
#pragma unroll
    for (int tj = 0; tj < NJ; ++tj) {
        if constexpr (CMODE == 0) {
#pragma unroll
            for (int ti = 0; ti < NI; ++ti) mfma_store<KIND>(acc[tj][ti], C, ldc, i + ti * E, j + tj * E, lane);
        } else {
            typename MT::out_t* Cl = mfma_lane_ptr<MT>(C, ldc, i, j + tj * E, lane);
            typename MT::out_t cv[NI][MT::NR];
#pragma unroll
            for (int ti = 0; ti < NI; ++ti)
#pragma unroll
                for (int r = 0; r < MT::NR; ++r) cv[ti][r] = Cl[ti * E + (int64_t)MT::reg_col(r) * ldc];
#pragma unroll
            for (int ti = 0; ti < NI; ++ti)
#pragma unroll
                for (int r = 0; r < MT::NR; ++r) Cl[ti * E + (int64_t)MT::reg_col(r) * ldc] = cv[ti][r] - acc[tj][ti][r];
        }
    }
}

// ---------------------------------------------------------------------------
// global -> LDS DMA
// ---------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void_t;

// LDS byte address of a pointer into shared memory, as the wave-uniform value the DMA wants
__device__ __forceinline__ unsigned lds_address(const void* p) {
    return __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_void_t*)p);
}

// global -> LDS DMA of 16 bytes per lane (1 KiB per wave instruction, lane-linear at the wave-uniform LDS byte address
// lds_dst).  Issued through inline asm ON PURPOSE: for the builtin the compiler books a pending LDS write on the VM
// counter and, unable to prove that the fragment reads of the OTHER buffer do not alias it, puts an `s_waitcnt vmcnt(0)`
// in front of the first ds_read of every K-tile -- the loads of tile t+1 were drained before tile t was touched and
// nothing overlapped (measured at N = 4096, int8, 4 channels, lower tiles: loads alone 0.124 ms, MFMAs alone 0.127 ms,
// together 0.217 ms).  The asm form is invisible to that bookkeeping; ordering is by the explicit counted waits +
// barriers of the callers' K loops.  M0 (the DMA destination base) is saved and restored in the same statement.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}

// Source-side XOR swizzle of the 16-byte chunks of an LDS row (slot p of row r holds global chunk p ^ dma_swz(r)) that
// makes the ds_read_b128 fragment reads conflict-free (lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} of the b128
// banking, MI355X_MICROARCH.md): rows of 128 bytes alternate between the two halves of the 64 banks, so the 8 rows of a
// group with the same parity need 8 different slots; rows of 64 bytes repeat every 4 rows, the 4 rows of a group with
// the same r mod 4 have (r >> 2) in {0,3,5,6} or {1,2,4,7} and need 4 different slots.
template <int KB> __device__ __forceinline__ int dma_swz(int r) {
    if constexpr (KB == 128) return (r >> 1) & 7;
    else return ((r >> 3) ^ (r >> 2)) & 3;
}

// ---------------------------------------------------------------------------
// Tile numbering (speed only).  Workgroups are dealt round-robin over the 8 XCDs, so ids b and b + 8 share an L2.
// ---------------------------------------------------------------------------
// Workgroup (or job) lin runs on XCD lin % 8: give every XCD one contiguous, equally long run of a sequence of `total`
// tiles (balanced, and neighbours in the run share operand panels through that XCD's L2); the last total % 8 keep
// their own number.
__device__ __forceinline__ int xcd_run(int lin, int total) {
    const int per = total >> 3;
    return (lin < 8 * per) ? (lin & 7) * per + (lin >> 3) : lin;
}

// (row, col), col <= row, of the t-th tile of a lower triangle enumerated row by row.  The strictly lower tiles in the
// same order are (row + 1, col).
__device__ __forceinline__ void tri_decode(int t, int& row, int& col) {
    row = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (row * (row + 1) / 2 > t) --row;
    while ((row + 1) * (row + 2) / 2 <= t) ++row;
    col = t - row * (row + 1) / 2;
}

// Full gm x gn grid: every XCD gets a contiguous range of the tile sequence, walked in 8-row groups, so the workgroups
// resident on an XCD at any time share operand rows through its L2.  Grids that do not divide keep (bi, bj).
__device__ __forceinline__ void xcd_swizzle_full(int lin, int gm, int gn, int& bi, int& bj) {
    const int nwg = gm * gn;
    if ((nwg & 7) == 0 && (gm & 7) == 0) {
        const int swz = xcd_run(lin, nwg);
        const int per_group = 8 * gn;
        const int grp = swz / per_group, within = swz - grp * per_group;
        bi = grp * 8 + (within & 7);
        bj = within >> 3;
    }
}

}  // namespace sdpsr
