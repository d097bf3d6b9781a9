// C = A' * B on the gfx950 matrix cores, column-major operands (A: k x m, B: k x n, so both
// are read along their contiguous dimension), MFMA tiles staged through LDS.
//
// Serves  mul!(X2, X, X)           src/partitions.jl:172   (X symmetric => X*X = X'X)
//         Q' * A * Q               src/eigen_decomposition.jl:203 (A symmetric)
//         A * F (first columns)    src/eigen_decomposition.jl:333
//
// Variants: int8 -> int32 (v_mfma_i32_32x32x32_i8), f32 (v_mfma_f32_32x32x2_f32, exact f32
// fma chain), f64 (v_mfma_f64_16x16x4_f64); the MFMA step, the accumulator layout, the LDS-DMA
// and the tile numbering are those of mfma_tile.h.  Two kernels, which differ in how a K-tile
// reaches LDS:
//   gemm_tn_dma_kernel<KIND, CMODE, TILE>  global -> LDS DMA into swizzled rows; TILE = 128 (4 waves,
//                                          a wave owns 64 x 64) or 256 (8 waves, a wave owns 128 x 64)
//   gemm_tn_kernel<KIND, CMODE>            register-staged into padded rows, 128 x 128: the fallback
//                                          for operands the DMA cannot take (launch_gemm)
// CMODE 0: C = A'B, 1: C -= A'B.
#include <cstdlib>
#include "sdpsr_internal.h"
#include "mfma_tile.h"

namespace sdpsr {

// The instances that exist: every KIND as 128-tiles with CMODE 0, f64 also with CMODE 1 (the list in
// gemm_set_device_attributes), and of those the ones below as 256-tiles as well.
constexpr bool gemm_has_256(int kind, int cmode) { return kind != KIND_F64 && cmode == 0; }
constexpr size_t dma_lds(int tile) { return 2 * 2 * tile * 128; }  // two buffers of two operand tiles: 64 / 128 KiB

// ---------------------------------------------------------------------------
// LDS-DMA staging (global_load_lds_dwordx4): no VGPR staging and no ds_write pass.  K-tile = 128 bytes
// per operand row; one wave instruction fills 8 rows x 128 B of the lane-linear LDS image, the XOR
// swizzle that makes the ds_read_b128 fragment reads conflict-free is applied on the per-lane SOURCE
// address (slot s of row r holds global chunk s ^ dma_swz(r)) and undone on the read.  Two LDS buffers:
// tile t+1 streams in while tile t feeds the MFMAs.
//
// TILE = 256 (two 64 KiB buffers, one workgroup per CU): the point of the larger tile is the LDS pipe.
// With 128 x 128 / 4 waves every K-tile costs as many LDS-read cycles (64 KiB at 128 B/clk) as MFMA
// cycles (one wave per SIMD, 16 MFMAs), so the kernel sat at ~30 % of the int8 peak.  With 256 x 256 a
// K-tile is 192 KiB of fragment reads (1536 clk) against 2 waves x 32 MFMAs per SIMD (2048 clk), and
// the L2 -> LDS traffic per MFMA halves.
// ---------------------------------------------------------------------------
template <int KIND, int CMODE, int TILE>
__global__ void __launch_bounds__(2 * TILE)
gemm_tn_dma_kernel(int64_t k, const typename MfmaTile<KIND>::in_t* __restrict__ Ag, int64_t lda,
                   const typename MfmaTile<KIND>::in_t* __restrict__ Bg, int64_t ldb,
                   typename MfmaTile<KIND>::out_t* __restrict__ Cg, int64_t ldc, int64_t strideA, int64_t strideB,
                   int64_t strideC, const uint32_t* __restrict__ nonsym_flag) {
    typedef MfmaTile<KIND> MT;
    constexpr int ES = sizeof(typename MT::in_t);
    constexpr int KB = 128;            // bytes of K per row per tile
    constexpr int KE = KB / ES;
    constexpr int OPB = TILE * KB;     // bytes per operand tile
    constexpr int WI = TILE / 2, WJ = 64;                    // a wave's part of the tile: WI (i) x WJ (j)
    constexpr int NI = WI / MT::EDGE, NJ = WJ / MT::EDGE;    // ... in MFMA blocks
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave & 1, wj = wave >> 1;
    int bi = blockIdx.x, bj = blockIdx.y;
    const int lin = blockIdx.y * gridDim.x + blockIdx.x;
    if (nonsym_flag && *nonsym_flag == 0u) {  // uniform
        // symmetric product (C = X'X) whose consumer only reads the lower triangle: lower-triangle tiles only, row-major
        // enumeration (bi, bj <= bi); the workgroups beyond the triangle have nothing to do
        const int ntri = gridDim.x * (gridDim.x + 1) / 2;
        if (lin >= ntri) return;
        tri_decode(xcd_run(lin, ntri), bi, bj);
    } else {
        xcd_swizzle_full(lin, gridDim.x, gridDim.y, bi, bj);
    }
    const int64_t i0 = (int64_t)bi * TILE;
    const int64_t j0 = (int64_t)bj * TILE;
    const char* Ab = reinterpret_cast<const char*>(Ag + (int64_t)blockIdx.z * strideA + i0 * lda);
    const char* Bb = reinterpret_cast<const char*>(Bg + (int64_t)blockIdx.z * strideB + j0 * ldb);
    typename MT::out_t* C = Cg + (int64_t)blockIdx.z * strideC;

    // an operand tile is TILE / 8 DMA instructions of 1 KiB (8 rows x 128 B); this wave issues
    // instructions wave*4 .. wave*4+3 of each operand tile
    int64_t srcA[4], srcB[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = 8 * (wave * 4 + s) + (lane >> 3);
        const int c = (lane & 7) ^ dma_swz<KB>(r);
        srcA[s] = (int64_t)r * lda * ES + c * 16;
        srcB[s] = (int64_t)r * ldb * ES + c * 16;
    }
    const unsigned lds0 = lds_address(smem);
    auto issue = [&](int buf, int64_t kt) {
        const int64_t kb = kt * KB;
        const unsigned dst = lds0 + (unsigned)(buf * 2 * OPB + (wave * 4) * 1024);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            glds16(Ab + srcA[s] + kb, dst + s * 1024);
            glds16(Bb + srcB[s] + kb, dst + OPB + s * 1024);
        }
    };
    const int64_t nk = k / KE;

    typename MT::acc_t acc[NJ][NI];  // [tj: blocks of the B side][ti: blocks of the A side]
#pragma unroll
    for (int a = 0; a < NJ; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b)
#pragma unroll
            for (int r = 0; r < MT::NR; ++r) acc[a][b][r] = 0;
    const int lrow = MT::row(lane), lgrp = MT::grp(lane);
    int rowA[NI], rowB[NJ];
#pragma unroll
    for (int t = 0; t < NI; ++t) rowA[t] = wi * WI + t * MT::EDGE + lrow;
#pragma unroll
    for (int t = 0; t < NJ; ++t) rowB[t] = wj * WJ + t * MT::EDGE + lrow;
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int64_t kt = 0; kt < nk; ++kt) {
        const int buf = (int)(kt & 1);
        if (kt + 1 < nk) issue(buf ^ 1, kt + 1);
        const char* tA = smem + buf * 2 * OPB;
        const char* tB = tA + OPB;
#pragma unroll
        for (int q = 0; q < KB / MT::QB; ++q) {
            typename MT::frag_t fi[NI], fj[NJ];
            const int ch = MT::chunk(q, lgrp);
#pragma unroll
            for (int t = 0; t < NI; ++t)
                fi[t] = *reinterpret_cast<const typename MT::frag_t*>(tA + rowA[t] * KB + ((ch ^ dma_swz<KB>(rowA[t])) << 4));
#pragma unroll
            for (int t = 0; t < NJ; ++t)
                fj[t] = *reinterpret_cast<const typename MT::frag_t*>(tB + rowB[t] * KB + ((ch ^ dma_swz<KB>(rowB[t])) << 4));
#pragma unroll
            for (int tj = 0; tj < NJ; ++tj)
#pragma unroll
                for (int ti = 0; ti < NI; ++ti) MT::step(fj[tj], fi[ti], acc[tj][ti]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    mfma_store_blocks<KIND, CMODE>(acc, C, ldc, i0 + wi * WI, j0 + wj * WJ, lane);
}

// ---------------------------------------------------------------------------
// Register-staged fallback: one workgroup = 4 waves = one 128 x 128 tile of C, a wave owns 64 x 64.
// K is walked in tiles of KB bytes per operand row, loaded to registers and written to LDS double-
// buffered (one barrier per K-tile); LDS rows are padded by 16 B so the ds_read_b128 fragment reads
// are bank-conflict free.
// ---------------------------------------------------------------------------
constexpr int BM = 128;   // rows of C per workgroup (i, from operand A)
constexpr int BN = 128;   // cols of C per workgroup (j, from operand B)
constexpr int NT = 256;   // threads
template <int KIND> constexpr int staged_kb() { return KIND == KIND_I8 ? 64 : 128; }  // bytes of K per operand row per K-tile
template <int KIND> constexpr size_t staged_lds() { return 2 * 2 * BM * (staged_kb<KIND>() + 16); }

template <int KIND, int CMODE>
__global__ void __launch_bounds__(NT)
gemm_tn_kernel(int64_t k, const typename MfmaTile<KIND>::in_t* __restrict__ Ag, int64_t lda,
               const typename MfmaTile<KIND>::in_t* __restrict__ Bg, int64_t ldb,
               typename MfmaTile<KIND>::out_t* __restrict__ Cg, int64_t ldc, int64_t strideA,
               int64_t strideB, int64_t strideC, const uint32_t* __restrict__ nonsym_flag) {
    typedef MfmaTile<KIND> MT;
    constexpr int KB = staged_kb<KIND>();
    constexpr int ES = sizeof(typename MT::in_t);
    constexpr int KE = KB / ES;          // k elements per K-tile
    constexpr int RS = KB + 16;          // padded LDS row stride (bytes)
    constexpr int CH = KB / 16;          // 16-byte chunks per row
    constexpr int LPT = BM * CH / NT;    // chunks per thread per operand (2 or 4)
    constexpr int OPB = BM * RS;         // bytes per operand tile in LDS
    constexpr int NB = 64 / MT::EDGE;    // MFMA blocks per wave and side

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // layout: [buf][operand][row][RS]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wi = wave & 1;   // wave position along i
    const int wj = wave >> 1;  // wave position along j

    const int64_t i0 = (int64_t)blockIdx.x * BM;
    const int64_t j0 = (int64_t)blockIdx.y * BN;
    // symmetric product (C = X'X) whose consumer only reads the lower triangle: tiles above the
    // diagonal are skipped while the device flag says the labels are symmetric
    if (nonsym_flag && i0 < j0 && *nonsym_flag == 0u) return;
    const char* Ab = reinterpret_cast<const char*>(Ag + (int64_t)blockIdx.z * strideA + i0 * lda);
    const char* Bb = reinterpret_cast<const char*>(Bg + (int64_t)blockIdx.z * strideB + j0 * ldb);
    typename MT::out_t* C = Cg + (int64_t)blockIdx.z * strideC;

    // staging assignment: chunk q = tid + s*NT -> row q / CH, chunk q % CH
    int srow[LPT], scol[LPT];
#pragma unroll
    for (int s = 0; s < LPT; ++s) {
        int q = tid + s * NT;
        srow[s] = q / CH;
        scol[s] = q % CH;
    }
    uint4 ra[LPT], rb[LPT];
    auto load_tile = [&](int64_t kt) {
        const int64_t kbyte = kt * KB;
#pragma unroll
        for (int s = 0; s < LPT; ++s) {
            ra[s] = *reinterpret_cast<const uint4*>(Ab + (int64_t)srow[s] * lda * ES + kbyte + scol[s] * 16);
            rb[s] = *reinterpret_cast<const uint4*>(Bb + (int64_t)srow[s] * ldb * ES + kbyte + scol[s] * 16);
        }
    };
    auto store_tile = [&](int buf) {
        char* base = smem + buf * 2 * OPB;
#pragma unroll
        for (int s = 0; s < LPT; ++s) {
            *reinterpret_cast<uint4*>(base + srow[s] * RS + scol[s] * 16) = ra[s];
            *reinterpret_cast<uint4*>(base + OPB + srow[s] * RS + scol[s] * 16) = rb[s];
        }
    };

    const int64_t nk = k / KE;
    typename MT::acc_t acc[NB][NB];
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < MT::NR; ++r) acc[a][b][r] = 0;
    const int lrow = MT::row(lane), lgrp = MT::grp(lane);

    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int64_t kt = 0; kt < nk; ++kt) {
        const int buf = (int)(kt & 1);
        if (kt + 1 < nk) load_tile(kt + 1);
        const char* tA = smem + buf * 2 * OPB;  // rows i
        const char* tB = tA + OPB;              // rows j
#pragma unroll
        for (int q = 0; q < KB / MT::QB; ++q) {
            typename MT::frag_t fi[NB], fj[NB];
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                fi[t] = *reinterpret_cast<const typename MT::frag_t*>(tA + (wi * 64 + t * MT::EDGE + lrow) * RS + MT::chunk(q, lgrp) * 16);
                fj[t] = *reinterpret_cast<const typename MT::frag_t*>(tB + (wj * 64 + t * MT::EDGE + lrow) * RS + MT::chunk(q, lgrp) * 16);
            }
#pragma unroll
            for (int tj = 0; tj < NB; ++tj)
#pragma unroll
                for (int ti = 0; ti < NB; ++ti) MT::step(fj[tj], fi[ti], acc[tj][ti]);
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }
    mfma_store_blocks<KIND, CMODE>(acc, C, ldc, i0 + wi * 64, j0 + wj * 64, lane);
}

// Dynamic-LDS limits are a per-device property of a kernel: sdpsr_create() calls this with the
// ctx's device current, so a process may hold ctxs on several GPUs (no process-global flags).
template <int KIND, int CMODE>
bool gemm_set_attributes_kind() {
    bool ok = true;
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_kernel<KIND, CMODE>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)staged_lds<KIND>());
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_dma_kernel<KIND, CMODE, 128>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)dma_lds(128));
    if constexpr (gemm_has_256(KIND, CMODE))
        ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_dma_kernel<KIND, CMODE, 256>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)dma_lds(256));
    return ok;
}
bool gemm_set_device_attributes() {
    bool ok = true;
    ok &= gemm_set_attributes_kind<KIND_I8, 0>();
    ok &= gemm_set_attributes_kind<KIND_F32, 0>();
    ok &= gemm_set_attributes_kind<KIND_F64, 0>();
    ok &= gemm_set_attributes_kind<KIND_F64, 1>();
    return ok;
}

template <int KIND, int CMODE = 0>
static void launch_gemm(hipStream_t s, int64_t m, int64_t n, int64_t k,
                        const typename MfmaTile<KIND>::in_t* A, int64_t lda,
                        const typename MfmaTile<KIND>::in_t* B, int64_t ldb,
                        typename MfmaTile<KIND>::out_t* C, int64_t ldc, int batch,
                        int64_t strideA, int64_t strideB, int64_t strideC, const uint32_t* nonsym_flag = nullptr) {
    dim3 grid((unsigned)(m / BM), (unsigned)(n / BN), (unsigned)batch);
    constexpr int ESZ = sizeof(typename MfmaTile<KIND>::in_t);
    if ((k * ESZ) % 128 == 0 && ((lda * ESZ) % 16) == 0 && ((ldb * ESZ) % 16) == 0 &&
        ((strideA * ESZ) % 16) == 0 && ((strideB * ESZ) % 16) == 0 &&
        (reinterpret_cast<uintptr_t>(A) % 16) == 0 && (reinterpret_cast<uintptr_t>(B) % 16) == 0) {
        if constexpr (gemm_has_256(KIND, CMODE)) {
            // 256 x 256 tiles pay off (6-15 % measured) once the launch has >= 4 workgroups per CU
            // (one resident workgroup per CU: fewer leave a ragged last round)
            const int64_t t2 = m / 256;
            const int64_t wgs = (nonsym_flag ? t2 * (t2 + 1) / 2 : t2 * (n / 256)) * batch;
            if (m % 256 == 0 && n % 256 == 0 && wgs >= 1024) {
                dim3 grid2((unsigned)(m / 256), (unsigned)(n / 256), (unsigned)batch);
                gemm_tn_dma_kernel<KIND, CMODE, 256><<<grid2, 512, dma_lds(256), s>>>(k, A, lda, B, ldb, C, ldc, strideA, strideB, strideC, nonsym_flag);
                return;
            }
        }
        gemm_tn_dma_kernel<KIND, CMODE, 128><<<grid, 256, dma_lds(128), s>>>(k, A, lda, B, ldb, C, ldc, strideA, strideB, strideC, nonsym_flag);
        return;
    }
    gemm_tn_kernel<KIND, CMODE><<<grid, NT, staged_lds<KIND>(), s>>>(k, A, lda, B, ldb, C, ldc, strideA, strideB, strideC, nonsym_flag);
}

void launch_gemm_tn_i8(hipStream_t s, int64_t m, int64_t n, int64_t k, const int8_t* A,
                       int64_t lda, const int8_t* B, int64_t ldb, int32_t* C, int64_t ldc,
                       int batch, int64_t strideA, int64_t strideB, int64_t strideC) {
    launch_gemm<KIND_I8>(s, m, n, k, A, lda, B, ldb, C, ldc, batch, strideA, strideB, strideC);
}
void launch_gemm_tn_f32(hipStream_t s, int64_t m, int64_t n, int64_t k, const float* A,
                        int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                        int batch, int64_t strideA, int64_t strideB, int64_t strideC) {
    launch_gemm<KIND_F32>(s, m, n, k, A, lda, B, ldb, C, ldc, batch, strideA, strideB, strideC);
}
void launch_gemm_tn_f64(hipStream_t s, int64_t m, int64_t n, int64_t k, const double* A,
                        int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                        int batch, int64_t strideA, int64_t strideB, int64_t strideC) {
    launch_gemm<KIND_F64>(s, m, n, k, A, lda, B, ldb, C, ldc, batch, strideA, strideB, strideC);
}
// C -= A' * B (the compact-WY updates of the back-transformation)
void launch_gemm_tn_f64_sub(hipStream_t s, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B,
                            int64_t ldb, double* C, int64_t ldc) {
    launch_gemm<KIND_F64, 1>(s, m, n, k, A, lda, B, ldb, C, ldc, 1, 0, 0, 0);
}

// C = X'X with only the lower-triangle tiles computed while *nonsym_flag == 0 (device-side
// decision, no host round trip); the consumer must then read C[i,j] for i >= j only
void launch_gemm_tn_i8_sym(hipStream_t s, int64_t n, int64_t k, const int8_t* X, int64_t ldx, int32_t* C, int64_t ldc,
                           int batch, int64_t strideX, int64_t strideC, const uint32_t* nonsym_flag, int num_cus, int variant) {
    // the persistent 256 x 256 launch of kernels_gemm_sym.hip when the shapes allow it (num_cus = 0: never)
    if (nonsym_flag && variant != 1 &&
        launch_i8_symsquare(s, n, k, X, ldx, C, ldc, batch, strideX, strideC, nonsym_flag, num_cus, variant))
        return;
    launch_gemm<KIND_I8>(s, n, n, k, X, ldx, X, ldx, C, ldc, batch, strideX, strideX, strideC, nonsym_flag);
}
void launch_gemm_tn_f32_sym(hipStream_t s, int64_t n, int64_t k, const float* X, int64_t ldx, float* C, int64_t ldc,
                            int batch, int64_t strideX, int64_t strideC, const uint32_t* nonsym_flag) {
    launch_gemm<KIND_F32>(s, n, n, k, X, ldx, X, ldx, C, ldc, batch, strideX, strideX, strideC, nonsym_flag);
}

}  // namespace sdpsr
