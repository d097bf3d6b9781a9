// C = X'X for T int8 channel matrices X (ld x ld, symmetric labels => X symmetric, so X'X = X X), the random square of
// the refinement loop:   mul!(X2, X, X)   src/partitions.jl:172
//
// One PERSISTENT launch: at most one workgroup per CU (8 waves, 128 KiB of LDS), every workgroup walks a static list of
// jobs.  Why not the 128 x 128 tiles of kernels_gemm.hip (round 3's product launch, 92 - 98 us at N = 4096, 2 channels):
// its counters (profiles/r04_pmc.json, i8x2_lower_128tiles_counters) say a tile takes 62.7 k clocks where its 512 MFMAs per wave
// need 32.8 k (two workgroups per CU), because the global -> LDS feed is at its per-CU limit -- 64 KiB per K-tile of
// 128 bytes and CU in 1960 clocks = 33 B/clk/CU = 70 GB/s per CU, the rate MI355X_MICROARCH.md gives for LDS gathers
// served by the L2 -- and that the 1056 tiles take three rounds on the 512 resident slots although they are 2.06 rounds
// of work.  Hence
//   * 256 x 256 macro-tiles (a wave owns 128 x 64): half the feed bytes per MFMA, 32 B/clk/CU at the full MFMA rate;
//   * the diagonal macro-tiles two per job, their 2 x 36 lower 32 x 32 blocks dealt 9 to a wave (a "full" wave has 8), so
//     that N = 4096, 2 channels is 240 + 16 = 256 jobs of 1.0 / 1.125 tile times: ONE round on 256 CUs, no tail;
//   * quarter tiles (128 x 128, 8 waves of 64 x 32) for the ragged last 128 rows of an order that is an odd multiple of
//     128 (N = 4104 -> 4224: 256 big jobs + 66 quarter tiles in a short second round);
//   * the K walk in a ring of four 64-byte LDS stages filled by LDS-DMA with counted waits (vmcnt(N), never a drain
//     inside the loop), so the feed does not idle between a stage's arrival and the next issue.
// 76 - 78 us at N = 4096, 2 channels (0.36 of the nominal int8 peak, MfmaUtil 0.40, 193 MB moved for 168 MB algorithmic).
// Where the rest goes, from ablation builds (profiles/r04_i8sym_ablation.txt): the MFMAs alone take 46 us (the matrix
// pipe under random int8 operands runs at ~1.6 GHz under the board's power cap), fragment reads + barriers add 7, the
// DMA 14, the 69 MB of results 9.5 -- the stages add up instead of overlapping, which is what a power budget does.
// The device flag decides as before: *nonsym_flag != 0 => every macro-tile of the full squares (no diagonal jobs).
//
// Exact integers (int32 accumulation of int8 products, |sum| <= 2^14 ld): the order in which K is consumed is free.
#include "sdpsr_internal.h"
#include "mfma_tile.h"

namespace sdpsr {

typedef MfmaTile<KIND_I8> I8Tile;

// What one wave does in one job: the fragments it reads per K-group and the 32 x 32 blocks it accumulates.
// fr[x]: row block (units of 32 rows) of fragment x inside the wave's part of a panel; fragments x < na come from the
// wave's row panel, the others from its column panel (a fragment serves as either MFMA operand: both are cut the same
// way).  Accumulator t multiplies the fragments tr[t] (rows of C) and tc[t] (columns of C) and lands at block
// (fr[tr[t]], fr[tc[t]]) of the wave's part.  wrows / wcols: rows / columns of the wave's part per step of the wave grid
// (wi = wave & 1, wj = wave >> 1); 0 x 0: a diagonal macro-tile, a single panel that every wave reads from its start.
struct SymRole {
    int wrows, wcols;
    int nf, na;
    int fr[7];
    int nacc;
    int tr[9];
    int tc[9];
};
enum { ROLE_FULL = 4, ROLE_QUARTER = 5 };
__device__ constexpr SymRole kSymRoles[6] = {
    // diagonal macro-tile: the 36 blocks (r, c), c <= r, of its 8 x 8 grid of 32 x 32 blocks, dealt nine to a wave
    {0, 0, 6, 6, {3, 4, 5, 0, 1, 2, 0}, 9, {0, 0, 0, 1, 1, 1, 2, 2, 2}, {3, 4, 5, 3, 4, 5, 3, 4, 5}},  // rows 3-5 x columns 0-2
    {0, 0, 7, 7, {6, 7, 0, 1, 2, 3, 4}, 9, {0, 0, 0, 1, 1, 1, 0, 1, 1}, {2, 3, 4, 2, 3, 4, 5, 5, 6}},  // rows 6-7 x columns 0-2, (6,3) (7,3) (7,4)
    {0, 0, 5, 5, {0, 1, 2, 3, 4, 0, 0}, 9, {0, 1, 1, 2, 2, 2, 3, 4, 4}, {0, 0, 1, 0, 1, 2, 3, 3, 4}},  // triangle of rows 0-2, (3,3) (4,3) (4,4)
    {0, 0, 5, 5, {3, 4, 5, 6, 7, 0, 0}, 9, {2, 2, 2, 3, 3, 3, 4, 4, 4}, {0, 1, 2, 1, 2, 3, 2, 3, 4}},  // (5,3..5) (6,4..6) (7,5..7)
    // full macro-tile (256 x 256): the wave's 128 x 64 part, rows from panel A, columns from panel B
    {128, 64, 6, 4, {0, 1, 2, 3, 0, 1, 0}, 8, {0, 1, 2, 3, 0, 1, 2, 3, 0}, {4, 4, 4, 4, 5, 5, 5, 5, 0}},
    // quarter tile (128 x 128): the wave's 64 x 32 part
    {64, 32, 3, 2, {0, 1, 0, 0, 0, 0, 0}, 2, {0, 1, 0, 0, 0, 0, 0, 0, 0}, {2, 2, 0, 0, 0, 0, 0, 0, 0}},
};

struct SymSquareArgs {
    const int8_t* X;
    int32_t* C;
    int64_t ldx, ldc, strideX, strideC;
    int k;  // rows of X (bytes of K per operand row), a multiple of the stage width
    int m;  // whole macro-tile rows: ld / 256 (rounded down)
    int rem;  // 1: ld is an odd multiple of 128 (a last unit row / column of quarter tiles)
    int T;  // channels
    const uint32_t* nonsym_flag;
};

constexpr int SYM_NT = 512;

template <int KB> struct SymCfg {
    static constexpr int NS = (KB == 64) ? 4 : 2;  // LDS ring stages (128 KiB either way)
    static constexpr int D = NS - 1;               // stages in flight ahead of the one being multiplied
    static constexpr int CH = KB / 16;             // 16-byte chunks per LDS row
    static constexpr int RPI = 1024 / KB;          // rows per DMA wave-instruction
    static constexpr int IPW = 256 / RPI / 8;      // DMA instructions per wave, operand panel and stage
    static constexpr int OPB = 256 * KB;           // bytes of one operand panel per stage
    static constexpr int STAGE = 2 * OPB;
    static constexpr int NQ = KB / 32;             // MFMA K-groups (32 bytes) per stage
};

// what a wave needs to walk K for one job
struct SymLane {
    unsigned lds0;  // LDS byte address of the ring
    int wave, lane, lane_off;  // lane_off: the lane's row inside a 32-row block, in bytes
};

// One job of one wave: ROLE_FULL = its part of a full macro-tile, ROLE_QUARTER = its part of a 128 x 128 "quarter" tile
// (the ragged last 128 rows / columns of a matrix whose order is an odd multiple of 128: panels of 128 rows, half the
// DMA instructions), ROLE 0..3 = nine blocks of a diagonal macro-tile (waves 0-3: the tile of panel A, waves 4-7: that
// of panel B).  Every wave of the workgroup passes the same nk + 1 barriers whatever its role.
template <int KB, int ROLE, bool LATE>
__device__ __forceinline__ void sym_job(const SymLane& L, const char* smem, const int8_t* pA, const int8_t* pB, int32_t* Cout, int64_t ldc,
                                        int nk, const int (&soff)[ROLE == ROLE_QUARTER ? 1 : SymCfg<KB>::IPW], const int (&coff)[SymCfg<KB>::NQ]) {
    typedef SymCfg<KB> CF;
    constexpr SymRole R = kSymRoles[ROLE];
    constexpr bool QUARTER = ROLE == ROLE_QUARTER;
    constexpr int NIS = QUARTER ? 1 : CF::IPW;  // DMA instructions per wave, panel and stage
    const int wave = L.wave;
    const int wi = wave & 1, wj = wave >> 1;
    I8Tile::acc_t acc[R.nacc];
#pragma unroll
    for (int t = 0; t < R.nacc; ++t)
#pragma unroll
        for (int r = 0; r < I8Tile::NR; ++r) acc[t][r] = 0;

    auto issue = [&](int slot, int kt) {
        const unsigned dst = L.lds0 + (unsigned)(slot * CF::STAGE + wave * NIS * 1024);
        const char* ga = reinterpret_cast<const char*>(pA) + (int64_t)kt * KB;
        const char* gb = reinterpret_cast<const char*>(pB) + (int64_t)kt * KB;
#pragma unroll
        for (int s = 0; s < NIS; ++s) {
            glds16(ga + soff[s], dst + s * 1024);
            glds16(gb + soff[s], dst + CF::OPB + s * 1024);
        }
    };
#pragma unroll
    for (int st = 0; st < CF::D; ++st)
        if (st < nk) issue(st, st);

    // fragments of one 32-byte K-group and the MFMAs on them
    typedef I8Tile::frag_t frag_t;
    auto load = [&](frag_t (&F)[R.nf], const char* sA, const char* sB, int q) {
        const char* rows = R.wrows ? sA + wi * R.wrows * KB : (wave < 4 ? sA : sB);
        const char* cols = sB + wj * R.wcols * KB;
#pragma unroll
        for (int x = 0; x < R.nf; ++x)
            F[x] = *reinterpret_cast<const frag_t*>((x < R.na ? rows : cols) + R.fr[x] * 32 * KB + L.lane_off + coff[q]);
    };
    auto mma = [&](const frag_t (&F)[R.nf]) {
#pragma unroll
        for (int t = 0; t < R.nacc; ++t) I8Tile::step(F[R.tc[t]], F[R.tr[t]], acc[t]);
    };

    // The two waves of a SIMD (w and w + 4) walk K half a stage apart: waves 4-7 ("late") keep the fragments of a
    // stage's last K-group in registers across the barrier and multiply them right behind it, while waves 0-3 wait for
    // their first reads of the new stage.
    constexpr bool late = LATE;
    frag_t Fc[R.nf];  // the late group's carried fragments
    for (int kt = 0; kt < nk; ++kt) {
        // stage kt has landed once at most the D - 1 younger stages of this wave are outstanding
        if (kt + CF::D - 1 < nk) {
            if constexpr (QUARTER) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // (D - 1) * 2 * NIS
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if constexpr (late) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the carried fragments are out of the ring
        __syncthreads();  // everybody's part of stage kt is in; nobody reads stage kt - 1 any more
        if (kt + CF::D < nk) issue((kt + CF::D) % CF::NS, kt + CF::D);
        const char* sA = smem + (kt % CF::NS) * CF::STAGE;
        const char* sB = sA + CF::OPB;
        if constexpr (!late) {
#pragma unroll
            for (int q = 0; q < CF::NQ; ++q) {
                frag_t F[R.nf];
                load(F, sA, sB, q);
                mma(F);
            }
        } else {
            if (kt > 0) mma(Fc);
#pragma unroll
            for (int q = 0; q < CF::NQ - 1; ++q) {
                frag_t F[R.nf];
                load(F, sA, sB, q);
                mma(F);
            }
            load(Fc, sA, sB, CF::NQ - 1);
        }
    }
    if constexpr (late) {
        if (nk > 0) mma(Fc);
    }
    __syncthreads();  // the ring is free for the next job's first stages

    if (!Cout) return;
#pragma unroll
    for (int t = 0; t < R.nacc; ++t)
        mfma_store<KIND_I8>(acc[t], Cout, ldc, wi * R.wrows + R.fr[R.tr[t]] * 32, wj * R.wcols + R.fr[R.tc[t]] * 32, L.lane);
}

template <int KB>
__global__ void __launch_bounds__(SYM_NT) i8_symsquare_kernel(SymSquareArgs a) {
    typedef SymCfg<KB> CF;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    SymLane L;
    L.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    L.lane = lane;
    L.lds0 = lds_address(smem);
    L.lane_off = I8Tile::row(lane) * KB;
    const int wave = L.wave;

    const bool sym = a.nonsym_flag && *a.nonsym_flag == 0u;  // uniform
    const int m = a.m, T = a.T;                 // m whole macro-tile rows; a.rem = 1: 128 more rows / columns
    const int tri = m * (m - 1) / 2;
    const int ndt = sym ? T * m : 0;            // diagonal macro-tiles ...
    const int ND = (ndt + 1) >> 1;              // ... two per job
    const int NF = sym ? T * tri : T * m * m;   // full macro-tiles
    const int nqc = a.rem ? (sym ? 2 * m + 1 : 4 * m + 1) : 0;  // quarter tiles per channel: the last unit row (+ column)
    const int NQ4 = T * nqc;
    const int NJ = NF + ND + NQ4;
    const int nk = a.k / KB;

    // DMA sources of this lane inside a panel (K offset excluded)
    int soff[CF::IPW];
#pragma unroll
    for (int s = 0; s < CF::IPW; ++s) {
        const int r = (wave * CF::IPW + s) * CF::RPI + lane / CF::CH;
        const int c = (lane % CF::CH) ^ dma_swz<KB>(r);
        soff[s] = r * (int)a.ldx + c * 16;
    }
    int soffq[1];  // quarter tiles: this wave's 16 rows of a 128-row panel
    {
        const int r = wave * CF::RPI + lane / CF::CH;
        soffq[0] = r * (int)a.ldx + ((lane % CF::CH) ^ dma_swz<KB>(r)) * 16;
    }
    // fragment reads: the lane's row of a 32-row block, its chunk of K-group q, un-swizzled
    int coff[CF::NQ];
#pragma unroll
    for (int q = 0; q < CF::NQ; ++q) coff[q] = (I8Tile::chunk(q, I8Tile::grp(lane)) ^ dma_swz<KB>(I8Tile::row(lane))) << 4;

    for (int job = blockIdx.x; job < NJ; job += gridDim.x) {
        if (job < NF) {
            const int f = xcd_run(job, NF);
            int c, I, J;
            if (sym) {
                c = f / tri;
                tri_decode(f - c * tri, I, J);  // strictly lower macro-tiles, row-major: (I, J), J < I, I = 1 .. m - 1
                ++I;
            } else {
                c = f / (m * m);
                const int t = f - c * m * m;
                J = t / m;
                I = t - J * m;
            }
            const int8_t* pA = a.X + (int64_t)c * a.strideX + (int64_t)I * 256 * a.ldx;
            const int8_t* pB = a.X + (int64_t)c * a.strideX + (int64_t)J * 256 * a.ldx;
            int32_t* cA = a.C + (int64_t)c * a.strideC + (int64_t)I * 256 + (int64_t)J * 256 * a.ldc;
            if (wave < 4) sym_job<KB, ROLE_FULL, false>(L, smem, pA, pB, cA, a.ldc, nk, soff, coff);
            else sym_job<KB, ROLE_FULL, true>(L, smem, pA, pB, cA, a.ldc, nk, soff, coff);
        } else if (job >= NF + ND) {
            // quarter tile of the ragged border: unit row 2 m x unit column u (u <= 2 m), or -- full squares only --
            // unit row u - (2 m + 1) x unit column 2 m
            const int q = job - NF - ND;
            const int c = q / nqc, u = q - c * nqc;
            const int ur = u <= 2 * m ? 2 * m : u - (2 * m + 1), uc = u <= 2 * m ? u : 2 * m;
            const int8_t* pA = a.X + (int64_t)c * a.strideX + (int64_t)ur * 128 * a.ldx;
            const int8_t* pB = a.X + (int64_t)c * a.strideX + (int64_t)uc * 128 * a.ldx;
            int32_t* cQ = a.C + (int64_t)c * a.strideC + (int64_t)ur * 128 + (int64_t)uc * 128 * a.ldc;
            if (wave < 4) sym_job<KB, ROLE_QUARTER, false>(L, smem, pA, pB, cQ, a.ldc, nk, soffq, coff);
            else sym_job<KB, ROLE_QUARTER, true>(L, smem, pA, pB, cQ, a.ldc, nk, soffq, coff);
        } else {
            const int d1 = 2 * (job - NF), d2 = d1 + 1;
            const int c1 = d1 / m, I1 = d1 - c1 * m;
            const int8_t* pA = a.X + (int64_t)c1 * a.strideX + (int64_t)I1 * 256 * a.ldx;
            int32_t* cA = a.C + (int64_t)c1 * a.strideC + (int64_t)I1 * 256 * (1 + a.ldc);
            const int8_t* pB = pA;
            int32_t* cB = nullptr;
            if (d2 < ndt) {
                const int c2 = d2 / m, I2 = d2 - c2 * m;
                pB = a.X + (int64_t)c2 * a.strideX + (int64_t)I2 * 256 * a.ldx;
                cB = a.C + (int64_t)c2 * a.strideC + (int64_t)I2 * 256 * (1 + a.ldc);
            }
            // waves 0-3: the tile of panel A, waves 4-7 (half a stage behind): that of panel B
            switch (wave) {
                case 0: sym_job<KB, 0, false>(L, smem, pA, pB, cA, a.ldc, nk, soff, coff); break;
                case 1: sym_job<KB, 1, false>(L, smem, pA, pB, cA, a.ldc, nk, soff, coff); break;
                case 2: sym_job<KB, 2, false>(L, smem, pA, pB, cA, a.ldc, nk, soff, coff); break;
                case 3: sym_job<KB, 3, false>(L, smem, pA, pB, cA, a.ldc, nk, soff, coff); break;
                case 4: sym_job<KB, 0, true>(L, smem, pA, pB, cB, a.ldc, nk, soff, coff); break;
                case 5: sym_job<KB, 1, true>(L, smem, pA, pB, cB, a.ldc, nk, soff, coff); break;
                case 6: sym_job<KB, 2, true>(L, smem, pA, pB, cB, a.ldc, nk, soff, coff); break;
                default: sym_job<KB, 3, true>(L, smem, pA, pB, cB, a.ldc, nk, soff, coff); break;
            }
        }
    }
}

bool gemm_sym_set_device_attributes() {
    bool ok = true;
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&i8_symsquare_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    return ok;
}

// Does the persistent launch pay for an n x n problem with T channels?  Its big jobs (lower-triangle macro-tiles of
// the whole 256-row part of the matrix, the diagonal ones two per job) come in rounds of one per CU, and a job is
// 35 - 40 us of work at N = 4096: the launch pays when the rounds are well filled (N = 4096, 2 channels: 256 jobs on 256
// CUs; N = 8192: 1024; N = 4104 -> ld 4224: the same 256 jobs plus 66 quarter tiles of the last 128 rows, a short
// second round).  A sparsely filled last round of big jobs or a small problem keeps the 128 x 128 tiles of
// kernels_gemm.hip, which spread over more CUs.
bool i8_symsquare_pays(int64_t n, int T, int num_cus) {
    if (num_cus < 1) return false;
    const int64_t m = ((n + 127) / 128 * 128) / 256;
    const int64_t jobs = (int64_t)T * m * (m - 1) / 2 + ((int64_t)T * m + 1) / 2;
    const int64_t rounds = (jobs + num_cus - 1) / num_cus;
    return 4 * jobs >= 3 * (int64_t)num_cus && 100 * jobs >= 85 * rounds * num_cus;
}

// true if the persistent kernel serves this launch (ld a multiple of 256, aligned operands)
bool launch_i8_symsquare(hipStream_t s, int64_t n, int64_t k, const int8_t* X, int64_t ldx, int32_t* C, int64_t ldc, int batch,
                         int64_t strideX, int64_t strideC, const uint32_t* nonsym_flag, int num_cus, int variant) {
    const bool forced = variant == 64;  // tests / measurements: the persistent launch at any size
    if (num_cus < 1 || !(forced || i8_symsquare_pays(n, batch, num_cus)) || n < 256 || (n % 128) != 0 || (k % 128) != 0 || (ldx % 16) != 0 || (strideX % 16) != 0 ||
        (reinterpret_cast<uintptr_t>(X) % 16) != 0 || n > 65536 || ldx > 65536)
        return false;
    SymSquareArgs a;
    a.X = X;
    a.C = C;
    a.ldx = ldx;
    a.ldc = ldc;
    a.strideX = strideX;
    a.strideC = strideC;
    a.k = (int)k;
    a.m = (int)(n / 256);
    a.rem = (n % 256) != 0 ? 1 : 0;
    a.T = batch;
    a.nonsym_flag = nonsym_flag;
    const int64_t jobs = (int64_t)batch * (a.m * a.m + (a.rem ? 4 * a.m + 1 : 0));  // upper bound (the full squares)
    const unsigned grid = (unsigned)std::min<int64_t>(jobs, num_cus);
    i8_symsquare_kernel<64><<<grid, SYM_NT, 128 * 1024, s>>>(a);
    return true;
}

}  // namespace sdpsr
