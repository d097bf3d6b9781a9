// The reduced PSD pencil Z_k(x) = sum_i x_i blks[i][k] and its adjoint g_i = sum_k <blks[i][k], S_k> from the triplets of
// sdpsr_block_images_sparse (sum(blkD.blks[i] .* x[i] for i = 1:dim(P)), docs/src/examples/ErdosRenyiThetaFunction.jl:83,
// QuadraticAssignmentProblems.jl:136, test/sd_problems.jl:46-52,127-134 of the reference).  blockop.cpp has the handle.
//
// The handle keeps the FULL entry list (an upper-triangle entry off the diagonal stands for two positions) as 16-byte records
// (key, idx, val) in two arrangements:
//   class-major     key = class, idx = position   -- the adjoint:  g[class]  = sum val * S[position]
//   position-major  key = position, idx = class   -- the forward:  Z[position] = sum val * x[class]
// A position is the flat index of (block, row, col) in the layout of one class of sdpsr_block_images.  Creation:
//   1. blockop_check_classptr_kernel, blockop_check_kernel: the validation (lowest offending index by an integer atomicMin on
//      the verdict words -- no atomic touches a position) and, per chunk of 1024 entries, the number of mirrored entries;
//   2. blockop_scan_kernel: the exclusive scan of those counts by one workgroup, and the full entry count;
//   3. blockop_expand_kernel: the class-major records, in input order with every mirror right behind its entry, and their positions;
//   4. the stable radix sort of (position, full index) (launch_radix_sort_pairs), blockop_gather_kernel: the position-major
//      records.  Stable: the entries of one position stay in class-major order.
// Both maps are then ONE kernel pair, the keyed sum y[key] = sum val * v[idx] over an arrangement sorted by key
// (blockop_keyed_sums_kernel + blockop_keyed_sums_carry_kernel), cut by position in the sorted array, never by key.
#include "host_internal.h"

namespace sdpsr {

namespace {

constexpr unsigned long long BO_NONE = ~0ull;
constexpr int BO_T = 256;
constexpr int BO_CHUNK = 1024;  // entries per workgroup of the creation passes: 4 rounds of 256

// class of entry e: classptr[i] <= e < classptr[i + 1] (classptr validated: monotone from 0 to nnz, d >= 1)
__device__ __forceinline__ uint32_t bo_class_of(const long long* __restrict__ classptr, int64_t d, int64_t e) {
    int64_t lo = 0, hi = d;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (classptr[mid] <= (long long)e) lo = mid; else hi = mid;
    }
    return (uint32_t)lo;
}

__device__ __forceinline__ unsigned long long bo_wave_min(unsigned long long m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_down(m, o, 64);
        m = y < m ? y : m;
    }
    return m;
}

__global__ void __launch_bounds__(BO_T)
blockop_check_classptr_kernel(int64_t d, int64_t nnz, const long long* __restrict__ classptr, unsigned long long* __restrict__ verdict) {
    unsigned long long bad = BO_NONE;
    for (int64_t i = (int64_t)blockIdx.x * BO_T + threadIdx.x; i <= d; i += (int64_t)gridDim.x * BO_T) {
        const long long a = classptr[i];
        if (i == 0 && a != 0) atomicMin(verdict + BOV_PTR0, 0ull);
        if (i == d && a != (long long)nnz) atomicMin(verdict + BOV_PTREND, 0ull);
        if (i < d && classptr[i + 1] < a && (unsigned long long)i < bad) bad = (unsigned long long)i;
    }
    bad = bo_wave_min(bad);
    if ((threadIdx.x & 63) == 0 && bad != BO_NONE) atomicMin(verdict + BOV_MONOTONE, bad);
}

// what an entry means: its block, row and column after the base, the verdict, and whether it has a mirror
struct BoEntry {
    int kind;  // 0 fine, 1 block outside [0, nb), 2 row / col outside [0, s), 3 row > col under UPPER
    uint32_t pos, mpos;
    bool mirror;
};
__device__ __forceinline__ BoEntry bo_entry(int64_t e, const int32_t* __restrict__ blk, const int32_t* __restrict__ row,
                                            const int32_t* __restrict__ col, int base, int upper, int nb, const uint32_t* __restrict__ pre,
                                            const int32_t* __restrict__ vs) {
    BoEntry r{0, 0u, 0u, false};
    const long long b = (long long)blk[e] - base;
    if (b < 0 || b >= nb) {
        r.kind = 1;
        return r;
    }
    const long long s = vs[b], i = (long long)row[e] - base, j = (long long)col[e] - base;
    if (i < 0 || i >= s || j < 0 || j >= s) {
        r.kind = 2;
        return r;
    }
    if (upper && i > j) {
        r.kind = 3;
        return r;
    }
    r.pos = pre[b] + (uint32_t)(i + j * s);
    r.mpos = pre[b] + (uint32_t)(j + i * s);
    r.mirror = upper && i != j;
    return r;
}

__global__ void __launch_bounds__(BO_T)
blockop_check_kernel(int64_t nnz, const int32_t* __restrict__ blk, const int32_t* __restrict__ row, const int32_t* __restrict__ col, int base,
                     int upper, int nb, const uint32_t* __restrict__ pre, const int32_t* __restrict__ vs,
                     unsigned long long* __restrict__ verdict, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wcnt[BO_T / 64];
    const int64_t e0 = (int64_t)blockIdx.x * BO_CHUNK;
    unsigned long long bad[3] = {BO_NONE, BO_NONE, BO_NONE};
    uint32_t mirrors = 0;
#pragma unroll
    for (int q = 0; q < BO_CHUNK / BO_T; ++q) {
        const int64_t e = e0 + q * BO_T + threadIdx.x;
        if (e >= nnz) continue;
        const BoEntry en = bo_entry(e, blk, row, col, base, upper, nb, pre, vs);
        if (en.kind && (unsigned long long)e < bad[en.kind - 1]) bad[en.kind - 1] = (unsigned long long)e;
        mirrors += en.mirror;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long m = bo_wave_min(bad[k]);
        if ((threadIdx.x & 63) == 0 && m != BO_NONE) atomicMin(verdict + BOV_BLOCK + k, m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mirrors += __shfl_down(mirrors, o, 64);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = mirrors;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// off[i] = cnt[0] + .. + cnt[i - 1] for i <= nchunks (64-bit), by one workgroup; verdict[BOV_TOTAL] = nnz + off[nchunks]
__global__ void __launch_bounds__(1024)
blockop_scan_kernel(int64_t nchunks, const uint32_t* __restrict__ cnt, long long* __restrict__ off, int64_t nnz,
                    unsigned long long* __restrict__ verdict) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < nchunks; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const long long x = i < nchunks ? (long long)cnt[i] : 0;
        long long incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        long long run = carry_s + incl - x;
        for (int k = 0; k < w; ++k) run += wsum[k];
        if (i < nchunks) off[i] = run;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = run + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        off[nchunks] = carry_s;
        verdict[BOV_TOTAL] = (unsigned long long)(nnz + carry_s);
    }
}

// the class-major records and their positions; full index of entry e = e + mirrors in front of it
__global__ void __launch_bounds__(BO_T)
blockop_expand_kernel(int64_t nnz, int64_t d, const long long* __restrict__ classptr, const int32_t* __restrict__ blk,
                      const int32_t* __restrict__ row, const int32_t* __restrict__ col, const double* __restrict__ val, int base, int upper,
                      int nb, const uint32_t* __restrict__ pre, const int32_t* __restrict__ vs, const long long* __restrict__ off,
                      uint4* __restrict__ rec, uint32_t* __restrict__ poskey) {
    __shared__ uint32_t wcnt[BO_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * BO_CHUNK;
    int64_t before = e0 + off[blockIdx.x];  // full index of the round's first entry
    for (int q = 0; q < BO_CHUNK / BO_T; ++q) {
        const int64_t e = e0 + q * BO_T + threadIdx.x;
        BoEntry en{0, 0u, 0u, false};
        if (e < nnz) en = bo_entry(e, blk, row, col, base, upper, nb, pre, vs);
        const unsigned long long bal = __ballot(en.mirror);
        if (lane == 0) wcnt[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t ex = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        for (int k = 0; k < w; ++k) ex += wcnt[k];
        const uint32_t round_total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (e < nnz) {
            const int64_t j = before + threadIdx.x + ex;
            const uint32_t cls = bo_class_of(classptr, d, e);
            const double v = val[e];
            const uint32_t lo = (uint32_t)__double2loint(v), hi = (uint32_t)__double2hiint(v);
            rec[j] = make_uint4(cls, en.pos, lo, hi);
            poskey[j] = en.pos;
            if (en.mirror) {
                rec[j + 1] = make_uint4(cls, en.mpos, lo, hi);
                poskey[j + 1] = en.mpos;
            }
        }
        before += BO_T + round_total;
        __syncthreads();  // wcnt is free again
    }
}

// position-major record p = the class-major record sidx[p] with key and idx exchanged
__global__ void __launch_bounds__(BO_T)
blockop_gather_kernel(int64_t n, const uint32_t* __restrict__ sidx, const uint4* __restrict__ rec, uint4* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * BO_T + threadIdx.x; p < n; p += (int64_t)gridDim.x * BO_T) {
        const uint4 r = rec[sidx[p]];
        out[p] = make_uint4(r.y, r.x, r.z, r.w);
    }
}

// What a wave leaves behind for the runs that cross the borders of its piece of the sorted array
struct BoCarry {
    long long head_o, tail_o;  // the run's key; -2: behind the end
    double head_x, tail_x;
    int single, pad;           // 1: the whole piece is one run (head only)
};

constexpr int BO_PIECE = 1024;        // sorted positions per wave: 16 tiles of 64
constexpr int BO_LDS_DOUBLES = 4096;  // the gathered vector is staged in LDS up to this length (32 KiB)

// y[key] = sum over the records of that key of val * v[idx]; the records are sorted by key, so a key's records are one RUN.
// SUMMATION ORDER of one run (a function of the arrangement alone, and every constant here is fixed): the array is cut into
// pieces of 1024 records, a piece into tiles of 64.  Inside a tile the run's terms are added by the segmented Hillis-Steele
// scan over the 64 lanes (six shuffle steps, partners at distance 1, 2, .., 32 inside the run); the tiles of a piece are added
// left to right onto the first, (((t0 + t1) + t2) + ..); the pieces of a run are added left to right in the same way by
// blockop_keyed_sums_carry_kernel.  A wave takes pieces blockIdx * 4 + wave, + 4 * gridDim, ..: which wave owns a piece does not
// enter, every partial sum has one owner and one slot.  A run that begins and ends inside one piece is stored here; the others
// leave their partial sums in carry[piece].  The caller has zeroed y: a key without a record keeps its +0.0.
// One 16-byte load per record; v (x: d doubles, S: sum s'_k^2 doubles) is read at random -- from LDS when it fits, else
// from global memory, where it stays in L2 behind the stream of records that is read once.
template <bool LDSV>
__global__ void __launch_bounds__(BO_T)
blockop_keyed_sums_kernel(int64_t n, const uint4* __restrict__ rec, const double* __restrict__ v, int nv, BoCarry* __restrict__ carry,
                          double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double sv[];
    if (LDSV) {
        for (int i = threadIdx.x; i < nv; i += BO_T) sv[i] = v[i];
        __syncthreads();
    }
    const double* vv = LDSV ? sv : v;
    const int lane = threadIdx.x & 63;
    const int64_t npieces = (n + BO_PIECE - 1) / BO_PIECE;
    for (int64_t piece = (int64_t)blockIdx.x * (BO_T / 64) + (threadIdx.x >> 6); piece < npieces; piece += (int64_t)gridDim.x * (BO_T / 64)) {
        const int64_t p0 = piece * BO_PIECE;
        // the open run: the one the previous tile ended in (wave-uniform)
        long long cur_o = 0;
        double cur_x = 0.0;
        bool boundary_seen = false;  // some run of this piece has ended: the open run is no longer the head
        for (int t = 0; t < BO_PIECE / 64 && p0 + t * 64 < n; ++t) {
            const int64_t p = p0 + t * 64 + lane;
            long long o = -2;
            double x = 0.0;
            if (p < n) {
                const uint4 r = rec[p];
                o = (long long)r.x;
                x = __hiloint2double((int)r.w, (int)r.z) * vv[r.y];
            }
            // inclusive sums inside the runs of the tile (equal o at distance k means one run: runs are contiguous)
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const double y = __shfl_up(x, k, 64);
                const long long oy = __shfl_up(o, k, 64);
                if (lane >= k && oy == o) x += y;
            }
            const long long first_o = __shfl(o, 0, 64);
            const long long next_o = __shfl_down(o, 1, 64);
            const bool continues = t > 0 && first_o == cur_o;  // the open run goes on in this tile
            if (t > 0 && !continues) {                         // it ended exactly at the tile border
                if (lane == 0) {
                    if (!boundary_seen) {
                        carry[piece].head_o = cur_o;
                        carry[piece].head_x = cur_x;
                    } else if (cur_o >= 0) {
                        out[cur_o] = cur_x;
                    }
                }
                boundary_seen = true;
            }
            const bool in_first = o == first_o;
            const double total = (continues && in_first) ? cur_x + x : x;
            const bool ends_here = lane < 63 && next_o != o;  // a run that ends inside the tile
            if (ends_here) {
                if (in_first && !boundary_seen) {
                    carry[piece].head_o = o;
                    carry[piece].head_x = total;
                } else if (o >= 0) {
                    out[o] = total;
                }
            }
            if (__ballot(ends_here) != 0ull) boundary_seen = true;
            cur_o = __shfl(o, 63, 64);
            cur_x = __shfl(total, 63, 64);
        }
        if (lane == 0) {
            if (!boundary_seen) {
                carry[piece].head_o = cur_o;
                carry[piece].head_x = cur_x;
                carry[piece].tail_o = cur_o;
                carry[piece].tail_x = 0.0;
                carry[piece].single = 1;
            } else {
                carry[piece].tail_o = cur_o;
                carry[piece].tail_x = cur_x;
                carry[piece].single = 0;
            }
        }
    }
}

// The runs that cross piece borders: thread w owns the run that BEGINS in piece w and leaves it (at most one: the piece's
// tail, or the piece itself when it is one run that begins at its first position), adds the heads of the following pieces
// left to right while the run goes on, and stores the sum.  A head whose run begins at the first position of a piece that
// holds further runs is complete and stored as it is.  One thread per run, a serial walk: a run of k pieces costs k
// dependent reads (k <= n / 1024, reached only when one key holds nearly every record).
__global__ void __launch_bounds__(256)
blockop_keyed_sums_carry_kernel(int64_t npieces, const BoCarry* __restrict__ carry, double* __restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= npieces) return;
    const BoCarry me = carry[w];
    bool head_begins = true;  // the head's run begins at the first position of piece w
    if (w > 0) {
        const BoCarry prev = carry[w - 1];
        head_begins = (prev.single ? prev.head_o : prev.tail_o) != me.head_o;
    }
    long long o;
    double acc;
    if (me.single) {
        if (!head_begins) return;  // a middle piece of somebody else's run
        o = me.head_o;
        acc = me.head_x;
    } else {
        if (head_begins && me.head_o >= 0) out[me.head_o] = me.head_x;
        o = me.tail_o;
        acc = me.tail_x;
    }
    if (o < 0) return;
    for (int64_t u = w + 1; u < npieces; ++u) {
        const BoCarry nx = carry[u];
        if (nx.head_o != o) break;
        acc += nx.head_x;
        if (!nx.single) break;
    }
    out[o] = acc;
}

}  // namespace

void launch_blockop_check_classptr(hipStream_t s, int64_t d, int64_t nnz, const int64_t* classptr, unsigned long long* verdict) {
    const unsigned grid = (unsigned)std::min<int64_t>((d + 1 + BO_T - 1) / BO_T, 2048);
    blockop_check_classptr_kernel<<<grid, BO_T, 0, s>>>(d, nnz, (const long long*)classptr, verdict);
}

int64_t blockop_chunks(int64_t nnz) { return (nnz + BO_CHUNK - 1) / BO_CHUNK; }

void launch_blockop_check(hipStream_t s, int64_t nnz, const int32_t* blk, const int32_t* row, const int32_t* col, int base, int upper, int nb,
                          const uint32_t* pre, const int32_t* vs, unsigned long long* verdict, uint32_t* cnt, int64_t* off) {
    const int64_t G = blockop_chunks(nnz);
    blockop_check_kernel<<<(unsigned)G, BO_T, 0, s>>>(nnz, blk, row, col, base, upper, nb, pre, vs, verdict, cnt);
    blockop_scan_kernel<<<1, 1024, 0, s>>>(G, cnt, (long long*)off, nnz, verdict);
}

void launch_blockop_expand(hipStream_t s, int64_t nnz, int64_t d, const int64_t* classptr, const int32_t* blk, const int32_t* row,
                           const int32_t* col, const double* val, int base, int upper, int nb, const uint32_t* pre, const int32_t* vs,
                           const int64_t* off, void* rec, uint32_t* poskey) {
    blockop_expand_kernel<<<(unsigned)blockop_chunks(nnz), BO_T, 0, s>>>(nnz, d, (const long long*)classptr, blk, row, col, val, base, upper, nb,
                                                                         pre, vs, (const long long*)off, (uint4*)rec, poskey);
}

void launch_blockop_gather(hipStream_t s, int64_t n, const uint32_t* sidx, const void* rec, void* out) {
    const unsigned grid = (unsigned)std::min<int64_t>((n + BO_T - 1) / BO_T, 8192);
    blockop_gather_kernel<<<grid, BO_T, 0, s>>>(n, sidx, (const uint4*)rec, (uint4*)out);
}

size_t blockop_carry_bytes(int64_t n) { return (size_t)((n + BO_PIECE - 1) / BO_PIECE) * sizeof(BoCarry); }

// out (zeroed by the caller) [key] = sum val * v[idx] over the n records sorted by key; nv = length of v
void launch_blockop_keyed_sums(hipStream_t s, int64_t n, const void* rec, const double* v, int64_t nv, void* carry, double* out) {
    if (n <= 0) return;
    const int64_t npieces = (n + BO_PIECE - 1) / BO_PIECE;
    const int64_t per_block = BO_T / 64;
    const unsigned grid = (unsigned)std::min<int64_t>((npieces + per_block - 1) / per_block, 2048);
    if (nv <= BO_LDS_DOUBLES)
        blockop_keyed_sums_kernel<true><<<grid, BO_T, (size_t)nv * 8, s>>>(n, (const uint4*)rec, v, (int)nv, (BoCarry*)carry, out);
    else
        blockop_keyed_sums_kernel<false><<<grid, BO_T, 0, s>>>(n, (const uint4*)rec, v, 0, (BoCarry*)carry, out);
    blockop_keyed_sums_carry_kernel<<<(unsigned)((npieces + 255) / 256), 256, 0, s>>>(npieces, (const BoCarry*)carry, out);
}

}  // namespace sdpsr
