// Block images as solver triplets (sdpsr_block_images_sparse, sparse_images.cpp): an order-preserving compaction of a window
// of dense block images -- the layout sdpsr_basis_image / sdpsr_block_images write -- into (block, row, col, value) entries
// with a per-class pointer array, as JuMP's PSDCone expressions and SDPA-sparse files take them (README.md:72-79,
// docs/src/examples/ReduceAndSolveJuMP.jl:56-84 of the reference).
//
// The VIRTUAL matrices.  Real input: block k of a class as it stands, order s'_k = s_k.  Complex input: the real embedding
// [Re -Im; Im Re] of order s'_k = 2 s_k (ReduceAndSolveJuMP.jl:59-76).  A class has V = sum s'_k^2 virtual elements, the window
// N = class_count * V of them, and the FLAT VIRTUAL INDEX g = class * V + (prefix of block k) + col * s'_k + row is the scan
// order the output keeps: class, block, column-major inside the block.
//
// Two sweeps over fixed chunks of the flat range -- never per class: 18 classes of 18 elements and 3479 classes of 55 000 are
// both real shapes.  One wave owns one chunk of SI_CHUNK consecutive g; a step of the wave covers 128 of them, lane l the pair
// (2l, 2l + 1), so a ballot's bit order IS the scan order.
//   sweep 1  cnt[chunk] = kept elements of the chunk (and the optional asymmetry maximum: non-negative doubles order as their
//            bit patterns do, so an integer atomic max is independent of the order it is applied in)
//   scan     off = exclusive int64 prefix of cnt, one workgroup, any length; off[nchunks] = nnz
//   sweep 2  evaluates the same predicate again; a kept element goes to off[chunk] + (kept in the wave's earlier steps) +
//            (kept in lower lanes of this step: popcount of the ballots below the lane).  The first element of every class --
//            kept or not -- stores that same position into classptr[class]: classes that end inside a chunk and runs of
//            classes with no entry at all need nothing else.
// No atomics decide a position, nothing is sorted: the output is a function of the input alone, on any grid.
// Loads: a real window is read in 16-byte pairs.  The caller's pointer may be 8 mod 16 (a window that starts at an odd element
// of a larger buffer); the chunks then start one element early (head = 1) so that every pair stays 16-byte aligned, and the
// two pairs that straddle the window's ends are read element by element.  The embedding reads the one component it needs of
// each complex number (8 bytes at stride 16).  Stores are plain vector stores.
// Flat index -> (block, row, col): the prefix table of s'_k^2 and the orders s'_k sit in LDS up to SI_LDS_BLOCKS blocks (in
// global memory beyond), searched by bisection -- hundreds of 1 x 1 blocks are a real shape.
#include "host_internal.h"
#include "sparse_images.h"

namespace sdpsr {

namespace {

constexpr int SI_STEP = 128;  // elements per wave step: 64 lanes x 2
constexpr int SI_WAVES = 4;   // waves (chunks in flight) per workgroup

struct ClassPos {
    int64_t cls;  // class of the window, 0-based
    int64_t rr;   // virtual index inside the class
};

struct BlockPos {
    int32_t k, row, col, order;  // block, position in the virtual block, s'_k
    int64_t pre;                 // prefix of s'^2 in front of block k
};

// (class, index in class) of the element dx >= 0 behind one whose class is cls0 and index in class r0
__device__ __forceinline__ ClassPos si_class_of(int64_t cls0, int64_t r0, int64_t dx, int64_t V) {
    const int64_t x = r0 + dx;  // dx < SI_CHUNK + 1
    if (x < V) return {cls0, x};
    if (V <= 0x7FFFFFFFll) {  // x < V + SI_CHUNK + 1 < 2^32
        const uint32_t xx = (uint32_t)x, vv = (uint32_t)V, q = xx / vv;
        return {cls0 + q, (int64_t)(xx - q * vv)};
    }
    return {cls0 + 1, x - V};  // V > SI_CHUNK: one class boundary per chunk at the most
}

__device__ __forceinline__ BlockPos si_block_of(int64_t rr, int nb, const int64_t* pre, const int32_t* vs) {
    int lo = 0, hi = nb;  // pre[lo] <= rr < pre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= rr) lo = mid;
        else hi = mid;
    }
    const int64_t p = pre[lo], o = rr - p;
    const int32_t sp = vs[lo];
    int32_t col;
    if ((uint64_t)o >> 32) col = (int32_t)(o / sp);
    else col = (int32_t)((uint32_t)o / (uint32_t)sp);
    return {lo, (int32_t)(o - (int64_t)col * sp), col, sp, p};
}

// element (row, col) of virtual block b of class cls
template <bool CX>
__device__ __forceinline__ double si_virtual(const SparseImagesArgs& a, int64_t cls, const BlockPos& b, int32_t row, int32_t col) {
    if (!CX) return a.blks[cls * a.S + b.pre + (int64_t)col * b.order + row];
    const int32_t s = b.order >> 1;
    const bool top = row < s, left = col < s;
    const int64_t z = cls * a.S + (b.pre >> 2) + (int64_t)(left ? col : col - s) * s + (top ? row : row - s);
    if (top == left) return a.blks[2 * z];
    const double im = a.blks[2 * z + 1];
    return top ? -im : im;
}

__device__ __forceinline__ bool si_kept(double v, double tol) { return !(fabs(v) <= tol); }

// the block table: LDS copy (dynamic shared memory) when it fits, else the global arrays
struct Table {
    const int64_t* pre;
    const int32_t* vs;
};
__device__ __forceinline__ Table si_table(const SparseImagesArgs& a, unsigned char* smem) {
    if (a.nb > SI_LDS_BLOCKS) return {a.pre, a.vs};
    int64_t* p = reinterpret_cast<int64_t*>(smem);
    int32_t* v = reinterpret_cast<int32_t*>(p + a.nb + 1);
    for (int i = threadIdx.x; i <= a.nb; i += blockDim.x) p[i] = a.pre[i];
    for (int i = threadIdx.x; i < a.nb; i += blockDim.x) v[i] = a.vs[i];
    __syncthreads();
    return {p, v};
}

// One step of a wave over the chunk that starts at flat index gb (may be -1: head): this lane's pair (g, g + 1), their values
// and validity.  Real input: one aligned 16-byte load when both lie inside the window.
template <bool CX>
__device__ __forceinline__ void si_load_real_pair(const SparseImagesArgs& a, int64_t g, bool ok0, bool ok1, double& v0, double& v1) {
    v0 = 0.0;
    v1 = 0.0;
    if (CX) return;
    if (ok0 && ok1) {
        const double2 p = *reinterpret_cast<const double2*>(a.blks + g);  // 16-byte aligned by the choice of head
        v0 = p.x;
        v1 = p.y;
    } else {
        if (ok0) v0 = a.blks[g];
        if (ok1) v1 = a.blks[g + 1];
    }
}

template <bool CX, bool ASYM>
__global__ void __launch_bounds__(64 * SI_WAVES)
sparse_images_count_kernel(SparseImagesArgs a, uint32_t* __restrict__ cnt, unsigned long long* __restrict__ asym) {
    extern __shared__ __align__(16) unsigned char si_smem[];
    const Table tb = si_table(a, si_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool decode = CX || ASYM || a.upper;
    double amax = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * SI_WAVES + wave; c < a.nchunks; c += (int64_t)gridDim.x * SI_WAVES) {
        const int64_t gb = c * SI_CHUNK - a.head, gq = gb < 0 ? 0 : gb;
        const int64_t cls0 = gq / a.V, r0 = gq - cls0 * a.V;
        uint32_t count = 0;
#pragma unroll 2
        for (int st = 0; st < SI_CHUNK / SI_STEP; ++st) {
            if (gb + st * SI_STEP >= a.N) break;  // wave-uniform
            const int64_t g = gb + st * SI_STEP + 2 * lane;
            const bool ok[2] = {g >= 0 && g < a.N, g + 1 < a.N};
            double v[2];
            si_load_real_pair<CX>(a, g, ok[0], ok[1], v[0], v[1]);
            bool keep[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                keep[j] = false;
                if (!ok[j]) continue;
                bool tri = true;
                if (decode) {
                    const ClassPos cp = si_class_of(cls0, r0, g + j - gq, a.V);
                    const BlockPos b = si_block_of(cp.rr, a.nb, tb.pre, tb.vs);
                    if (CX) v[j] = si_virtual<true>(a, cp.cls, b, b.row, b.col);
                    tri = !a.upper || b.row <= b.col;
                    if (ASYM && b.row < b.col) {
                        const double w = si_virtual<CX>(a, cp.cls, b, b.col, b.row);
                        const double dlt = fabs(v[j] - w);
                        if (dlt > amax) amax = dlt;
                    }
                }
                keep[j] = tri && si_kept(v[j], a.tol);
            }
            count += (uint32_t)__popcll(__ballot(keep[0])) + (uint32_t)__popcll(__ballot(keep[1]));
        }
        if (lane == 0) cnt[c] = count;
    }
    if (ASYM) {
        for (int d = 32; d >= 1; d >>= 1) {
            const double o = __shfl_xor(amax, d);
            if (o > amax) amax = o;
        }
        if (lane == 0 && amax > 0.0) atomicMax(asym, (unsigned long long)__double_as_longlong(amax));
    }
}

// off[0 .. n] = exclusive prefix of cnt[0 .. n), *total = off[n].  One workgroup of 1024, 4096 counts per round, any n.
__global__ void __launch_bounds__(1024)
sparse_images_scan_kernel(int64_t n, const uint32_t* __restrict__ cnt, int64_t* __restrict__ off, int64_t* __restrict__ total,
                          int64_t* __restrict__ total2) {
    __shared__ int64_t wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += 4096) {
        const int64_t i = base + 4 * (int64_t)tid;
        uint32_t cv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = i + j < n ? cnt[i + j] : 0u;
        const int64_t t = (int64_t)cv[0] + cv[1] + cv[2] + cv[3];
        int64_t incl = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int64_t woff = 0, all = 0;
        for (int w = 0; w < 16; ++w) {
            const int64_t x = wsum[w];
            if (w < wave) woff += x;
            all += x;
        }
        int64_t e = carry + woff + incl - t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < n) off[i + j] = e;
            e += cv[j];
        }
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        off[n] = carry;
        *total = carry;
        if (total2) *total2 = carry;
    }
}

// store == 0 (more entries than the caller's capacity): classptr only, and only the chunks that hold the first element of a class
template <bool CX>
__global__ void __launch_bounds__(64 * SI_WAVES)
sparse_images_fill_kernel(SparseImagesArgs a, const int64_t* __restrict__ off, int store, int64_t cap, int64_t* __restrict__ classptr,
                          int32_t* __restrict__ blk, int32_t* __restrict__ row, int32_t* __restrict__ col, double* __restrict__ val) {
    extern __shared__ __align__(16) unsigned char si_smem[];
    const Table tb = si_table(a, si_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t c = (int64_t)blockIdx.x * SI_WAVES + wave; c < a.nchunks; c += (int64_t)gridDim.x * SI_WAVES) {
        const int64_t gb = c * SI_CHUNK - a.head, gq = gb < 0 ? 0 : gb;
        const int64_t cls0 = gq / a.V, r0 = gq - cls0 * a.V;
        if (!store) {
            const int64_t next_start = r0 == 0 ? gq : gq + (a.V - r0);  // first class start at or behind gq
            if (next_start >= gb + SI_CHUNK || next_start >= a.N) continue;
        }
        int64_t pos = off[c];
#pragma unroll 2
        for (int st = 0; st < SI_CHUNK / SI_STEP; ++st) {
            if (gb + st * SI_STEP >= a.N) break;  // wave-uniform
            const int64_t g = gb + st * SI_STEP + 2 * lane;
            const bool ok[2] = {g >= 0 && g < a.N, g + 1 < a.N};
            double v[2];
            si_load_real_pair<CX>(a, g, ok[0], ok[1], v[0], v[1]);
            bool keep[2], start[2] = {false, false};
            ClassPos cp[2];
            BlockPos b[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                keep[j] = false;
                if (!ok[j]) continue;
                cp[j] = si_class_of(cls0, r0, g + j - gq, a.V);
                start[j] = cp[j].rr == 0;
                bool tri = true, located = false;
                if (CX || a.upper) {
                    b[j] = si_block_of(cp[j].rr, a.nb, tb.pre, tb.vs);
                    located = true;
                    if (CX) v[j] = si_virtual<true>(a, cp[j].cls, b[j], b[j].row, b[j].col);
                    tri = !a.upper || b[j].row <= b[j].col;
                }
                keep[j] = tri && si_kept(v[j], a.tol);
                if (keep[j] && store && !located) b[j] = si_block_of(cp[j].rr, a.nb, tb.pre, tb.vs);
            }
            const unsigned long long m0 = __ballot(keep[0]), m1 = __ballot(keep[1]);
            int64_t p[2];
            p[0] = pos + __popcll(m0 & below) + __popcll(m1 & below);
            p[1] = p[0] + (keep[0] ? 1 : 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (start[j]) classptr[cp[j].cls] = p[j];
                if (store && keep[j] && p[j] < cap) {
                    blk[p[j]] = b[j].k + a.base;
                    row[p[j]] = b[j].row + a.base;
                    col[p[j]] = b[j].col + a.base;
                    val[p[j]] = v[j];
                }
            }
            pos += __popcll(m0) + __popcll(m1);
        }
    }
}

int si_grid(const SparseImagesArgs& a, int num_cus) {
    const int64_t want = (a.nchunks + SI_WAVES - 1) / SI_WAVES, cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
    return (int)std::max<int64_t>(1, std::min(want, cap));
}

size_t si_lds_bytes(const SparseImagesArgs& a) { return a.nb > SI_LDS_BLOCKS ? 0 : (size_t)(a.nb + 1) * 8 + (size_t)a.nb * 4; }

}  // namespace

void launch_sparse_images_count(hipStream_t s, const SparseImagesArgs& a, int is_complex, uint32_t* cnt, unsigned long long* asym, int num_cus) {
    const dim3 grid(si_grid(a, num_cus)), block(64 * SI_WAVES);
    const size_t lds = si_lds_bytes(a);
    if (is_complex) {
        if (asym) hipLaunchKernelGGL((sparse_images_count_kernel<true, true>), grid, block, lds, s, a, cnt, asym);
        else hipLaunchKernelGGL((sparse_images_count_kernel<true, false>), grid, block, lds, s, a, cnt, asym);
    } else {
        if (asym) hipLaunchKernelGGL((sparse_images_count_kernel<false, true>), grid, block, lds, s, a, cnt, asym);
        else hipLaunchKernelGGL((sparse_images_count_kernel<false, false>), grid, block, lds, s, a, cnt, asym);
    }
}

void launch_sparse_images_scan(hipStream_t s, int64_t nchunks, const uint32_t* cnt, int64_t* off, int64_t* total, int64_t* total2) {
    hipLaunchKernelGGL(sparse_images_scan_kernel, dim3(1), dim3(1024), 0, s, nchunks, cnt, off, total, total2);
}

void launch_sparse_images_fill(hipStream_t s, const SparseImagesArgs& a, int is_complex, const int64_t* off, int store, int64_t cap,
                               int64_t* classptr, int32_t* blk, int32_t* row, int32_t* col, double* val, int num_cus) {
    const dim3 grid(si_grid(a, num_cus)), block(64 * SI_WAVES);
    const size_t lds = si_lds_bytes(a);
    if (is_complex) hipLaunchKernelGGL((sparse_images_fill_kernel<true>), grid, block, lds, s, a, off, store, cap, classptr, blk, row, col, val);
    else hipLaunchKernelGGL((sparse_images_fill_kernel<false>), grid, block, lds, s, a, off, store, cap, classptr, blk, row, col, val);
}

}  // namespace sdpsr
