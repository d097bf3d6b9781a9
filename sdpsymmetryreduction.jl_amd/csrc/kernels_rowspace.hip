// Kernels of sdpsr_compress_constraints (rowspace.cpp): an orthonormal basis of the row space of M = [newA | b]
// (docs/src/examples/ReduceAndSolveJuMP.jl:44-50: svd(M').U[:, 1:rank(M)]').  M is m x ncols, column-major with leading
// dimension m, m <= 1024 and ncols long: every kernel walks columns, a column is m contiguous doubles.
//   rowspace_absmax / rowspace_scale_copy   W = M * 2^-e, e the exponent of max |M| (no square overflows); non-finite flag
//   rowspace_gram / rowspace_gram_reduce    G = W W' on the fp64 matrix cores, K split over waves, partials summed in z order
//   rowspace_rotate                          W <- J W in place, a chunk of columns per workgroup staged in LDS
//   rowspace_lead / rowspace_write           sign of each kept row, then out = permuted, normalised, dropped rows; nnz
// Every sum has an order fixed by (m, ncols); the only atomic is the integer count of non-zeros.
#include <cfloat>

#include "host_internal.h"

namespace sdpsr {

namespace {

typedef double rs_v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double rs_entry(int64_t e, int64_t md, const double* __restrict__ A, const double* __restrict__ b) {
    return e < md ? A[e] : b[e - md];
}

// pmax[block] = max |M[e]| over the block's entries (0 for none); flag[0] = 1 if an entry is not finite
__global__ void __launch_bounds__(256)
rowspace_absmax_kernel(int64_t total, int64_t md, const double* __restrict__ A, const double* __restrict__ b,
                       double* __restrict__ pmax, uint32_t* __restrict__ flag) {
    __shared__ double smax[256];
    __shared__ uint32_t sbad[256];
    double mx = 0.0;
    uint32_t bad = 0;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        const double a = fabs(rs_entry(e, md, A, b));
        if (!(a <= DBL_MAX)) bad = 1;  // Inf and NaN
        else if (a > mx) mx = a;
    }
    smax[threadIdx.x] = mx;
    sbad[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]);
            sbad[threadIdx.x] |= sbad[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pmax[blockIdx.x] = smax[0];
        if (sbad[0]) flag[0] = 1;  // (every writer stores the same word)
    }
}

// the power of two that brings mx into [0.5, 1): shared by the kernel below and the host (rowspace.cpp)
__host__ __device__ inline double rowspace_scale_of(double mx) {
    if (!(mx > 0.0)) return 1.0;
    int e;
    (void)frexp(mx, &e);
    e = -e;
    if (e > 1000) e = 1000;  // (denormal input: stay inside the exponent range)
    return ldexp(1.0, e);
}

// W[e] = M[e] * scale; info[0] = max |M|, info[1] = 1.0 if an entry is not finite -- and then W is NOT written
__global__ void __launch_bounds__(256)
rowspace_scale_copy_kernel(int64_t total, int64_t md, const double* __restrict__ A, const double* __restrict__ b,
                           const double* __restrict__ pmax, int nblk, const uint32_t* __restrict__ flag,
                           double* __restrict__ W, double* __restrict__ info) {
    __shared__ double smax[256];
    double mx = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) mx = fmax(mx, pmax[i]);
    smax[threadIdx.x] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]);
        __syncthreads();
    }
    mx = smax[0];
    const bool bad = flag[0] != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = mx;
        info[1] = bad ? 1.0 : 0.0;
    }
    if (bad) return;
    const double scale = rowspace_scale_of(mx);
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += step) W[e] = rs_entry(e, md, A, b) * scale;
}

// block pair `pair` of the lower triangle -> (bp, bq), bq <= bp
__device__ __forceinline__ void rs_pair(int pair, int* bp, int* bq) {
    int p = 0;
    while ((p + 1) * (p + 2) / 2 <= pair) ++p;
    *bp = p;
    *bq = pair - p * (p + 1) / 2;
}

// One WAVE = one (block pair, K split z): the 64 x 64 block G[bp, bq] of W W' over the columns [z cps, (z + 1) cps).
// v_mfma_f64_16x16x4_f64 takes one double per lane from each operand, row lane & 15 at k = lane >> 4: four columns of W,
// sixteen rows each, read where they lie (16 contiguous doubles per quarter wave) -- no transposed copy, no LDS.  Rows >= m
// and columns >= the split's end enter as zeros.  D[i][j]: i = (lane >> 4) + 4 reg from the FIRST operand's tile, j = lane & 15
// from the second's.  Partials: P[((z * npairs + pair) * 64 + i) * 64 + j].
__global__ void __launch_bounds__(256)
rowspace_gram_kernel(int m, int64_t ncols, const double* __restrict__ W, int Z, int64_t cps, int npairs, double* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int z = blockIdx.y * 4 + wave;
    if (z >= Z) return;
    int bp, bq;
    rs_pair(blockIdx.x, &bp, &bq);
    const int r16 = lane & 15, kq = lane >> 4;
    const int64_t c_begin = (int64_t)z * cps;
    const int64_t c_end = c_begin + cps < ncols ? c_begin + cps : ncols;
    int rp[4], rq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        rp[t] = bp * 64 + t * 16 + r16;
        rq[t] = bq * 64 + t * 16 + r16;
    }
    rs_v4d acc[4][4];
#pragma unroll
    for (int tp = 0; tp < 4; ++tp)
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) acc[tp][tq] = rs_v4d{0.0, 0.0, 0.0, 0.0};
    const bool diag = bp == bq;  // uniform
    // tiles of 16 rows that hold a row < m (uniform): the others would multiply zeros -- their accumulators stay 0.0
    const int ntp = m - bp * 64 >= 64 ? 4 : (m - bp * 64 + 15) / 16, ntq = m - bq * 64 >= 64 ? 4 : (m - bq * 64 + 15) / 16;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += 4) {
        const int64_t c = c0 + kq;
        const bool cv = c < c_end;
        const double* col = W + (cv ? c : c_begin) * (int64_t)m;  // (an address inside W either way)
        double x[4], y[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = (cv && rp[t] < m) ? col[rp[t]] : 0.0;
        if (diag) {
#pragma unroll
            for (int t = 0; t < 4; ++t) y[t] = x[t];
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) y[t] = (cv && rq[t] < m) ? col[rq[t]] : 0.0;
        }
#pragma unroll
        for (int tp = 0; tp < 4; ++tp)
#pragma unroll
            for (int tq = 0; tq < 4; ++tq)
                if (tp < ntp && tq < ntq) acc[tp][tq] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[tp], y[tq], acc[tp][tq], 0, 0, 0);
    }
    double* p = P + ((int64_t)z * npairs + blockIdx.x) * 4096;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp)
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
#pragma unroll
            for (int v = 0; v < 4; ++v) p[(tp * 16 + kq + 4 * v) * 64 + tq * 16 + r16] = acc[tp][tq][v];
}

// G[p, q] = G[q, p] = sum_z P[z][pair][i][j], z ascending; one thread per entry of the lower triangle's blocks
__global__ void __launch_bounds__(256)
rowspace_gram_reduce_kernel(int m, int Z, int npairs, const double* __restrict__ P, double* __restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (pair, i, j)
    if (e >= (int64_t)npairs * 4096) return;
    const int pair = (int)(e >> 12), i = (int)(e >> 6) & 63, j = (int)e & 63;
    int bp, bq;
    rs_pair(pair, &bp, &bq);
    const int p = bp * 64 + i, q = bq * 64 + j;
    if (p >= m || q >= m || q > p) return;
    double acc = 0.0;
    for (int z = 0; z < Z; ++z) acc += P[(int64_t)z * npairs * 4096 + e];
    G[p + (int64_t)q * m] = acc;
    G[q + (int64_t)p * m] = acc;
}

// W[:, c] <- J W[:, c] for the workgroup's cc columns: the columns are staged in LDS (so the update is in place), J
// (column-major, J[i + k m]) sits in LDS too when j_lds, and comes through the caches otherwise.  Thread <-> row i of four
// columns: consecutive threads read consecutive J[i + k m] and four broadcast W values.  sum over k ascending.
__global__ void __launch_bounds__(256)
rowspace_rotate_kernel(int m, int64_t ncols, int cc, int j_lds, const double* __restrict__ J, double* __restrict__ W) {
    extern __shared__ double rs_smem[];
    double* sW = rs_smem;                  // cc columns of m
    double* sJ = rs_smem + (size_t)cc * m;  // m x m (j_lds)
    const int64_t c0 = (int64_t)blockIdx.x * cc;
    const int nc = (int)(ncols - c0 < cc ? ncols - c0 : cc);
    const int cnt = nc * m;
    double* Wc = W + c0 * m;
    for (int o = threadIdx.x; o < cnt; o += 256) sW[o] = Wc[o];
    if (j_lds)
        for (int o = threadIdx.x; o < m * m; o += 256) sJ[o] = J[o];
    __syncthreads();
    const double* Jp = j_lds ? sJ : J;
    // a thread's unit: row i of four neighbouring columns -- one J value feeds four sums (columns >= nc repeat the last one and
    // are not stored)
    const int units = ((nc + 3) / 4) * m;
    for (int u = threadIdx.x; u < units; u += 256) {
        const int g = u / m, i = u - g * m;
        const double* w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = sW + (4 * g + q < nc ? 4 * g + q : nc - 1) * m;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < m; ++k) {
            const double j = Jp[i + (size_t)k * m];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += j * w[q][k];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * g + q < nc) Wc[(4 * g + q) * m + i] = acc[q];
    }
}

// sig[k] = +-sigma[k], the sign of the first entry of largest magnitude of row perm[k] of W (k < r; one workgroup per row)
__global__ void __launch_bounds__(256)
rowspace_lead_kernel(int m, int64_t ncols, const double* __restrict__ W, const int32_t* __restrict__ perm,
                     const double* __restrict__ sigma, double* __restrict__ sig) {
    __shared__ double sa[256];
    __shared__ int64_t si[256];
    const int k = blockIdx.x;
    const double* row = W + perm[k];
    double best = -1.0;
    int64_t at = 0;
    for (int64_t c = threadIdx.x; c < ncols; c += 256) {  // (ascending per thread: the first of equals stays)
        const double a = fabs(row[c * m]);
        if (a > best) {
            best = a;
            at = c;
        }
    }
    sa[threadIdx.x] = best;
    si[threadIdx.x] = at;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double a = sa[threadIdx.x + w];
            const int64_t i = si[threadIdx.x + w];
            if (a > sa[threadIdx.x] || (a == sa[threadIdx.x] && i < si[threadIdx.x])) {
                sa[threadIdx.x] = a;
                si[threadIdx.x] = i;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) sig[k] = row[si[0] * m] < 0.0 ? -sigma[k] : sigma[k];
}

// out[k, c] = W[perm[k], c] / sig[k] for k < r, |.| <= droptol -> 0.0, rows >= r -> 0.0; W may be out (columns staged in
// LDS).  nnz += the non-zeros written (integer atomic: the count does not depend on the order).
__global__ void __launch_bounds__(256)
rowspace_write_kernel(int m, int64_t ncols, int cc, int r, const double* W, const int32_t* __restrict__ perm,
                      const double* __restrict__ sig, double droptol, double* out, unsigned long long* __restrict__ nnz) {
    extern __shared__ double rs_smem[];
    __shared__ unsigned int scount;
    double* sW = rs_smem;
    const int64_t c0 = (int64_t)blockIdx.x * cc;
    const int nc = (int)(ncols - c0 < cc ? ncols - c0 : cc);
    const int cnt = nc * m;
    if (threadIdx.x == 0) scount = 0;
    for (int o = threadIdx.x; o < cnt; o += 256) sW[o] = W[c0 * m + o];
    __syncthreads();
    unsigned int mine = 0;
    for (int o = threadIdx.x; o < cnt; o += 256) {
        const int cl = o / m, k = o - cl * m;
        double v = 0.0;
        if (k < r) {
            v = sW[cl * m + perm[k]] / sig[k];
            if (fabs(v) <= droptol) v = 0.0;
            mine += v != 0.0;
        }
        out[c0 * m + o] = v;
    }
    if (mine) atomicAdd(&scount, mine);
    __syncthreads();
    if (threadIdx.x == 0 && scount) atomicAdd(nnz, (unsigned long long)scount);
}

}  // namespace

double rowspace_scale(double max_abs) { return rowspace_scale_of(max_abs); }

// The K split of the Gram product: a function of (m, ncols) alone -- not of the device -- so that equal inputs give equal bytes
void rowspace_gram_shape(int64_t m, int64_t ncols, int* npairs, int* Z, int64_t* cps) {
    const int64_t nb = (m + 63) / 64;
    *npairs = (int)(nb * (nb + 1) / 2);
    int64_t z = (ncols + 63) / 64;
    const int64_t zmax = std::max<int64_t>(1, 2048 / *npairs);
    z = std::min(std::max<int64_t>(z, 1), zmax);
    *cps = round_up((ncols + z - 1) / z, 4);
    *Z = (int)std::max<int64_t>(1, (ncols + *cps - 1) / *cps);
}
size_t rowspace_gram_partial_doubles(int64_t m, int64_t ncols) {
    int npairs, Z;
    int64_t cps;
    rowspace_gram_shape(m, ncols, &npairs, &Z, &cps);
    return (size_t)Z * npairs * 4096;
}
int rowspace_absmax_blocks(int64_t total) { return (int)std::min<int64_t>(1024, std::max<int64_t>(1, (total + 2047) / 2048)); }

// W = [A | b] * 2^-e (b may be nullptr: md == total); info[0] = max |M|, info[1] = non-finite verdict; pmax: rowspace_absmax_blocks(total)
void launch_rowspace_scale(hipStream_t s, int64_t total, int64_t md, const double* A, const double* b, double* pmax, uint32_t* flag,
                           double* W, double* info) {
    const int nblk = rowspace_absmax_blocks(total);
    rowspace_absmax_kernel<<<nblk, 256, 0, s>>>(total, md, A, b, pmax, flag);
    rowspace_scale_copy_kernel<<<nblk, 256, 0, s>>>(total, md, A, b, pmax, nblk, flag, W, info);
}

// G (m x m, both triangles) = W W'; P: rowspace_gram_partial_doubles(m, ncols)
void launch_rowspace_gram(hipStream_t s, int64_t m, int64_t ncols, const double* W, double* P, double* G) {
    int npairs, Z;
    int64_t cps;
    rowspace_gram_shape(m, ncols, &npairs, &Z, &cps);
    rowspace_gram_kernel<<<dim3(npairs, (Z + 3) / 4), 256, 0, s>>>((int)m, ncols, W, Z, cps, npairs, P);
    rowspace_gram_reduce_kernel<<<npairs * 16, 256, 0, s>>>((int)m, Z, npairs, P, G);
}

// columns per workgroup of the two kernels that stage columns in LDS (64 KiB, no attribute), and whether J fits beside them
int rowspace_chunk(int64_t m, bool* j_lds) {
    const int64_t lds = 8000;  // doubles: 64 KiB less the kernels' static words
    const bool fits = m * m + m <= lds / 2;
    if (j_lds) *j_lds = fits;
    const int64_t room = (j_lds && fits) ? lds - m * m : lds;
    return (int)std::min<int64_t>(64, std::max<int64_t>(1, room / m));
}

void launch_rowspace_rotate(hipStream_t s, int64_t m, int64_t ncols, const double* J, double* W) {
    bool j_lds;
    const int cc = rowspace_chunk(m, &j_lds);
    const size_t bytes = ((size_t)cc * m + (j_lds ? (size_t)m * m : 0)) * 8;
    rowspace_rotate_kernel<<<(unsigned)((ncols + cc - 1) / cc), 256, bytes, s>>>((int)m, ncols, cc, j_lds ? 1 : 0, J, W);
}

// perm, sigma: r entries used (device); sig: r doubles of scratch; nnz: one zeroed 64-bit word
void launch_rowspace_finish(hipStream_t s, int64_t m, int64_t ncols, int64_t r, const double* W, const int32_t* perm,
                            const double* sigma, double* sig, double droptol, double* out, unsigned long long* nnz) {
    if (r > 0) rowspace_lead_kernel<<<(unsigned)r, 256, 0, s>>>((int)m, ncols, W, perm, sigma, sig);
    const int cc = rowspace_chunk(m, nullptr);
    rowspace_write_kernel<<<(unsigned)((ncols + cc - 1) / cc), 256, (size_t)cc * m * 8, s>>>((int)m, ncols, cc, (int)r, W, perm, sig,
                                                                                           droptol, out, nnz);
}

}  // namespace sdpsr
