// The canonical pass of a sparse-constraints handle (sdpsr_sparse_create, sparse_handle.cpp) on the device: what
// canonicalize_csr (setup_csr.cpp) does on one host thread -- validate, sort each row by column (stable), sum duplicates in
// input order, drop zeros, uint32 columns -- for the A of src/partitions.jl:117-142 and README.md:57-60, plus the symmetry
// predicate of csr_rows_symmetric.  The arrays these kernels leave behind equal the host function's bit for bit.
//
// Streaming passes over the nnz raw entries (int64 column, double value: 16 bytes per entry):
//   1. canon_check_rowptr_kernel / canon_check_entries_kernel: the verdict words of CanonVerdict (lowest bad row, lowest bad
//      column entry, lowest non-finite entry by 64-bit integer atomicMin after a wave reduction; "some row is not strictly
//      increasing"), and the columns as uint32 with a keep flag per entry for the route without a sort;
//   2. only if some row is not strictly increasing: canon_row_ids_kernel, two stable radix sorts (launch_radix_sort_pairs:
//      by column, then by row -- the rows of a CSR input are contiguous, so each row's segment keeps its place),
//      canon_gather_sorted_kernel, canon_runs_kernel (one thread per run of equal (row, column) adds the run's values left
//      to right: s = v0; s += v1; ... exactly the host's loop);
//   3. compaction of the kept entries: canon_count_kernel per chunk of CANON_CHUNK positions, canon_scan_kernel (int64,
//      one workgroup), canon_fill_kernel -- no atomics on positions, so equal inputs give equal bytes;
//   4. canon_rowptr_kernel: the new rowptr is the new position of every old row boundary;
//   5. canon_symmetry_kernel: binary search of the transposed index of every off-diagonal entry within its row.
// No floating-point atomics anywhere.
#include "host_internal.h"

namespace sdpsr {

namespace {

constexpr int CANON_T = 256, CANON_E = 8;  // a workgroup owns CANON_CHUNK consecutive positions, a thread 8 consecutive ones
static_assert(CANON_T * CANON_E == CANON_CHUNK, "chunk = threads x entries per thread");

inline int grid_for(int64_t work, int per_block, int cap) {
    int64_t g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(x, o, 64);
        x = y < x ? y : x;
    }
    return x;
}

// the row of position p: rowptr[i] - base <= p < rowptr[i + 1] - base.  Reads rowptr[0 .. m] only, whatever it holds (the
// check kernels run before rowptr is known to be valid).  m >= 1.
__device__ __forceinline__ int64_t row_of(const long long* __restrict__ rowptr, int64_t m, long long base, int64_t p) {
    int64_t lo = 0, hi = m;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] - base <= (long long)p) lo = mid; else hi = mid;
    }
    return lo;
}

// rowptr[0] == base, monotone (the lowest row i with rowptr[i + 1] < rowptr[i]), rowptr[m] - base == nnz
__global__ void __launch_bounds__(256)
canon_check_rowptr_kernel(int64_t m, int64_t nnz, const long long* __restrict__ rowptr, long long base, CanonVerdict* __restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        if (rowptr[0] != base) v->rowptr0_bad = 1ull;  // (plain stores: one writer)
        if (rowptr[m] - base != (long long)nnz) v->nnz_mismatch = 1ull;
    }
    unsigned long long bad = CANON_NO_INDEX;
    for (int64_t i = t; i < m; i += stride)
        if (rowptr[i + 1] < rowptr[i] && (unsigned long long)i < bad) bad = (unsigned long long)i;
    bad = wave_min_u64(bad);
    if ((threadIdx.x & 63) == 0 && bad != CANON_NO_INDEX) atomicMin(&v->bad_row, bad);
}

struct EntryCheck {
    unsigned long long bad_col = CANON_NO_INDEX, bad_val = CANON_NO_INDEX;
    bool unsorted = false;
};

// one raw entry: range and finiteness, "not strictly increasing inside its row", its uint32 column and keep flag
__device__ __forceinline__ void check_entry(int64_t p, long long k_raw, long long k_prev_raw, double x, const long long* __restrict__ rowptr,
                                            int64_t m, long long base, int64_t len, EntryCheck& r, uint32_t& col, unsigned char& keep) {
    const long long k = k_raw - base;
    if ((k < 0 || k >= (long long)len) && (unsigned long long)p < r.bad_col) r.bad_col = (unsigned long long)p;
    if (!isfinite(x) && (unsigned long long)p < r.bad_val) r.bad_val = (unsigned long long)p;
    if (p > 0 && k_raw <= k_prev_raw) {  // a row boundary, or a row that needs the sort
        const int64_t i = row_of(rowptr, m, base, p);
        if (rowptr[i] - base != (long long)p) r.unsorted = true;
    }
    col = (uint32_t)k;
    keep = x != 0.0 ? 1 : 0;
}

// VEC: colind and val are 16-byte aligned -- four entries per step with 16-byte loads and stores; else one by one (a
// caller's device pointer need not be aligned)
template <bool VEC>
__global__ void __launch_bounds__(256)
canon_check_entries_kernel(int64_t nnz, int64_t m, int64_t len, const long long* __restrict__ rowptr, const long long* __restrict__ colind,
                           const double* __restrict__ val, long long base, uint32_t* __restrict__ col32, unsigned char* __restrict__ keep,
                           CanonVerdict* __restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    EntryCheck r;
    const int64_t nnz4 = VEC ? nnz >> 2 : 0;
    if (VEC) {
        for (int64_t g = t; g < nnz4; g += stride) {
            const int64_t p = g << 2;
            const longlong2 k01 = reinterpret_cast<const longlong2*>(colind)[2 * g], k23 = reinterpret_cast<const longlong2*>(colind)[2 * g + 1];
            const double2 x01 = reinterpret_cast<const double2*>(val)[2 * g], x23 = reinterpret_cast<const double2*>(val)[2 * g + 1];
            const long long kp = p > 0 ? colind[p - 1] : 0;
            uint4 c;
            uchar4 f;
            check_entry(p, k01.x, kp, x01.x, rowptr, m, base, len, r, c.x, f.x);
            check_entry(p + 1, k01.y, k01.x, x01.y, rowptr, m, base, len, r, c.y, f.y);
            check_entry(p + 2, k23.x, k01.y, x23.x, rowptr, m, base, len, r, c.z, f.z);
            check_entry(p + 3, k23.y, k23.x, x23.y, rowptr, m, base, len, r, c.w, f.w);
            reinterpret_cast<uint4*>(col32)[g] = c;
            reinterpret_cast<uchar4*>(keep)[g] = f;
        }
    }
    for (int64_t p = (nnz4 << 2) + t; p < nnz; p += stride)
        check_entry(p, colind[p], p > 0 ? colind[p - 1] : 0, val[p], rowptr, m, base, len, r, col32[p], keep[p]);
    const unsigned long long bc = wave_min_u64(r.bad_col), bv = wave_min_u64(r.bad_val);
    const bool any_unsorted = __ballot(r.unsorted) != 0ull;
    if ((threadIdx.x & 63) == 0) {
        if (bc != CANON_NO_INDEX) atomicMin(&v->bad_col, bc);
        if (bv != CANON_NO_INDEX) atomicMin(&v->bad_val, bv);
        if (any_unsorted) v->unsorted = 1ull;  // (a plain store: all writers write the same value)
    }
}

// row[p] of every raw entry (the second sort's keys); rowptr is valid here
__global__ void __launch_bounds__(256)
canon_row_ids_kernel(int64_t nnz, int64_t m, const long long* __restrict__ rowptr, long long base, uint32_t* __restrict__ row) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += stride) row[p] = (uint32_t)row_of(rowptr, m, base, p);
}

// key2[q] = row of the entry at position q of the column order
__global__ void __launch_bounds__(256)
canon_gather_u32_kernel(int64_t nnz, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nnz; q += stride) dst[q] = src[idx[q]];
}

// behind both sorts: position q of the (row, column) order holds position pos2[q] of the column order
__global__ void __launch_bounds__(256)
canon_gather_sorted_kernel(int64_t nnz, const uint32_t* __restrict__ pos2, const uint32_t* __restrict__ col1, const uint32_t* __restrict__ idx1,
                           uint32_t* __restrict__ col_sorted, uint32_t* __restrict__ idx_sorted) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nnz; q += stride) {
        const uint32_t i = pos2[q];
        col_sorted[q] = col1[i];
        idx_sorted[q] = idx1[i];
    }
}

// One thread per run of equal (row, column): s = v0; s += v1; ... over the run's entries in input order (the sorts are
// stable).  sum[q] and keep[q] = (s != 0) at the run's head, keep = 0 at its other positions.  A long run is slow, never wrong.
__global__ void __launch_bounds__(256)
canon_runs_kernel(int64_t nnz, const uint32_t* __restrict__ row_sorted, const uint32_t* __restrict__ col_sorted,
                  const uint32_t* __restrict__ idx_sorted, const double* __restrict__ val, double* __restrict__ sum,
                  unsigned char* __restrict__ keep, CanonVerdict* __restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nnz; q += stride) {
        const uint32_t r = row_sorted[q], k = col_sorted[q];
        const bool head = q == 0 || row_sorted[q - 1] != r || col_sorted[q - 1] != k;
        if (!head) {
            keep[q] = 0;
            continue;
        }
        double s = val[idx_sorted[q]];
        for (int64_t t = q + 1; t < nnz && row_sorted[t] == r && col_sorted[t] == k; ++t) s += val[idx_sorted[t]];
        bad |= !isfinite(s);
        sum[q] = s;
        keep[q] = s != 0.0 ? 1 : 0;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) v->dup_nonfinite = 1ull;
}

__device__ __forceinline__ uint32_t load_keep8(int64_t n, int64_t e0, const unsigned char* __restrict__ keep) {  // bit q: keep[e0 + q]
    uint32_t bits = 0;
    if (e0 + CANON_E <= n) {
        const uint2 w = *reinterpret_cast<const uint2*>(keep + e0);  // (e0 is a multiple of 8: aligned)
#pragma unroll
        for (int q = 0; q < 4; ++q) bits |= (((w.x >> (8 * q)) & 0xFFu) ? 1u : 0u) << q;
#pragma unroll
        for (int q = 0; q < 4; ++q) bits |= (((w.y >> (8 * q)) & 0xFFu) ? 1u : 0u) << (4 + q);
    } else {
        for (int q = 0; q < CANON_E; ++q)
            if (e0 + q < n && keep[e0 + q]) bits |= 1u << q;
    }
    return bits;
}

// cnt[chunk] = kept entries of the chunk
__global__ void __launch_bounds__(CANON_T)
canon_count_kernel(int64_t n, const unsigned char* __restrict__ keep, long long* __restrict__ cnt) {
    __shared__ uint32_t wsum[CANON_T / 64];
    const int64_t e0 = (int64_t)blockIdx.x * CANON_CHUNK + (int64_t)threadIdx.x * CANON_E;
    uint32_t c = e0 < n ? (uint32_t)__popc(load_keep8(n, e0, keep)) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < CANON_T / 64; ++k) s += wsum[k];
        cnt[blockIdx.x] = (long long)s;
    }
}

// exclusive scan of cnt[0 .. G) in place by one workgroup; cnt[G] and *total = the sum
__global__ void __launch_bounds__(1024)
canon_scan_kernel(int64_t G, long long* __restrict__ cnt, unsigned long long* __restrict__ total) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < G; b0 += 1024) {
        const int64_t i = b0 + threadIdx.x;
        const long long x = i < G ? cnt[i] : 0;
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
        if (i < G) cnt[i] = run;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = run + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        cnt[G] = carry_s;
        *total = (unsigned long long)carry_s;
    }
}

// the kept entries of a chunk, in order, to off[chunk] + rank inside the chunk; rel[p] = kept entries of p's chunk before p
__global__ void __launch_bounds__(CANON_T)
canon_fill_kernel(int64_t n, const unsigned char* __restrict__ keep, const uint32_t* __restrict__ col, const double* __restrict__ x,
                  const long long* __restrict__ off, uint32_t* __restrict__ col_out, double* __restrict__ val_out,
                  unsigned short* __restrict__ rel) {
    __shared__ uint32_t wsum[CANON_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * CANON_CHUNK + (int64_t)threadIdx.x * CANON_E;
    const uint32_t bits = e0 < n ? load_keep8(n, e0, keep) : 0u;
    const uint32_t c = (uint32_t)__popc(bits);
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t r = incl - c;
    for (int k = 0; k < w; ++k) r += wsum[k];
    const long long o0 = off[blockIdx.x];
#pragma unroll
    for (int q = 0; q < CANON_E; ++q) {
        const int64_t e = e0 + q;
        if (e < n) {
            rel[e] = (unsigned short)r;
            if ((bits >> q) & 1u) {
                col_out[o0 + r] = col[e];
                val_out[o0 + r] = x[e];
                ++r;
            }
        }
    }
}

// the new rowptr: the new position of every old row boundary (0-based)
__global__ void __launch_bounds__(256)
canon_rowptr_kernel(int64_t m, int64_t n, const long long* __restrict__ rowptr, long long base, const long long* __restrict__ off,
                    const unsigned short* __restrict__ rel, long long* __restrict__ out) {
    const int64_t G = (n + CANON_CHUNK - 1) / CANON_CHUNK;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += stride) {
        const int64_t p = rowptr[i] - base;
        out[i] = p >= n ? off[G] : off[p / CANON_CHUNK] + (long long)rel[p];
    }
}

// csr_rows_symmetric on canonical arrays: an off-diagonal entry whose transposed index is absent from its row, or present
// with other bits, stores 1 (all writers write the same value)
__global__ void __launch_bounds__(256)
canon_symmetry_kernel(int64_t nnz, int64_t m, uint64_t n, const long long* __restrict__ rowptr, const uint32_t* __restrict__ col,
                      const double* __restrict__ val, CanonVerdict* __restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool miss = false;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += stride) {
        const uint64_t k = col[p], r = k % n, q = k / n;
        if (r == q) continue;
        const uint32_t t = (uint32_t)(q + r * n);
        const int64_t i = row_of(rowptr, m, 0, p);
        int64_t lo = rowptr[i], hi = rowptr[i + 1];  // lower_bound of t in col[lo .. hi)
        const int64_t end = hi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (col[mid] < t) lo = mid + 1; else hi = mid;
        }
        if (lo == end || col[lo] != t || __double_as_longlong(val[lo]) != __double_as_longlong(val[p])) miss = true;
    }
    if (__ballot(miss) != 0ull && (threadIdx.x & 63) == 0) v->asymmetric = 1ull;
}

// sdpsr_sparse_export: the canonical arrays as int64 / int64 with the caller's base
__global__ void __launch_bounds__(256)
canon_export_kernel(int64_t m, int64_t nnz, const long long* __restrict__ rowptr, const uint32_t* __restrict__ col, long long base,
                    long long* __restrict__ rowptr_out, long long* __restrict__ col_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t; i <= m; i += stride) rowptr_out[i] = rowptr[i] + base;
    for (int64_t p = t; p < nnz; p += stride) col_out[p] = (long long)col[p] + base;
}

}  // namespace

void launch_canon_check(hipStream_t s, int64_t len, int64_t m, int64_t nnz, const int64_t* rowptr, const int64_t* colind, const double* val,
                        int base, uint32_t* col32, unsigned char* keep, CanonVerdict* verdict) {
    canon_check_rowptr_kernel<<<grid_for(m, 256 * 8, 2048), 256, 0, s>>>(m, nnz, (const long long*)rowptr, (long long)base, verdict);
    if (nnz <= 0) return;
    const bool vec = (((uintptr_t)colind | (uintptr_t)val) & 15u) == 0;
    if (vec)
        canon_check_entries_kernel<true><<<grid_for(nnz, 256 * 16, 4096), 256, 0, s>>>(nnz, m, len, (const long long*)rowptr, (const long long*)colind,
                                                                                     val, (long long)base, col32, keep, verdict);
    else
        canon_check_entries_kernel<false><<<grid_for(nnz, 256 * 16, 4096), 256, 0, s>>>(nnz, m, len, (const long long*)rowptr, (const long long*)colind,
                                                                                      val, (long long)base, col32, keep, verdict);
}

void launch_canon_row_ids(hipStream_t s, int64_t nnz, int64_t m, const int64_t* rowptr, int base, uint32_t* row) {
    canon_row_ids_kernel<<<grid_for(nnz, 256 * 8, 4096), 256, 0, s>>>(nnz, m, (const long long*)rowptr, (long long)base, row);
}

void launch_canon_gather_u32(hipStream_t s, int64_t nnz, const uint32_t* idx, const uint32_t* src, uint32_t* dst) {
    canon_gather_u32_kernel<<<grid_for(nnz, 256 * 8, 4096), 256, 0, s>>>(nnz, idx, src, dst);
}

void launch_canon_runs(hipStream_t s, int64_t nnz, const uint32_t* pos2, const uint32_t* col1, const uint32_t* idx1, const uint32_t* row_sorted,
                       const double* val, uint32_t* col_sorted, uint32_t* idx_sorted, double* sum, unsigned char* keep, CanonVerdict* verdict) {
    canon_gather_sorted_kernel<<<grid_for(nnz, 256 * 8, 4096), 256, 0, s>>>(nnz, pos2, col1, idx1, col_sorted, idx_sorted);
    canon_runs_kernel<<<grid_for(nnz, 256 * 4, 8192), 256, 0, s>>>(nnz, row_sorted, col_sorted, idx_sorted, val, sum, keep, verdict);
}

void launch_canon_count_scan(hipStream_t s, int64_t n, const unsigned char* keep, int64_t* cnt, CanonVerdict* verdict) {
    const int64_t G = canon_chunks(n);
    if (G > 0) canon_count_kernel<<<(unsigned)G, CANON_T, 0, s>>>(n, keep, (long long*)cnt);
    canon_scan_kernel<<<1, 1024, 0, s>>>(G, (long long*)cnt, &verdict->total);
}

void launch_canon_fill(hipStream_t s, int64_t n, int64_t m, const unsigned char* keep, const uint32_t* col, const double* x, const int64_t* cnt,
                       const int64_t* rowptr, int base, unsigned short* rel, int64_t* rowptr_out, uint32_t* col_out, double* val_out) {
    const int64_t G = canon_chunks(n);
    if (G > 0) canon_fill_kernel<<<(unsigned)G, CANON_T, 0, s>>>(n, keep, col, x, (const long long*)cnt, col_out, val_out, rel);
    canon_rowptr_kernel<<<grid_for(m + 1, 256, 2048), 256, 0, s>>>(m, n, (const long long*)rowptr, (long long)base, (const long long*)cnt, rel,
                                                                   (long long*)rowptr_out);
}

void launch_canon_symmetry(hipStream_t s, int64_t nnz, int64_t m, int64_t n, const int64_t* rowptr, const uint32_t* col, const double* val,
                           CanonVerdict* verdict) {
    if (nnz <= 0 || m <= 0) return;
    canon_symmetry_kernel<<<grid_for(nnz, 256 * 4, 8192), 256, 0, s>>>(nnz, m, (uint64_t)n, (const long long*)rowptr, col, val, verdict);
}

void launch_canon_export(hipStream_t s, int64_t m, int64_t nnz, const int64_t* rowptr, const uint32_t* col, int base, int64_t* rowptr_out,
                         int64_t* col_out) {
    canon_export_kernel<<<grid_for(std::max<int64_t>(nnz, m + 1), 256 * 8, 4096), 256, 0, s>>>(m, nnz, (const long long*)rowptr, col, (long long)base,
                                                                                           (long long*)rowptr_out, (long long*)col_out);
}

}  // namespace sdpsr
