// Reduced-SDP assembly from a sparse A: newA = A * PMat, newC = C' * PMat with PMat = hcat(vec(P.matrix .== i) for i = 1:dim(P))
// (README.md:57-60, test/sd_problems.jl:32-37,113-118) for A in canonical CSR (rows contiguous, columns sorted, no zeros).
//
// A keyed sum: non-zero j of row r adds val[j] to out[r, labels[col[j]] - 1].  Three steps, none with a floating-point atomic:
//   1. csr_entry_labels_kernel: key[j] = labels[col[j]] (0 = no column; a label beyond d is made 0 here, so that nothing
//      is ever indexed by it -- labels_exceed_kernel reports it);
//   2. the stable radix sort of (key[j], j) by key (launch_radix_sort_pairs, kernels_blockdiag.hip).  The entries of a row
//      are consecutive j, so behind the sort the entries of one (label, row) pair are one contiguous RUN, in column order;
//   3. csr_class_sums_kernel + csr_class_sums_carry_kernel: the segmented sum over the runs.
// Any d: the only storage that grows with d is the m x d output itself.  Rows of any lengths: the work is cut by position in
// the sorted array, never by row.
#include "host_internal.h"

namespace sdpsr {

namespace {

inline int grid_for(int64_t work, int per_block, int cap = 1 << 20) {
    int64_t g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// flag[0] |= 1 if some label exceeds d (16-byte loads from the first 16-byte boundary on; head and tail one by one: a caller's
// device pointer need not be aligned)
__global__ void __launch_bounds__(256)
labels_exceed_kernel(int64_t len, const uint32_t* __restrict__ L, uint32_t d, uint32_t* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)L & 15u)) & 15u) >> 2);
    if (head > len) head = len;
    const int64_t len4 = (len - head) >> 2;
    bool bad = false;
    if (t < head) bad |= L[t] > d;
    for (int64_t g = t; g < len4; g += stride) {
        const uint4 l = reinterpret_cast<const uint4*>(L + head)[g];
        bad |= l.x > d || l.y > d || l.z > d || l.w > d;
    }
    for (int64_t e = head + (len4 << 2) + t; e < len; e += stride) bad |= L[e] > d;
    if (bad) atomicOr(flag, 1u);  // (an integer flag: order does not matter)
}

__device__ __forceinline__ uint32_t entry_label(const uint32_t* __restrict__ L, uint32_t col, uint32_t d) {
    const uint32_t l = L[col];  // the 4-byte random read
    return l > d ? 0u : l;
}

// key[j] = label of entry j's column; col is streamed with 16-byte loads, the keys are stored the same way
__global__ void __launch_bounds__(256)
csr_entry_labels_kernel(int64_t nnz, const uint32_t* __restrict__ col, const uint32_t* __restrict__ L, uint32_t d,
                        uint32_t* __restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nnz4 = nnz >> 2;
    for (int64_t g = t; g < nnz4; g += stride) {
        const uint4 c = reinterpret_cast<const uint4*>(col)[g];
        uint4 k;
        k.x = entry_label(L, c.x, d);
        k.y = entry_label(L, c.y, d);
        k.z = entry_label(L, c.z, d);
        k.w = entry_label(L, c.w, d);
        reinterpret_cast<uint4*>(key)[g] = k;
    }
    for (int64_t j = (nnz4 << 2) + t; j < nnz; j += stride) key[j] = entry_label(L, col[j], d);
}

// What a wave leaves behind for the runs that cross the borders of its piece of the sorted array
struct RcCarry {
    long long head_o, tail_o;  // output index (label - 1) * m + row of the run; -1: label 0 (no column), -2: behind the end
    double head_x, tail_x;
    int single, pad;           // 1: the whole piece is one run (head only)
};

constexpr int RC_T = 256;                      // 4 waves
constexpr int RC_PIECE = 1024;                 // sorted positions per wave: 16 tiles of 64
constexpr int RC_ROWPTR_LDS = 2048;            // rowptr is searched in LDS up to this m

// Segmented sum over the sorted entries.  SUMMATION ORDER of one run (a function of the inputs alone: the positions in the
// sorted array are, and every constant below is fixed): the array is cut into pieces of 1024 positions, a piece into tiles
// of 64.  Inside a tile the run's entries are added by the segmented Hillis-Steele scan over the 64 lanes (six shuffle
// steps, partners at distance 1, 2, .., 32 inside the run); the tiles of a piece are added left to right onto the first,
// (((t0 + t1) + t2) + ..); the pieces of a run are added left to right in the same way by csr_class_sums_carry_kernel.
// Neither the number of workgroups that run at a time nor their order enters: every partial sum has one owner and one slot.
// A run that begins and ends inside one piece is stored to out here; the others leave their partial sums in carry[piece].
__global__ void __launch_bounds__(RC_T)
csr_class_sums_kernel(int64_t nnz, int64_t m, const long long* __restrict__ rowptr, const uint32_t* __restrict__ skey,
                      const uint32_t* __restrict__ sidx, const double* __restrict__ val, RcCarry* __restrict__ carry,
                      double* __restrict__ out) {
    __shared__ long long srp[RC_ROWPTR_LDS + 1];
    const bool rp_lds = m <= RC_ROWPTR_LDS;
    if (rp_lds)
        for (int i = threadIdx.x; i <= (int)m; i += RC_T) srp[i] = rowptr[i];
    __syncthreads();
    const long long* rp = rp_lds ? srp : rowptr;
    const int lane = threadIdx.x & 63;
    const int64_t piece = (int64_t)blockIdx.x * (RC_T / 64) + (threadIdx.x >> 6);
    const int64_t p0 = piece * RC_PIECE;
    if (p0 >= nnz) return;
    // the open run: the one the previous tile ended in (wave-uniform)
    long long cur_o = 0;
    double cur_x = 0.0;
    bool boundary_seen = false;  // some run of this piece has ended: the open run is no longer the head
    for (int t = 0; t < RC_PIECE / 64 && p0 + t * 64 < nnz; ++t) {
        const int64_t p = p0 + t * 64 + lane;
        long long o = -2;
        double v = 0.0;
        if (p < nnz) {
            const uint32_t lab = skey[p];
            o = -1;
            if (lab != 0u) {
                const uint32_t j = sidx[p];
                int64_t lo = 0, hi = m;  // rowptr[lo] <= j < rowptr[hi]
                while (hi - lo > 1) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (rp[mid] <= (long long)j) lo = mid; else hi = mid;
                }
                o = (long long)(lab - 1u) * m + lo;
                v = val[j];
            }
        }
        // inclusive sums inside the runs of the tile (equal o at distance k means one run: runs are contiguous)
        double x = v;
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

// The runs that cross piece borders: thread w owns the run that BEGINS in piece w and leaves it (at most one: the piece's
// tail, or the piece itself when it is one run that begins at its first position), adds the heads of the following pieces
// left to right while the run goes on, and stores the sum.  A head whose run begins at the first position of a piece that
// holds further runs is complete and stored as it is.  One thread per run, a serial walk: a run of k pieces costs k
// dependent reads (k <= nnz / 1024, reached only when one (label, row) pair holds nearly every entry).
__global__ void __launch_bounds__(256)
csr_class_sums_carry_kernel(int64_t npieces, const RcCarry* __restrict__ carry, double* __restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= npieces) return;
    const RcCarry me = carry[w];
    bool head_begins = true;  // the head's run begins at the first position of piece w
    if (w > 0) {
        const RcCarry prev = carry[w - 1];
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
        const RcCarry nx = carry[u];
        if (nx.head_o != o) break;
        acc += nx.head_x;
        if (!nx.single) break;
    }
    out[o] = acc;
}

}  // namespace

void launch_labels_exceed(hipStream_t s, int64_t len, const uint32_t* L, int64_t d, uint32_t* flag) {
    const uint32_t dd = d > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)d;
    labels_exceed_kernel<<<grid_for(len, 256 * 16, 2048), 256, 0, s>>>(len, L, dd, flag);
}

void launch_csr_entry_labels(hipStream_t s, int64_t nnz, const uint32_t* col, const uint32_t* L, int64_t d, uint32_t* key) {
    const uint32_t dd = d > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)d;
    csr_entry_labels_kernel<<<grid_for(nnz, 256 * 16, 4096), 256, 0, s>>>(nnz, col, L, dd, key);
}

size_t csr_class_sums_carry_bytes(int64_t nnz) { return (size_t)((nnz + RC_PIECE - 1) / RC_PIECE) * sizeof(RcCarry); }

void launch_csr_class_sums(hipStream_t s, int64_t nnz, int64_t m, const int64_t* rowptr, const uint32_t* key_sorted,
                           const uint32_t* idx_sorted, const double* val, void* carry, double* out) {
    const int64_t npieces = (nnz + RC_PIECE - 1) / RC_PIECE;
    const int64_t per_block = RC_T / 64;
    csr_class_sums_kernel<<<(unsigned)((npieces + per_block - 1) / per_block), RC_T, 0, s>>>(
        nnz, m, (const long long*)rowptr, key_sorted, idx_sorted, val, (RcCarry*)carry, out);
    csr_class_sums_carry_kernel<<<(unsigned)((npieces + 255) / 256), 256, 0, s>>>(npieces, (const RcCarry*)carry, out);
}

}  // namespace sdpsr
