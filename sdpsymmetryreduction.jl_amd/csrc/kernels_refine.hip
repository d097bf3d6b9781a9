// The canonical partition refinement for gfx950: its driver (launch_refine) and every pass but the insert -- clear,
// count, scan, rank, small rank, label, label with the symmetry check.  The passes are laid out in refine_table.h; the
// insert pass lives in refine_insert.h and is compiled per source family in kernels_insert_*.hip.
//
// Reference semantics restated here:
//   Partition(M), refine! src/partitions.jl:24-35,44-66
#include <type_traits>
#include "sdpsr_internal.h"
#include "kernel_util.h"
#include "sig_sources.h"
#include "refine_table.h"
#include "sym_tile_pass.h"

namespace sdpsr {

uint32_t refine_first_cap() { return REFINE_FIRST_CAP; }

size_t refine_block_entries() { return REFINE_BLOCK; }
uint32_t refine_small_k() { return SMALL_K; }
size_t refine_counters_bytes() { return (size_t)(LIST_OFF + SMALL_K) * sizeof(uint32_t); }

// thread t of the block owns entries base + 4t .. 4t+3 (index order matters here)
__device__ __forceinline__ int first_flags(int64_t len, int64_t base,
                                           const uint32_t* __restrict__ slot,
                                           const RefSlot* __restrict__ tab, int* flags,
                                           uint32_t* slots) {
    int cnt = 0;
    const int64_t e0 = base + (int64_t)threadIdx.x * REFINE_PER_THREAD;
#pragma unroll
    for (int q = 0; q < REFINE_PER_THREAD; ++q) {
        const int64_t e = e0 + q;
        uint32_t sl = (e < len) ? slot[e] : NO_SLOT;
        slots[q] = sl;
        int f = 0;
        if (sl != NO_SLOT) f = (tab[sl].min == (uint32_t)e);
        flags[q] = f;
        cnt += f;
    }
    return cnt;
}

__global__ void __launch_bounds__(REFINE_THREADS)
refine_count_kernel(int64_t len, const uint32_t* __restrict__ slot,
                    const RefSlot* __restrict__ tab, uint32_t* __restrict__ blk_cnt,
                    const uint32_t* __restrict__ counters) {
    __shared__ int sh[REFINE_THREADS / 64];
    if (counters[0] <= SMALL_K) return;  // ranked by refine_small_rank_kernel
    const int64_t nblk = (len + REFINE_BLOCK - 1) / REFINE_BLOCK;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        int flags[REFINE_PER_THREAD];
        uint32_t slots[REFINE_PER_THREAD];
        int cnt = first_flags(len, blk * REFINE_BLOCK, slot, tab, flags, slots);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < REFINE_THREADS / 64; ++w) t += sh[w];
            blk_cnt[blk] = (uint32_t)t;
        }
        __syncthreads();
    }
}

// exclusive scan of blk_cnt[0..nblk) in place; counters[2] = total
__global__ void __launch_bounds__(1024)
refine_scan_kernel(int64_t nblk, uint32_t* __restrict__ blk_cnt, uint32_t* counters) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    if (counters[0] <= SMALL_K) return;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t base = 0; base < nblk; base += 1024) {
        const int64_t i = base + threadIdx.x;
        uint32_t v = (i < nblk) ? blk_cnt[i] : 0u;
        uint32_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t woff = 0;
        for (int k = 0; k < w; ++k) woff += wsum[k];
        uint32_t incl = x + woff + carry;
        if (i < nblk) blk_cnt[i] = incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) counters[2] = carry;
}

__global__ void __launch_bounds__(REFINE_THREADS)
refine_rank_kernel(int64_t len, const uint32_t* __restrict__ slot,
                   const RefSlot* __restrict__ tab, const uint32_t* __restrict__ blk_off,
                   uint32_t* __restrict__ tab_lab, const uint32_t* __restrict__ counters, uint32_t* __restrict__ first_idx) {
    __shared__ int wsum[REFINE_THREADS / 64];
    if (counters[0] <= SMALL_K) return;
    const int64_t nblk = (len + REFINE_BLOCK - 1) / REFINE_BLOCK;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        int flags[REFINE_PER_THREAD];
        uint32_t slots[REFINE_PER_THREAD];
        int cnt = first_flags(len, blk * REFINE_BLOCK, slot, tab, flags, slots);
        int x = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int woff = 0;
        for (int k = 0; k < w; ++k) woff += wsum[k];
        int excl = x - cnt + woff;
        uint32_t lab = blk_off[blk] + (uint32_t)excl;
#pragma unroll
        for (int q = 0; q < REFINE_PER_THREAD; ++q)
            if (flags[q]) {
                tab_lab[slots[q]] = ++lab;
                // first occurrence of class `lab` (its class representative for the verify_* passes of kernels_class_compare.hip)
                if (first_idx && lab <= REFINE_FIRST_CAP) first_idx[lab - 1] = (uint32_t)(blk * REFINE_BLOCK + (int64_t)threadIdx.x * REFINE_PER_THREAD + q);
            }
        __syncthreads();
    }
}

// <= SMALL_K classes: label of a class = 1 + number of classes with a smaller first index
__global__ void __launch_bounds__(1024)
refine_small_rank_kernel(const RefSlot* __restrict__ tab, uint32_t* __restrict__ tab_lab,
                         uint32_t* __restrict__ counters, uint32_t* __restrict__ first_idx) {
    __shared__ uint32_t s_min[SMALL_K];
    const uint32_t K = counters[0];
    if (K > SMALL_K) return;
    const uint32_t i = threadIdx.x;
    uint32_t slot = 0, mine = 0;
    if (i < K) {
        slot = counters[LIST_OFF + i];
        mine = tab[slot].min;
        s_min[i] = mine;
    }
    __syncthreads();
    if (i < K) {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < K; ++j) rank += (s_min[j] < mine);
        tab_lab[slot] = rank + 1;
        if (first_idx) first_idx[rank] = mine;  // K <= SMALL_K <= REFINE_FIRST_CAP
    }
    if (i == 0) counters[2] = K;
}

// tab_sig = 0, tab_min = 0xFFFFFFFF, counters[0..16) = 0 in one launch
__global__ void refine_clear_kernel(int64_t cap, RefSlot* __restrict__ tab, uint32_t* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < cap; i += stride) {
        *reinterpret_cast<uint4*>(&tab[i]) = make_uint4(0u, 0u, 0xFFFFFFFFu, 0u);
    }
    if (t0 < LIST_OFF) counters[t0] = 0u;
}

// A pass the host is going to repeat (table overflow, or more classes than the one-workgroup
// ranking was launched for) must leave labels_out alone: a computed signature source may read the
// old labels from that very array.  slot may be labels_out itself (array source: in place).
__global__ void refine_label_kernel(int64_t len, const uint32_t* slot, uint32_t* labels_out,
                                    const uint32_t* __restrict__ tab_lab, const uint32_t* __restrict__ counters,
                                    int expect_small, uint32_t* __restrict__ host_counters, uint32_t host_seq) {
    // the last kernel of a refinement hands the counters (inserted, overflow flag, classes) to the host itself: a
    // store into pinned host memory instead of a separate 16-byte copy launch (~5 us + a launch gap per refinement)
    // ... and then the stamp: the host may go on as soon as it sees it (ctx_wait_word), the rest of this pass is behind it in the stream
    // (one thread writes all three and then the stamp: ctx_wait_word reads every counter as soon as the stamp lands, and
    // only program order -- not the lockstep of a wave -- puts the counters before it)
    if (host_counters && blockIdx.x == 0 && threadIdx.x == 0) {
        host_counters[0] = counters[0];
        host_counters[1] = counters[1];
        host_counters[2] = counters[2];
        __threadfence_system();
        host_counters[3] = host_seq;
    }
    if (counters[1] || (expect_small && counters[0] > SMALL_K)) return;
    // four consecutive entries per thread and trip: one 16-byte load, four gathers in flight together, one 16-byte store (one
    // entry per trip was a load, a wait, a gather, a wait and a store, sixteen times per thread; round 4)
    typedef uint32_t rl_u32x4 __attribute__((ext_vector_type(4)));
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (16-byte accesses only when both arrays allow them: the labels may be a caller's device pointer)
    const int64_t len4 = ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(labels_out)) & 15) ? 0 : (len >> 2);
    const rl_u32x4* slot4 = reinterpret_cast<const rl_u32x4*>(slot);
    rl_u32x4* out4 = reinterpret_cast<rl_u32x4*>(labels_out);
    for (int64_t q = t0; q < len4; q += stride) {
        const rl_u32x4 sl = __builtin_nontemporal_load(&slot4[q]);
        rl_u32x4 o;
        o.x = (sl.x == NO_SLOT) ? 0u : tab_lab[sl.x];
        o.y = (sl.y == NO_SLOT) ? 0u : tab_lab[sl.y];
        o.z = (sl.z == NO_SLOT) ? 0u : tab_lab[sl.z];
        o.w = (sl.w == NO_SLOT) ? 0u : tab_lab[sl.w];
        out4[q] = o;
    }
    for (int64_t e = 4 * len4 + t0; e < len; e += stride) {
        const uint32_t sl = __builtin_nontemporal_load(&slot[e]);
        labels_out[e] = (sl == NO_SLOT) ? 0u : tab_lab[sl];
    }
}

// refine_label_kernel for an n x n label matrix, with the symmetry check of the NEW labels folded in
// (check_symmetric_kernel would read them again).  counters[3] = 1 if the labels are NOT symmetric
// (counters are cleared by refine_clear_kernel).
template <bool VEC4>
__global__ void __launch_bounds__(256)
refine_label_sym_kernel(int64_t n, const uint32_t* slot, uint32_t* labels_out,
                        const uint32_t* __restrict__ tab_lab, uint32_t* __restrict__ counters, int expect_small) {
    __shared__ uint32_t tile[64][65];
    if (counters[1] || (expect_small && counters[0] > SMALL_K)) return;
    if (blockIdx.x < blockIdx.y) return;  // lower triangle of tile pairs
    if (sym_tile_pass<VEC4>(n, slot, labels_out, MapSlotLabel{tab_lab}, tile)) counters[3] = 1u;
}

// does launch_refine run the one-workgroup-per-CU insert kernel for this source (RefineWs::mid)?
bool refine_mid_supports(const SigSource& q) {
    bool mid = false;
    with_source(q, [&](const auto& src) { mid = std::decay_t<decltype(src)>::kMid; });
    return mid;
}

// false: the source has no insert kernel (not sig_source_fusable), nothing was launched
bool launch_refine(hipStream_t s, int64_t len, const SigSource& q, uint32_t* slot, uint32_t* labels_out,
                   const RefineWs& ws, int64_t sym_n) {
    if (!sig_source_fusable(q)) return false;
    const size_t cap = (size_t)1 << ws.log2cap;
    refine_clear_kernel<<<grid_for((int64_t)cap, 256), 256, 0, s>>>((int64_t)cap, ws.tab, ws.counters);
    const int64_t nblk = (len + REFINE_BLOCK - 1) / REFINE_BLOCK;
    // 116 VGPRs + 32 KiB of LDS: four workgroups are resident per CU; with few classes (LDS-level
    // work) launch exactly one round of resident workgroups -- a fifth per CU would run alone
    const int per_cu = (ws.log2cap <= 16) ? 4 : 5;  // many classes: bound by the global table, a few more workgroups help
    const int gcap = 256 * per_cu;
    with_source(q, [&](const auto& src) { launch_insert(s, gcap, len, src, slot, ws, cap); });
    const int g2 = (int)(nblk < 256 * 8 ? nblk : 256 * 8);
    // ws.expect_small: the host predicts <= SMALL_K classes (from the previous refinement) and
    // launches the one-workgroup ranking only; it checks counters[0] afterwards and repeats the
    // pass with expect_small = 0 on a misprediction (the three general kernels would exit at once
    // anyway, but three empty launches cost ~15 us of a ~150 us refinement)
    refine_small_rank_kernel<<<1, 1024, 0, s>>>(ws.tab, ws.tab_lab, ws.counters, ws.first_idx);
    if (!ws.expect_small) {
        // more than SMALL_K classes: ranked from the table's side (kernels_refine_bucket.hip: one bit per first index, rank
        // records per 64 entries) -- work on the classes and on len / 64 words.  The entry-level count / scan / rank passes
        // stay for callers without that workspace.
        if (!(ws.rank_ws && launch_rank_slots(s, len, (int64_t)cap, ws.tab, ws.tab_lab, ws.counters, SMALL_K, ws.first_idx,
                                              REFINE_FIRST_CAP, ws.rank_ws, ws.rank_ws_bytes))) {
            refine_count_kernel<<<g2, REFINE_THREADS, 0, s>>>(len, slot, ws.tab, ws.blk_cnt, ws.counters);
            refine_scan_kernel<<<1, 1024, 0, s>>>(nblk, ws.blk_cnt, ws.counters);
            refine_rank_kernel<<<g2, REFINE_THREADS, 0, s>>>(len, slot, ws.tab, ws.blk_cnt,
                                                             ws.tab_lab, ws.counters, ws.first_idx);
        }
    }
    if (sym_n > 0 && sym_n * sym_n == len) {  // labels of an n x n matrix: the symmetry verdict comes with the label pass
        const unsigned t = (unsigned)((sym_n + 63) / 64);
        if (sym_n % 4 == 0) refine_label_sym_kernel<true><<<dim3(t, t), 256, 0, s>>>(sym_n, slot, labels_out, ws.tab_lab, ws.counters, ws.expect_small);
        else refine_label_sym_kernel<false><<<dim3(t, t), 256, 0, s>>>(sym_n, slot, labels_out, ws.tab_lab, ws.counters, ws.expect_small);
    } else {
        refine_label_kernel<<<grid_for(len, 256), 256, 0, s>>>(len, slot, labels_out, ws.tab_lab, ws.counters, ws.expect_small, ws.host_counters, ws.host_seq);
    }
    return true;
}

}  // namespace sdpsr
