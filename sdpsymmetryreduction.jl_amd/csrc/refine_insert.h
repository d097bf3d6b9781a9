// The insert pass of the canonical refinement (pass A of refine_table.h): the two insert kernels with their helpers and
// launchers, as templates over the signature source.  Included by the kernels_insert_*.hip files only: each names the
// sources of its family once (SDPSR_INSERT_INSTANTIATE, SDPSR_INSERT_MID_ATTRIBUTE below), and that is where their insert
// kernels are compiled.
#pragma once
#include <cstdlib>
#include <type_traits>
#include "sdpsr_internal.h"
#include "kernel_util.h"
#include "sig_sources.h"
#include "refine_table.h"

namespace sdpsr {

// development aid (-DLK_TIMING and SDPSR_DEBUG): wall-clock stamps (100 MHz) of the phases of the first four chunks of the
// first / middle / last workgroup of an insert launch
// (ri_dbg: one pointer per translation unit, written by the launcher of the same file that launches the stamped kernel)
#ifdef LK_TIMING
bool dbg_on();  // ctx.cpp (SDPSR_DEBUG)
static __device__ long long* ri_dbg = nullptr;
#define RI_STAMP(i)                                                                                                      \
    do {                                                                                                                  \
        if (ri_dbg && threadIdx.x == 0 && ri_it < 4 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1 || blockIdx.x == gridDim.x / 2)) { \
            const int which = blockIdx.x == 0 ? 0 : (blockIdx.x == gridDim.x - 1 ? 2 : 1);                               \
            ri_dbg[(which * 4 + ri_it) * 8 + (i)] = wall_clock64();                                                       \
        }                                                                                                                 \
    } while (0)
#else
#define RI_STAMP(i)
#endif

// One workgroup dedups INSERT_CHUNK entries in an LDS table before touching the global one.
// An entry whose LDS probe sequence gets long (many distinct signatures in the chunk) goes to
// the global table directly instead.
constexpr int LDS_MAX_PROBES = 24;

// SRC: where the signatures come from (see the Src* functors); INSERT_PER_THREAD entries per
// thread and chunk (16 for the plain array, 8 for the computed sources: their loads and hashes
// of one chunk are all live before the first probe)
// (Round 4 measured a 1024-thread instance with an 8192-slot table in dynamic LDS for the mid regime of 1024 .. 4096
// classes, where the 2048-slot table thrashes and every entry goes to the L2-resident global table: 306 us against 316 us
// for the insert pass at 3000 classes, N = 4096 -- with thousands of distinct signatures the lookups are random LDS
// accesses, 4-5 lanes per bank, and cost what the L2 lookups cost; removed.  THREADS stays a parameter.)
template <class SRC, int INSERT_PER_THREAD, int LDS_SLOTS, int THREADS = REFINE_THREADS>
__global__ void __launch_bounds__(THREADS)
refine_insert_kernel(int64_t len, const SRC src,
                     uint32_t* __restrict__ slot_out, RefSlot* __restrict__ tab, uint32_t mask, uint32_t* counters) {
    constexpr int INSERT_CHUNK = THREADS * INSERT_PER_THREAD;
    // The LDS table lives across the chunks of a workgroup: a signature is published to the
    // global table only the first time the workgroup meets it (its chunks come in increasing
    // index order, so that chunk also holds the workgroup's smallest index of the class); later
    // chunks reuse the resolved global slot.  The table is reset when it gets half full.
    extern __shared__ __attribute__((aligned(16))) unsigned long long ri_dyn[];
    __shared__ unsigned long long l_sig_st[LDS_SLOTS <= 2048 ? LDS_SLOTS : 1];
    __shared__ uint32_t l_min_st[LDS_SLOTS <= 2048 ? LDS_SLOTS : 1];
    __shared__ uint32_t l_gslot_st[LDS_SLOTS <= 2048 ? LDS_SLOTS : 1];
    unsigned long long* l_sig = LDS_SLOTS <= 2048 ? l_sig_st : ri_dyn;
    uint32_t* l_min = LDS_SLOTS <= 2048 ? l_min_st : reinterpret_cast<uint32_t*>(ri_dyn + LDS_SLOTS);
    uint32_t* l_gslot = LDS_SLOTS <= 2048 ? l_gslot_st : reinterpret_cast<uint32_t*>(ri_dyn + LDS_SLOTS) + LDS_SLOTS;
    __shared__ uint32_t l_count, l_overflow, l_new;
    constexpr uint32_t PENDING = 0xFFFFFFFEu;
    const int64_t nchunk = (len + INSERT_CHUNK - 1) / INSERT_CHUNK;
    bool need_clear = true, bypass = false;
    // (Round 3 tried issuing the loads of a workgroup's NEXT chunk before hashing and probing the current one -- PMC
    // showed two thirds of the wave cycles in s_waitcnt on the chunk's own loads.  The prefetched registers took the
    // joint source from 71 to 172 VGPRs (2 waves per SIMD instead of 7) and the pass got SLOWER at every grid size
    // tried, 1-6 workgroups per CU: refine phase of theta_c32xk128 0.91-1.17 ms against 0.79.  Latency is hidden by
    // resident workgroups here, not by software pipelining; removed.
    // Two more forms measured and removed in round 3 (both bit-exact on the golden partitions): per-old-class candidate
    // lists in LDS compared word by word, so that only NEW classes are hashed (joint pass 94 us against 80, with 8 or 4
    // candidates per class: the extra LDS reads cost more than the nine 64-bit multiplies they replace); and the waves
    // of a workgroup running free inside a chunk -- creator lanes resolve their own slots, other waves spin on the LDS
    // word, one barrier per chunk instead of three -- 80.3 us against 79.6: the barriers are not what the waves wait for.)
    int ri_it = -1;
    (void)ri_it;
    for (int64_t blk = blockIdx.x; blk < nchunk; blk += gridDim.x) {
        ++ri_it;
        RI_STAMP(0);
        if (need_clear) {
            for (int i = threadIdx.x; i < LDS_SLOTS; i += THREADS) {
                l_sig[i] = 0ull;
                l_min[i] = 0xFFFFFFFFu;
            }
            if (threadIdx.x == 0) l_count = 0;
        }
        if (threadIdx.x == 0) {
            l_overflow = __builtin_nontemporal_load(&counters[1]);
            l_new = 0;
        }
        __syncthreads();
        RI_STAMP(1);
        if (l_overflow) return;  // uniform: the host repeats the pass with a larger table
        const int64_t base = blk * INSERT_CHUNK;
        if (bypass) {
            // many classes (the previous chunk half filled the LDS table on its own): the LDS level only costs probes,
            // every entry goes to the global table directly.  The table is write-once, so the usual case -- the signature
            // already sits in its home slot -- is a plain read: eight entries' home slots are read together, then their
            // minima (round 5; entry by entry this was two dependent L2 round trips per entry, 340 us at 3000 classes and
            // 16.7 M entries).  Whatever the read does not settle (an empty or foreign slot) takes the probing path.
            constexpr int BB = INSERT_PER_THREAD < 8 ? INSERT_PER_THREAD : 8;
#pragma unroll
            for (int q0 = 0; q0 < INSERT_PER_THREAD; q0 += BB) {
                uint64_t sb[BB];
                unsigned long long cur[BB];
                uint32_t outs[BB], mn[BB];
#pragma unroll
                for (int q = 0; q < BB; ++q) {
                    const int64_t e = base + (q0 + q) * THREADS + threadIdx.x;
                    sb[q] = (e < len) ? src(e) : 0ull;
                }
#pragma unroll
                for (int q = 0; q < BB; ++q) {  // the home slot, signature and minimum in one 16-byte gather
                    const uint4 rec = sb[q] ? *reinterpret_cast<const uint4*>(&tab[(uint32_t)sb[q] & mask]) : make_uint4(0u, 0u, 0u, 0u);
                    cur[q] = (unsigned long long)rec.x | ((unsigned long long)rec.y << 32);
                    mn[q] = rec.z;
                }
#pragma unroll
                for (int q = 0; q < BB; ++q) {
                    outs[q] = NO_SLOT;
                    if (sb[q]) {
                        if (cur[q] == sb[q]) {
                            outs[q] = (uint32_t)sb[q] & mask;
                        } else {
                            outs[q] = global_find_or_insert(sb[q], tab, mask, counters);
                            mn[q] = outs[q] != NO_SLOT ? tab[outs[q]].min : 0u;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < BB; ++q) {
                    const int64_t e = base + (q0 + q) * THREADS + threadIdx.x;
                    if (outs[q] != NO_SLOT && mn[q] > (uint32_t)e) atomicMin(&tab[outs[q]].min, (uint32_t)e);
                    if (e < len) slot_out[e] = outs[q];
                }
            }
            continue;
        }
        // >= 0: LDS slot; -1: zero signature; <= -2: already resolved global slot (-2 - g)
        int myslot[INSERT_PER_THREAD];
        // all 16 signature loads are issued before the first probe: the probe loop contains LDS
        // atomics, which the compiler will not move global loads across
        uint64_t sgs[INSERT_PER_THREAD];
        bool walked = false;
        if constexpr (SRC::kIJ) {
            if (src.walks()) {  // uniform
                walked = true;
                const int nn = src.order();
                const bool low = src.lower();
                uint32_t wi = 0, wj = 0;
                if (base + threadIdx.x < len) IjWalk::locate(nn, low, base + threadIdx.x, wi, wj);
                // SRC::kFetchBatch entries are loaded before their signatures are formed.  `sgs[q] = sig(fetch(..))` entry by entry,
                // with the walk's column-wrap loop between two entries, compiles to load - wait - hash per entry: eight dependent
                // memory round trips per chunk (round 4, profiles/r04_insert_phases.txt: 9-10 us of a 14 us chunk for the pair
                // source, 4.5-7 of 10 for the channel source).  The batch is bounded by registers: all 8 entries at once take
                // the channel source from 71 to 138 registers and the joint source to 199 (2-3 resident workgroups per CU instead
                // of 5) and make them slower, 65 -> 73 and 82 -> 114 us.  Kept where it measured faster: the pair source with all 8
                // (71 -> 54 us, four workgroups per CU), the channel source with 4 (65 -> 58 us); the joint source stays at 1.
                constexpr int FB = SRC::kFetchBatch;
                static_assert(INSERT_PER_THREAD % FB == 0, "");
#pragma unroll
                for (int q0 = 0; q0 < INSERT_PER_THREAD; q0 += FB) {
                    typename SRC::Raw raws[FB];
#pragma unroll
                    for (int q = 0; q < FB; ++q) {
                        const int64_t e = base + (q0 + q) * THREADS + threadIdx.x;
                        if (e < len) raws[q] = src.fetch(wi, wj, e);
                        IjWalk::step(nn, low, wi, wj, THREADS);
                    }
#pragma unroll
                    for (int q = 0; q < FB; ++q) {
                        const int64_t e = base + (q0 + q) * THREADS + threadIdx.x;
                        sgs[q0 + q] = (e < len) ? src.sig(raws[q]) : 0ull;
                    }
                }
            }
        }
        if (!walked) {
#pragma unroll
            for (int q = 0; q < INSERT_PER_THREAD; ++q) {
                const int64_t e = base + q * THREADS + threadIdx.x;
                sgs[q] = (e < len) ? src(e) : 0ull;
            }
        }
        RI_STAMP(2);
#pragma unroll
        for (int q = 0; q < INSERT_PER_THREAD; ++q) {
            const int64_t e = base + q * THREADS + threadIdx.x;
            const uint64_t sg = sgs[q];
            myslot[q] = -1;
            if (sg) {
                uint32_t idx = (uint32_t)(sg >> 40) & (LDS_SLOTS - 1);
                int probes = 0;
                int placed = 0;  // 1: found, 2: inserted by this thread
                while (probes < LDS_MAX_PROBES) {
                    unsigned long long cur = l_sig[idx];
                    if (cur == sg) {
                        placed = 1;
                        break;
                    }
                    if (cur == 0ull) {
                        unsigned long long old = atomicCAS(&l_sig[idx], 0ull, (unsigned long long)sg);
                        if (old == 0ull) {
                            placed = 2;
                            break;
                        }
                        if (old == sg) {
                            placed = 1;
                            break;
                        }
                    }
                    idx = (idx + 1) & (LDS_SLOTS - 1);
                    ++probes;
                }
                if (placed) {
                    if (placed == 2) {
                        l_gslot[idx] = PENDING;
                        atomicAdd(&l_count, 1u);
                        l_new = 1u;
                    }
                    // l_min only decreases: a plain read that is already <= e makes the atomic a
                    // no-op (true for every entry after the first of its class in this thread's
                    // increasing index order, i.e. almost always when classes are few)
                    if (l_min[idx] > (uint32_t)e) atomicMin(&l_min[idx], (uint32_t)e);
                    myslot[q] = (int)idx;
                } else {
                    const uint32_t g = global_find_or_insert(sg, tab, mask, counters);
                    if (g != NO_SLOT) {
                        if (tab[g].min > (uint32_t)e) atomicMin(&tab[g].min, (uint32_t)e);
                        myslot[q] = -2 - (int)g;
                    }
                }
            }
        }
        RI_STAMP(3);
        __syncthreads();
        RI_STAMP(4);
        // publish the signatures this workgroup has not resolved yet (few classes: nothing new after the first chunks,
        // the scan of the table and its barrier are skipped; l_new is uniform after the barrier above)
        if (l_new) {
        for (int i = threadIdx.x; i < LDS_SLOTS; i += THREADS) {
            if (l_sig[i] != 0ull && l_gslot[i] == PENDING) {
                const uint32_t g = global_find_or_insert(l_sig[i], tab, mask, counters);
                // tab_min only ever decreases, so a (possibly stale) plain read that is already
                // <= our candidate proves the atomic cannot change anything: skip it.
                if (g != NO_SLOT) {
                    const uint32_t mine = l_min[i];
                    if (tab[g].min > mine) atomicMin(&tab[g].min, mine);
                }
                l_gslot[i] = g;
            }
        }
        __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < INSERT_PER_THREAD; ++q) {
            const int64_t e = base + q * THREADS + threadIdx.x;
            if (e < len) {
                uint32_t out = NO_SLOT;
                if (myslot[q] >= 0) out = l_gslot[myslot[q]];
                else if (myslot[q] <= -2) out = (uint32_t)(-2 - myslot[q]);
                slot_out[e] = out;
            }
        }
        RI_STAMP(5);
        need_clear = l_count > LDS_SLOTS / 2;  // uniform (read after the barrier above)
        bypass = need_clear;
        __syncthreads();
        RI_STAMP(6);
    }
}

// ---------------------------------------------------------------------------
// The insert pass for the MID regime: ~500 .. 5000 classes.  There the 2048-slot LDS table of the kernel above
// thrashes and every entry becomes a 16-byte gather from the L2-resident global table: one L1 miss per lane, ~5-9 clocks
// per entry and CU, 270-300 us for 16.7 M entries (round 5, profiles/r05_refine_warm_3000_classes_kernel_stats.csv).
// Here ONE workgroup per CU keeps every signature it has met in 128 KB of LDS (MID_SLOTS x {8-byte signature, 4-byte
// word, 4-byte minimum}); a lookup is two LDS reads issued together, eight entries at a time, and the waves run FREE:
// no barrier after the table is cleared.
// The lane whose compare-and-swap puts a signature into the LDS table publishes it: global find-or-insert, minimum, then
// the slot's word = (ordinal of the workgroup's chunk << 20) | global slot.  An entry that finds the word still
// pending is set aside and looked at again behind the chunk's other entries (a bounded number of times; asking the global
// table itself is what thousands of lanes of one large new class would do at the same moment).  The minimum: the workgroup's chunks come in
// increasing index order, so an entry of chunk j cannot lower the minimum of a class published in an OLDER chunk (word
// ordinal < j) and takes its slot at once -- the steady state.  Otherwise (same or newer chunk: the waves drift apart)
// it lowers the slot's LDS minimum first and goes to the global minimum only if it did -- the LDS minimum only ever holds
// indices whose owners do go there.  A table that fills up (probe sequences beyond MID_MAX_PROBES) sends the extra
// signatures to the global table entry by entry.
// A short first launch (PER = 1: sixteen workgroups, one entry per thread, publishing behind a barrier) goes over the first
// 16 384 entries; the full launch preloads its LDS tables with what that published (launch_insert_mid).
// Measured and not kept (3000 classes, N = 4096, stamps below): a barrier per chunk with the new signatures published from a
// list (143 us against 133: every wave sits through every other wave's latencies); the work of a chunk ordered by kind --
// all home slots, then each lane walking only ITS entries that need probing, then the global home slots of all entries
// that need them in one batch -- with the entry picked by select chains (180 us: one lane in five is not in its home
// slot and the probing step, 6-12 us of a chunk, is where the time goes either way).
// ---------------------------------------------------------------------------
constexpr int MID_THREADS = 1024;
constexpr int MID_SLOTS = 8192;
constexpr int MID_PER = 8;
constexpr int MID_MAX_PROBES = 16;
constexpr int MID_FIRST_WGS = 16;  // workgroups that go first, 1024 entries each
constexpr uint32_t MID_PENDING = 0xFFFFFFFFu;
constexpr size_t MID_LDS_BYTES = (size_t)MID_SLOTS * 16;
constexpr int MID_MAX_LOG2CAP = 20;  // the word's low 20 bits; ordinals < 2^11 (len < 2^31, >= 1024-entry chunks, 256 workgroups)

__device__ __forceinline__ uint32_t mid_direct(uint64_t sg, uint32_t e, RefSlot* tab, uint32_t mask, uint32_t* counters) {
    const uint32_t g = global_find_or_insert(sg, tab, mask, counters);
    if (g != NO_SLOT && tab[g].min > e) atomicMin(&tab[g].min, e);
    return g;
}

// What a thread holds of an entry between its loads and its signature: the signature itself (array source) or the raw
// operands of a computed source (SRC::Raw -- the loads of the next chunk stay in flight as raw words, the hash runs when
// the chunk's turn comes).
template <class SRC> struct MidTraits {
    using Raw = typename SRC::Raw;
    static __device__ __forceinline__ uint64_t sig(const SRC& s, const Raw& r) { return s.sig(r); }
};
template <> struct MidTraits<SrcArray> {
    using Raw = uint64_t;
    static __device__ __forceinline__ uint64_t sig(const SrcArray&, const uint64_t& r) { return r; }
};
// the loads of the chunk at `base`, all unconditional (an entry beyond the end reads entry 0 and is masked later)
template <class SRC, int PER>
__device__ __forceinline__ void mid_fetch(const SRC& src, int64_t len, int64_t base, typename MidTraits<SRC>::Raw (&r)[PER]) {
    if constexpr (!SRC::kIJ) {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int64_t e = base + q * MID_THREADS + threadIdx.x;
            r[q] = src(e < len ? e : len - 1);
        }
    } else {
        const bool walk = src.walks();  // uniform
        const int nn = src.order();
        const bool low = src.lower();
        uint32_t wi = 0, wj = 0;
        if (walk) {
            const int64_t e0 = base + threadIdx.x;
            IjWalk::locate(nn, low, e0 < len ? e0 : len - 1, wi, wj);
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int64_t e = base + q * MID_THREADS + threadIdx.x;
            const bool valid = e < len;
            if (walk) {
                r[q] = src.fetch(valid ? wi : 0u, valid ? wj : 0u, valid ? e : 0);
                IjWalk::step(nn, low, wi, wj, MID_THREADS);
            } else {
                const int64_t ec = valid ? e : 0;
                r[q] = src.fetch((uint32_t)ec, 0u, ec);  // (flat: entry e of every operand)
            }
        }
    }
}

#ifdef LK_TIMING
#define MID_STAMP(i)                                                                                                        \
    do {                                                                                                                     \
        if (ri_dbg && (threadIdx.x == 0 || threadIdx.x == 512) && ord < 10 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2)) \
            ri_dbg[(((blockIdx.x ? 1 : 0) * 2 + (threadIdx.x ? 1 : 0)) * 10 + ord) * 8 + (i)] = wall_clock64();                \
    } while (0)
#else
#define MID_STAMP(i)
#endif

// PER: entries per thread and chunk (8; 1 for the few workgroups that go first over the first 8192 entries)
template <class SRC, int PER>
__global__ void __launch_bounds__(MID_THREADS)
refine_insert_mid_kernel(int64_t len, const SRC src, uint32_t* __restrict__ slot_out, RefSlot* __restrict__ tab, uint32_t mask,
                         uint32_t* counters, int preload) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long mid_dyn[];
    unsigned long long* l_sig = mid_dyn;
    uint32_t* l_word = reinterpret_cast<uint32_t*>(mid_dyn + MID_SLOTS);
    uint32_t* l_min = l_word + MID_SLOTS;
    __shared__ uint32_t l_full, l_stop;
    constexpr int CHUNK = MID_THREADS * PER;
    const int64_t nchunk = (len + CHUNK - 1) / CHUNK;
    for (int i = threadIdx.x; i < MID_SLOTS; i += MID_THREADS) {
        l_sig[i] = 0ull;
        l_word[i] = MID_PENDING;
        l_min[i] = 0xFFFFFFFFu;
    }
    if (threadIdx.x == 0) {
        l_full = 0;
        l_stop = 0;
    }
    __syncthreads();
    uint32_t ord = 0;  // ordinal of this workgroup's chunk
    if (preload) {
        // The workgroups that went first (launch below) have published the classes of the first entries of the array, with
        // their final minima: no later index can lower them.  Every workgroup of the full launch starts with those in its LDS
        // table, as if met in a chunk before its first -- instead of meeting them one by one in its first chunk, eight steps of
        // two or three dependent L2 round trips each (48 us of the 122 us this kernel took at 3000 classes).
        for (uint32_t g = threadIdx.x; g <= mask; g += MID_THREADS) {
            const uint4 rec = *reinterpret_cast<const uint4*>(&tab[g]);
            const unsigned long long sg = (unsigned long long)rec.x | ((unsigned long long)rec.y << 32);
            if (!sg) continue;
            uint32_t idx = __umulhi((uint32_t)(sg >> 32), (uint32_t)MID_SLOTS);
            for (int probes = 0; probes < MID_MAX_PROBES; ++probes) {
                if (atomicCAS(&l_sig[idx], 0ull, sg) == 0ull) {  // (the global table holds a signature once)
                    l_word[idx] = g;  // ordinal 0
                    break;
                }
                idx = (idx + 1) & (MID_SLOTS - 1);
            }
        }
        if (threadIdx.x == 0 && counters[1]) l_stop = 1u;  // the table was too small already for the first entries: the host repeats the pass
        __syncthreads();
        if (l_stop) return;
        ord = 1;
    }
    // The signatures of the NEXT chunk are in flight while this one is looked up.  The loads are unconditional (index
    // clamped): a load under a branch makes the number of outstanding loads unknown to the compiler, and every wait
    // becomes a wait for all of them -- the prefetch included.
    // (A source whose raw entries of a chunk do not fit 32 registers loads them when the chunk's turn comes: the joint source's
    // 56 prefetched registers made SrcJoint<2, 2> spill, 107 us per launch.)
    using RawT = typename MidTraits<SRC>::Raw;
    constexpr bool PF = sizeof(RawT) * PER <= 128;
    RawT nxt[PER];
    if constexpr (PF) mid_fetch<SRC, PER>(src, len, (int64_t)blockIdx.x * CHUNK, nxt);
    for (int64_t blk = blockIdx.x; blk < nchunk; blk += gridDim.x, ++ord) {
        const int64_t base = blk * CHUNK;
        uint64_t sgs[PER];
        uint32_t home[PER];  // LDS slot: the home slot first, the slot found or taken after the probing step
        unsigned long long cur[PER];
        uint32_t word[PER];
        MID_STAMP(0);
        if constexpr (!PF) mid_fetch<SRC, PER>(src, len, base, nxt);
#pragma unroll
        for (int q = 0; q < PER; ++q) sgs[q] = (base + q * MID_THREADS + threadIdx.x < len) ? MidTraits<SRC>::sig(src, nxt[q]) : 0ull;
        if constexpr (PF) mid_fetch<SRC, PER>(src, len, (blk + gridDim.x) * CHUNK, nxt);
        // (the overflow flag: thread 0 reads it for the workgroup -- 4096 waves asking one address every chunk queue up there)
        if (threadIdx.x == 0 && counters[1]) l_stop = 1u;
        // the home slots of all entries, both words, before anything depends on them
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            home[q] = __umulhi((uint32_t)(sgs[q] >> 32), (uint32_t)MID_SLOTS);
            cur[q] = l_sig[home[q]];
            word[q] = l_word[home[q]];
        }
        const bool full = l_full != 0;
        const bool overflow = l_stop != 0;
#ifdef LK_TIMING
        if (cur[0] == 1ull) continue;  // (never: the stamp below waits for the LDS reads)
#endif
        MID_STAMP(1);
        uint32_t deferred = 0, lowered = 0;  // bit q: entry q waits for another lane to publish its signature / has lowered the slot's LDS minimum
        if constexpr (PER == 1) {
            // The workgroups that go first: one chunk each (gridDim.x = nchunk), every signature new to the workgroup, and with
            // few classes a thousand lanes meet the same one at the same moment.  Barrier-free, every lane that finds the word
            // pending asks the global table itself: 16 384 lanes on a handful of addresses (99 us at 3 classes).  Here the lanes
            // only leave their index in the slot's LDS minimum; after a barrier the lane that inserted the signature publishes
            // it with that minimum; after another everybody reads the word.
            const int64_t e = base + threadIdx.x;
            const uint64_t sg = sgs[0];
            uint32_t idx = home[0];
            int placed = (sg && cur[0] == sg) ? 1 : 0;
            if (sg && !placed) {
                for (int probes = 0; probes < MID_MAX_PROBES; ++probes) {
                    const unsigned long long c = l_sig[idx];
                    if (c == sg) {
                        placed = 1;
                        break;
                    }
                    if (c == 0ull) {
                        const unsigned long long old = atomicCAS(&l_sig[idx], 0ull, (unsigned long long)sg);
                        if (old == 0ull) {
                            placed = 2;
                            break;
                        }
                        if (old == sg) {
                            placed = 1;
                            break;
                        }
                    }
                    idx = (idx + 1) & (MID_SLOTS - 1);
                }
            }
            if (placed && l_min[idx] > (uint32_t)e) atomicMin(&l_min[idx], (uint32_t)e);
            __syncthreads();
            uint32_t out = NO_SLOT;
            if (placed == 2) {
                out = global_find_or_insert(sg, tab, mask, counters);
                if (out != NO_SLOT) {
                    const uint32_t mine = l_min[idx];
                    if (tab[out].min > mine) atomicMin(&tab[out].min, mine);
                    l_word[idx] = (ord << 20) | out;
                }
            } else if (sg && !placed) {
                out = mid_direct(sg, (uint32_t)e, tab, mask, counters);  // (a probe sequence beyond MID_MAX_PROBES)
            }
            __syncthreads();
            if (placed == 1) {
                const uint32_t w = l_word[idx];
                out = w != MID_PENDING ? (w & 0xFFFFFu) : NO_SLOT;  // (pending still: the global table has overflowed)
            }
            if (e < len) slot_out[e] = out;
            (void)full;
            (void)word;
            (void)overflow;
            return;
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int64_t e = base + q * MID_THREADS + threadIdx.x;
            const uint64_t sg = sgs[q];
            uint32_t out = NO_SLOT;
            if (sg) {
                if (cur[q] == sg && (word[q] >> 20) < ord) {  // published in an older chunk: the steady state (a pending word is all ones)
                    out = word[q] & 0xFFFFFu;
                } else {
                    // probe (the table is insert-only, signatures are write-once)
                    uint32_t idx = home[q];
                    int placed = cur[q] == sg ? 1 : 0;  // 1: found, 2: inserted here
                    if (!placed) {
                        for (int probes = 0; probes < MID_MAX_PROBES; ++probes) {
                            const unsigned long long c = l_sig[idx];
                            if (c == sg) {
                                placed = 1;
                                break;
                            }
                            if (c == 0ull) {
                                if (full) break;  // (no new signatures into a table whose probe sequences have got long)
                                const unsigned long long old = atomicCAS(&l_sig[idx], 0ull, (unsigned long long)sg);
                                if (old == 0ull) {
                                    placed = 2;
                                    break;
                                }
                                if (old == sg) {
                                    placed = 1;
                                    break;
                                }
                            }
                            idx = (idx + 1) & (MID_SLOTS - 1);
                        }
                    }
                    if (!placed) {
                        if (!full) l_full = 1u;
                        out = mid_direct(sg, (uint32_t)e, tab, mask, counters);
                    } else {
                        const uint32_t w = placed == 2 ? MID_PENDING : l_word[idx];
                        if (w != MID_PENDING && (w >> 20) < ord) {
                            out = w & 0xFFFFFu;
                        } else {
                            // same or newer chunk, or not published yet: this entry may hold the class's smallest index
                            const bool lowers = l_min[idx] > (uint32_t)e && atomicMin(&l_min[idx], (uint32_t)e) > (uint32_t)e;
                            if (w != MID_PENDING) {
                                out = w & 0xFFFFFu;
                                if (lowers && tab[out].min > (uint32_t)e) atomicMin(&tab[out].min, (uint32_t)e);
                            } else if (placed == 2) {
                                out = global_find_or_insert(sg, tab, mask, counters);
                                if (out != NO_SLOT) {
                                    if (lowers && tab[out].min > (uint32_t)e) atomicMin(&tab[out].min, (uint32_t)e);
                                    l_word[idx] = (ord << 20) | out;
                                }
                            } else {
                                // Somebody else is publishing this signature right now.  Asking the global table too is what
                                // every lane of a LARGE new class would do at the same moment (a class that is absent from the
                                // entries the first workgroups saw -- ER(7) x K_72 is not vertex-transitive -- met by thousands of
                                // lanes of every workgroup in its first chunk: 90 us instead of 45).  The entry waits its turn
                                // after the chunk's other entries; the word is there by then.
                                home[q] = idx;
                                deferred |= 1u << q;
                                if (lowers) lowered |= 1u << q;
                                continue;
                            }
                        }
                    }
                }
            }
            if (e < len) slot_out[e] = out;
        }
        for (int tries = 0; deferred && tries < 64; ++tries) {
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                if (!((deferred >> q) & 1u)) continue;
                const uint32_t w = l_word[home[q]];
                if (w == MID_PENDING) continue;
                const uint32_t e = (uint32_t)(base + q * MID_THREADS + threadIdx.x);
                const uint32_t out = w & 0xFFFFFu;
                if (((lowered >> q) & 1u) && tab[out].min > e) atomicMin(&tab[out].min, e);
                slot_out[e] = out;
                deferred &= ~(1u << q);
            }
            if (deferred) __builtin_amdgcn_s_sleep(16);
        }
        if (deferred) {  // (the publisher got no slot: the global table has overflowed, the host repeats the pass)
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                if (!((deferred >> q) & 1u)) continue;
                const uint32_t e = (uint32_t)(base + q * MID_THREADS + threadIdx.x);
                const uint32_t out = global_find_or_insert(sgs[q], tab, mask, counters);
                if (out != NO_SLOT && ((lowered >> q) & 1u) && tab[out].min > e) atomicMin(&tab[out].min, e);
                slot_out[e] = out;
            }
        }
        MID_STAMP(2);
        if (overflow) return;  // the host repeats the pass with a larger table (each wave leaves on its own: no barriers in this loop)
    }
}

// Which sources have the one-workgroup-per-CU kernel (SRC::kMid; each costs two more instantiations of a large kernel):
// the ones the loop of admissible_subspace runs on the benchmark shapes and the array source.
// (Measured and not kept: the joint source.  SrcJoint<2, 2> with its raw entries prefetched spills (107 us per launch at
// N = 4104), without the prefetch it takes 78 - 88 + 8 us against 71 + 18 for the 256-thread kernel.  The channel source gains
// only with the deferral in the kernel: ER(7) x K_72 is not vertex-transitive, and its large classes that the first
// workgroups never saw took the full launch from 47 to 90 us.)

template <class SRC>
bool mid_set_attributes_kind() {
    static_assert(SRC::kMid, "");
    bool ok = true;
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&refine_insert_mid_kernel<SRC, MID_PER>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)MID_LDS_BYTES);
    ok &= hipSuccess == hipFuncSetAttribute(reinterpret_cast<const void*>(&refine_insert_mid_kernel<SRC, 1>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)MID_LDS_BYTES);
    return ok;
}

template <class SRC>
static void launch_insert_mid(hipStream_t s, int64_t len, const SRC& src, uint32_t* slot, const RefineWs& ws, size_t cap) {
    const int64_t nchunk = (len + MID_THREADS * MID_PER - 1) / (MID_THREADS * MID_PER);
    // A few workgroups first, over the first entries (as in launch_insert, and for the same reason: 256 workgroups publishing
    // the same signatures at the same moment are compare-and-swaps and minimum atomics on one address each; the first 16 384
    // entries hold all but a dozen of 3000 classes, with their smallest indices).  Sixteen workgroups with one entry per
    // thread: one round of probing and publishing each.  The full launch preloads its LDS tables with what they published.
    const bool first = nchunk > 4 && !(ws.mid & 2);
    if (first)
        refine_insert_mid_kernel<SRC, 1><<<MID_FIRST_WGS, MID_THREADS, MID_LDS_BYTES, s>>>((int64_t)MID_THREADS * MID_FIRST_WGS, src, slot, ws.tab,
                                                                                       (uint32_t)(cap - 1), ws.counters, 0);
#ifdef LK_TIMING
    long long* dbg = nullptr;
    if (dbg_on()) {
        hipMalloc(&dbg, 4 * 10 * 8 * 8);
        hipMemset(dbg, 0, 4 * 10 * 8 * 8);
        hipStreamSynchronize(s);
        hipMemcpyToSymbol(HIP_SYMBOL(ri_dbg), &dbg, sizeof(dbg));
    }
#endif
    refine_insert_mid_kernel<SRC, MID_PER><<<(unsigned)(nchunk < 256 ? nchunk : 256), MID_THREADS, MID_LDS_BYTES, s>>>(
        len, src, slot, ws.tab, (uint32_t)(cap - 1), ws.counters, first ? 1 : 0);
#ifdef LK_TIMING
    if (dbg) {
        hipStreamSynchronize(s);
        long long h[4 * 10 * 8];
        hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost);
        for (int w = 0; w < 4; ++w)
            for (int o = 0; o < 10; ++o) {
                const long long* t = &h[(w * 10 + o) * 8];
                if (!t[0]) continue;
                fprintf(stderr, "[mid timing] wg=%d wave=%d chunk=%d: start %8.2f us, home slots read +%6.2f, chunk done +%6.2f\n", w / 2, (w % 2) * 8, o,
                        (t[0] - h[0]) * 0.01, (t[1] - t[0]) * 0.01, (t[2] - t[0]) * 0.01);
            }
        long long* z = nullptr;
        hipMemcpyToSymbol(HIP_SYMBOL(ri_dbg), &z, sizeof(z));
        hipFree(dbg);
    }
#endif
}

// SLOTS: entries of the workgroup's LDS table (16 bytes each): 2048 -> four workgroups per CU,
// 1024 -> up to eight (the computed sources are bound by their hash arithmetic and by the
// barriers between the phases of a chunk: more resident workgroups overlap those phases)
template <class SRC>
void launch_insert(hipStream_t s, int g_chunks_cap, int64_t len, const SRC& src, uint32_t* slot, const RefineWs& ws,
                   size_t cap) {
    constexpr int PER = SRC::kInsertPer, SLOTS = SRC::kLdsSlots;
    if constexpr (SRC::kMid) {
        if (ws.mid) {
            launch_insert_mid<SRC>(s, len, src, slot, ws, cap);
            return;
        }
    }
    const int64_t nchunk = (len + REFINE_THREADS * PER - 1) / (REFINE_THREADS * PER);
    // resident workgroups per CU, measured 2..8: 5 is the minimum of a flat curve (sdpsr_opts.insert_wgs_per_cu overrides)
    // (a fetch-first source holds its raw entries in registers: 126 of them, four workgroups per CU are resident)
    if (SLOTS == 1024) g_chunks_cap = 256 * (ws.insert_wgs_per_cu > 0 ? ws.insert_wgs_per_cu : (SRC::kFetchBatch >= 8 ? 4 : 5));
    const int g = (int)(nchunk < g_chunks_cap ? nchunk : g_chunks_cap);
#ifdef LK_TIMING
    long long* dbg = nullptr;
    if (dbg_on()) {
        hipMalloc(&dbg, 3 * 4 * 8 * 8);
        hipMemset(dbg, 0, 3 * 4 * 8 * 8);
        hipMemcpyToSymbol(HIP_SYMBOL(ri_dbg), &dbg, sizeof(dbg));
    }
#endif
    // Few classes: every workgroup meets the same few dozen signatures in its first chunk and publishes them to the global
    // table at the same moment -- ~1000 compare-and-swaps and minimum atomics per signature on one address each, 12-20 us
    // of the first chunk (why the pair source took 78 us at 34 classes and 55 us at 3).  ONE workgroup
    // goes first over the first chunk: it publishes what that chunk holds with their smallest indices, and the full
    // launch then finds those signatures by plain reads (slots are write-once) and minima it cannot lower.
    if (ws.log2cap <= 12 && nchunk > 4) {
        const int64_t first = (int64_t)REFINE_THREADS * PER;
        refine_insert_kernel<SRC, PER, SLOTS><<<1, REFINE_THREADS, 0, s>>>(first < len ? first : len, src, slot, ws.tab,
                                                                    (uint32_t)(cap - 1), ws.counters);
    }
    refine_insert_kernel<SRC, PER, SLOTS><<<g, REFINE_THREADS, 0, s>>>(len, src, slot, ws.tab,
                                                                (uint32_t)(cap - 1), ws.counters);
#ifdef LK_TIMING
    if (dbg) {
        hipStreamSynchronize(s);
        long long h[3 * 4 * 8];
        hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost);
        for (int w = 0; w < 3; ++w)
            for (int it = 0; it < 4; ++it) {
                const long long* t = &h[(w * 4 + it) * 8];
                if (!t[0]) continue;
                fprintf(stderr, "[insert timing] %s grid=%d len=%lld wg=%d chunk=%d:", __PRETTY_FUNCTION__ + 40, g, (long long)len, w, it);
                for (int i = 1; i < 7; ++i) fprintf(stderr, " %6.2f", t[i] ? (t[i] - t[0]) * 0.01 : -1.0);
                fprintf(stderr, "  (start rel. to wg0 chunk0 %.2f)\n", (t[0] - h[0]) * 0.01);
            }
        long long* z = nullptr;
        hipMemcpyToSymbol(HIP_SYMBOL(ri_dbg), &z, sizeof(z));
        hipFree(dbg);
    }
#endif
}

// A family file lists its sources once, as  #define FAMILY(X) X(SrcA) X(SrcB<1, 2>) ...  and expands the list twice:
// FAMILY(SDPSR_INSERT_INSTANTIATE) compiles launch_insert<SRC> -- and the insert kernels it launches -- for every source;
// FAMILY(SDPSR_INSERT_MID_ATTRIBUTE), inside the file's attribute setter (`bool ok` in scope), sets the dynamic-LDS
// attribute of the mid kernels of exactly the sources with SRC::kMid.
template <class SRC>
bool mid_set_attributes_if_mid() {
    if constexpr (SRC::kMid) return mid_set_attributes_kind<SRC>();
    else return true;
}
#define SDPSR_INSERT_INSTANTIATE(...) \
    template void launch_insert<__VA_ARGS__>(hipStream_t, int, int64_t, const __VA_ARGS__&, uint32_t*, const RefineWs&, size_t);
#define SDPSR_INSERT_MID_ATTRIBUTE(...) ok &= mid_set_attributes_if_mid<__VA_ARGS__>();

}  // namespace sdpsr
