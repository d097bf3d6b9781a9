// The global hash table of the canonical refinement: its constants and the find-or-insert that the insert kernels
// (refine_insert.h) run; the ranking and label passes (kernels_refine.hip) and the class-compare checks read the constants.
// Below them, the declarations through which the refinement driver reaches the insert pass of another translation unit.
#pragma once
#include "sdpsr_internal.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// Canonical refinement of 64-bit signatures.
//
//   pass A  every block dedups its REFINE_BLOCK entries in an LDS hash table (sig -> min
//           index), then publishes each distinct signature once to the global table
//           (write-once 64-bit CAS slots + atomicMin of the first index); the global slot
//           of every entry is parked in labels_out.
//   pass B  per block: count entries that are the first occurrence of their class.
//   scan    exclusive scan of the block counts (one block).
//   pass C  rank first occurrences inside the block -> label of the class (1-based, in
//           column-major first-occurrence order = the reference's canonical numbering).
//   pass D  labels_out[e] = label of its slot.
// ---------------------------------------------------------------------------
constexpr int REFINE_THREADS = 256;
constexpr int REFINE_PER_THREAD = 4;
constexpr int REFINE_BLOCK = REFINE_THREADS * REFINE_PER_THREAD;  // 1024 entries
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
constexpr int MAX_PROBES = 512;
// Few-classes fast path: the first SMALL_K distinct signatures also append their global slot to
// a list (counters[LIST_OFF + i]); when the whole partition has <= SMALL_K classes one workgroup
// ranks those slots by first index and the three entry-level ranking passes exit at once.
constexpr uint32_t SMALL_K = 1024;
constexpr int LIST_OFF = 16;
// classes whose first-occurrence index the ranking passes also write to RefineWs::first_idx
constexpr uint32_t REFINE_FIRST_CAP = 65536;

__device__ __forceinline__ uint32_t global_find_or_insert(uint64_t sg, RefSlot* tab,
                                                          uint32_t mask, uint32_t* counters) {
    // (the overflow flag is checked once per chunk by the caller: after an overflow the host
    // repeats the pass with a larger table, nobody should keep walking a full one)
    uint32_t idx = (uint32_t)sg & mask;
    for (int probe = 0; probe < MAX_PROBES; ++probe) {
        // a probe sequence that gets long in a table that has overflowed meanwhile (the flag goes up at 75 %) stops:
        // the host repeats the pass with a larger table anyway.  (A refinement that jumps from a handful of classes to
        // ~len/2 -- partitions without symmetry -- used to walk up to MAX_PROBES slots of the full table for every
        // remaining entry: 1.0 and 1.5 ms per failed attempt at len = 524 800, configs[1].)
        if ((probe & 7) == 7 && __builtin_nontemporal_load(&counters[1])) return NO_SLOT;
        unsigned long long cur = tab[idx].sig;  // slots are write-once: a stale read can only be 0
        if (cur == sg) return idx;
        if (cur == 0ull) {
            unsigned long long old = atomicCAS(&tab[idx].sig, 0ull, (unsigned long long)sg);
            if (old == 0ull) {
                // (one atomic per wave for the lanes that are here together -- ballot, leader, prefix count -- measured: no gain where it
                // could matter, the first workgroups of the one-workgroup-per-CU kernel, and four more registers in every insert kernel:
                // SrcChan<int, 2> went from 5 to 4 resident workgroups per CU, 65 -> 81 us per refinement)
                const uint32_t cnt = atomicAdd(&counters[0], 1u);
                if (cnt < SMALL_K) counters[LIST_OFF + cnt] = idx;
                if (cnt + 1 > (mask >> 1) + (mask >> 2)) counters[1] = 1u;  // > 75% full
                return idx;
            }
            if (old == sg) return idx;
        }
        idx = (idx + 1) & mask;
    }
    counters[1] = 1u;  // overflow: host retries with a larger table
    return NO_SLOT;
}

// The insert pass of a signature source (refine_insert.h).  Every instance is compiled in exactly one of the
// kernels_insert_*.hip files, one per source family; launch_refine (kernels_refine.hip) sees this declaration only, and a
// source without an instance fails the link of the library.
template <class SRC>
__attribute__((visibility("hidden"))) void launch_insert(hipStream_t s, int g_chunks_cap, int64_t len, const SRC& src, uint32_t* slot,
                                                         const RefineWs& ws, size_t cap);

}  // namespace sdpsr
