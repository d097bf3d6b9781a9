// What sparse_images.cpp (the entry point sdpsr_block_images_sparse) and kernels_sparse_images.hip (its three kernels) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdpsr {

constexpr int SI_CHUNK = 2048;       // flat virtual elements per chunk: one wave, one count, one offset
constexpr int SI_LDS_BLOCKS = 2048;  // the block table lives in LDS up to this many blocks, in global memory beyond

struct SparseImagesArgs {
    const double* blks;  // the window: class_count * S doubles, or complex numbers as (re, im) pairs
    int64_t N;           // virtual elements of the window, class_count * V
    int64_t V;           // virtual elements of a class: sum of s'_k^2
    int64_t S;           // stored elements of a class: sum of s_k^2 (doubles or complex numbers)
    int64_t nchunks;     // ceil((N + head) / SI_CHUNK)
    const int64_t* pre;  // nb + 1: pre[k] = sum of s'_j^2 over j < k
    const int32_t* vs;   // nb: s'_k
    double tol;
    int32_t nb;
    int32_t head;  // real input at 8 mod 16: 1 -- chunk c starts at flat index c * SI_CHUNK - 1, every 16-byte pair is aligned
    int32_t upper;
    int32_t base;
};

// cnt[nchunks]; asym (may be nullptr): bit pattern of the maximum, zeroed by the caller
void launch_sparse_images_count(hipStream_t s, const SparseImagesArgs& a, int is_complex, uint32_t* cnt, unsigned long long* asym, int num_cus);
// off[nchunks + 1]; *total = *total2 = off[nchunks] (total2 may be nullptr)
void launch_sparse_images_scan(hipStream_t s, int64_t nchunks, const uint32_t* cnt, int64_t* off, int64_t* total, int64_t* total2);
// classptr[0 .. class_count) always; the triplets (cap entries each) when store != 0
void launch_sparse_images_fill(hipStream_t s, const SparseImagesArgs& a, int is_complex, const int64_t* off, int store, int64_t cap,
                               int64_t* classptr, int32_t* blk, int32_t* row, int32_t* col, double* val, int num_cus);

}  // namespace sdpsr
