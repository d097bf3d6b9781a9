// sdpsr_block_images_sparse: the PSD blocks of the reduced SDP as the triplets a solver interface takes (README.md:72-79,
// test/sd_problems.jl:46-52, docs/src/examples/ReduceAndSolveJuMP.jl:56-84 of the reference; the complex route's real
// embedding :59-76).  Validation, the block table, workspaces and the capacity rule live here; the two sweeps and the scan
// are kernels_sparse_images.hip.
#include <cmath>
#include <vector>

#include "host_internal.h"
#include "sparse_images.h"

using namespace sdpsr;

extern "C" {

// Buffers of its own ("bis_*"); nothing the ctx keeps for its block diagonalisations or for sdpsr_basis_image is touched.
int sdpsr_block_images_sparse(sdpsr_ctx* c, int32_t nblocks, const int32_t* blk_sizes, int64_t class_count, const void* blks, int is_complex,
                              int triangle, double tol, int index_base, int64_t capacity, int64_t* classptr, int32_t* blk, int32_t* row,
                              int32_t* col, double* val, int64_t* nnz, double* max_asym, int mem) {
    CHECK_CTX(c);
    if (!blk_sizes || !classptr || !nnz) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: blk_sizes, classptr or nnz is NULL");
    if (nblocks < 1 || class_count < 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: nblocks < 1 or class_count < 0");
    if (!blks && class_count > 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: blks is NULL");
    if (capacity < 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: capacity < 0");
    if (capacity > 0 && (!blk || !row || !col || !val)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: a triplet array is NULL with capacity > 0");
    if (!(tol >= 0)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: tol is negative or NaN");
    if (index_base != 0 && index_base != 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: index_base is 0 or 1");
    if (triangle != SDPSR_TRI_UPPER && triangle != SDPSR_TRI_FULL) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: triangle is SDPSR_TRI_UPPER or SDPSR_TRI_FULL");
    // the block table of the virtual matrices; every count is checked on the way: the window's virtual elements and its bytes fit int64
    std::vector<int64_t> pre((size_t)nblocks + 1, 0);
    std::vector<int32_t> vs((size_t)nblocks);
    const char* too_large = "block_images_sparse: the element count does not fit int64 (or a virtual block's order does not fit int32)";
    int64_t S = 0;
    for (int32_t k = 0; k < nblocks; ++k) {
        const int64_t s = blk_sizes[k], sp = is_complex ? 2 * s : s;
        if (s < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: a block size is < 1");
        if (sp > 0x7FFFFFFEll) return ctx_fail(c, SDPSR_BAD_ARGUMENT, too_large);
        vs[k] = (int32_t)sp;
        if (__builtin_add_overflow(pre[k], sp * sp, &pre[k + 1]) || __builtin_add_overflow(S, s * s, &S)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, too_large);
    }
    const int64_t V = pre[nblocks];
    int64_t N = 0, bytes = 0;
    if (__builtin_mul_overflow(class_count, V, &N) || __builtin_mul_overflow(N, (int64_t)16, &bytes)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, too_large);
    const bool host = mem != SDPSR_MEM_DEVICE;
    hipStream_t s = c->stream;
    if (class_count == 0) {  // no kernel
        *nnz = 0;
        if (max_asym) *max_asym = 0.0;
        if (host) {
            classptr[0] = 0;
        } else {
            HIP_TRY(c, hipMemsetAsync(classptr, 0, 8, s));
            HIP_TRY(c, ctx_sync_stream(c, s));
        }
        return SDPSR_OK;
    }
    if (!host && ((uintptr_t)blks & 7u)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "block_images_sparse: blks is not aligned to 8 bytes");
    const uint64_t h2d0 = c->h2d_bytes, d2h0 = c->d2h_bytes;
    const size_t in_doubles = (size_t)class_count * (size_t)S * (is_complex ? 2 : 1);
    int st = SDPSR_OK;
    const double* in = in_dev(c, "bis_in", (const double*)blks, in_doubles, mem, &st);
    int64_t* d_ptr = out_dev(c, "bis_ptr", classptr, (size_t)class_count + 1, mem, &st);
    if (st || !in || !d_ptr) return st ? st : SDPSR_OUT_OF_MEMORY;
    SparseImagesArgs a{};
    a.blks = in;
    a.N = N;
    a.V = V;
    a.S = S;
    a.head = (!is_complex && ((uintptr_t)in & 15u)) ? 1 : 0;
    a.nchunks = (N + a.head + SI_CHUNK - 1) / SI_CHUNK;
    a.tol = tol;
    a.nb = nblocks;
    a.upper = triangle == SDPSR_TRI_UPPER;
    a.base = index_base;
    int64_t* d_pre = (int64_t*)ctx_buf(c, "bis_pre", pre.size() * 8);
    int32_t* d_vs = (int32_t*)ctx_buf(c, "bis_vs", vs.size() * 4);
    uint32_t* cnt = (uint32_t*)ctx_buf(c, "bis_cnt", (size_t)a.nchunks * 4);
    int64_t* off = (int64_t*)ctx_buf(c, "bis_off", ((size_t)a.nchunks + 1) * 8);
    int64_t* d_res = (int64_t*)ctx_buf(c, "bis_res", 16);  // [0] nnz, [1] the asymmetry maximum's bits
    if (!d_pre || !d_vs || !cnt || !off || !d_res) return SDPSR_OUT_OF_MEMORY;
    st = h2d_sync(c, d_pre, pre.data(), pre.size() * 8);
    if (!st) st = h2d_sync(c, d_vs, vs.data(), vs.size() * 4);
    if (st) return st;
    a.pre = d_pre;
    a.vs = d_vs;
    HIP_TRY(c, hipMemsetAsync(d_res, 0, 16, s));
    launch_sparse_images_count(s, a, is_complex, cnt, max_asym ? (unsigned long long*)(d_res + 1) : nullptr, c->num_cus);
    launch_sparse_images_scan(s, a.nchunks, cnt, off, d_res, d_ptr + class_count);
    HIP_TRY(c, hipGetLastError());
    // the one host wait in front of the second sweep: nnz decides the capacity rule
    int64_t res[2] = {0, 0};
    st = d2h_sync(c, res, d_res, 16);
    if (st) return st;
    const int64_t total = res[0];
    const bool store = total <= capacity && total > 0;
    int32_t *d_blk = blk, *d_row = row, *d_col = col;
    double* d_val = val;
    if (host && store) {
        d_blk = (int32_t*)ctx_buf(c, "bis_blk", (size_t)total * 4);
        d_row = (int32_t*)ctx_buf(c, "bis_row", (size_t)total * 4);
        d_col = (int32_t*)ctx_buf(c, "bis_col", (size_t)total * 4);
        d_val = (double*)ctx_buf(c, "bis_val", (size_t)total * 8);
        if (!d_blk || !d_row || !d_col || !d_val) return SDPSR_OUT_OF_MEMORY;
    }
    launch_sparse_images_fill(s, a, is_complex, off, store ? 1 : 0, store ? total : 0, d_ptr, d_blk, d_row, d_col, d_val, c->num_cus);
    HIP_TRY(c, hipGetLastError());
    if (host) {
        HIP_TRY(c, hipMemcpyAsync(classptr, d_ptr, ((size_t)class_count + 1) * 8, hipMemcpyDeviceToHost, s));
        if (store) {  // nnz entries, not capacity
            HIP_TRY(c, hipMemcpyAsync(blk, d_blk, (size_t)total * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(row, d_row, (size_t)total * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(col, d_col, (size_t)total * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(val, d_val, (size_t)total * 8, hipMemcpyDeviceToHost, s));
        }
    }
    HIP_TRY(c, ctx_sync_stream(c, s));  // outputs are complete on return in both memory spaces
    // what this entry moved: the window, the result words and the outputs (the block table's words are not part of its account)
    c->h2d_bytes = h2d0 + (host ? (uint64_t)in_doubles * 8 : 0);
    c->d2h_bytes = d2h0 + 16 + (host ? ((uint64_t)class_count + 1) * 8 + (store ? (uint64_t)total * 20 : 0) : 0);
    *nnz = total;
    if (max_asym) {
        double m;
        memcpy(&m, &res[1], 8);
        *max_asym = m;
    }
    return SDPSR_OK;
}

}  // extern "C"
