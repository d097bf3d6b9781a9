// The reduced PSD pencil on the device: Z_k(x) = sum_i x_i blks[i][k] (sum(blkD.blks[i] .* x[i] for i = 1:dim(P)),
// docs/src/examples/ErdosRenyiThetaFunction.jl:83, QuadraticAssignmentProblems.jl:136, test/sd_problems.jl:46-52,127-134 of
// the reference), its adjoint, and the spectra of all blocks in one call.  sdpsr_blockop is the handle made from the triplets
// of sdpsr_block_images_sparse; validation, workspaces and the byte accounts live here, the kernels in kernels_blockop.hip
// (operator) and kernels_batched.hip (spectra of the blocks of order <= 64).
#include <new>

#include "host_internal.h"

using namespace sdpsr;

namespace sdpsr {

// out[0 .. nout) = the keyed sums of one arrangement of the handle's records with dv: stream-ordered, no host wait
int blockop_map_enqueue(sdpsr_ctx* c, const sdpsr_blockop* op, bool adjoint, const double* dv, void* carry, double* dout) {
    const int64_t nv = adjoint ? op->sum_sq : op->d, nout = adjoint ? op->d : op->sum_sq;
    if (nout == 0) return SDPSR_OK;
    HIP_TRY(c, hipMemsetAsync(dout, 0, (size_t)nout * 8, c->stream));  // a key without an entry: +0.0
    launch_blockop_keyed_sums(c->stream, op->nnz_full, adjoint ? op->by_class : op->by_pos, dv, nv, carry, dout);
    return SDPSR_OK;
}

}  // namespace sdpsr

namespace {

// the block table: virtual orders, the prefix of their squares; false with a message left in the ctx
bool block_table(sdpsr_ctx* c, const char* who, int32_t nblocks, const int32_t* blk_sizes, std::vector<uint32_t>& pre, int64_t& sum_sq, int64_t& sum_s) {
    if (nblocks < 1 || !blk_sizes) {
        ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": nblocks < 1 or blk_sizes is NULL");
        return false;
    }
    pre.assign((size_t)nblocks + 1, 0u);
    sum_sq = sum_s = 0;
    for (int32_t k = 0; k < nblocks; ++k) {
        const int64_t s = blk_sizes[k];
        if (s < 1) {
            ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": a block size is < 1");
            return false;
        }
        sum_sq += s * s;  // (s < 2^31 and the running sum < 2^32: no overflow)
        sum_s += s;
        if (sum_sq >= (int64_t(1) << 32)) {
            ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": sum s_k^2 >= 2^32: positions are indexed with 32 bits");
            return false;
        }
        pre[(size_t)k + 1] = (uint32_t)sum_sq;
    }
    return true;
}

std::string verdict_message(const unsigned long long* v) {
    const unsigned long long none = ~0ull;
    if (v[BOV_PTR0] != none) return "blockop_create: classptr[0] != 0";
    if (v[BOV_MONOTONE] != none) return "blockop_create: classptr is not monotone at index " + std::to_string(v[BOV_MONOTONE]);
    if (v[BOV_PTREND] != none) return "blockop_create: classptr[d] != nnz";
    const unsigned long long lowest = std::min(v[BOV_BLOCK], std::min(v[BOV_RANGE], v[BOV_TRIANGLE]));
    if (lowest == none) return "";
    if (v[BOV_BLOCK] == lowest) return "blockop_create: entry " + std::to_string(lowest) + ": block index outside [0, nblocks)";
    if (v[BOV_RANGE] == lowest) return "blockop_create: entry " + std::to_string(lowest) + ": row or column outside [0, s_k)";
    return "blockop_create: entry " + std::to_string(lowest) + ": row > col under SDPSR_TRI_UPPER";
}

int create_impl(sdpsr_ctx* c, int32_t nblocks, const std::vector<uint32_t>& pre, int64_t d, int64_t nnz, const int64_t* classptr,
                const int32_t* blk, const int32_t* row, const int32_t* col, const double* val, int triangle, int base, int mem,
                sdpsr_blockop* h) {
    hipStream_t s = c->stream;
    const bool host = mem != SDPSR_MEM_DEVICE;
    const uint64_t h2d0 = c->h2d_bytes, d2h0 = c->d2h_bytes;
    int st = SDPSR_OK;
    // the arrays on the device: the caller's own, or copies in the ctx's workspace
    const int64_t* dptr = classptr ? in_dev(c, "bop_in_ptr", classptr, (size_t)d + 1, mem, &st) : nullptr;
    const int32_t *dblk = blk, *drow = row, *dcol = col;
    const double* dval = val;
    if (nnz > 0) {
        dblk = in_dev(c, "bop_in_blk", blk, (size_t)nnz, mem, &st);
        drow = in_dev(c, "bop_in_row", row, (size_t)nnz, mem, &st);
        dcol = in_dev(c, "bop_in_col", col, (size_t)nnz, mem, &st);
        dval = in_dev(c, "bop_in_val", val, (size_t)nnz, mem, &st);
    }
    const int64_t G = blockop_chunks(nnz);
    unsigned long long* dverdict = (unsigned long long*)ctx_buf(c, "bop_verdict", BOV_WORDS * 8);
    uint32_t* dpre = (uint32_t*)ctx_buf(c, "bop_pre", pre.size() * 4);
    int32_t* dvs = (int32_t*)ctx_buf(c, "bop_vs", h->sizes.size() * 4);
    uint32_t* cnt = (uint32_t*)ctx_buf(c, "bop_cnt", (size_t)std::max<int64_t>(G, 1) * 4);
    int64_t* off = (int64_t*)ctx_buf(c, "bop_off", (size_t)(G + 1) * 8);
    if (!st && (!dverdict || !dpre || !dvs || !cnt || !off)) st = SDPSR_OUT_OF_MEMORY;
    if (!st) st = h2d_sync(c, dpre, pre.data(), pre.size() * 4);
    if (!st) st = h2d_sync(c, dvs, h->sizes.data(), h->sizes.size() * 4);
    if (st) {
        (void)ctx_sync_stream(c, s);  // (pageable sources: nothing reads them after the return)
        return st;
    }
    HIP_TRY(c, hipMemsetAsync(dverdict, 0xFF, BOV_WORDS * 8, s));  // nothing found yet
    if (dptr) launch_blockop_check_classptr(s, d, nnz, dptr, dverdict);
    if (nnz > 0) launch_blockop_check(s, nnz, dblk, drow, dcol, base, triangle == SDPSR_TRI_UPPER, nblocks, dpre, dvs, dverdict, cnt, off);
    HIP_TRY(c, hipGetLastError());
    // the one host wait of a creation: is the input well-formed, and the full entry count, which sizes the handle's arrays
    unsigned long long v[BOV_WORDS];
    st = d2h_sync(c, v, dverdict, sizeof(v));
    if (st) return st;
    const std::string bad = verdict_message(v);
    if (!bad.empty()) return ctx_fail(c, SDPSR_BAD_ARGUMENT, bad);
    const int64_t nf = nnz > 0 ? (int64_t)v[BOV_TOTAL] : 0;
    if (nf >= (int64_t(1) << 32)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop_create: full entry count >= 2^32: entries are indexed with 32 bits");
    h->nnz_full = nf;
    if (nf > 0) {
        if (hipMalloc(&h->by_class, (size_t)nf * 16) != hipSuccess || hipMalloc(&h->by_pos, (size_t)nf * 16) != hipSuccess) {
            (void)hipGetLastError();
            return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "sdpsr_blockop_create: device memory");
        }
        uint32_t* poskey = (uint32_t*)ctx_buf(c, "bop_poskey", (size_t)nf * 4);
        uint32_t *kA = (uint32_t*)ctx_buf(c, "bop_ka", (size_t)nf * 4), *kB = (uint32_t*)ctx_buf(c, "bop_kb", (size_t)nf * 4);
        uint32_t *vA = (uint32_t*)ctx_buf(c, "bop_va", (size_t)nf * 4), *vB = (uint32_t*)ctx_buf(c, "bop_vb", (size_t)nf * 4);
        uint32_t* hist = (uint32_t*)ctx_buf(c, "bop_hist", radix_sort_hist_words(nf) * 4);
        if (!poskey || !kA || !kB || !vA || !vB || !hist) return SDPSR_OUT_OF_MEMORY;
        launch_blockop_expand(s, nnz, d, dptr, dblk, drow, dcol, dval, base, triangle == SDPSR_TRI_UPPER, nblocks, dpre, dvs, off, h->by_class, poskey);
        // stable by position: the entries of one position keep their class-major order
        launch_radix_sort_pairs(s, nf, std::max(1, ceil_log2((uint64_t)h->sum_sq)), poskey, kA, kB, vA, vB, hist);
        launch_blockop_gather(s, nf, vB, h->by_class, h->by_pos);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, ctx_sync_stream(c, s));  // the handle is complete on return (and the caller's arrays are free)
    }
    // what this entry moved: the arrays and the verdict words (the block table's words are not part of its account)
    c->h2d_bytes = h2d0 + (host ? (dptr ? (uint64_t)(d + 1) * 8 : 0) + (uint64_t)nnz * 20 : 0);
    c->d2h_bytes = d2h0 + BOV_WORDS * 8;
    return SDPSR_OK;
}

int check_op(sdpsr_ctx* c, const sdpsr_blockop* op, const char* who) {
    if (!op) return ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": no handle");
    if (op->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, std::string(who) + ": the handle lives on another device");
    return SDPSR_OK;
}

// the public form of blockop_map_enqueue: v (nv elements) and out (nout) in `mem`; every element of out is written
int keyed_map(sdpsr_ctx* c, const sdpsr_blockop* op, bool adjoint, const double* v, int64_t nv, double* out, int64_t nout, int mem,
              const char* in_name, const char* out_name) {
    if ((nv > 0 && !v) || (nout > 0 && !out)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop: a NULL vector");
    if (nout == 0) return SDPSR_OK;
    hipStream_t s = c->stream;
    int st = SDPSR_OK;
    const double* dv = in_dev(c, in_name, v, (size_t)nv, mem, &st);
    double* dout = out_dev(c, out_name, out, (size_t)nout, mem, &st);
    void* carry = ctx_buf(c, "bop_carry", blockop_carry_bytes(op->nnz_full));
    if (st || !dout || !carry) {
        (void)ctx_sync_stream(c, s);
        return st ? st : SDPSR_OUT_OF_MEMORY;
    }
    st = blockop_map_enqueue(c, op, adjoint, dv, carry, dout);
    if (st) return st;
    HIP_TRY(c, hipGetLastError());
    return out_finish(c, out, dout, (size_t)nout, mem);
}

}  // namespace

extern "C" {

int sdpsr_blockop_create(sdpsr_ctx* c, int32_t nblocks, const int32_t* blk_sizes, int64_t d, int64_t nnz, const int64_t* classptr,
                         const int32_t* blk, const int32_t* row, const int32_t* col, const double* val, int triangle, int index_base, int mem,
                         sdpsr_blockop** out) {
    CHECK_CTX(c);
    if (!out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop_create: the handle pointer is NULL");
    *out = nullptr;
    if (index_base != 0 && index_base != 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop_create: index_base is 0 or 1");
    if (triangle != SDPSR_TRI_UPPER && triangle != SDPSR_TRI_FULL) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop_create: triangle is SDPSR_TRI_UPPER or SDPSR_TRI_FULL");
    if (d < 0 || d > 0x7FFFFFFFll || nnz < 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop_create: d < 0, d >= 2^31 or nnz < 0");
    if (nnz >= (int64_t(1) << 32)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop_create: full entry count >= 2^32: entries are indexed with 32 bits");
    if (nnz > 0 && (!classptr || !blk || !row || !col || !val)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blockop_create: a NULL array with nnz > 0");
    std::vector<uint32_t> pre;
    int64_t sum_sq = 0, sum_s = 0;
    if (!block_table(c, "blockop_create", nblocks, blk_sizes, pre, sum_sq, sum_s)) return SDPSR_BAD_ARGUMENT;
    sdpsr_blockop* h = new (std::nothrow) sdpsr_blockop();
    if (!h) return SDPSR_OUT_OF_MEMORY;
    h->device = c->device;
    h->d = d;
    h->sum_sq = sum_sq;
    h->sizes.assign(blk_sizes, blk_sizes + nblocks);
    const int st = create_impl(c, nblocks, pre, d, nnz, classptr, blk, row, col, val, triangle, index_base, mem, h);
    if (st) {
        (void)ctx_sync_stream(c, c->stream);  // (nothing of this call is in flight when its arrays are freed)
        sdpsr_blockop_destroy(h);
        return st;
    }
    *out = h;
    return SDPSR_OK;
}

int sdpsr_blockop_destroy(sdpsr_blockop* op) {
    if (!op) return SDPSR_OK;
    DeviceGuard dg(op->device);
    if (op->by_class) hipFree(op->by_class);
    if (op->by_pos) hipFree(op->by_pos);
    delete op;
    return SDPSR_OK;
}

int sdpsr_blockop_info(const sdpsr_blockop* op, int64_t* d, int32_t* nblocks, int64_t* sum_sq, int64_t* nnz_full) {
    if (!op) return SDPSR_BAD_ARGUMENT;
    if (d) *d = op->d;
    if (nblocks) *nblocks = (int32_t)op->sizes.size();
    if (sum_sq) *sum_sq = op->sum_sq;
    if (nnz_full) *nnz_full = op->nnz_full;
    return SDPSR_OK;
}

int sdpsr_blockop_apply(sdpsr_ctx* c, const sdpsr_blockop* op, const double* x, double* Z, int mem) {
    CHECK_CTX(c);
    const int st = check_op(c, op, "blockop_apply");
    if (st) return st;
    return keyed_map(c, op, false, x, op->d, Z, op->sum_sq, mem, "bop_x", "bop_z");
}

int sdpsr_blockop_adjoint(sdpsr_ctx* c, const sdpsr_blockop* op, const double* S, double* g, int mem) {
    CHECK_CTX(c);
    const int st = check_op(c, op, "blockop_adjoint");
    if (st) return st;
    return keyed_map(c, op, true, S, op->sum_sq, g, op->d, mem, "bop_s", "bop_g");
}

int sdpsr_blocks_syev(sdpsr_ctx* c, int32_t nblocks, const int32_t* blk_sizes, const double* Z, double* w, double* V, int mem) {
    CHECK_CTX(c);
    if (!Z || !w) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "blocks_syev: Z or w is NULL");
    std::vector<uint32_t> pre;
    int64_t sum_sq = 0, sum_s = 0;
    if (!block_table(c, "blocks_syev", nblocks, blk_sizes, pre, sum_sq, sum_s)) return SDPSR_BAD_ARGUMENT;
    hipStream_t s = c->stream;
    int st = SDPSR_OK;
    const double* dZ = in_dev(c, "bsy_z", Z, (size_t)sum_sq, mem, &st);
    double* dW = out_dev(c, "bsy_w", w, (size_t)sum_s, mem, &st);
    double* dV = V ? out_dev(c, "bsy_v", V, (size_t)sum_sq, mem, &st) : nullptr;
    if (st) {
        (void)ctx_sync_stream(c, s);
        return st;
    }
    // the blocks of order <= 64: ONE launch (first those of order >= 2, a workgroup each, then those of order 1)
    std::vector<BlocksSyevJob> jobs;
    std::vector<int32_t> large;
    std::vector<int64_t> woff((size_t)nblocks);
    int max_n = 0, njac = 0, n1 = 0;
    int64_t wo = 0, max_large = 0;
    for (int32_t k = 0; k < nblocks; ++k) {
        woff[k] = wo;
        wo += blk_sizes[k];
    }
    for (int32_t k = 0; k < nblocks; ++k)
        if (blk_sizes[k] >= 2 && blk_sizes[k] <= 64) {
            jobs.push_back({(int64_t)pre[k], woff[k], blk_sizes[k], 0});
            max_n = std::max(max_n, (int)blk_sizes[k]);
            ++njac;
        }
    for (int32_t k = 0; k < nblocks; ++k) {
        if (blk_sizes[k] == 1) {
            jobs.push_back({(int64_t)pre[k], woff[k], 1, 0});
            ++n1;
        } else if (blk_sizes[k] > 64) {
            large.push_back(k);
            max_large = std::max<int64_t>(max_large, blk_sizes[k]);
        }
    }
    bool not_converged = false;
    if (!jobs.empty()) {
        BlocksSyevJob* djobs = (BlocksSyevJob*)ctx_buf(c, "bsy_jobs", jobs.size() * sizeof(BlocksSyevJob));
        int* dflag = (int*)ctx_buf(c, "bsy_flag", 16);
        if (!djobs || !dflag) return SDPSR_OUT_OF_MEMORY;
        st = h2d_sync(c, djobs, jobs.data(), jobs.size() * sizeof(BlocksSyevJob));
        if (st) return st;
        HIP_TRY(c, hipMemsetAsync(dflag, 0, 16, s));
        launch_blocks_syev64(s, djobs, njac, n1, max_n, dZ, dW, dV, dflag);
        HIP_TRY(c, hipGetLastError());
        int flag = 0;
        st = d2h_sync(c, &flag, dflag, 4);
        if (st) return st;
        not_converged = flag != 0;
    }
    // the larger ones one by one through sdpsr_syev_f64 (a block is a contiguous s_k x s_k matrix: leading dimension s_k)
    if (!large.empty()) {
        double* scratch = dV ? nullptr : (double*)ctx_buf(c, "bsy_vscratch", (size_t)max_large * max_large * 8);
        if (!dV && !scratch) return SDPSR_OUT_OF_MEMORY;
        for (int32_t k : large) {
            st = sdpsr_syev_f64(c, blk_sizes[k], dZ + pre[k], dW + woff[k], dV ? dV + pre[k] : scratch, SDPSR_MEM_DEVICE);
            if (st == SDPSR_NOT_CONVERGED) {
                not_converged = true;
                continue;
            }
            if (st) return st;
        }
    }
    if (dV) {
        st = out_finish(c, V, dV, (size_t)sum_sq, mem);
        if (st) return st;
    }
    st = out_finish(c, w, dW, (size_t)sum_s, mem);
    if (st) return st;
    if (not_converged) return ctx_fail(c, SDPSR_NOT_CONVERGED, "blocks_syev: the Jacobi sweep limit was reached; outputs are written as they stand");
    return SDPSR_OK;
}

}  // extern "C"
