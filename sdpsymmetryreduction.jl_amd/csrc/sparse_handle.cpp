// The sparse-constraints handle: the constraint matrix A of src/partitions.jl:117-142 (setup stage, projL of src/utils.jl:58-66)
// and of newA = A * PMat (README.md:57-60, docs/src/examples/ReduceAndSolveJuMP.jl:42-51) brought into canonical CSR form ONCE,
// on the device, from host or device arrays; sdpsr_admissible_setup_sparse / _subspace_sparse (setup_csr.cpp) and
// sdpsr_reduce_constraints_sparse (reduce_csr.cpp) then read it where it lies.  The canonical form is the one
// canonicalize_csr (setup_csr.cpp) defines, bit for bit; the kernels are in kernels_csr_canon.hip, the host arithmetic of
// the pass in csr_canon.h (DESIGN.md "A device-resident sparse A").
#include <new>

#include "host_internal.h"

using namespace sdpsr;

namespace {

// the verdict words as they stand on the device now: one small copy into the ctx's pinned words and one host wait
int read_verdict(sdpsr_ctx* c, const CanonVerdict* dv, CanonVerdict& v) {
    uint32_t* pin = c->pinned_small + PINNED_SMALL_CANON.first;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(pin, dv, sizeof(CanonVerdict), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    c->d2h_bytes += sizeof(CanonVerdict);
    std::memcpy(&v, pin, sizeof(CanonVerdict));
    return SDPSR_OK;
}

int create_impl(sdpsr_ctx* c, int64_t len, int64_t m, int64_t nnz, const int64_t* rowptr, const int64_t* colind, const double* val, int base,
                int mem, sdpsr_sparse* h) {
    hipStream_t s = c->stream;
    h->device = c->device;
    h->len = len;
    h->m = m;
    const int64_t n = canon_square_root(len);
    if (m == 0) {  // (as the host pass: nothing is read)
        if (hipMalloc((void**)&h->rowptr, 8) != hipSuccess) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "sdpsr_sparse_create: device memory");
        HIP_TRY(c, hipMemsetAsync(h->rowptr, 0, 8, s));
        HIP_TRY(c, ctx_sync_stream(c, s));
        h->rows_symmetric = n > 0;
        return SDPSR_OK;
    }
    // raw arrays on the device: the caller's own, or copies in the ctx's workspace
    const int64_t* drp = rowptr;
    const int64_t* dci = colind;
    const double* dv = val;
    int st = SDPSR_OK;
    if (mem != SDPSR_MEM_DEVICE) {
        drp = in_dev(c, "canon_raw_rowptr", rowptr, (size_t)(m + 1), mem, &st);
        if (nnz > 0) {
            dci = in_dev(c, "canon_raw_col", colind, (size_t)nnz, mem, &st);
            dv = in_dev(c, "canon_raw_val", val, (size_t)nnz, mem, &st);
        }
        if (st) {
            (void)ctx_sync_stream(c, s);  // (pageable sources: nothing reads them after the return)
            return st;
        }
    }
    const int64_t G = canon_chunks(nnz);
    CanonVerdict* dverdict = (CanonVerdict*)ctx_buf(c, "canon_verdict", sizeof(CanonVerdict));
    uint32_t* col32 = (uint32_t*)ctx_buf(c, "canon_col32", (size_t)std::max<int64_t>(nnz, 1) * 4);
    unsigned char* keep = (unsigned char*)ctx_buf(c, "canon_keep", (size_t)std::max<int64_t>(nnz, 1));
    unsigned short* rel = (unsigned short*)ctx_buf(c, "canon_rel", (size_t)std::max<int64_t>(nnz, 1) * 2);
    int64_t* cnt = (int64_t*)ctx_buf(c, "canon_cnt", (size_t)(G + 1) * 8);
    if (!dverdict || !col32 || !keep || !rel || !cnt || !c->pinned_small) {
        (void)ctx_sync_stream(c, s);
        return SDPSR_OUT_OF_MEMORY;
    }
    CanonVerdict v;
    static_assert(offsetof(CanonVerdict, rowptr0_bad) == 24, "the three lowest-index words come first");
    HIP_TRY(c, hipMemsetAsync(dverdict, 0xFF, 24, s));  // no lowest index yet (CANON_NO_INDEX), nothing raised
    HIP_TRY(c, hipMemsetAsync((char*)dverdict + 24, 0, sizeof(CanonVerdict) - 24, s));
    launch_canon_check(s, len, m, nnz, drp, dci, dv, base, col32, keep, dverdict);
    st = read_verdict(c, dverdict, v);  // host wait 1: is the input well-formed, does any row need the sort
    if (st) return st;
    const std::string bad = canon_validation_message(v);
    if (!bad.empty()) return ctx_fail(c, SDPSR_BAD_ARGUMENT, bad);
    // rowptr is monotone from index_base to index_base + nnz from here on, every column is inside [0, len)
    const uint32_t* ccol = col32;  // column and value of every position of the (row, column) order, and which positions stay
    const double* cval = dv;
    if (v.unsorted) {
        uint32_t* row = (uint32_t*)ctx_buf(c, "canon_row", (size_t)nnz * 4);
        uint32_t *k1A = (uint32_t*)ctx_buf(c, "canon_k1a", (size_t)nnz * 4), *k1B = (uint32_t*)ctx_buf(c, "canon_k1b", (size_t)nnz * 4);
        uint32_t *v1A = (uint32_t*)ctx_buf(c, "canon_v1a", (size_t)nnz * 4), *v1B = (uint32_t*)ctx_buf(c, "canon_v1b", (size_t)nnz * 4);
        uint32_t *k2A = (uint32_t*)ctx_buf(c, "canon_k2a", (size_t)nnz * 4), *k2B = (uint32_t*)ctx_buf(c, "canon_k2b", (size_t)nnz * 4);
        uint32_t *v2A = (uint32_t*)ctx_buf(c, "canon_v2a", (size_t)nnz * 4), *v2B = (uint32_t*)ctx_buf(c, "canon_v2b", (size_t)nnz * 4);
        uint32_t* hist = (uint32_t*)ctx_buf(c, "canon_hist", radix_sort_hist_words(nnz) * 4);
        double* sum = (double*)ctx_buf(c, "canon_sum", (size_t)nnz * 8);
        if (!row || !k1A || !k1B || !v1A || !v1B || !k2A || !k2B || !v2A || !v2B || !hist || !sum) return SDPSR_OUT_OF_MEMORY;
        launch_canon_row_ids(s, nnz, m, drp, base, row);
        // stable by column, then stable by row: the (row, column) order with duplicates in input order
        launch_radix_sort_pairs(s, nnz, canon_sort_bits((uint64_t)len), col32, k1A, k1B, v1A, v1B, hist);
        uint32_t* key2 = col32;  // (the first sort has read its keys)
        launch_canon_gather_u32(s, nnz, v1B, row, key2);
        launch_radix_sort_pairs(s, nnz, canon_sort_bits((uint64_t)m), key2, k2A, k2B, v2A, v2B, hist);
        // (k1A, v1A: free behind the first sort) the sorted columns and the raw index of every position; the runs' sums
        launch_canon_runs(s, nnz, v2B, k1B, v1B, k2B, dv, k1A, v1A, sum, keep, dverdict);
        ccol = k1A;
        cval = sum;
    }
    launch_canon_count_scan(s, nnz, keep, cnt, dverdict);
    st = read_verdict(c, dverdict, v);  // host wait 2: the canonical count, which sizes the handle's arrays
    if (st) return st;
    if (v.dup_nonfinite) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "duplicate entries sum to a non-finite value");
    h->nnz = (int64_t)v.total;
    if (hipMalloc((void**)&h->rowptr, (size_t)(m + 1) * 8) != hipSuccess ||
        (h->nnz > 0 && (hipMalloc((void**)&h->col, (size_t)h->nnz * 4) != hipSuccess || hipMalloc((void**)&h->val, (size_t)h->nnz * 8) != hipSuccess))) {
        (void)hipGetLastError();
        return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "sdpsr_sparse_create: device memory");
    }
    launch_canon_fill(s, nnz, m, keep, ccol, cval, cnt, drp, base, rel, h->rowptr, h->col, h->val);
    if (n > 0) launch_canon_symmetry(s, h->nnz, m, n, h->rowptr, h->col, h->val, dverdict);
    st = read_verdict(c, dverdict, v);  // host wait 3: the arrays are complete, the symmetry verdict
    if (st) return st;
    h->rows_symmetric = n > 0 && !v.asymmetric;
    return SDPSR_OK;
}

}  // namespace

extern "C" {

int sdpsr_sparse_create(sdpsr_ctx* c, int64_t len, int64_t m, int64_t nnz, const int64_t* rowptr, const int64_t* colind, const double* val,
                        int index_base, int mem, sdpsr_sparse** out) {
    CHECK_CTX(c);
    if (!out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    *out = nullptr;
    if (index_base != 0 && index_base != 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "index_base must be 0 or 1");
    int st = check_len(c, len);
    if (st) return st;
    if (m < 0 || nnz < 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    if (m > 0x7FFFFFFF) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "m too large");
    if (nnz >= (int64_t(1) << 32)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "nnz >= 2^32: the entries of A are indexed with 32 bits");
    if (m == 0 && nnz != 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowptr[m] - index_base != nnz");
    if (m > 0 && !rowptr) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "rowptr is NULL");
    if (nnz > 0 && (!colind || !val)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "colind / val is NULL");
    sdpsr_sparse* h = new (std::nothrow) sdpsr_sparse();
    if (!h) return SDPSR_OUT_OF_MEMORY;
    st = create_impl(c, len, m, nnz, rowptr, colind, val, index_base, mem, h);
    if (st) {
        (void)ctx_sync_stream(c, c->stream);  // (nothing of this call is in flight when its arrays are freed)
        sdpsr_sparse_destroy(h);
        return st;
    }
    *out = h;
    return SDPSR_OK;
}

int sdpsr_sparse_destroy(sdpsr_sparse* A) {
    if (!A) return SDPSR_OK;
    DeviceGuard dg(A->device);
    if (A->rowptr) hipFree(A->rowptr);
    if (A->col) hipFree(A->col);
    if (A->val) hipFree(A->val);
    delete A;
    return SDPSR_OK;
}

int sdpsr_sparse_info(const sdpsr_sparse* A, int64_t* len, int64_t* m, int64_t* nnz_canonical, int* rows_symmetric) {
    if (!A) return SDPSR_BAD_ARGUMENT;
    if (len) *len = A->len;
    if (m) *m = A->m;
    if (nnz_canonical) *nnz_canonical = A->nnz;
    if (rows_symmetric) *rows_symmetric = A->rows_symmetric;
    return SDPSR_OK;
}

int sdpsr_sparse_export(sdpsr_ctx* c, const sdpsr_sparse* A, int index_base, int64_t* rowptr, int64_t* colind, double* val, int mem) {
    CHECK_CTX(c);
    if (!A) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "no sparse handle");
    if (A->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "the sparse handle lives on another device");
    if (index_base != 0 && index_base != 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "index_base must be 0 or 1");
    if (!rowptr || (A->nnz > 0 && (!colind || !val))) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    hipStream_t s = c->stream;
    const int64_t m = A->m, nnz = A->nnz;
    int st = SDPSR_OK;
    int64_t* drp = out_dev(c, "canon_exp_rowptr", rowptr, (size_t)(m + 1), mem, &st);
    int64_t* dci = nnz > 0 ? out_dev(c, "canon_exp_col", colind, (size_t)nnz, mem, &st) : nullptr;
    if (st) return st;
    launch_canon_export(s, m, nnz, A->rowptr, A->col, index_base, drp, dci);
    HIP_TRY(c, hipGetLastError());
    if (mem == SDPSR_MEM_DEVICE) {
        if (nnz > 0) HIP_TRY(c, hipMemcpyAsync(val, A->val, (size_t)nnz * 8, hipMemcpyDeviceToDevice, s));
    } else {
        HIP_TRY(c, hipMemcpyAsync(rowptr, drp, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, s));
        if (nnz > 0) {
            HIP_TRY(c, hipMemcpyAsync(colind, dci, (size_t)nnz * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(val, A->val, (size_t)nnz * 8, hipMemcpyDeviceToHost, s));
        }
        c->d2h_bytes += (size_t)(m + 1) * 8 + (size_t)nnz * 16;
    }
    HIP_TRY(c, ctx_sync_stream(c, s));
    return SDPSR_OK;
}

}  // extern "C"
