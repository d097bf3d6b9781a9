// Reduced-SDP assembly from a sparse constraint matrix given as CSR: newA = A * PMat, newC = C' * PMat
// (README.md:57-60, test/sd_problems.jl:32-37,113-118, docs/src/examples/ReduceAndSolveJuMP.jl:42-51).  The rows are validated
// and canonicalised on the host by the CSR setup's canonicalize_csr (O(nnz)), uploaded as CSR and summed per (row, class) on
// the device (kernels_reduce_csr.hip, DESIGN.md "A * PMat from a sparse A").
#include "host_internal.h"

using namespace sdpsr;

extern "C" {

// A * PMat (README.md:57-60)
int sdpsr_reduce_constraints(sdpsr_ctx* c, int64_t len, const uint32_t* labels, int64_t d, int64_t m, const double* A,
                             double* out, int mem) {
    CHECK_CTX(c);
    if (!labels || !A || !out || d < 1 || m < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = check_len(c, len);
    if (st) return st;
    const uint32_t* dL = labels_in_dev(c, "prim_in_a", labels, len, mem, &st);
    const double* dA = in_dev(c, "red_a", A, (size_t)len * m, mem, &st);
    double* dO = out_dev(c, "red_out", out, (size_t)m * d, mem, &st);
    const int64_t chunk = reduce_columns_chunk(len, m, d);
    double* part = (double*)ctx_buf(c, "red_part", (size_t)((len + chunk - 1) / chunk) * d * m * 8);
    // labels beyond d never index the accumulators (the kernel skips the entry and raises the flag)
    uint32_t* flag = (uint32_t*)ctx_buf(c, "prim_flag", 64);
    if (st || !part || !flag || !c->pinned_small) return st ? st : SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemsetAsync(flag, 0, 4, c->stream));
    if (!launch_reduce_columns(c->stream, len, m, d, dL, dA, part, dO, flag))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "dim(P) * min(m, 64) too large for the LDS accumulators");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->pinned_small, flag, 4, hipMemcpyDeviceToHost, c->stream));
    st = out_finish(c, out, dO, (size_t)m * d, mem);
    if (st) return st;
    if (c->pinned_small[0]) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "reduce_constraints: a label exceeds d = dim(P)");
    return SDPSR_OK;
}

int sdpsr_reduce_constraints_csr(sdpsr_ctx* c, int64_t len, const uint32_t* labels, int64_t d, int64_t m, const int64_t* rowptr,
                                 const int64_t* colind, const double* val, int index_base, double* out, int mem) {
    CHECK_CTX(c);
    if (!labels || d < 1 || m < 0 || (m > 0 && !out)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = check_len(c, len);
    if (st) return st;
    if (d > len) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "d > len: more classes than entries");
    if (m > 0x7FFFFFFF) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "m too large");
    CanonCsr A;
    st = canonicalize_csr(c, len, m, rowptr, colind, val, index_base, A);
    if (st) return st;
    const int64_t nnz = (int64_t)A.col.size();
    if (nnz >= (int64_t(1) << 32))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "nnz >= 2^32: the entries of A are indexed with 32 bits");
    if (m == 0) return SDPSR_OK;  // an empty result
    int64_t* drp = nullptr;
    uint32_t* dcol = nullptr;
    double* dval = nullptr;
    if (nnz > 0) {
        hipStream_t s = c->stream;
        drp = (int64_t*)ctx_buf(c, "csr_rowptr", (size_t)(m + 1) * 8);  // (the CSR buffers of the setup entries)
        dcol = (uint32_t*)ctx_buf(c, "csr_col", (size_t)nnz * 4);
        dval = (double*)ctx_buf(c, "csr_val", (size_t)nnz * 8);
        if (!drp || !dcol || !dval) return SDPSR_OUT_OF_MEMORY;
        // (pageable sources: A lives until the return, and the stream is waited for before it)
        HIP_TRY(c, hipMemcpyAsync(drp, A.rowptr.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dcol, A.col.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dval, A.val.data(), (size_t)nnz * 8, hipMemcpyHostToDevice, s));
        c->h2d_bytes += (size_t)(m + 1) * 8 + (size_t)nnz * 12;
    }
    st = reduce_from_device_csr(c, len, labels, d, m, drp, dcol, dval, nnz, out, mem);
    if (st && nnz > 0) (void)ctx_sync_stream(c, c->stream);  // (a failure before the assembly's own wait: the copies still read A)
    return st;
}

// the same assembly on a handle's arrays (sdpsr_sparse_create): no host pass, no upload of A
int sdpsr_reduce_constraints_sparse(sdpsr_ctx* c, const sdpsr_sparse* A, const uint32_t* labels, int64_t d, double* out, int mem) {
    CHECK_CTX(c);
    if (!A) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "no sparse handle");
    if (A->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "the sparse handle lives on another device");
    if (!labels || d < 1 || (A->m > 0 && !out)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    if (d > A->len) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "d > len: more classes than entries");
    if (A->m == 0) return SDPSR_OK;  // an empty result
    return reduce_from_device_csr(c, A->len, labels, d, A->m, A->rowptr, A->col, A->val, A->nnz, out, mem);
}

}  // extern "C"

// The assembly from canonical CSR arrays that are on the device already (m >= 1): every kernel sees the same inputs with the
// same launch geometry whether the arrays came from the host pass or from a handle
int sdpsr::reduce_from_device_csr(sdpsr_ctx* c, int64_t len, const uint32_t* labels, int64_t d, int64_t m, const int64_t* drp,
                                  const uint32_t* dcol, const double* dval, int64_t nnz, double* out, int mem) {
    int st = SDPSR_OK;
    hipStream_t s = c->stream;
    const uint32_t* dL = labels_in_dev(c, "prim_in_a", labels, len, mem, &st);
    double* dO = out_dev(c, "red_out", out, (size_t)m * d, mem, &st);
    uint32_t* flag = (uint32_t*)ctx_buf(c, "prim_flag", 64);
    if (st || !dO || !flag || !c->pinned_small) return st ? st : SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemsetAsync(flag, 0, 4, s));
    launch_labels_exceed(s, len, dL, d, flag);
    // every element of out is written: exact zeros first, then one store per (row, class) pair that has entries
    HIP_TRY(c, hipMemsetAsync(dO, 0, (size_t)m * d * 8, s));
    if (nnz > 0) {
        uint32_t* key = (uint32_t*)ctx_buf(c, "redc_key", (size_t)nnz * 4);
        uint32_t* kA = (uint32_t*)ctx_buf(c, "redc_key_a", (size_t)nnz * 4);
        uint32_t* kB = (uint32_t*)ctx_buf(c, "redc_key_b", (size_t)nnz * 4);
        uint32_t* vA = (uint32_t*)ctx_buf(c, "redc_idx_a", (size_t)nnz * 4);
        uint32_t* vB = (uint32_t*)ctx_buf(c, "redc_idx_b", (size_t)nnz * 4);
        uint32_t* hist = (uint32_t*)ctx_buf(c, "redc_hist", radix_sort_hist_words(nnz) * 4);
        void* carry = ctx_buf(c, "redc_carry", csr_class_sums_carry_bytes(nnz));
        if (!key || !kA || !kB || !vA || !vB || !hist || !carry) return SDPSR_OUT_OF_MEMORY;
        launch_csr_entry_labels(s, nnz, dcol, dL, d, key);
        int bits = 1;
        while (((int64_t)1 << bits) <= d) ++bits;
        launch_radix_sort_pairs(s, nnz, bits, key, kA, kB, vA, vB, hist);
        launch_csr_class_sums(s, nnz, m, drp, kB, vB, dval, carry, dO);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->pinned_small, flag, 4, hipMemcpyDeviceToHost, s));
    st = out_finish(c, out, dO, (size_t)m * d, mem);
    if (st) return st;
    if (c->pinned_small[0]) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "reduce_constraints_csr: a label exceeds d = dim(P)");
    return SDPSR_OK;
}
