// basis_image(Q, P; atol) over ComplexF64 (src/diagonalize.jl:64-89, _constraints :42-50; called with the desymmetrized
// partition by src/compat.jl:54-57) of a caller's Q_hat for a window of classes: entry point sdpsr_basis_image_complex.
// The entries grouped by class, the chunk cutting and the descriptors are those of the real path (blockdiag.cpp); the two
// kernel routes are kernels_complex_image.hip.
#include <algorithm>
#include <vector>

#include "host_internal.h"
#include "iso_classes.h"

using namespace sdpsr;

namespace {

// The routes over one state, as BasisImage (blockdiag.cpp) has them for the real path.  The vectors are the sources of
// asynchronous uploads: the state lives until the entry's last host wait.
struct ComplexImage {
    sdpsr_ctx* c;
    hipStream_t s;
    int64_t n, d_all, S1, S;
    int64_t first, count;  // the window
    const double* Qrm;     // n x S1 complex, row-major interleaved
    double* out;           // the window's count * S complex numbers
    double atol;
    const std::vector<int32_t>& sizes;
    BlockLayout lay;
    std::vector<int32_t> desc;
    std::vector<int64_t> chunk_ptr, cb, ce;

    // A function of (n, d, the block sizes) alone -- never of the window, so that a window's bits are those of the full call
    // under `auto` too: the real path's threshold (average class below 4096 entries and every block within what the outer
    // kernel supports: outer; else chunk).  two_stage (1) counts as auto: those kernels rely on a symmetric partition.
    int route() const {
        const int force = c->opts.basis_image_kernel;
        if (force == 3) return SDPSR_BI_ROUTE_CHUNK;
        const bool fits = cx_image_outer_supports(lay.max_size, lay.nb, d_all);
        if (fits && (force == 2 || (d_all > 0 && n * n / d_all < 4096))) return SDPSR_BI_ROUTE_OUTER;
        return SDPSR_BI_ROUTE_CHUNK;
    }

    int outer(const uint32_t* ent, const std::vector<int64_t>& class_ptr) {
        const int nb = lay.nb;
        int32_t* d_col = (int32_t*)ctx_buf(c, "bic_col", (size_t)nb * 4);
        int32_t* d_sz = (int32_t*)ctx_buf(c, "bic_sz", (size_t)nb * 4);
        int64_t* d_off = (int64_t*)ctx_buf(c, "bic_off", (size_t)nb * 8);
        int64_t* d_cls = (int64_t*)ctx_buf(c, "bic_cls_ptr", (size_t)(count + 2) * 8);
        if (!d_col || !d_sz || !d_off || !d_cls) return SDPSR_OUT_OF_MEMORY;
        int st = h2d_sync(c, d_col, lay.col(), (size_t)nb * 4);
        if (!st) st = h2d_sync(c, d_sz, lay.size(), (size_t)nb * 4);
        if (!st) st = h2d_sync(c, d_off, lay.off.data(), (size_t)nb * 8);
        if (!st) st = h2d_sync(c, d_cls, class_ptr.data(), (size_t)(count + 2) * 8);
        if (st) return st;
        launch_cx_image_outer(s, n, count, S1, S, nb, lay.max_size, Qrm, ent, d_cls, d_col, d_sz, d_off, atol, out);
        return SDPSR_OK;
    }

    int chunk(const uint32_t* ent, const std::vector<int64_t>& class_ptr) {
        cut_chunks(class_ptr, count, 4096, chunk_ptr, cb, ce);
        desc = pair_descriptor(sizes, S);
        const int64_t nch = (int64_t)cb.size();
        int64_t* d_chunk_ptr = (int64_t*)ctx_buf(c, "bic_chunk_ptr", (size_t)(count + 1) * 8);
        int64_t* d_cb = (int64_t*)ctx_buf(c, "bic_cb", (size_t)std::max<int64_t>(nch, 1) * 8);
        int64_t* d_ce = (int64_t*)ctx_buf(c, "bic_ce", (size_t)std::max<int64_t>(nch, 1) * 8);
        int32_t* d_desc = (int32_t*)ctx_buf(c, "bic_desc", (size_t)2 * S * 4);
        double* partial = (double*)ctx_buf(c, "bic_partial", (size_t)std::max<int64_t>(nch * S, 1) * 16);
        if (!d_chunk_ptr || !d_cb || !d_ce || !d_desc || !partial) return SDPSR_OUT_OF_MEMORY;
        HIP_TRY(c, hipMemcpyAsync(d_chunk_ptr, chunk_ptr.data(), (size_t)(count + 1) * 8, hipMemcpyHostToDevice, s));
        if (nch) {
            HIP_TRY(c, hipMemcpyAsync(d_cb, cb.data(), (size_t)nch * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(d_ce, ce.data(), (size_t)nch * 8, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(c, hipMemcpyAsync(d_desc, desc.data(), (size_t)2 * S * 4, hipMemcpyHostToDevice, s));
        launch_cx_image_chunk(s, n, count, S1, S, Qrm, ent, d_desc, d_desc + S, d_chunk_ptr, nch, d_cb, d_ce, partial, out, atol);
        return SDPSR_OK;
    }
};

}  // namespace

extern "C" {

// Buffers of its own ("bic_*") for the labels, Q_hat, its row-major copy, the output and every descriptor: neither the ctx's
// block diagonalisations (bd_*, bdc_*) nor the real entry's arrays (bie_*) are touched.  The entry grouping shares the real
// path's sort workspaces, which carry nothing from one call to the next.
int sdpsr_basis_image_complex(sdpsr_ctx* c, int64_t n, const uint32_t* P, int64_t d, int32_t nblocks, const int32_t* blk_sizes,
                              const double* Q_hat, int64_t class_first, int64_t class_count, double atol, double* blks, int32_t* route,
                              double* phase_ms, int mem) {
    CHECK_CTX(c);
    if (!P || !blk_sizes || !Q_hat || !blks) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    if (n < 1 || d < 0 || nblocks < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments: n < 1, d < 0 or nblocks < 1");
    int64_t S1 = 0, S = 0;
    for (int32_t k = 0; k < nblocks; ++k) {
        if (blk_sizes[k] < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a block size is < 1");
        S1 += blk_sizes[k];
        S += (int64_t)blk_sizes[k] * blk_sizes[k];
        if (S1 > n) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "the block sizes sum to more than n");
    }
    if (class_count < 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "class_count < 0");
    if (class_count > 0 && (class_first < 1 || class_first > d || class_count > d - class_first + 1))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "the window of classes is not inside 1 .. d");
    int st = check_len(c, n * n);
    if (st) return st;
    if (route) *route = 0;
    if (class_count == 0) return SDPSR_OK;
    if (!c->pinned_small) return SDPSR_OUT_OF_MEMORY;
    hipStream_t s = c->stream;
    const int64_t len = n * n;
    const size_t out_count = (size_t)class_count * S;  // complex numbers
    const uint64_t h2d0 = c->h2d_bytes, d2h0 = c->d2h_bytes;
    TotalEvents ev_total(phase_ms != nullptr, s);
    uint32_t* L = (uint32_t*)ctx_buf(c, "bic_labels", (size_t)len * 4);
    uint32_t* flag = (uint32_t*)ctx_buf(c, "bic_flag", 64);
    double* Qrm = (double*)ctx_buf(c, "bic_qrm", (size_t)n * S1 * 16);
    if (!L || !flag || !Qrm) return SDPSR_OUT_OF_MEMORY;
    const double* Qcm = in_dev(c, "bic_qhat", Q_hat, (size_t)2 * n * S1, mem, &st);
    double* out = out_dev(c, "bic_blks", blks, 2 * out_count, mem, &st);
    if (st || !Qcm || !out) return st ? st : SDPSR_OUT_OF_MEMORY;
    // the labels come in and are judged in the same pass.  Of the two verdicts only "a label exceeds d" counts here: a
    // desymmetrized partition is not symmetric and neither route needs it to be
    HIP_TRY(c, hipMemsetAsync(flag, 0, 8, s));
    const uint32_t dmax = (uint32_t)std::min<int64_t>(d, 0xFFFFFFFFll);
    if (mem == SDPSR_MEM_DEVICE && c->label_width == 32) {
        launch_copy_check_labels(s, n, P, L, dmax, flag);
    } else {  // host arrays and narrow labels arrive through labels_fetch; the check runs over them in place
        st = labels_fetch(c, L, P, (size_t)len, mem);
        if (st) return st;
        launch_copy_check_labels(s, n, L, L, dmax, flag);
    }
    uint32_t* verdict = c->pinned_small + PINNED_SMALL_LABEL_CHECK.first;
    HIP_TRY(c, hipMemcpyAsync(verdict, flag, 8, hipMemcpyDeviceToHost, s));
    launch_cx_rowmajor(s, n, S1, Qcm, Qrm);
    const std::vector<int32_t> sizes(blk_sizes, blk_sizes + nblocks);
    ComplexImage ci{c, s, n, d, S1, S, class_first, class_count, Qrm, out, atol < 0 ? 1e-12 * (double)n : atol, sizes, block_layout(sizes), {}, {}, {}, {}};
    const int kind = ci.route();
    // _constraints(P): entries grouped by class (src/diagonalize.jl:42-50); the keys are window-relative, labels outside the
    // window -- of any value -- are the skipped class 0
    uint32_t* ent = nullptr;
    std::vector<int64_t> class_ptr;
    st = sort_entries_by_label(c, len, class_count, L, &ent, class_ptr, (uint32_t)class_first);
    if (st) return st;
    st = kind == SDPSR_BI_ROUTE_OUTER ? ci.outer(ent, class_ptr) : ci.chunk(ent, class_ptr);
    if (st) return st;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, ctx_sync_stream(c, s));
    // what this entry moved: the arrays and the verdicts (the routes' descriptor words are not part of its account)
    c->h2d_bytes = h2d0 + (mem != SDPSR_MEM_DEVICE ? (uint64_t)len * (c->label_width / 8) + (uint64_t)n * S1 * 16 : 0);
    c->d2h_bytes = d2h0 + (mem != SDPSR_MEM_DEVICE ? 0 : 8);
    if (verdict[1]) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "basis_image: a label exceeds d = dim(P)");
    if (mem != SDPSR_MEM_DEVICE) {
        HIP_TRY(c, hipMemcpyAsync(blks, out, out_count * 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, ctx_sync_stream(c, s));
        c->d2h_bytes += out_count * 16;
    }
    if (route) *route = kind;
    if (phase_ms) {
        const float ms = ev_total.stop(s);
        for (int i = 0; i < SDPSR_T_COUNT; ++i) phase_ms[i] = 0;
        phase_ms[SDPSR_T_IMAGE] = ms;
        phase_ms[SDPSR_T_TOTAL] = ms;
    }
    return SDPSR_OK;
}

}  // extern "C"
