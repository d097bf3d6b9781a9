// One reduction in one call: admissible_subspace (src/partitions.jl:109-190) followed by
// blockDiagonalize (src/compat.jl:46-68) on its result, the partition never leaving the device and
// the host never waiting between the stages (the three separate entry points each return with their
// outputs complete, include/sdpsr.h: two host synchronisations and one label copy + symmetry pass per
// reduction that a caller who wants both results does not need).
#include <algorithm>
#include <cstring>
#include <new>

#include "host_internal.h"

using namespace sdpsr;

namespace sdpsr {
// mem_in: where CL / X0L / U live; mem_out: where P_out / blks / Q_hat live
int jordan_reduce_impl(sdpsr_ctx* c, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r, double atol, double epsilon,
                       uint32_t* P_out, int64_t* dim_out, int32_t* iters_out, int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* blks,
                       int64_t blks_capacity, double* Q_hat, int64_t qhat_capacity, double* phase_ms, int mem_in, int mem_out) {
    const int mem = mem_out;
    CHECK_CTX(c);
    if (!dim_out || n < 1 || !(epsilon > 0) || blks_capacity < 0 || qhat_capacity < 0 || (blks_capacity > 0 && !blks) ||
        (qhat_capacity > 0 && !Q_hat))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const int64_t len = n * n;
    int st = check_len(c, len);
    if (st) return st;
    hipStream_t s = c->stream;
    // what a repeat of this reduction (a wrong guess, below) starts from again: the seed position and the caller's one-shot
    // hint (a call's draws depend on the seed position, the inputs and the opts, never on what ran on the ctx before)
    const uint64_t stream_at_entry = c->stream_counter;
    const int hint_at_entry = c->hint_symmetric_basis;
    // the partition is formed where blockDiagonalize reads its labels: in the caller's device buffer P_out when there
    // is one (no copy at all), else in the ctx buffer "bd_labels"
    // (narrow labels, sdpsr_set_label_width: the ctx buffer too; P_out receives the narrowed result once dim(S) is known to fit)
    const bool in_place = mem == SDPSR_MEM_DEVICE && P_out != nullptr && c->label_width == 32;
    uint32_t* L = in_place ? P_out : (uint32_t*)ctx_buf(c, "bd_labels", (size_t)len * 4);
    if (!L) return SDPSR_OUT_OF_MEMORY;
    c->bd_valid = false;
    c->bd_q_valid = false;
    c->bd_qrm_current = false;
    c->bd_labels_ext = nullptr;
    double pm_a[SDPSR_T_COUNT] = {}, pm_b[SDPSR_T_COUNT] = {}, pm_i[SDPSR_T_COUNT] = {};
    int labels_sym = 0;
    c->deferred_verdict = false;
    c->initial_guess_pending = false;
    // the loop's deferred tail lives inside this call: on the successful path it has been enqueued (below) well before the last host wait; an
    // error return drops what is left of it, so that no later call on the ctx enqueues segments that point into this call's arguments
    struct DropTail {
        sdpsr_ctx* c;
        ~DropTail() {
            c->deferred_tail.count = c->deferred_tail.next = 0;
            c->check_stats.window_open = -1;  // (an error return may leave a window open: the next reduction's first upload must not close it)
        }
    } drop_tail{c};
    c->check_stats.window_open = -1;
    // A wrong guess of the loop (its input closed, its initial partition the recorded one) voids the run: the reduction is done again from the
    // caller's seed position with the caller's hint, and this time nothing is guessed (predict_closed is off, the record is gone).
    auto repeat_without_guesses = [&](uint32_t dv, uint32_t dv_spec, uint32_t dv_init) -> int {
        c->predict_closed = false;
        c->initial_record = InitialRecord{};
        if (dv_init != 0) ++c->initial_guesses_violated;
        c->check_stats.voided[0] = dv, c->check_stats.voided[1] = dv_spec, c->check_stats.voided[2] = dv_init;
        if (dbg_on())
            fprintf(stderr, "[sdpsr] jordan_reduce: %s%s%s (deferred verdicts: verify %u, speculative %u, initial partition %u): reduction repeated\n",
                    dv_init != 0 ? "the initial partition was not the recorded one" : "", dv_init != 0 && (dv != 0 || dv_spec != 0) ? "; " : "",
                    dv != 0 ? "the input was not closed after all" : (dv_spec != 0 ? "the confirm round found a split" : ""), dv, dv_spec, dv_init);
        // the repeat makes the draws of a call that took no guess, with the caller's hint
        c->stream_counter = stream_at_entry;
        c->hint_symmetric_basis = hint_at_entry;
        if (mem_in != SDPSR_MEM_DEVICE) {  // host inputs: the loop's copies in its input buffers (loop.cpp, same names and sizes), no second upload
            CL = (const double*)ctx_buf(c, "adm_cl", (size_t)len * 8);
            X0L = (const double*)ctx_buf(c, "adm_x0", (size_t)len * 8);
            if (U) U = (const double*)ctx_buf(c, "adm_u", (size_t)len * std::max<int64_t>(r, 1) * 8);
            if (!CL || !X0L || (r > 0 && !U)) return SDPSR_OUT_OF_MEMORY;
            mem_in = SDPSR_MEM_DEVICE;
        }
        return jordan_reduce_impl(c, n, CL, X0L, U, r, atol, epsilon, P_out, dim_out, iters_out, nblocks, sum_sq, sum_s, blks, blks_capacity, Q_hat,
                                  qhat_capacity, phase_ms, mem_in, mem_out);
    };
    // An early way out while the guessed initial partition's verdict is unread: with stale labels the loop or a later step may report an error
    // that is not real.  The rest of the tail is enqueued (nothing may stay registered), the stream waited for and the word read; violated:
    // the reduction is repeated instead of the error reported.
    auto leave = [&](int st_err) -> int {
        if (!c->initial_guess_pending) return st_err;
        c->initial_guess_pending = false;
        c->deferred_verdict = false;
        flush_deferred_tail(c);
        if (ctx_sync_stream(c, s) != hipSuccess) return st_err == STATUS_REPEAT_REDUCTION ? ctx_fail(c, SDPSR_HIP_ERROR, "hipStreamSynchronize failed") : st_err;
        const uint32_t dv_init = initial_guess_violated(c);
        if (dv_init != 0) return repeat_without_guesses(0, 0, dv_init);
        return st_err == STATUS_REPEAT_REDUCTION ? ctx_fail(c, SDPSR_BAD_STATE, "jordan_reduce: a repeat was asked for without a violated verdict") : st_err;
    };
    c->allow_deferred_verdict = !(c->opts.flags & SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT);  // (the loop's last verdicts may ride on this reduction's later host waits, see sdpsr_internal.h)
    // A guessed reduction refines nothing, so its labels are the record's: where the partition is formed in the caller's buffer, the loop
    // may leave the pass that writes it to the deferred tail and name the ctx's copy of the same labels for blockDiagonalize
    // (c->labels_on_record; loop.cpp, check_round).  Host outputs and narrow labels deliver P_out in front of blockDiagonalize, a
    // timed call launches everything in the loop: both keep the old order, like SDPSR_FLAG_LABELS_BEFORE_BLOCKDIAG.
    c->record_labels_allowed = in_place && !phase_ms && !(c->opts.flags & SDPSR_FLAG_LABELS_BEFORE_BLOCKDIAG);
    c->labels_on_record = nullptr;
    st = admissible_subspace_impl(c, n, CL, X0L, U, r, atol, L, dim_out, iters_out, phase_ms ? pm_a : nullptr, mem_in, SDPSR_MEM_DEVICE,
                                  /*final_sync=*/false, &labels_sym);
    c->allow_deferred_verdict = false;
    c->record_labels_allowed = false;
    // blockDiagonalize's labels: L, or the record's copy of them while the pass that writes L waits in the tail.  Everything that
    // remembers the pointer (bd_labels_ext, bd_trusted_symmetric) then remembers the ctx's copy, which holds the same labels; P_out
    // itself is complete behind the flush below, in front of the images and of the copy into "bd_labels".
    const uint32_t* Lbd = c->labels_on_record ? c->labels_on_record : L;
    c->labels_on_record = nullptr;
    const int st_loop = st;
    if (st && st != SDPSR_NOT_CONVERGED) return leave(st);
    // more classes than the ctx's label width holds (the reference's InexactError of Partition{T}): the reduction stops behind the loop,
    // P_out untouched -- reported below, once the stream has been waited for and the loop's deferred verdicts are in
    const bool overflow = P_out && label_width_overflows(c, (uint64_t)*dim_out);
    if (P_out && !in_place && !overflow) {  // stream-ordered; complete when the call returns (it ends with a synchronisation on every path)
        st = labels_deliver(c, P_out, L, (size_t)len, mem);
        if (st) return leave(st);
    }
    const int64_t d = *dim_out;
    int32_t nb = 0;
    int64_t S = 0, S1 = 0;
    if (!overflow && Lbd != L) ++c->check_stats.on_record;
    st = overflow ? SDPSR_OK
                  : block_diagonalize_impl(c, n, Lbd, d, epsilon, &nb, &S, &S1, phase_ms ? pm_b : nullptr, SDPSR_MEM_DEVICE, labels_sym != 0,
                                           /*final_sync=*/false, in_place);
    // whatever blockDiagonalize did (a failure included): the rest of the deferred tail goes in front of the images' kernels and of the
    // wait behind which the verdicts are read
    flush_deferred_tail(c);
    if (nblocks) *nblocks = nb;
    if (sum_sq) *sum_sq = S;
    if (sum_s) *sum_s = S1;
    bool images_done = false;
    if (st == SDPSR_OK && !overflow && blks && d * S <= blks_capacity && (!Q_hat || n * S1 <= qhat_capacity)) {
        st = sdpsr_block_images(c, blks, (Q_hat && n * S1 <= qhat_capacity) ? Q_hat : nullptr, phase_ms ? pm_i : nullptr, mem);  // ends synchronised
        images_done = st == SDPSR_OK;
    }
    if (in_place) {
        // the caller's buffer stops serving phase 2 when this call returns: a later sdpsr_block_images (images not
        // delivered here) finds the labels in the ctx buffer.  On every path out of this block the ctx forgets the
        // caller's pointer; a failed hand-over also drops the pending phase 2 (it would read a buffer the caller owns).
        struct Forget {
            sdpsr_ctx* c;
            bool ok = false;
            ~Forget() {
                c->bd_labels_ext = nullptr;
                c->bd_trusted_symmetric = nullptr;
                if (!ok) c->bd_valid = false;
            }
        } forget{c};
        if (!images_done && c->bd_valid) {
            uint32_t* keep = (uint32_t*)ctx_buf(c, "bd_labels", (size_t)len * 4);
            if (!keep) return leave(SDPSR_OUT_OF_MEMORY);
            const hipError_t ek = hipMemcpyAsync(keep, P_out, (size_t)len * 4, hipMemcpyDeviceToDevice, s);
            if (ek != hipSuccess) return leave(ctx_fail(c, SDPSR_HIP_ERROR, std::string("hipMemcpyAsync: ") + hipGetErrorString(ek)));
        } else if (images_done) {
            c->bd_valid = false;  // nothing left for a second sdpsr_block_images to work on (sizes and Q_hat stay available)
        }
        forget.ok = true;
    }
    if (!images_done) {  // (sdpsr_block_images ends synchronised, and nothing has been enqueued since)
        flush_deferred_tail(c);  // (nothing is pending here; a verdict must never be read with its segment not enqueued)
        const hipError_t e = ctx_sync_stream(c, s);
        if (e != hipSuccess && st == SDPSR_OK) st = ctx_fail(c, SDPSR_HIP_ERROR, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    if (c->deferred_verdict || c->initial_guess_pending) {
        // The stream has been waited for: the verdicts the loop left unread are in.  A violated one means the loop started from a partition
        // that is not this input's (the initial guess), or stopped on one that one more step would have refined -- whatever blockDiagonalize
        // made of it (a failure included) is void; the reduction is done again, this time reading the verdicts where they arise.
        const volatile uint32_t* ps = c->pinned_small;
        const uint32_t dv = c->deferred_verdict ? ps[PINNED_SMALL_DEFERRED_VERIFY.first] : 0u;
        const uint32_t dv_spec = c->deferred_verdict ? ps[PINNED_SMALL_DEFERRED_SPECULATIVE.first] : 0u;
        const uint32_t dv_init = c->initial_guess_pending ? initial_guess_violated(c) : 0u;  // (with the overflow word of the labels' 8-bit shadow)
        c->deferred_verdict = false;
        c->initial_guess_pending = false;
        if (dv != 0 || dv_spec != 0 || dv_init != 0) {
            const int st2 = repeat_without_guesses(dv, dv_spec, dv_init);
            if (phase_ms)  // the voided run's time was spent too
                for (int i = 0; i < SDPSR_T_COUNT; ++i) phase_ms[i] += pm_a[i] + pm_b[i] + pm_i[i];
            return st2;
        }
    }
    if (phase_ms) {
        for (int i = 0; i < SDPSR_T_COUNT; ++i) phase_ms[i] = pm_a[i] + pm_b[i] + pm_i[i];
    }
    if (overflow && st == SDPSR_OK) return label_width_fail(c, "jordan_reduce: admissible_subspace", (uint64_t)d);
    if (st == SDPSR_OK && P_out && !in_place) st = labels_delivered(c);  // (the narrowing pass's own flag: dim(S) fits, so do the labels)
    return st ? st : st_loop;
}
}  // namespace sdpsr

extern "C" int sdpsr_jordan_reduce(sdpsr_ctx* c, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r,
                                   double atol, double epsilon, uint32_t* P_out, int64_t* dim_out, int32_t* iters_out,
                                   int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* blks, int64_t blks_capacity,
                                   double* Q_hat, int64_t qhat_capacity, double* phase_ms, int mem) {
    return jordan_reduce_impl(c, n, CL, X0L, U, r, atol, epsilon, P_out, dim_out, iters_out, nblocks, sum_sq, sum_s, blks, blks_capacity, Q_hat,
                              qhat_capacity, phase_ms, mem, mem);
}

// ---------------------------------------------------------------------------
// Upload once, reduce many times: the problem handle (include/sdpsr.h)
// ---------------------------------------------------------------------------
extern "C" int sdpsr_problem_create(sdpsr_ctx* c, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r, int hint, int mem,
                                    sdpsr_problem** out) {
    CHECK_CTX(c);
    if (!out || !CL || !X0L || n < 1 || r < 0 || (r > 0 && !U)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    *out = nullptr;
    const int64_t len = n * n;
    int st = check_len(c, len);
    if (st) return st;
    DeviceGuard dg(c->device);
    sdpsr_problem* p = new (std::nothrow) sdpsr_problem();
    if (!p) return SDPSR_OUT_OF_MEMORY;
    p->device = c->device;
    p->n = n;
    p->r = r;
    p->hint = hint & 3;
    const size_t vb = (size_t)len * 8;
    auto fail = [&](int code, const char* what) {
        sdpsr_problem_destroy(p);
        return ctx_fail(c, code, what);
    };
    if (hipMalloc((void**)&p->CL, vb) != hipSuccess || hipMalloc((void**)&p->X0, vb) != hipSuccess ||
        (r > 0 && hipMalloc((void**)&p->U, vb * (size_t)r) != hipSuccess))
        return fail(SDPSR_OUT_OF_MEMORY, "sdpsr_problem_create: device memory");
    const hipMemcpyKind kind = mem == SDPSR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (hipMemcpyAsync(p->CL, CL, vb, kind, c->stream) != hipSuccess || hipMemcpyAsync(p->X0, X0L, vb, kind, c->stream) != hipSuccess ||
        (r > 0 && hipMemcpyAsync(p->U, U, vb * (size_t)r, kind, c->stream) != hipSuccess))
        return fail(SDPSR_HIP_ERROR, "sdpsr_problem_create: copy");
    if (mem != SDPSR_MEM_DEVICE) c->h2d_bytes += vb * (size_t)(2 + r);
    if (ctx_sync_stream(c, c->stream) != hipSuccess) return fail(SDPSR_HIP_ERROR, "sdpsr_problem_create: synchronisation");
    *out = p;
    return SDPSR_OK;
}

extern "C" int sdpsr_problem_destroy(sdpsr_problem* p) {
    if (!p) return SDPSR_OK;
    DeviceGuard dg(p->device);
    if (p->CL) hipFree(p->CL);
    if (p->X0) hipFree(p->X0);
    if (p->U) hipFree(p->U);
    delete p;
    return SDPSR_OK;
}

extern "C" int sdpsr_problem_reduce(sdpsr_ctx* c, const sdpsr_problem* p, double atol, double epsilon, uint32_t* P_out, int64_t* dim_out,
                                    int32_t* iters_out, int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* blks, int64_t blks_capacity,
                                    double* Q_hat, int64_t qhat_capacity, double* phase_ms, int mem_out) {
    CHECK_CTX(c);
    if (!p || p->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdpsr_problem_reduce: no problem, or one of another device");
    c->hint_symmetric_basis = p->hint;
    return jordan_reduce_impl(c, p->n, p->CL, p->X0, p->U, p->r, atol, epsilon, P_out, dim_out, iters_out, nblocks, sum_sq, sum_s, blks,
                              blks_capacity, Q_hat, qhat_capacity, phase_ms, SDPSR_MEM_DEVICE, mem_out);
}

extern "C" int sdpsr_problem_reduce_batch(sdpsr_ctx* c, const sdpsr_problem* p, int32_t R, const uint64_t* seeds, double atol, double epsilon,
                                          uint32_t* const* P_out, int64_t* dim_out, int32_t* iters_out, int32_t* nblocks, int64_t* sum_sq,
                                          int64_t* sum_s, double* const* blks, const int64_t* blks_capacity, int32_t* status, int mem_out) {
    CHECK_CTX(c);
    if (!p || p->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "sdpsr_problem_reduce_batch: no problem, or one of another device");
    return jordan_reduce_batch_impl(c, R, seeds, p->n, p->CL, p->X0, p->U, p->r, p->hint, atol, epsilon, P_out, dim_out, iters_out, nblocks, sum_sq,
                                    sum_s, blks, blks_capacity, status, SDPSR_MEM_DEVICE, mem_out);
}
