// Internal declarations shared by the host orchestration (api.cpp) and the kernel
// translation units.  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <map>
#include <functional>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/sdpsr.h"
#include "sdpsr_hash.h"

namespace sdpsr { struct SytrdGraphCache; }  // kernels_sytrd.hip

// ---------------------------------------------------------------------------
// grow-only named device buffers: no hipMalloc inside steady-state loops
// ---------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

namespace sdpsr {
// Where the insert pass takes its signatures from: an array (SIG_ARRAY), or computed on the fly
// (the signatures never travel through HBM).  Each kind is defined by one functor of
// sig_sources.h (SrcPair, SrcProj<r>, SrcChan<CT, T>, SrcJoint<r, T>).
// `sig` is the array (SIG_ARRAY) or len entries of scratch for the paths that need one
// (launch_sig_materialize: sort / bucket, an overflowed table, a shape without a functor instance).
enum { SIG_ARRAY = 0, SIG_PAIR = 1, SIG_PROJ = 2, SIG_CHAN_I32 = 3, SIG_CHAN_F32 = 4, SIG_JOINT_I32 = 5 };  // JOINT: SIG_PROJ and SIG_CHAN_I32 fields together (packed)
struct SigSource {
    int kind = SIG_ARRAY;
    uint64_t* sig = nullptr;
    const double *a = nullptr, *b = nullptr;                      // SIG_PAIR: bit patterns of (a[e], b[e])
    const double *U = nullptr, *coef = nullptr;                   // SIG_PROJ: rounded x - U coef, x drawn from L and key; U: r matrices of n x n
    const uint32_t* L = nullptr;                                  // old labels (SIG_PROJ, SIG_CHAN_*)
    int r = 0;
    uint64_t key = 0;
    double atol = 0, scale = 1;
    int64_t n = 0, ld = 0;                                        // matrix order (SIG_PROJ, SIG_CHAN_*, SIG_JOINT_I32; SIG_PAIR when packed); ld: SIG_CHAN_* / JOINT: T channels of ld x ld in C
    int T = 0;
    const void* C = nullptr;
    int packed = 0;                                               // lower triangle only, densely packed (symmetric labels; SIG_PROJ: and symmetric basis, needs n)
    int lab_packed = 0;                                           // (with packed) L is the packed lower triangle itself: label of packed entry e = L[e]
    const uint8_t* L8 = nullptr;                                  // (with lab_packed) a byte copy of L, every label <= 255: the verify passes read it instead (the label width of the source: 8 when set)
};

// kernels_square_check.hip: "is X_t^2 constant on the classes (0 on label 0)?" for G rounds of T channels without forming X_t^2, from the
// packed labels (Lp8: their byte copy, or null) and the representatives.  Stream order: ref_and_pass (class constants c, then the ONE pass
// over the labels, which writes the full n x n label matrix to Lfull unless that is null), then verdict (y, w, the (round, channel)
// equality bits, and a 1 into flag[g][0] -- pinned host words the caller has cleared -- for every round with a channel that differs).
constexpr int SQUARE_CHECK_MAX_CLASSES = 255;
constexpr int64_t SQUARE_CHECK_MAX_ORDER = 1 << 15;
struct SquareCheck {
    int64_t n = 0, d = 0;
    int G = 0, T = 0;
    uint64_t key[2] = {0, 0};
    const uint32_t* Lp = nullptr;
    const uint8_t* Lp8 = nullptr;
    const uint32_t* first_idx = nullptr;
    uint32_t* Lfull = nullptr;
    uint32_t* flag[2] = {nullptr, nullptr};
    // workspace (square_check_ws_carve): c [G T][d]; part_x, part_c [G T][nb][64 nb], nb = ceil(n / 64); y, w [G T][64 nb];
    // esum [G T][nb][2]; bits [G T]
    int32_t *c = nullptr, *part_x = nullptr;
    int64_t *part_c = nullptr, *y = nullptr, *w = nullptr;
    uint64_t* esum = nullptr;
    uint32_t* bits = nullptr;
};

// The tail of the loop's guessed-closed path that sdpsr_jordan_reduce defers: up to two segments registered on the ctx instead of
// launched.  Nothing in blockDiagonalize reads what they write, so they are enqueued -- same stream, same kernels, same arguments --
// where the host would otherwise leave the stream idle: behind the products of the module growth whose read-backs the host waits for
// (compress.cpp, Module::ortho_step).  Every other route enqueues them before it enqueues anything of its own.  Two kinds:
//   DEFERRED_SQUARE  (loop.cpp, verify_round; SDPSR_FLAG_SQUARE_EVERY_VERDICT): the int8 square of a gathered element and the verify
//                    pass over its product, one segment per round
//   DEFERRED_CHECK   (loop.cpp, initial_partition and check_round): launches whose only product is a verdict word.  Segment "pair":
//                    the compare of the guessed initial partition (launch_verify_pair).  Segment "round": the dot products of the
//                    projection (launch_proj_coef_lower), the projection compare (launch_verify_projection) and the square check's
//                    verdict kernels (launch_square_check_verdict), in the loop's order.  The square check's class constants and its
//                    pass (launch_square_check_ref_and_pass) stay in the loop -- the pass writes the full labels blockDiagonalize
//                    reads -- unless blockDiagonalize reads the record's copy of them (InitialRecord::Lfull; loop.cpp, check_round):
//                    then they are segment "pass", the first of the two, and the pair check moves into segment "round" behind it.
// A segment carries its keys: every key is drawn in the loop, where it always was.
enum { DEFERRED_SQUARE = 0, DEFERRED_CHECK = 1 };
struct DeferredSegment {
    int kind = DEFERRED_SQUARE;
    // --- DEFERRED_SQUARE ---
    const int8_t* X = nullptr;  // the gathered channels (the gather itself ran in the loop)
    int32_t* C = nullptr;       // their squares
    SigSource q;                // the verify pass's source (q.C == C); DEFERRED_CHECK: the projection compare's source
    void* vref = nullptr;
    uint32_t* flag = nullptr;   // the verdict's word of c->pinned_small (DEFERRED_CHECK: the pair check's, or the round's first)
    bool speculative = false;   // counts as a speculative square
    // --- DEFERRED_CHECK --- (what is set is launched in the order of the fields)
    bool sq_pass = false;       // launch_square_check_ref_and_pass(sq): writes sq.Lfull, the caller's labels
    bool pair = false;          // launch_verify_pair(n, a, b, Lp, pair_d, first, pair_flag, Lp8)
    int64_t pair_d = 0;
    uint32_t* pair_flag = nullptr;
    const double *a = nullptr, *b = nullptr;
    const uint32_t* Lp = nullptr;
    const uint8_t* Lp8 = nullptr;
    int64_t n = 0, d = 0;
    const uint32_t* first = nullptr;
    bool proj_coef = false;     // launch_proj_coef_lower(n, q.r, q.U, Lp, 1, q.key, partial, nblk, coef, Lp8); coef == q.coef
    double* partial = nullptr;
    double* coef = nullptr;
    int nblk = 0;
    bool proj_verify = false;   // launch_verify_projection(q, d, first, flag)
    bool verdict = false;       // launch_square_check_verdict(sq): sq.flag[0] == flag, sq.flag[1] the second word
    SquareCheck sq;
};
constexpr int DEFERRED_SEGMENTS = 2;
struct DeferredTail {
    DeferredSegment seg[DEFERRED_SEGMENTS];
    int count = 0, next = 0;  // registered, enqueued
    int64_t ld = 0, d = 0;
    int T = 0;
    const uint32_t* zero_flag = nullptr;
    const uint32_t* first = nullptr;  // "ref_first" of the packed labels
};
// what the check segments did on a ctx, and the host time of the two windows they ride in (sdpsr_profile_deferred_checks)
struct DeferredCheckStats {
    uint64_t registered = 0, in_ride = 0, outside_ride = 0;
    uint64_t window_ns[2] = {0, 0}, window_count[2] = {0, 0};  // [0] class-sum step, [1] growth rounds: wait returned -> next enqueue
    int window_open = -1;
    uint64_t window_t0 = 0;
    uint32_t voided[3] = {0, 0, 0};  // the words as the last voided reduction read them (reduce.cpp): verify, speculative, initial partition
    uint64_t on_record = 0;  // reductions whose blockDiagonalize read the record's copy of the labels (sdpsr_profile_recorded_labels)
};
constexpr uint32_t DEFERRED_NEVER_RAN = 0xDEFE44EDu;  // what a verdict word holds until its segment is enqueued: reads as "violated"
// "adm_lpacked" (Lp) and "ref_first" (first) describe the initial partition of the last loop call: order n, d0 classes, labels symmetric
// narrow: "adm_lpacked8" (Lp8) is a byte copy of Lp (d0 <= 255) -- the 8-bit shadow the guessed-closed path streams instead of Lp
// Lfull: "adm_lfull_rec" holds the full symmetric n x n labels that belong to Lp (copied from the output of the unguessed call that
// made the record): blockDiagonalize of a guessed reduction starts on them while the pass that writes the caller's copy is deferred
struct InitialRecord {
    bool valid = false;
    int64_t n = 0, d0 = 0;
    const uint32_t *Lp = nullptr, *first = nullptr;
    int sym = 0;
    bool narrow = false;
    const uint8_t* Lp8 = nullptr;
    const uint32_t* Lfull = nullptr;
};
// the loop's outcome "the initial partition was not the recorded one: repeat the reduction" -- never leaves jordan_reduce_impl
constexpr int STATUS_REPEAT_REDUCTION = -0x5250;
}  // namespace sdpsr

struct sdpsr_ctx {
    int device = 0;
    int num_cus = 256;
    uint64_t seed = 0;
    uint64_t stream_counter = 0;  // fresh RNG stream per randomize call
    sdpsr_opts opts{};
    int label_width = 32;  // sdpsr_set_label_width: bits of every label array that crosses the interface (labels.cpp); inside, labels are uint32
    int psd_max_order = 64;  // sdpsr_set_psd_max_order: the largest block order sdpsr_psd_project / sdpsr_sdp_solve take, 64 or 128 (sdp_solve.cpp)
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;  // lazily created: work that overlaps a one-workgroup kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_wait = nullptr;
    hipEvent_t ev_bt_fork = nullptr, ev_bt_join = nullptr;  // eigen.cpp: first pass of the back-transformation beside the tridiagonal solver
    hipStream_t main_shadow = nullptr;  // the main stream while `stream` temporarily points at side_stream
    bool own_stream = false;
    std::string err;
    double dbg_last_ms = 0;  // SDPSR_DEBUG traces: time of the previous mark
    std::map<std::string, DevBuf, std::less<>> bufs;  // (transparent comparator: looked up by string_view, no allocation per ctx_buf call)
    void* pinned = nullptr;  // small pinned host scratch for scalar read-backs
    size_t pinned_bytes = 0;
    uint32_t* pinned_small = nullptr;  // 256 B pinned: flags read back without their own synchronisation
    void* h2d_ring = nullptr;  // pinned ring for small stream-ordered uploads (no sync per upload)
    int h2d_ring_next = 0;
    void* rocblas = nullptr;  // rocblas_handle, created lazily
    sdpsr::SytrdGraphCache* sytrd_graphs = nullptr;  // captured launch sequences of the tridiagonalisation
    // --- block-diagonalisation state kept between phase 1 and phase 2 ---
    int64_t bd_n = 0, bd_d = 0;
    std::vector<int32_t> bd_sizes;
    int64_t bd_sum_s = 0, bd_sum_sq = 0;
    bool bd_valid = false;
    // complex path (sdpsr_block_diagonalize_complex): its own state, n <= 64
    int64_t bdc_n = 0, bdc_d = 0, bdc_sum_s = 0, bdc_sum_sq = 0;
    std::vector<int32_t> bdc_sizes;
    bool bdc_valid = false;
    uint32_t bd_sym_epoch = 0;            // != 0: "bd_symflag"[0] == epoch <=> bd_sym_labels are NOT symmetric (copy + check pass of blockDiagonalize)
    const uint32_t* bd_sym_labels = nullptr;
    const uint32_t* bd_labels_ext = nullptr;  // sdpsr_jordan_reduce: the labels of the pending phase 2 live in the caller's device buffer, not in "bd_labels"
    const uint32_t* bd_trusted_symmetric = nullptr;  // labels the library made itself and knows to be symmetric (sdpsr_jordan_reduce)
    uint32_t epoch_counter = 0;
    // "ref_first"[l - 1] = first-occurrence index of class l in the label array `first_idx_labels` (written by the
    // ranking pass of the refinement that made those labels); nullptr = not available (sort path, other arrays)
    const uint32_t* first_idx_labels = nullptr;
    int hint_symmetric_basis = 0;         // sdpsr_hint_symmetric_basis: applies to the next admissible_subspace call
    std::vector<int64_t> adm_dims;        // dimension trajectory of the last admissible_subspace call (sdpsr_dimension_trajectory)
    bool bd_q_valid = false;  // "bd_qhat" holds Q_hat of the last diagonalize (even when check_block_sizes failed)
    bool bd_labels_owned = false;
    // "bd_qrm" is the row-major copy of the Q_hat in "bd_qhat" (the module lift stores both): sdpsr_block_images skips its transpose.
    // Cleared by every other writer of "bd_qhat" and when either buffer is reallocated.
    bool bd_qrm_current = false;
    // hash table capacity hint (log2) for the next refine
    int table_log2_hint = 12;
    uint64_t refine_passes = 0;  // relabel passes refine_signatures has run on this ctx, repeats included (sdpsr_profile_refine_source)
    hipEvent_t ev[2 * SDPSR_T_COUNT] = {};
    // sdpsr_jordan_reduce_batch: this ctx runs one restart on a fiber of the calling thread; a host wait for one of its
    // streams polls and hands the thread to the other restarts (ctx_sync_stream).  nullptr outside a batch call.
    void (*yield_fn)(void*) = nullptr;
    void* yield_arg = nullptr;
    std::vector<sdpsr_ctx*> batch_children;  // the ctxs of restarts 1 .. R - 1 (created on demand, destroyed with this ctx)
    uint64_t h2d_bytes = 0, d2h_bytes = 0;   // bytes this ctx has moved over PCIe (sdpsr_transfer_bytes)
    // the loop's branch predictor: the previous admissible_subspace call on this ctx (order predict_n) found its input closed in
    // the first iteration -- the next call of that order runs the confirm round speculatively behind the first verify pass
    bool predict_closed = false;
    int64_t predict_n = 0;
    // what the loop has done on this ctx (sdpsr_profile_loop_counts): squares launched by admissible_subspace, of those the
    // speculative ones, and the symmetric-basis hint bits its last run used
    uint64_t squares_launched = 0, squares_speculative = 0;
    // guessed-closed first iterations judged by the square check (two rounds each, counted above as two squares, one speculative), and
    // those of them that formed a real square behind a "violated" verdict read in the loop; sdpsr_profile_square_checks
    uint64_t square_checks = 0, square_check_fallbacks = 0;
    int hint_used = 0;
    uint64_t host_waits = 0;                 // host waits for one of this ctx's streams (ctx_sync_stream); sdpsr_profile_host_waits
    uint32_t report_seq = 0;                 // stamps of the label passes' reports to pinned memory (ctx_wait_word)
    // sdpsr_jordan_reduce: the loop may leave the verdicts of its LAST verify passes (first iteration of an input predicted
    // closed: the verify pass and the speculative confirm round) unread and return "converged"; the reduction goes on in stream
    // order and reads them behind its next host waits (reduce.cpp) -- one host wait less per reduction.  Violated verdicts
    // discard everything and the reduction is repeated without the guess.
    bool allow_deferred_verdict = false;
    bool deferred_verdict = false;  // both wait in c->pinned_small (host_internal.h: PINNED_SMALL_DEFERRED_*) and must be 0
    sdpsr::DeferredTail deferred_tail;  // ... and the launches that produce them (and the initial guess's word), while they are not enqueued yet
    sdpsr::DeferredCheckStats check_stats;
    // The loop's second guess (loop.cpp, initial_partition): the last loop call on this ctx found its input closed, so "adm_lpacked" /
    // "ref_first" still hold its INITIAL partition -- the next call of sdpsr_jordan_reduce checks that partition against its inputs
    // (launch_verify_pair) instead of rebuilding it, and the verdict rides with the two above.  Dropped by every refinement, by a
    // violated verdict, and by ctx_buf when it frees either buffer (or "adm_lpacked8", the labels' 8-bit shadow).
    sdpsr::InitialRecord initial_record;
    bool initial_guess_pending = false;  // this reduction took the guess; its word (PINNED_SMALL_DEFERRED_INITIAL) has not been read
    // sdpsr_jordan_reduce forms the partition in the caller's device buffer, untimed, without SDPSR_FLAG_LABELS_BEFORE_BLOCKDIAG: the
    // loop may keep the record's full labels and defer the pass that writes the caller's (set around the loop call only) ...
    bool record_labels_allowed = false;
    const uint32_t* labels_on_record = nullptr;  // ... and has done so: blockDiagonalize reads these; the caller's are written by segment "pass"
    uint64_t initial_guesses = 0, initial_guesses_violated = 0;  // sdpsr_profile_initial_guess
    uint64_t label_narrowings = 0;  // launches that made the 8-bit shadow of the packed labels (loop.cpp, initial_partition); sdpsr_profile_narrow_labels
    bool symflag_zero = false;  // every word of "adm_symflag" is 0 (the loop's last call wrote none of them)
};

// sdpsr_problem_create: the loop's inputs, device-resident, shared (read-only) by every reduction / restart that names them
struct sdpsr_problem {
    int device = 0;
    int64_t n = 0, r = 0;
    double *CL = nullptr, *X0 = nullptr, *U = nullptr;  // hipMalloc'ed, owned
    int hint = 0;  // sdpsr_hint_symmetric_basis bits that hold for these inputs
};

// sdpsr_sparse_create: a sparse constraint matrix in canonical CSR form, device-resident, shared (read-only) by every entry that names it
struct sdpsr_sparse {
    int device = 0;
    int64_t len = 0, m = 0, nnz = 0;  // nnz: canonical entries
    int64_t* rowptr = nullptr;        // m + 1, 0-based; hipMalloc'ed, owned (like col and val)
    uint32_t* col = nullptr;          // sorted per row, no duplicates
    double* val = nullptr;            // no zeros
    int rows_symmetric = 0;           // len = n^2 and every row is a symmetric n x n matrix bit for bit
};

// sdpsr_blockop_create: the full entry list of the reduced PSD pencil as 16-byte records (uint32 key, uint32 idx, double val),
// device-resident, shared (read-only) by every apply / adjoint that names it (kernels_blockop.hip)
struct sdpsr_blockop {
    int device = 0;
    int64_t d = 0, sum_sq = 0, nnz_full = 0;
    std::vector<int32_t> sizes;  // the virtual orders s'_k
    void* by_class = nullptr;    // nnz_full records sorted by class (key = class, idx = position); hipMalloc'ed, owned
    void* by_pos = nullptr;      // the same records sorted by position (key = position, idx = class)
};

// one block of sdpsr_blocks_syev's single launch (kernels_batched.hip): where it starts in Z / V and in w, and its order
struct BlocksSyevJob {
    int64_t zoff, woff;
    int32_t n, pad;
};

// one block of sdpsr_psd_project's single launch (kernels_psd.hip): where it starts in Z / P, its order and its index
struct PsdJob {
    int64_t zoff;
    int32_t n, blk;
};

// Host wait for a stream of ctx c (every wait of the library goes through here).  Inside a batch call the wait polls and
// hands the thread to the other restarts' fibers.  hipStreamQuery records its "not ready" as the thread's last error, and
// all fibers share that slot: exactly that value is dropped on every way out (a fiber whose first query succeeds must not
// inherit another fiber's "not ready" either), anything else -- a failed launch of this restart, recorded before the
// wait -- is handed to the caller as the wait's result instead of being cleared with it.
inline hipError_t ctx_sync_stream(sdpsr_ctx* c, hipStream_t s) {
    if (c) ++c->host_waits;
    if (!c || !c->yield_fn) return hipStreamSynchronize(s);
    const hipError_t before = hipPeekAtLastError();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) {
            if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();
            if (e == hipSuccess && before != hipSuccess && before != hipErrorNotReady) return before;
            return e;
        }
        c->yield_fn(c->yield_arg);
    }
}

// Wait for a REPORT instead of for the stream: a kernel has been told to store its result words into pinned host memory and
// then the stamp `seq` into *w (system-scope fence in between).  The label pass of a refinement knows its counters when it
// STARTS -- the ranking kernels before it produced them -- so the host has them ~15 us before the pass ends and enqueues the
// next kernels meanwhile (they follow in stream order).  Only for callers whose own return is covered by a later wait for
// the stream (the loop of admissible_subspace): the stream is NOT idle when this returns.  The stream is still asked now
// and then: a failed launch or a kernel that never reports must not hang the host.
inline hipError_t ctx_wait_word(sdpsr_ctx* c, hipStream_t s, const volatile uint32_t* w, uint32_t seq) {
    ++c->host_waits;
    const hipError_t before = hipPeekAtLastError();
    bool queried = false;
    hipError_t res = hipSuccess;
    for (unsigned spins = 1;; ++spins) {
        if (*w == seq) break;
        if (c->yield_fn || (spins & 2047u) == 0) {
            queried = true;
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) {  // drained (or failed): the report is there, or will never be
                res = e != hipSuccess ? e : (*w == seq ? hipSuccess : hipErrorUnknown);
                break;
            }
            if (c->yield_fn) c->yield_fn(c->yield_arg);
        } else {
            __builtin_ia32_pause();
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (queried && hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();
    if (res == hipSuccess && before != hipSuccess && before != hipErrorNotReady) return before;
    return res;
}

void* ctx_buf(sdpsr_ctx* c, const char* name, size_t bytes);  // throws std::bad_alloc-like via status
int ctx_fail(sdpsr_ctx* c, int status, const std::string& msg);

#define HIP_TRY(c, expr)                                                              \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess)                                                         \
            return ctx_fail((c), SDPSR_HIP_ERROR,                                     \
                            std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

namespace sdpsr {

// ---------------------------------------------------------------------------
// kernels_gather.hip: fills, channel gathers, padded copies
// ---------------------------------------------------------------------------
// M[e] = values[L[e]-1] (0 -> 0.0)
void launch_fill_f64(hipStream_t s, int64_t len, const uint32_t* L, const double* values, int64_t d,
                     double* M, uint32_t* bad_flag);
// M[e] = uniform(key, L[e])
void launch_randomize_f64(hipStream_t s, int64_t len, const uint32_t* L, uint64_t key, double* M);
// in-place clamp+round
void launch_clamp_round(hipStream_t s, int64_t len, double* a, double atol, double scale);
// int8 / f32 channel matrices, padded to ld (>= n, multiple of 16), zero in the padding.
// X[t] is at X + t*ld*ld.
void launch_gather_i8(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* L,
                      uint64_t key, int8_t* X, int64_t dmax = 0);
void launch_gather_f32(hipStream_t s, int64_t n, int64_t ld, int T, int vmax, const uint32_t* L,
                       uint64_t key, float* X);
void launch_gather_f64_padded(hipStream_t s, int64_t n, int64_t ld, const uint32_t* L,
                              uint64_t key, double* X);
// Lfull != nullptr: the kernel also writes the full n x n label matrix (leading dimension n) that the packed triangle describes
// Lp8 != nullptr (here and below): a byte copy of the packed labels, every label <= 255 -- the kernel streams it instead of Lp, same results
void launch_gather_i8_sym_packed(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* Lp, uint64_t key, int8_t* X,
                                 int64_t dmax, uint32_t* Lfull = nullptr, const uint8_t* Lp8 = nullptr);
// dense copy with padding: dst[ld x ld] <- src[n x n], zero padding (templated by bytes)
void launch_unpad_mirror_lower_i32(hipStream_t s, int64_t n, int64_t ld, const int32_t* src, int32_t* dst);
void launch_pad_copy(hipStream_t s, int64_t n, int64_t ld, const void* src, void* dst,
                     int elem_bytes);
void launch_unpad_copy(hipStream_t s, int64_t n, int64_t ld, const void* src, void* dst,
                       int elem_bytes);

// ---------------------------------------------------------------------------
// kernels_projection.hip
// ---------------------------------------------------------------------------
// projection: coef[k] = sum_e U[e,k] * x[e] with x[e] = uniform(key, L[e]) (Lx == nullptr)
// or x[e] = xin[e].  partial: r * nblk doubles scratch.
void launch_proj_coef(hipStream_t s, int64_t len, int64_t r, const double* U, const uint32_t* L,
                      uint64_t key, const double* xin, double* partial, int nblk, double* coef);
void launch_proj_coef_lower(hipStream_t s, int64_t n, int64_t r, const double* U, const uint32_t* L, int lab_packed,
                            uint64_t key, double* partial, int nblk, double* coef, const uint8_t* Lp8 = nullptr);
void launch_proj_coef_probe(hipStream_t s, int64_t len, int64_t n, int64_t r, const double* U, const uint32_t* L, uint64_t key,
                            double* partial, int nblk, double* coef);
// y[e] = x[e] - sum_k U[e,k] coef[k]; optional outputs: yout (rounded value, fp64),
// sig (signature chained on L).  x as above.
void launch_proj_apply(hipStream_t s, int64_t len, int64_t r, const double* U, const uint32_t* L,
                       uint64_t key, const double* xin, const double* coef, double atol,
                       double scale, int do_round, double* yout, uint64_t* sig);

// ---------------------------------------------------------------------------
// kernels_signature.hip
// ---------------------------------------------------------------------------
// signatures.  sig = 0 <=> (L == 0 and key == 0).  L may be nullptr (all zero labels).
void launch_sig_f64(hipStream_t s, int64_t len, const uint32_t* L, const double* v, uint64_t* sig);
void launch_sig_f64_rounded(hipStream_t s, int64_t n, int64_t ld, const uint32_t* L,
                            const double* v, double atol, double scale, uint64_t* sig);
void launch_sig_u32(hipStream_t s, int64_t len, const uint32_t* L, const uint32_t* k,
                    uint64_t* sig);
void launch_sig_u64(hipStream_t s, int64_t len, const uint64_t* k, uint64_t* sig);
// T channels of int32 / f32 squares, padded ld, C[t] at C + t*ld*ld; packed: the lower triangle only, written densely
// (column j at offset j n - j (j - 1) / 2); lab_packed: L is packed the same way
void launch_sig_i32(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* L,
                    const int32_t* C, uint64_t* sig, int packed = 0, int lab_packed = 0);
void launch_sig_f32(hipStream_t s, int64_t n, int64_t ld, int T, const uint32_t* L,
                    const float* C, uint64_t* sig, int packed = 0, int lab_packed = 0);
bool sig_source_fusable(const SigSource& q);
bool launch_sig_materialize(hipStream_t s, int64_t len, const SigSource& q, uint64_t* sig);  // false: nothing writes this source out

// ---------------------------------------------------------------------------
// kernels_refine.hip (the insert pass: kernels_insert_*.hip, one file per source family)
// ---------------------------------------------------------------------------
// canonical relabel of signatures (hash table + first-occurrence ranking).
// Workspace layout is owned by the caller (see refine_workspace_bytes).
// slot of the refinement's global table: signature and first index side by side -- ONE 16-byte gather per look-up (a gather that
// misses the L1 costs ~5 clocks per lane on this part: signature and minimum in separate arrays were two of them per entry)
struct RefSlot {
    unsigned long long sig;
    uint32_t min;
    uint32_t pad;
};
struct RefineWs {
    RefSlot* tab;        // cap
    uint32_t* tab_lab;   // cap
    uint32_t* blk_cnt;   // nblk + 1
    int insert_wgs_per_cu = 0;  // sdpsr_opts.insert_wgs_per_cu (0 = default)
    uint32_t* host_counters = nullptr;  // pinned host memory: counters[0..2] are also stored there by the label pass (plain label pass only)
    uint32_t host_seq = 0;              // ... and then this stamp into word 3: the host may read the three words once it sees the stamp
    int mid = 0;           // array source, ~1000 .. 6000 classes predicted: the one-workgroup-per-CU LDS table (refine_insert_mid_kernel)
    int expect_small = 0;  // host prediction: <= refine_small_k() classes (see launch_refine)
    uint32_t* first_idx = nullptr;  // optional: first-occurrence index of class l at [l - 1], l <= refine_first_cap()
    void* rank_ws = nullptr;        // refine_rank_slots_workspace_bytes(len): the ranking of more than refine_small_k() classes
    size_t rank_ws_bytes = 0;
    uint32_t* counters;  // [0] = inserted, [1] = overflow flag, [2] = nparts, [16..] slot list (refine_counters_bytes())
    int log2cap;
    int nblk;
};
size_t refine_block_entries();
size_t refine_counters_bytes();
uint32_t refine_small_k();
uint32_t refine_first_cap();
// slot: len entries of scratch; labels_out may alias q.L (it is written only by a pass that succeeded)
// sym_n > 0 (and len == sym_n^2): the label pass also checks the new labels for symmetry, counters[3] = 1 if NOT symmetric
bool refine_mid_supports(const SigSource& q);  // RefineWs::mid is honoured for this source
bool launch_refine(hipStream_t s, int64_t len, const SigSource& q, uint32_t* slot, uint32_t* labels_out,
                   const RefineWs& ws, int64_t sym_n = 0);  // false: q is not sig_source_fusable

// ---------------------------------------------------------------------------
// kernels_class_compare.hip
// ---------------------------------------------------------------------------
size_t verify_ref_bytes(int64_t d);
size_t uconst_ref_bytes(int64_t d, int64_t r);
// The two checks below are ONE launch up to verify_lds_cap() classes (the table of representatives is built in LDS by every workgroup, `ref` is
// not touched) and then clear flag[0] with a store from the HOST before they enqueue the pass: `flag` is pinned host memory, and the verdict of
// the previous pass on that word has been read.  More classes: table kernel (which clears the word on the device) + compare pass.
int verify_lds_cap();
bool launch_basis_constant_on_classes(hipStream_t s, int64_t n, int64_t r, const double* U, const uint32_t* Lp, int64_t d,
                                      const uint32_t* first_idx, double atol, double scale, void* ref, uint32_t* flag);
bool launch_verify_no_split(hipStream_t s, const SigSource& q, int64_t d, const uint32_t* first_idx, void* ref, uint32_t* flag);
bool verify_no_split_supports(const SigSource& q, int64_t d);  // launch_verify_no_split has an instance for this shape
// "would the refinement of SIG_PAIR (a, b; packed lower triangle) write Lp and first_idx again?"  d <= verify_lds_cap() classes: one launch,
// flag[0] (pinned host memory, cleared from the host) stays 0 exactly then.  false: d outside [1, verify_lds_cap()], nothing enqueued
bool launch_verify_pair(hipStream_t s, int64_t n, const double* a, const double* b, const uint32_t* Lp, int64_t d, const uint32_t* first_idx,
                        uint32_t* flag, const uint8_t* Lp8 = nullptr);
// the projection half of the joint verdict alone (q: SIG_JOINT_I32 with 1 <= q.r <= 4, packed labels, d <= verify_lds_cap()): the rounded
// projected value of every entry against its class representative's; flag as above.  false: no instance, nothing enqueued
bool launch_verify_projection(hipStream_t s, const SigSource& q, int64_t d, const uint32_t* first_idx, uint32_t* flag);
// kernels_square_check.hip (SquareCheck: above, with the deferred tail that carries one)
bool square_check_supports(int64_t n, int64_t d, int G, int T);
size_t square_check_ws_bytes(int64_t n, int64_t d, int G, int T);
// sets the workspace pointers (n, d, G, T set); returns the bytes.  gap (a multiple of 16): bytes left untouched in front of every array and
// behind the last one (the test entry's sentinels)
size_t square_check_ws_carve(SquareCheck& q, void* ws, size_t gap = 0);
void launch_square_check_ref_and_pass(hipStream_t s, const SquareCheck& q);
void launch_square_check_verdict(hipStream_t s, const SquareCheck& q);
// loop.cpp: enqueue the next max_segments segments of the ctx's deferred tail on c->stream (none pending: nothing happens).
// in_ride: the caller is the module growth's ride (compress.cpp, Module::ortho_step) -- only counted (DeferredCheckStats)
void flush_deferred_tail(sdpsr_ctx* c, int max_segments = DEFERRED_SEGMENTS, bool in_ride = false);
inline bool deferred_tail_pending(const sdpsr_ctx* c) { return c->deferred_tail.next < c->deferred_tail.count; }
// The two windows of blockDiagonalize in which the host works while the stream has nothing of blockDiagonalize's own (compress.cpp):
// opened when the wait for a growth step's product returns, closed by whatever the host enqueues next (an upload, a label product,
// the lift).  Steady-clock time, accumulated per ctx; read through sdpsr_profile_deferred_checks.
uint64_t steady_ns();
inline void deferred_window_open(sdpsr_ctx* c, int which) { c->check_stats.window_open = which, c->check_stats.window_t0 = steady_ns(); }
inline void deferred_window_close(sdpsr_ctx* c) {
    DeferredCheckStats& t = c->check_stats;
    if (t.window_open < 0) return;
    t.window_ns[t.window_open] += steady_ns() - t.window_t0, ++t.window_count[t.window_open];
    t.window_open = -1;
}
// kernels_module.hip: one thread stores `seq` into a word of coherent pinned host memory, behind a system-scope fence: what the
// kernels before it in the stream stored into pinned memory is complete when the host sees the stamp (ctx_wait_word)
void launch_report_stamp(hipStream_t s, uint32_t* host_word, uint32_t seq);

// kernels_refine_sort.hip: radix-sort relabel for the many-classes regime
size_t refine_bucketed_workspace_bytes(int64_t len);
bool refine_bucket_set_device_attributes();
bool launch_refine_bucketed(hipStream_t s, int64_t len, const uint64_t* sig, uint32_t* labels_out, void* ws, size_t ws_bytes,
                            uint32_t* counters, uint32_t* first_idx, uint32_t first_cap, uint32_t* host_counters = nullptr, uint32_t host_seq = 0);
size_t refine_rank_slots_workspace_bytes(int64_t len);
bool launch_rank_slots(hipStream_t s, int64_t len, int64_t cap, const RefSlot* tab, uint32_t* tab_lab,
                       uint32_t* counters, uint32_t small_k, uint32_t* first_idx, uint32_t first_cap, void* ws, size_t ws_bytes);
// distinct-signature estimate of a signature array from <= 65536 sampled entries; host_out (pinned, 4 words): non-zero
// entries sampled, distinct signatures among them, signatures seen once, seen twice.  Returns the sample size (0: failed)
size_t refine_sample_workspace_bytes();
int64_t launch_refine_sample(hipStream_t s, int64_t len, const uint64_t* sig, void* ws, uint32_t* host_out);
size_t refine_sorted_workspace_bytes(int64_t len);
bool launch_refine_sorted(hipStream_t s, int64_t len, const uint64_t* sig, uint32_t* labels_out, void* ws, size_t ws_bytes,
                          uint32_t* counters);

// ---------------------------------------------------------------------------
// kernels_label_util.hip
// ---------------------------------------------------------------------------
void launch_max_pair_code(hipStream_t s, int64_t len, const uint32_t* p1, const uint32_t* p2, uint64_t d1, uint64_t* out);
void launch_transpose_labels(hipStream_t s, int64_t n, const uint32_t* L, uint32_t* Lt);
void launch_labels_checksum(hipStream_t s, int64_t len, const uint32_t* L, uint64_t* partial, uint64_t* out);
void launch_unpack_symmetric_labels(hipStream_t s, int64_t n, const uint32_t* Lp, uint32_t* L);
// symmetric-labels check: flag[0] = 1 if some L[i,j] != L[j,i]
void launch_check_symmetric(hipStream_t s, int64_t n, const uint32_t* L, uint32_t* flag);
void launch_copy_check_symmetric(hipStream_t s, int64_t n, const uint32_t* src, uint32_t* dst, uint32_t* flag, uint32_t epoch);
// dst = src (n x n labels; dst == src allowed) with two verdicts from the same tiles:
// flag[0] = 1 if src is not symmetric, flag[1] = 1 if a label exceeds dmax.  The caller clears flag[0..1] first.
void launch_copy_check_labels(hipStream_t s, int64_t n, const uint32_t* src, uint32_t* dst, uint32_t dmax, uint32_t* flag);

// ---------------------------------------------------------------------------
// kernels_dense_setup.hip: the small dense algebra of setup_dense.cpp and reduce_csr.cpp
// ---------------------------------------------------------------------------
int64_t reduce_columns_chunk(int64_t len, int64_t m, int64_t d);
bool launch_reduce_columns(hipStream_t s, int64_t len, int64_t m, int64_t d, const uint32_t* L, const double* A,
                           double* partial, double* out, uint32_t* bad_flag);
void launch_transpose_rows(hipStream_t s, int64_t len, int64_t m, const double* A, double* R);
void launch_col_norms2(hipStream_t s, int64_t len, int64_t k, const double* V, double* partial, int nblk, double* out);
void launch_scale_copy(hipStream_t s, int64_t len, const double* v, double alpha, double* out);
void launch_rank1_update(hipStream_t s, int64_t len, int64_t m, double* R, const double* u, const double* dots);
void launch_sub_round(hipStream_t s, int64_t len, const double* a, const double* b, double atol, double scale, double* out);

// kernels_module.hip / setup-stage helpers used across api.cpp
void launch_symmetrize(hipStream_t s, int64_t m, int64_t ld, double* B);
void launch_tall_times_small(hipStream_t s, int64_t n, int64_t ldi, const double* In, int kk, const double* S,
                             int lds_, int ncols, double alpha, double beta, double* out, int64_t ldo);
// The form launch_label_spmm_multi gives a shape (kernels_module.hip): matrix cores (label_spmm_mfma_kernel<tile, G>, tile = JT
// tiles of 16 columns of W) or VALU (label_spmm_sload_kernel<tile, G>, tile = WMAX), the column range split over z workgroups
// of cols_per_block columns each.  false: shape not supported.
struct LabelSpmmForm {
    int mfma, tile, z, cols_per_block;
};
bool label_spmm_select(int64_t n, int64_t d, int G, int w, LabelSpmmForm* f);
// Two elements on one W in one pass over the labels, each result to its own destination: Y0 = A(keys[0]) W, Y1 = A(keys[1]) W
// (w <= 64).  The form is label_spmm_select(n, d, 1, w)'s matrix-core form, run as label_spmm_mfma_kernel<tile, 2>: both results
// are bit for bit those of two one-element launches.  label_spmm_pair_select says whether the pair can run (false: n < 64,
// w > 64, or the class tables do not fit) and with which form; partials: label_spmm_pair_partial_doubles(n) doubles.
bool label_spmm_pair_select(int64_t n, int64_t d, int w, LabelSpmmForm* f);
size_t label_spmm_pair_partial_doubles(int64_t n);
bool launch_label_spmm_pair(hipStream_t s, int64_t n, const uint32_t* L, const uint64_t* keys, int64_t d, const double* W, int64_t ldw,
                            int w, double* partials, double* Y0, int64_t ldy0, double* Y1, int64_t ldy1);

// Kernels with more than 64 KiB of dynamic LDS carry a per-DEVICE attribute: sdpsr_create() sets
// them all with the ctx's device current (no process-global "already set" flags) and fails when one
// attribute call does (false: a later launch would otherwise fail with an opaque error).
bool gemm_set_device_attributes();
bool blockdiag_set_device_attributes();
bool module_set_device_attributes();
bool dense_setup_set_device_attributes();
bool insert_array_pair_set_device_attributes();  // kernels_insert_*.hip: the mid kernels of the sources with SRC::kMid
bool insert_proj_set_device_attributes();
bool insert_chan_set_device_attributes();
bool insert_joint_set_device_attributes();
bool sytrd_set_device_attributes();
bool small_syev_set_device_attributes();
bool stedc_set_device_attributes();
bool batched_set_device_attributes();
bool psd_set_device_attributes();
bool backtransform_set_device_attributes();
bool complex_set_device_attributes();
// kernels_complex.hip (complex path of blockDiagonalize, n <= 64; planes re / im, ld = n)
void launch_cx_embed(hipStream_t s, int64_t n, const double* Hr, const double* Hi, int64_t ld2, double* M);
void launch_cx_embed_adjoint(hipStream_t s, int64_t n, const double* Zr, const double* Zi, int64_t ld2, double* M);
void launch_cx_newton_schulz_factor(hipStream_t s, int64_t m, int64_t ld, double* K);
void launch_cx_unstack(hipStream_t s, int64_t n, int64_t cols, const double* E, int64_t ld2, double* Vr, double* Vi, int64_t ldv);
void launch_cx_rot(hipStream_t s, int64_t n, int64_t cols, int64_t ld2, const double* E, double* R);
void launch_cx_zero_pad(hipStream_t s, int64_t m, int64_t mc, int64_t ld, int64_t ldc, double* A);
void launch_cx_combine(hipStream_t s, int64_t n, int64_t ld2, const double* E, const int32_t* desc, const double* coef, double* Vr,
                       double* Vi);
void launch_cx_stack(hipStream_t s, int64_t n, int64_t cols, const double* Vr, const double* Vi, int64_t ldv, int64_t ld2, double* E);
void launch_cx_block_norms_general(hipStream_t s, int64_t n, int64_t ldn, const double* Gr, const double* Gi, const int32_t* space_of,
                                   int neig, unsigned long long* norms);
// the largest order of the complex path (sdpsr.h)
constexpr int64_t SDPSR_CX_MAX_N = 4096;
// dynamic LDS of cx_irreducible_general_kernel at order n, 0 when the order does not fit a workgroup's LDS; the launcher and the
// kernel's function attribute both come from here.  The launcher returns false, with nothing launched, where this says 0.
size_t cx_irreducible_general_lds_bytes(int64_t n);
bool launch_cx_irreducible_general(hipStream_t s, int64_t n, const double* Hr, const double* Hi, const double* Vr, const double* Vi,
                                   const int32_t* desc, int ncols, double atol, double* Qhat);
void launch_cx_basis_image_sorted(hipStream_t s, int64_t n, int64_t d, int64_t S, const uint32_t* ent, const int64_t* cls_ptr,
                                  const double* Qhat, const int32_t* descA, const int32_t* descB, double atol, double* out);
void launch_cx_gather_herm(hipStream_t s, int64_t n, const uint32_t* L, uint64_t key, double* Hr, double* Hi);
void launch_cx_heev(hipStream_t s, int64_t n, const double* Hr, const double* Hi, double* w, double* Vr, double* Vi, int* info);
void launch_cx_block_norms(hipStream_t s, int64_t n, const double* Hr, const double* Hi, const double* Vr, const double* Vi,
                           const int32_t* space_of, int neig, unsigned long long* norms);
void launch_cx_irreducible(hipStream_t s, int64_t n, const double* Hr, const double* Hi, const double* Vr, const double* Vi,
                           const int32_t* desc, int ncols, double atol, double* Qhat);
void launch_cx_basis_image(hipStream_t s, int64_t n, int64_t d, int64_t S, const uint32_t* L, const double* Qhat,
                           const int32_t* descA, const int32_t* descB, double atol, double* out);
// kernels_complex_image.hip: basis_image over C for a caller's Q_hat (sdpsr_basis_image_complex).  Qrm: n x S1 complex,
// row-major, (re, im) interleaved; out: the window's d * S complex numbers; ent / cls_ptr / chunks as on the real path
void launch_cx_rowmajor(hipStream_t s, int64_t n, int64_t S1, const double* Qcm, double* Qrm);
void launch_cx_image_chunk(hipStream_t s, int64_t n, int64_t d, int64_t S1, int64_t S, const double* Qrm, const uint32_t* ent,
                           const int32_t* descA, const int32_t* descB, const int64_t* chunk_ptr, int64_t nchunks,
                           const int64_t* chunk_begin, const int64_t* chunk_end, double* partial, double* out, double atol);
bool cx_image_outer_supports(int max_s, int nblocks, int64_t d);
void launch_cx_image_outer(hipStream_t s, int64_t n, int64_t d, int64_t S1, int64_t S, int nblocks, int max_s, const double* Qrm,
                           const uint32_t* ent, const int64_t* cls_ptr, const int32_t* blk_col, const int32_t* blk_size,
                           const int64_t* blk_off, double atol, double* out);
// kernels_batched.hip: `count` runs of eigen_decomposition on one partition of order n <= 64
void launch_eigdec_batched64(hipStream_t s, int64_t n, int64_t d, int64_t count, const uint32_t* L, const double* values,
                             uint64_t seed, uint64_t stream_base, double atol, int32_t* status, int32_t* neig,
                             int32_t* nclasses, int num_cus);
// kernels_sytrd_look.hip: the panel form with one launch per column (the launches are emitted by kernels_sytrd.hip)
struct SytrdLookArgs {
    double* A;  // n x n, leading dimension ld (multiple of 128, <= 8192), lower triangle referenced
    int64_t ld;
    int n;
    double* PT;        // ld x 64 row-major panel [V | W] (the layout of the trailing update's MFMA kernel)
    double* PTc;       // 64 x ld: the same panel column-major (the layout a row's owner thread reads)
    double* P;         // [2][ld / 128][ld]: partial products of the unnormalised column, one slot per partner block
    double* acol;      // [2][ld]: the updated column of the launch
    double* rec_norm;  // [2][ld / 128]: partial |a|^2 of the rows of a block
    double* rec_dots;  // [2][ld / 128][64]: partial [V'a | W'a]
    double* rec_vaz;   // [2][vaz_cap]: partial a'(A0 a), two per tile
    int64_t vaz_cap;
    double *d, *e, *tau;
};
const void* sytrd_look_kernel_fn(int mode, int64_t ld);
void sytrd_graph_cache_destroy(SytrdGraphCache* g);
void sytrd_graph_cache_stats(const SytrdGraphCache* g, uint64_t* hits, uint64_t* misses, double* instantiate_ms);

// ---------------------------------------------------------------------------
// kernels_gemm.hip:  C = A' * B (column-major), MFMA tiles staged through LDS.
// Operands must be padded: k multiple of KT, m and n multiples of 128, pointers 16-B
// aligned, lda/ldb multiples of 16 bytes.
// ---------------------------------------------------------------------------
// num_cus > 0: the persistent 256 x 256 launch (kernels_gemm_sym.hip) when n is a multiple of 256; variant =
// sdpsr_opts.square_kernel (0 = by size, 1 = 128 x 128 tiles of kernels_gemm.hip, 64 = persistent forced)
void launch_gemm_tn_i8_sym(hipStream_t s, int64_t n, int64_t k, const int8_t* X, int64_t ldx, int32_t* C, int64_t ldc,
                           int batch, int64_t strideX, int64_t strideC, const uint32_t* nonsym_flag, int num_cus = 0,
                           int variant = 0);
bool launch_i8_symsquare(hipStream_t s, int64_t n, int64_t k, const int8_t* X, int64_t ldx, int32_t* C, int64_t ldc, int batch,
                         int64_t strideX, int64_t strideC, const uint32_t* nonsym_flag, int num_cus, int variant);
bool i8_symsquare_pays(int64_t n, int T, int num_cus);
bool gemm_sym_set_device_attributes();
void launch_gemm_tn_f32_sym(hipStream_t s, int64_t n, int64_t k, const float* X, int64_t ldx, float* C, int64_t ldc,
                            int batch, int64_t strideX, int64_t strideC, const uint32_t* nonsym_flag);
void launch_gemm_tn_i8(hipStream_t s, int64_t m, int64_t n, int64_t k, const int8_t* A,
                       int64_t lda, const int8_t* B, int64_t ldb, int32_t* C, int64_t ldc,
                       int batch, int64_t strideA, int64_t strideB, int64_t strideC);
void launch_gemm_tn_f32(hipStream_t s, int64_t m, int64_t n, int64_t k, const float* A,
                        int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                        int batch, int64_t strideA, int64_t strideB, int64_t strideC);
void launch_gemm_tn_f64(hipStream_t s, int64_t m, int64_t n, int64_t k, const double* A,
                        int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                        int batch, int64_t strideA, int64_t strideB, int64_t strideC);
// C -= A' * B
void launch_gemm_tn_f64_sub(hipStream_t s, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B,
                            int64_t ldb, double* C, int64_t ldc);

// ---------------------------------------------------------------------------
// kernels_blockdiag.hip
// ---------------------------------------------------------------------------
// norms[bi*neig+bj] = max |M[i,j]| over the (bi,bj) eigenspace block; space_of[n] maps an
// index to its eigenspace.  norms must be zeroed (as uint64 bit patterns of doubles).
void launch_small_qtaq_block_norms(hipStream_t s, int64_t n, int64_t ld, const double* A, const double* Q,
                                   const int32_t* space_of, int neig, unsigned long long* norms, double* Mout, double* Tout = nullptr);
// the same with the eigenvalue clustering on the device (|dv| > atol starts a new eigenspace) and everything the
// host needs next in one packed device buffer: [status, sweeps, -, -, eigenspaces | 64 B][space_of n | padded to
// 64 B][values n][norms neig * neig]  (einfo: the eigensolver's "eig_info")
size_t small_cluster_pack_bytes(int64_t n);
void launch_small_cluster_qtaq_block_norms(hipStream_t s, int64_t n, int64_t ld, const double* A, const double* Q,
                                           const double* evals, double atol, const int* einfo, char* pack, double* Tout);
void launch_coupling_symmetrize_minmax(hipStream_t s, int neig, unsigned long long* norms, const int32_t* dims, unsigned long long* stat);
void launch_coupling_count(hipStream_t s, int neig, const unsigned long long* norms, const double* edges17, unsigned long long* stat);
void launch_coupling_bits(hipStream_t s, int neig, const unsigned long long* norms, double thr, unsigned long long* bits);
void launch_block_norms(hipStream_t s, int64_t n, int64_t ld, const double* M,
                        const int32_t* space_of, int neig, unsigned long long* norms);
// out[j] = sum_i Q[i, col0 + j] * a[i], j < m   (Q' a over a column range)
void launch_gemv_t(hipStream_t s, int64_t n, int64_t ld, const double* Q, int64_t col0,
                   int64_t m, const double* a, double* out);
// dst[i] (+)= alpha_dev[0] * sum_j Q[i, col0+j] * w[j]
void launch_gemv_n_scaled(hipStream_t s, int64_t n, int64_t ld, const double* Q, int64_t col0,
                          int64_t m, const double* w, const double* inv_norm, double* dst);
void launch_irreducible_pairs(hipStream_t s, int64_t n, int64_t ld, const double* Q, const double* Bf, int npairs,
                              int max_m2, const int32_t* desc, double* Qhat);
void launch_copy_cols(hipStream_t s, int64_t n, int64_t count, const int32_t* src_cols, const int32_t* dst_cols,
                      const double* src, int64_t ld_src, double* dst, int64_t ld_dst);
void launch_clamptol(hipStream_t s, int64_t len, double* a, double atol);
// norm2 of a vector -> out[0] = 1/||v||
void launch_inv_norm(hipStream_t s, int64_t m, const double* v, double* out);

// basis image.  Qrm: row-major n x S1 (Q_hat rows contiguous).  entries sorted by class:
// ent[e] = linear index, class_ptr[d+1].  desc: per output (colA, colB) pairs (S of them).
void launch_basis_image(hipStream_t s, int64_t n, int64_t d, int64_t S1, int64_t S,
                        const double* Qrm, const uint32_t* ent, const int64_t* class_ptr,
                        const int32_t* descA, const int32_t* descB, const int64_t* chunk_ptr,
                        int64_t nchunks_total, const int32_t* chunk_class,
                        const int64_t* chunk_begin, const int64_t* chunk_end, double* partial,
                        double* out, double atol);
bool basis_image_two_stage_fits(int64_t n, int64_t d, int64_t S1);
void launch_basis_image_outer(hipStream_t s, int64_t n, int64_t d, int64_t S1, int64_t S, int nblocks, int max_s,
                              const double* Qrm, const uint32_t* ent, const int64_t* cls_ptr,
                              const int32_t* blk_col, const int32_t* blk_size, const int64_t* blk_off, double atol,
                              double* out);
// A window of classes (first, d): in the launchers below that take `first`, d counts the classes first .. first + d - 1; labels
// are read through the window where they are loaded (class l - first + 1 inside, the skipped class 0 outside), tables,
// workspaces and outputs have d slabs.  (1, d) is the whole partition.  plain (the shortcuts' launchers): the window is (1, d) and
// every label is known to be <= d -- the ctx's own labels -- so the pair class-sum kernel uses them as they are.
// out[r + i*n] = sum over c with L[c + r*n] == first+i of x[c]   (class sums of a vector, i < d)
bool class_sums_supports(int64_t n, int64_t d, int64_t ldo);
void launch_class_sums(hipStream_t s, int64_t n, int64_t d, const uint32_t* L, const double* x, double* out, int64_t ldo, uint32_t first = 1);
// the pair class-sum pass of the basis_image shortcuts alone (tests): X n pairs, Y d * n pairs (interleaved); returns the waves
// per workgroup it ran with, 0 (nothing launched) when d is beyond its tables
int launch_class_sums_pair(hipStream_t s, int64_t n, int64_t d, uint32_t first, bool plain, const uint32_t* L, const double* X, double* Y);
void launch_basis_image_two_stage(hipStream_t s, int64_t n, int64_t d, uint32_t first, int64_t S1, int64_t S,
                                  const uint32_t* L, const double* Qrm, double* T, const int32_t* colA,
                                  const int32_t* colB, double atol, double* out);
size_t basis_image_commutative_workspace_doubles(int64_t n, int64_t d);
size_t basis_image_blocks_workspace_doubles(int64_t n, int64_t d);
bool launch_basis_image_blocks(hipStream_t s, int64_t n, int64_t d, uint32_t first, int64_t S1, int64_t S, int nblocks, const int32_t* blk_col, const int32_t* blk_size,
                               const int64_t* blk_off, const uint32_t* L, const double* Qrm, uint64_t key, int only, double atol, double tol, double* ws,
                               double* out, uint32_t* flag, bool plain = false);
bool launch_basis_image_fix_pair(hipStream_t s, int64_t n, int64_t d, uint32_t first, int64_t S1, const uint32_t* L, const double* Qrm, int k1, int k2,
                                 double atol, double* ws, double* out, bool plain = false);
bool launch_basis_image_commutative(hipStream_t s, int64_t n, int64_t d, uint32_t first, int64_t S1, const uint32_t* L, const double* Qrm, uint64_t key,
                                    double atol, double tol, double* ws, double* out, uint32_t* flag, bool plain = false);
void launch_transpose_to_rowmajor(hipStream_t s, int64_t n, int64_t S1, const double* Qcm,
                                  double* Qrm);
void launch_blocks_syev64(hipStream_t s, const BlocksSyevJob* jobs, int njac, int n1, int max_n, const double* Z, double* w, double* V,
                          int* flag);
// kernels_psd.hip: P_k = V max(w, 0) V' of the blocks of order <= 64 in one launch (jobs: the njac of order >= 2, then the n1 of
// order 1; max_n: the largest order; flag: one zeroed int -- bit 1 sweep limit, bit 2 a NaN / Inf).  Lam == nullptr: the plain
// form Z -> P, lam_min (one per block) optional.  Otherwise the solver's fused form: Z = Bx, P = S (previous iterate in, new one
// out), Lam <- (Bx + Lam) - S+, D = S+ - Lam+, slots[2 blk], [2 blk + 1] = the block's |Bx - S+|^2, |S+ - S|^2.
void launch_psd_project(hipStream_t s, const PsdJob* jobs, int njac, int n1, int max_n, const double* Z, double* P, double* lam_min,
                        double* Lam, double* D, double* slots, int* flag);
// The blocks of order 65 .. 128 (a ctx with psd_max_order = 128), one workgroup each, in a launch of their own.  jobs: the nmid
// mid jobs, those with psd_mid_v_in_global(n) FIRST: block b of the grid keeps its eigenvectors in slice b (PSD_MID_VSLICE
// doubles) of vscratch, which may be nullptr when no job needs one.  lds: the largest psd_mid_lds_bytes(n) of the jobs.
constexpr size_t PSD_MID_VSLICE = 128 * 128;
bool psd_mid_v_in_global(int n);
size_t psd_mid_lds_bytes(int n);
void launch_psd_project_mid(hipStream_t s, const PsdJob* jobs, int nmid, size_t lds, const double* Z, double* P, double* lam_min,
                            double* Lam, double* D, double* slots, double* vscratch, int* flag);
// kernels_sdp.hip: the setup and the affine step of sdpsr_sdp_solve (sdp_solve.cpp); stream-ordered, no host wait
void launch_sdp_record_class(hipStream_t s, int64_t n, const void* rec, uint32_t* cls);
void launch_sdp_gram(hipStream_t s, int64_t d, int64_t n, const void* rec_by_class_pos, int64_t* cptr, double* M);  // cptr: d + 1
void launch_sdp_scale_columns(hipStream_t s, int64_t d, const double* w, double* V);
void launch_sdp_gemm(hipStream_t s, int64_t m, int64_t n, int64_t k, const double* A, int64_t ar, int64_t ac, const double* B, int64_t br,
                     int64_t bc, double alpha, double beta, double* C, int64_t ldc);
void launch_sdp_affine_step(hipStream_t s, int64_t d, int nonneg, double rho, const double* Kt, const double* x0, const double* adj,
                            const double* chat, const double* uml_in, double* x, double* u, double* lam, double* uml_out, double* vs);
void launch_sdp_verdict(hipStream_t s, int64_t d, const double* vs, int64_t nblocks, const double* bs, double* pinned_out);
void launch_sdp_rescale(hipStream_t s, int64_t d, int64_t n, double f, const double* u, double* lam, double* uml, const double* S, double* Lam,
                        double* D);
void launch_sdp_scaled_copy(hipStream_t s, int64_t n, double f, const double* in, double* out);
// Stable LSD radix sort of the pairs (keys[e], e), e < len < 2^32, by the low `bits` bits of the key (4 bits per pass; the
// keys must not exceed them).  kA / kB / vA / vB: len words each, hist: radix_sort_hist_words(len).  The sorted keys and
// indices end in (kB, vB).  No atomics on the way: the order is a function of the keys alone.  (first, cnt): the first pass
// reads the keys through that window of classes; the default leaves every key as it is.
size_t radix_sort_hist_words(int64_t len);
void launch_radix_sort_pairs(hipStream_t s, int64_t len, int bits, const uint32_t* keys, uint32_t* kA, uint32_t* kB, uint32_t* vA,
                             uint32_t* vB, uint32_t* hist, uint32_t first = 1, uint32_t cnt = 0xFFFFFFFFu);
// stable sort of entries by label (label 0 dropped): ent sorted, hist[d+1]; the d classes from `first` on
int sort_entries_by_label(sdpsr_ctx* c, int64_t len, int64_t d, const uint32_t* L,
                          uint32_t** ent_out, std::vector<int64_t>& class_ptr_host, uint32_t first = 1);

// ---------------------------------------------------------------------------
// eigen.cpp (rocSOLVER)
// ---------------------------------------------------------------------------
// A (n x n, leading dimension lda) is overwritten with the eigenvectors; w[n] ascending.
// host_w (optional): the eigenvalues are also delivered to the host, riding on the status read-back
// after_launch: called once the eigensolver's kernels are enqueued, before the read-back synchronises
// defer_readback: return right after the launches; the status stays in ctx buffer "eig_info" for the caller's next read-back
int syev_device(sdpsr_ctx* c, int64_t n, double* A, int64_t lda, double* w, double* host_w = nullptr,
                const std::function<void()>* after_launch = nullptr, bool defer_readback = false);
void* ctx_pinned(sdpsr_ctx* c, size_t bytes);
void destroy_handle(sdpsr_ctx* c);

}  // namespace sdpsr
