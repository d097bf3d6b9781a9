// Host-side declarations shared by the orchestration translation units (ctx.cpp, primitives.cpp,
// loop.cpp, eigdec.cpp, compress.cpp, blockdiag.cpp, complex.cpp) and by the measurement library
// (prof/).  Nothing here is part of the ABI.
#pragma once
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "agree_plan.h"
#include "csr_canon.h"
#include "iso_classes.h"
#include "sdpsr_internal.h"

// sdpsr_comm_create (comm.cpp): one rank's handle of an RCCL communicator on the device of the ctx it was created on
struct sdpsr_comm {
    int device = 0;
    int32_t world = 1, rank = 0;
    void* nccl = nullptr;  // ncclComm_t
};

namespace sdpsr {

// SDPSR_DEBUG=1: host wall-clock marks on stderr (relative to the ctx's previous mark); the only
// environment variable the library reads, and it changes no result
bool dbg_on();
void dbg_mark(sdpsr_ctx* c, const char* what);

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        hipGetDevice(&prev);
        if (prev != dev) hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur;
        hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) hipSetDevice(prev);
    }
};

template <typename T>
const T* in_dev(sdpsr_ctx* c, const char* name, const T* p, size_t count, int mem, int* st) {
    if (mem == SDPSR_MEM_DEVICE || p == nullptr) return p;
    T* d = (T*)ctx_buf(c, name, count * sizeof(T));
    if (!d) {
        *st = SDPSR_OUT_OF_MEMORY;
        return nullptr;
    }
    if (hipMemcpyAsync(d, p, count * sizeof(T), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        *st = ctx_fail(c, SDPSR_HIP_ERROR, std::string("H2D copy of ") + name);
        return nullptr;
    }
    c->h2d_bytes += count * sizeof(T);
    return d;
}

template <typename T>
T* out_dev(sdpsr_ctx* c, const char* name, T* p, size_t count, int mem, int* st) {
    if (mem == SDPSR_MEM_DEVICE) return p;
    T* d = (T*)ctx_buf(c, name, count * sizeof(T));
    if (!d) *st = SDPSR_OUT_OF_MEMORY;
    return d;
}

template <typename T>
int out_finish(sdpsr_ctx* c, T* host, const T* dev, size_t count, int mem) {
    // outputs are complete on return in both memory spaces (ordering rule of sdpsr.h)
    if (mem != SDPSR_MEM_DEVICE) {
        HIP_TRY(c, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
        c->d2h_bytes += count * sizeof(T);
    }
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    return SDPSR_OK;
}

// ---- label arrays at the ctx's interface width (sdpsr_set_label_width; labels.cpp) ----
// At width 32 the three templates above under another name: same buffers, same bytes counted.  At 16 / 8 the named buffer is
// ALWAYS the ctx's own uint32 array, in both memory spaces: an input is widened into it (host arrays: count * B / 8 bytes
// uploaded into the staging buffer "lab_stage" first), an output is formed in it and narrowed into the caller's array by
// labels_out_finish (host arrays: narrowed into "lab_stage", count * B / 8 bytes copied out).
const uint32_t* labels_in_dev(sdpsr_ctx* c, const char* name, const uint32_t* p, size_t count, int mem, int* st);
uint32_t* labels_out_dev(sdpsr_ctx* c, const char* name, uint32_t* p, size_t count, int mem, int* st);
int labels_out_finish(sdpsr_ctx* c, uint32_t* p, const uint32_t* dev, size_t count, int mem);
// the pieces, for the entries that copy labels by hand: the caller's array (ctx's width, memory space mem) into / from a uint32
// device array, stream-ordered, no host wait; labels_delivered checks the narrowing pass's flag once the stream has been waited for
int labels_fetch(sdpsr_ctx* c, uint32_t* dst32, const uint32_t* p, size_t count, int mem);
int labels_deliver(sdpsr_ctx* c, uint32_t* p, const uint32_t* src32, size_t count, int mem);
int labels_delivered(sdpsr_ctx* c);
// a partition of `classes` classes cannot be delivered at the ctx's width (the reference's InexactError of Partition{T}, src/partitions.jl:29):
// decided on the host from the count, before any label is written
bool label_width_overflows(const sdpsr_ctx* c, uint64_t classes);
int label_width_fail(sdpsr_ctx* c, const char* where, uint64_t classes);
// kernels_labels.hip
void launch_labels_narrow(hipStream_t s, int64_t len, const uint32_t* in, void* out, int bits, uint32_t* flag, int num_cus);
void launch_labels_widen(hipStream_t s, int64_t len, const void* in, int bits, uint32_t* out, int num_cus);
// kernels_agree.hip: keys[e] = sum_i arrays[i][e] * mult[i] mod 2^64 (0 <= R <= 64 device arrays of `bits`-wide labels)
void launch_meet_keys(hipStream_t s, int64_t len, int R, const void* const* arrays, const uint64_t* mult, int bits, uint64_t* keys, int num_cus);
// comm.cpp: the collectives of the agreement (agree.cpp), on ctx's stream; comm != nullptr.  comm_usable: comm lives on ctx's device.
// all_gather: `bytes` of host memory per rank into table (world * bytes, host, rank order) through device staging and ONE read-back;
// all_reduce_sum_u64 / broadcast_dev: device memory in place, stream-ordered, no host wait
int comm_usable(sdpsr_ctx* c, const sdpsr_comm* comm);
int comm_all_gather(sdpsr_ctx* c, sdpsr_comm* comm, const void* mine, size_t bytes, void* table);
int comm_all_reduce_sum_u64(sdpsr_ctx* c, sdpsr_comm* comm, uint64_t* dev, int64_t count);
int comm_broadcast_dev(sdpsr_ctx* c, sdpsr_comm* comm, void* dev, size_t bytes, int32_t root);
// loop.cpp: sdpsr_desymmetrize on uint32 device labels, in place
int desymmetrize_device(sdpsr_ctx* c, int64_t n, uint32_t* L, int64_t* dim, int32_t* iters);

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

bool ctx_ensure_side(sdpsr_ctx* c);
int d2h_sync(sdpsr_ctx* c, void* host, const void* dev, size_t bytes);
// Upload of a small host array.  Up to 32 KiB go through a ring of pinned slots and stay
// stream-ordered (the caller's buffer is free on return, no host wait)
int h2d_sync(sdpsr_ctx* c, void* dev, const void* host, size_t bytes);
inline int ceil_log2(uint64_t x) {
    int l = 0;
    while ((uint64_t(1) << l) < x) ++l;
    return l;
}
// sdpsr_ctx::table_log2_hint as a refinement of len entries that ended with `classes` classes leaves it: a table with at most an
// eighth of its slots taken, between 2^12 slots and the full size of the input (two slots per entry)
inline int refine_table_hint(int64_t len, uint64_t classes) {
    const int full = std::max(12, ceil_log2((uint64_t)len * 2));
    return std::min(full, std::max(12, ceil_log2(classes * 8 + 1)));
}

double round_scale(const sdpsr_ctx* c, double atol);
bool label_overflows(const sdpsr_ctx* c, uint64_t value);
int label_overflow_fail(sdpsr_ctx* c, const char* where, uint64_t value);
uint64_t next_key(sdpsr_ctx* c);
int check_len(sdpsr_ctx* c, int64_t len);
// reduce.cpp / batch.cpp: the entry points with the memory spaces of the inputs and of the outputs named separately
int jordan_reduce_impl(sdpsr_ctx* c, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r, double atol, double epsilon,
                       uint32_t* P_out, int64_t* dim_out, int32_t* iters_out, int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* blks,
                       int64_t blks_capacity, double* Q_hat, int64_t qhat_capacity, double* phase_ms, int mem_in, int mem_out);
int jordan_reduce_batch_impl(sdpsr_ctx* c, int32_t R, const uint64_t* seeds, int64_t n, const double* CL, const double* X0L, const double* U,
                             int64_t r, int hint, double atol, double epsilon, uint32_t* const* P_out, int64_t* dim_out, int32_t* iters_out,
                             int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* const* blks, const int64_t* blks_capacity,
                             int32_t* status, int mem_in, int mem_out);

// ---- phase timing with events; collected after the syncs the loop needs anyway ----
struct PhaseTimer {
    sdpsr_ctx* c;
    double acc[SDPSR_T_COUNT] = {};
    struct Pending {
        int slot;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    bool enabled;
    PhaseTimer(sdpsr_ctx* ctx, bool en) : c(ctx), enabled(en) {}
    ~PhaseTimer() {
        for (auto e : pool) hipEventDestroy(e);
        for (auto& p : pending) {
            hipEventDestroy(p.a);
            hipEventDestroy(p.b);
        }
    }
    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        hipEventCreate(&e);
        return e;
    }
    int cur_slot = -1;
    hipEvent_t cur_a{};
    void begin(int slot) {
        if (!enabled) return;
        cur_slot = slot;
        cur_a = get();
        hipEventRecord(cur_a, c->stream);
    }
    void end() {
        if (!enabled || cur_slot < 0) return;
        hipEvent_t b = get();
        hipEventRecord(b, c->stream);
        pending.push_back({cur_slot, cur_a, b});
        cur_slot = -1;
    }
    void collect() {  // intervals whose end event has not completed yet stay pending
        std::vector<Pending> later;
        for (auto& p : pending) {
            float ms = 0;
            const hipError_t e = hipEventElapsedTime(&ms, p.a, p.b);
            if (e == hipErrorNotReady) {
                later.push_back(p);
                continue;
            }
            if (e == hipSuccess) acc[p.slot] += ms;
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        (void)hipGetLastError();
        pending.swap(later);
    }
};

// closes the phase it opened on every exit path; collect: as the successful path does behind this phase
struct PhaseScope {
    PhaseTimer& tm;
    bool collect;
    PhaseScope(PhaseTimer& t, int slot, bool col) : tm(t), collect(col) { tm.begin(slot); }
    ~PhaseScope() {
        tm.end();
        if (collect) tm.collect();
    }
};

// start / stop events of a whole entry point (phase_ms[SDPSR_T_TOTAL]); freed on every exit path
struct TotalEvents {
    hipEvent_t a = nullptr, b = nullptr;
    TotalEvents(bool enabled, hipStream_t s) {
        if (!enabled) return;
        if (hipEventCreate(&a) != hipSuccess) a = nullptr;
        if (hipEventCreate(&b) != hipSuccess) b = nullptr;
        if (a) hipEventRecord(a, s);
    }
    ~TotalEvents() {
        if (a) hipEventDestroy(a);
        if (b) hipEventDestroy(b);
    }
    float stop(hipStream_t s) {  // records the end, waits for it, returns the milliseconds
        float ms = 0;
        if (!a || !b) return ms;
        hipEventRecord(b, s);
        hipEventSynchronize(b);
        hipEventElapsedTime(&ms, a, b);
        return ms;
    }
    TotalEvents(const TotalEvents&) = delete;
    TotalEvents& operator=(const TotalEvents&) = delete;
};

// ---- the words of c->pinned and c->pinned_small that kernels (and small copies) report into: one table for the loop (loop.cpp), the
// refinement (primitives.cpp) and the reduction's deferred verdicts (reduce.cpp).  uint32 words [first, first + count); no two regions share a
// word, and the symmetry probe's r doubles, the only variable-length report, start behind them all: (char*)c->pinned + PINNED_FIXED_BYTES
struct PinnedWords { size_t first, count; };
constexpr PinnedWords PINNED_REFINE{0, 4};  // the refinement's counters as its label pass stores them:
enum { REFINE_INSERTED = 0, REFINE_OVERFLOW = 1, REFINE_CLASSES = 2, REFINE_STAMP = 3 };  // (STAMP: the report's sequence number; the fused symmetry verdict when the counters are copied)
constexpr PinnedWords PINNED_SYMMETRY{8, 1};          // != 0: the new labels are NOT symmetric
constexpr PinnedWords PINNED_VERIFY{128, 1};          // != 0: an entry differs from its class representative (verify pass)
constexpr PinnedWords PINNED_SPECULATIVE{144, 1};     // the same for the speculative confirm round
constexpr PinnedWords PINNED_BASIS_CONSTANT{192, 1};  // != 0: some U_k is not constant on the classes
constexpr PinnedWords PINNED_SAMPLE{224, 4};          // sample of the signatures: non-zero, distinct, seen once, seen twice
constexpr size_t PINNED_FIXED_BYTES = 1024;
// basis_image's shortcuts (blockdiag.cpp): a count, then one verdict per column / block, from this word on.  Variable length: the tail runs
// over the loop's words behind it; the shortcut waits for the stream and reads its words before it returns
constexpr PinnedWords PINNED_BASIS_IMAGE_VERDICTS{64, 1};
constexpr PinnedWords PINNED_SMALL_FLAG{0, 1};                   // c->pinned_small (256 B): the flag of the one-shot entries ("a label exceeds d", symmetry)
constexpr PinnedWords PINNED_SMALL_LABEL_CHECK{2, 2};             // sdpsr_basis_image: [0] != 0 the caller's P is not symmetric, [1] != 0 a label exceeds d
constexpr PinnedWords PINNED_SMALL_ROWSPACE_NNZ{4, 2};            // sdpsr_compress_constraints: the 64-bit count of non-zeros left in the kept rows
constexpr PinnedWords PINNED_SMALL_DEFERRED_VERIFY{8, 1};        // sdpsr_jordan_reduce: the two verdicts the loop left unread (c->deferred_verdict)
constexpr PinnedWords PINNED_SMALL_DEFERRED_SPECULATIVE{24, 1};
constexpr PinnedWords PINNED_SMALL_DEFERRED_INITIAL{16, 1};       // ... and the one of the guessed initial partition (c->initial_guess_pending)
constexpr PinnedWords PINNED_SMALL_DEFERRED_NARROW{20, 1};        // ... != 0: a label did not fit the 8-bit shadow made behind that guess (read with it: "violated")
constexpr PinnedWords PINNED_SMALL_GRAM_STAMP{32, 1};           // module growth: the stamp behind a round's Gram products (compress.cpp, ortho_step)
constexpr PinnedWords PINNED_SMALL_CANON{44, 18};                // sdpsr_sparse_create: the nine 64-bit words of CanonVerdict (csr_canon.h)
constexpr PinnedWords PINNED_SMALL_NARROW{40, 1};                // != 0: a label did not fit the narrow type (kernels_labels.hip); cleared by the host before each pass
constexpr bool pinned_words_disjoint(std::initializer_list<PinnedWords> w, size_t bytes) {
    for (const PinnedWords* a = w.begin(); a != w.end(); ++a) {
        if (a->count == 0 || (a->first + a->count) * 4 > bytes) return false;
        for (const PinnedWords* b = w.begin(); b != a; ++b)
            if (a->first < b->first + b->count && b->first < a->first + a->count) return false;
    }
    return true;
}
static_assert(pinned_words_disjoint({PINNED_REFINE, PINNED_SYMMETRY, PINNED_BASIS_IMAGE_VERDICTS, PINNED_VERIFY, PINNED_SPECULATIVE, PINNED_BASIS_CONSTANT, PINNED_SAMPLE}, PINNED_FIXED_BYTES) &&
              PINNED_FIXED_BYTES % sizeof(double) == 0, "two reports share a word of c->pinned, or one reaches into the symmetry probe's doubles");
static_assert(pinned_words_disjoint({PINNED_SMALL_FLAG, PINNED_SMALL_LABEL_CHECK, PINNED_SMALL_ROWSPACE_NNZ, PINNED_SMALL_DEFERRED_VERIFY, PINNED_SMALL_DEFERRED_SPECULATIVE, PINNED_SMALL_DEFERRED_INITIAL, PINNED_SMALL_DEFERRED_NARROW, PINNED_SMALL_GRAM_STAMP, PINNED_SMALL_NARROW, PINNED_SMALL_CANON}, 256) &&
              (PINNED_SMALL_CANON.first * 4) % 8 == 0 && PINNED_SMALL_CANON.count * 4 == sizeof(CanonVerdict), "two reports share a word of c->pinned_small");
inline uint32_t* pinned_report(sdpsr_ctx* c, PinnedWords w) {  // the pinned words of one report (nullptr: no pinned buffer)
    uint32_t* p = (uint32_t*)ctx_pinned(c, PINNED_FIXED_BYTES);
    return p ? p + w.first : nullptr;
}
// The verdict of a guessed initial partition (c->initial_guess_pending), once the stream has been waited for: the pair check's word, and
// the overflow word of the narrowing launch made behind that guess (cleared with the guess; it stays 0 where no shadow was made)
inline uint32_t initial_guess_violated(const sdpsr_ctx* c) {
    const volatile uint32_t* ps = c->pinned_small;
    return ps[PINNED_SMALL_DEFERRED_INITIAL.first] | ps[PINNED_SMALL_DEFERRED_NARROW.first];
}

// canonical refinement of a signature source / array (primitives.cpp)
// early: return as soon as the label pass has REPORTED the class count (ctx_wait_word) -- the pass itself is still running; only
// for a caller that goes on in stream order and waits for the stream before its own return
int refine_signatures(sdpsr_ctx* c, int64_t len, const SigSource& src_in, uint32_t* labels, int64_t* nparts, int64_t sym_n = 0,
                      uint32_t* symflag_dev = nullptr, int* sym_out = nullptr, bool early = false);
int refine_signatures(sdpsr_ctx* c, int64_t len, const uint64_t* sig, uint32_t* labels, int64_t* nparts, int64_t sym_n = 0,
                      uint32_t* symflag_dev = nullptr, int* sym_out = nullptr, bool early = false);

// loop.cpp / blockdiag.cpp: the bodies of the entry points, chainable without host synchronisation in between
// (reduce.cpp: sdpsr_jordan_reduce)
int admissible_subspace_impl(sdpsr_ctx* c, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r, double atol,
                             uint32_t* P_out, int64_t* dim_out, int32_t* iters_out, double* phase_ms, int mem, int mem_out,
                             bool final_sync, int* labels_sym_out);
// setup_dense.cpp: the setup stage of the dense entry in pieces, shared with the CSR entries (setup_csr.cpp)
int setup_mgs(sdpsr_ctx* c, int64_t len, int64_t m, double* R, double* U, double* partial, int nblk, double* coef,
              std::vector<std::vector<double>>& coeffs, std::vector<int64_t>& piv, int64_t* r_out);
std::vector<double> min_norm_coefficients(int64_t r, const std::vector<int64_t>& piv, const std::vector<std::vector<double>>& coeffs,
                                          const double* b);
int setup_tail(sdpsr_ctx* c, int64_t n, int64_t r, const double* U, const std::vector<double>& y, double atol, double* v1, double* v2,
               double* dCL, double* dX0, double* partial, int nblk, double* coef);
// trusted_symmetric: the caller made the labels and knows; in_place (device labels only): no copy into ctx buffer
// "bd_labels" -- P itself serves phase 2 (c->bd_labels_ext) until the caller ends that arrangement
int block_diagonalize_impl(sdpsr_ctx* c, int64_t n, const uint32_t* P, int64_t d, double epsilon, int32_t* nblocks, int64_t* sum_sq,
                           int64_t* sum_s, double* phase_ms, int mem, bool trusted_symmetric, bool final_sync, bool in_place = false,
                           bool labels_are_u32 = true);  // false (the public entry): P has the ctx's label width

// ---- blockDiagonalize: host pieces and drivers (eigdec.cpp, compress.cpp) ----
struct EigInfo {
    std::vector<double> vals;
    std::vector<int> ptrs;  // 0-based boundaries, size neig+1
    std::vector<int> kpart; // root of every eigenspace
    // "bd_t" holds T = A2 Q for the ONE generic element A2 whose couplings decided the classes
    // (false after extra coupling elements: the decisive block may come from any of them)
    bool t_valid = false;
};

// Source of "generic elements" for the dense driver: the label gather (gen == nullptr,
// randomize!(A, P)) or a compressed representation B = W' A W of it (module-compression driver).
struct ElemGen {
    // writes an (n_eff x n_eff, leading dimension ld_eff, zero padded) symmetric matrix
    std::function<int(double* dst)> make;
    // optional: start making the NEXT element into dst on a side stream (returns 0 if started),
    // and make the main stream wait for it
    std::function<int(double* dst)> prefetch;
    std::function<int()> join;
    // optional: mark the fork point on the main stream NOW; a later prefetch() starts from this
    // point (so that the eigensolver can be enqueued first and its launches do not wait behind the
    // prefetch's host-side launch work)
    std::function<int()> fork;
};
int make_element(sdpsr_ctx* c, const ElemGen* gen, int64_t n, int64_t ld, const uint32_t* L, double* dst);
// iso_classes.h holds the host arithmetic (Otsu threshold, union-find, class structure, layouts); this adds the one error message
int isomorphism_classes(sdpsr_ctx* c, const std::vector<double>& norms, int neig, double atol, std::vector<int>& kpart);
// the same with the coupling matrix on the device (symmetrised in place there); trace: what the host formed on the way (tests)
struct CouplingTrace {
    double edges[17];
    double thr;
};
int isomorphism_classes_device(sdpsr_ctx* c, unsigned long long* dnorms, int neig, const std::vector<int32_t>& dims, double atol,
                               std::vector<int>& kpart, CouplingTrace* trace = nullptr);
// EigDec::couple(): T = A Q into Tp, M = Q' T into Ap (all ld x ld, padded), then the block maxima of M raise dnorms
void couple_block_norms(hipStream_t s, int64_t n, int64_t ld, double* Ap, const double* Q, double* Tp, const int32_t* dspace, int neig,
                        unsigned long long* dnorms);
// Irreducible::launch_pairs(): the columns of Q-hat of the 7-int pair descriptors, by the pair kernel or one by one
bool irreducible_pairs_fit_lds(int64_t max_m2);
int irreducible_pairs(sdpsr_ctx* c, int64_t n, int64_t ld, const double* Q, const double* Bf, const std::vector<int32_t>& pairs,
                      int64_t max_m2, double* Qhat, int route = -1, int* ran = nullptr);
int irreducible_pairs_one_by_one(sdpsr_ctx* c, int64_t n, int64_t ld, const double* Q, const double* Bf, const std::vector<int32_t>& pairs,
                                 double* Qhat);
int eigen_decomposition_device(sdpsr_ctx* c, int64_t n, const uint32_t* L, double atol, EigInfo& info, PhaseTimer& tm,
                               const ElemGen* gen = nullptr, int64_t expect_dim = -1);
// status used internally when a driver of diagonalize hands over to the dense one
constexpr int DRIVER_FALLBACK = -1000;
int driver_fallback(sdpsr_ctx* c, const std::string& why);
int dense_diagonalize(sdpsr_ctx* c, int64_t n, const uint32_t* L, const ElemGen* gen, double atol, EigInfo& info,
                      std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, PhaseTimer& tm, int64_t expect_dim = -1);
int gemm_tn_splitk(sdpsr_ctx* c, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B, int64_t ldb,
                   double* C, int64_t ldc, const char* partials = "splitk_partials");
// host_C (optional, pinned host memory, mp x np like C): filled by the product itself when the exact-shape kernel
// runs; *host_filled says whether it did (the padded split-K path does not)
bool gram_tn_is_skinny(int64_t ma, int64_t nb);  // the route gram_tn takes: the exact-shape kernel (true) or split-K
int gram_tn(sdpsr_ctx* c, int64_t ma, int64_t nb, int64_t k, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
            int64_t mp, int64_t np, double* host_C = nullptr, bool* host_filled = nullptr);
int compressed_diagonalize(sdpsr_ctx* c, int64_t n, const uint32_t* L, int64_t d, double atol, EigInfo& info,
                           std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, PhaseTimer& tm);
bool compression_eligible(const sdpsr_ctx* c, int64_t n, int64_t d);

// small_eigen_host.cpp: the compressed problem (order w <= 64) on the host
int host_syev(int n, const double* A, int lda, double* w, double* Z, int ldz);  // host_syev.cpp
void host_count_edges17(const double* x, size_t n, const double* ed, int64_t* hist);
void host_gemm_tn(int m, int n, int k, const double* A, int lda, const double* B, int ldb, double* C, int ldc);
int murota_small_host(sdpsr_ctx* c, int w, const double* B1, const std::function<int(double*)>& next_element, double atol,
                      int64_t expect_dim, std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, std::vector<double>& Qs);

// ---- kernel launchers used by the host files only (kernels_module.hip, kernels_sytrd.hip, ...) ----
void launch_symmetrize(hipStream_t s, int64_t m, int64_t ld, double* B);
void launch_extract_symmetric(hipStream_t s, int64_t m, int64_t mp, const double* src, int64_t lds_, double* dst);
void launch_splitk_reduce(hipStream_t s, int64_t len, int Z, int64_t stride, const double* P, double* C);
size_t gram_small_partial_doubles(int64_t k, int ma, int nb);
void launch_gram_small(hipStream_t s, int64_t k, int ma, int nb, const double* A, int64_t lda, const double* B, int64_t ldb,
                       double* partials, double* C, int64_t ldc, int mp, int np, double* host_C = nullptr);
size_t label_spmm_partial_doubles(int64_t n, int w);
bool launch_label_spmm_multi(hipStream_t s, int64_t n, const uint32_t* L, const uint64_t* keys, int G, int64_t d, const double* W,
                             int64_t ldw, int w, double* partials, double* Y, int64_t ldy);
bool launch_label_spmm(hipStream_t s, int64_t n, const uint32_t* L, uint64_t key, int64_t d, const double* W,
                       int64_t ldw, int w, double* partials, double* Y, int64_t ldy);
void launch_tall_times_small(hipStream_t s, int64_t n, int64_t ldi, const double* In, int kk, const double* S,
                             int lds_, int ncols, double alpha, double beta, double* out, int64_t ldo);
void launch_normalize_columns(hipStream_t s, int64_t n, int64_t ld, double* H, int64_t hstride, const double* X,
                         int64_t ldx, int nruns, double* norm0);
void launch_random_vector(hipStream_t s, int64_t n, uint64_t key, double* x);
// random_vector + normalize_columns (one run) as one single-workgroup launch: x, h = x / |x| and norm0[0] = |x|, bit for bit
void launch_seed_vector(hipStream_t s, int64_t n, uint64_t key, double* x, double* h, double* norm0);
// rows n .. ld-1 of `cols` columns of M <- 0 (nothing launched when ld == n)
void launch_pad_rows(hipStream_t s, int64_t n, int64_t ld, int64_t cols, double* M);
// launch_tall_times_small with a workgroup per 64 rows that owns every output column (ncols <= 64): `out` may alias columns of
// In.  The same sums bit for bit.  false: ncols beyond the form, nothing launched.
bool tall_times_small_rows_supports(int ncols);
bool launch_tall_times_small_rows(hipStream_t s, int64_t n, int64_t ldi, const double* In, int kk, const double* S, int lds_, int ncols,
                                  double alpha, double beta, double* out, int64_t ldo);
// the lift in one launch: Qcm = clamptol(In S, atol) (ld n) and its row-major copy Qrm[i * ncols + c]; false: ncols > 64
bool launch_lift_clamped(hipStream_t s, int64_t n, int64_t ldi, const double* In, int kk, const double* S, int lds_, int ncols, double atol,
                         double* Qcm, double* Qrm);
void launch_fill_test_sig(hipStream_t s, int64_t len, int64_t nclasses, uint64_t* sig);
size_t sytrd_workspace_doubles(int64_t n, int64_t ld);
void launch_sytrd(sdpsr_ctx* c, int64_t n, double* A, int64_t ld, double* d, double* e, double* tau, double* ws);
void launch_sytrd_symv_sweep(hipStream_t s, int64_t n, double* A, int64_t ld, double* d, double* e, double* tau, double* ws);
// kernels_setup_csr.hip: the CSR setup stage (setup_csr.cpp)
void launch_csr_densify(hipStream_t s, int64_t len, int64_t m, const int64_t* rowptr, const uint32_t* col, const double* val, double* W);
size_t gram_tall_partial_doubles(int64_t len, int64_t m);
void launch_gram_tall(hipStream_t s, int64_t len, int64_t m, const double* W, double* partials, double* host_G);
void launch_apply_upper_inverse(hipStream_t s, int64_t len, int64_t m, double* W, const int32_t* piv, const double* Xrow);
bool launch_small_syev(hipStream_t s, int64_t n, double* A, int64_t lda, double* w, double* Vtmp, int* info);
// kernels_sytrd.hip: the range of sdpsr_syev_f64.  dst (ld x ld, padding zeroed by the caller) <- src (n x n) with the lower triangle
// times 2^-e, e chosen on the device from max |a| (0 inside [2^-400, 2^400]); slot: 16 bytes of device memory that keep 2^e for
// launch_syev_unscale_values (w *= 2^e).  With e = 0 neither changes a bit.
void launch_syev_scaled_copy(hipStream_t s, int64_t n, const double* src, int64_t ld, double* dst, void* slot);
void launch_syev_unscale_values(hipStream_t s, int64_t n, double* w, const void* slot);
// kernels_stedc.hip: divide and conquer for the tridiagonal problem (eigen.cpp has the calling sequence)
size_t stedc_workspace_bytes(int64_t ld);
size_t stedc_descriptors(int64_t ld, std::vector<int>& out);
void* stedc_descriptor_slot(void* ws, int64_t ld);
bool launch_stedc(hipStream_t s, int64_t n, int64_t ld, const double* d, const double* e, double* w, double* Z, double* W1, double* W2,
                  void* ws);
void launch_stedc_check(hipStream_t s, int64_t n, const double* a, const double* b, int pre, int* info);
// eigen.cpp: the two halves of the back-transformation Z <- Q Z, both issued on c->stream (syev_device points c->stream at the
// side stream around the first half when it can fork; the test entry sdpsr_profile_backtransform runs both on the main stream)
int backtransform_prepare(sdpsr_ctx* c, int64_t n, const double* A, int64_t ld, const double* tau);
int backtransform_apply(sdpsr_ctx* c, int64_t n, int64_t ld, double* Z);

// setup_csr.cpp: what a CSR input means, for every entry that takes one (the setup entries, sdpsr_reduce_constraints_csr).
// Validates (SDPSR_BAD_ARGUMENT with a message, before any kernel) and brings the rows into canonical form.
struct CanonCsr {
    std::vector<int64_t> rowptr;  // m + 1, 0-based
    std::vector<uint32_t> col;    // sorted per row, no duplicates
    std::vector<double> val;      // no zeros
};
int canonicalize_csr(sdpsr_ctx* c, int64_t len, int64_t m, const int64_t* rowptr, const int64_t* colind, const double* val, int base,
                     CanonCsr& out);
// setup_csr.cpp / reduce_csr.cpp: the parts behind "canonical CSR is on the device" (rowptr int64 0-based, columns uint32 sorted per
// row, no duplicates, no zeros) -- shared by the _csr entries (host pass + upload) and the _sparse entries (a handle's arrays)
struct CsrSetupOut {
    double *CL = nullptr, *X0 = nullptr;
    const double* U = nullptr;  // len x r on the device
    int64_t r = 0;
    int hint = 0;
    int32_t info = SDPSR_SETUP_NO_CONSTRAINTS;
};
int setup_from_device_csr(sdpsr_ctx* c, int64_t n, int64_t m, const int64_t* drp, const uint32_t* dcol, const double* dval, int64_t nnz,
                          bool symmetric, const double* b, const double* C, double atol, CsrSetupOut& o);
int reduce_from_device_csr(sdpsr_ctx* c, int64_t len, const uint32_t* labels, int64_t d, int64_t m, const int64_t* drp, const uint32_t* dcol,
                           const double* dval, int64_t nnz, double* out, int mem);
// kernels_csr_canon.hip: the canonical pass on the device (sparse_handle.cpp); every launcher is stream-ordered, no host wait
void launch_canon_check(hipStream_t s, int64_t len, int64_t m, int64_t nnz, const int64_t* rowptr, const int64_t* colind, const double* val,
                        int base, uint32_t* col32, unsigned char* keep, CanonVerdict* verdict);
void launch_canon_row_ids(hipStream_t s, int64_t nnz, int64_t m, const int64_t* rowptr, int base, uint32_t* row);
void launch_canon_gather_u32(hipStream_t s, int64_t nnz, const uint32_t* idx, const uint32_t* src, uint32_t* dst);
void launch_canon_runs(hipStream_t s, int64_t nnz, const uint32_t* pos2, const uint32_t* col1, const uint32_t* idx1, const uint32_t* row_sorted,
                       const double* val, uint32_t* col_sorted, uint32_t* idx_sorted, double* sum, unsigned char* keep, CanonVerdict* verdict);
void launch_canon_count_scan(hipStream_t s, int64_t n, const unsigned char* keep, int64_t* cnt, CanonVerdict* verdict);  // cnt: canon_chunks(n) + 1
void launch_canon_fill(hipStream_t s, int64_t n, int64_t m, const unsigned char* keep, const uint32_t* col, const double* x, const int64_t* cnt,
                       const int64_t* rowptr, int base, unsigned short* rel, int64_t* rowptr_out, uint32_t* col_out, double* val_out);
void launch_canon_symmetry(hipStream_t s, int64_t nnz, int64_t m, int64_t n, const int64_t* rowptr, const uint32_t* col, const double* val,
                           CanonVerdict* verdict);
void launch_canon_export(hipStream_t s, int64_t m, int64_t nnz, const int64_t* rowptr, const uint32_t* col, int base, int64_t* rowptr_out,
                         int64_t* col_out);
// kernels_reduce_csr.hip: A * PMat from canonical CSR (reduce_csr.cpp)
void launch_labels_exceed(hipStream_t s, int64_t len, const uint32_t* L, int64_t d, uint32_t* flag);
void launch_csr_entry_labels(hipStream_t s, int64_t nnz, const uint32_t* col, const uint32_t* L, int64_t d, uint32_t* key);
size_t csr_class_sums_carry_bytes(int64_t nnz);
void launch_csr_class_sums(hipStream_t s, int64_t nnz, int64_t m, const int64_t* rowptr, const uint32_t* key_sorted,
                           const uint32_t* idx_sorted, const double* val, void* carry, double* out);
// kernels_blockop.hip: the reduced PSD pencil from triplets (blockop.cpp).  The verdict words of the creation passes, 64 bits
// each, all ones = nothing found: the lowest offending index of each kind, and the full entry count
enum { BOV_PTR0 = 0, BOV_MONOTONE = 1, BOV_PTREND = 2, BOV_BLOCK = 3, BOV_RANGE = 4, BOV_TRIANGLE = 5, BOV_TOTAL = 6, BOV_WORDS = 7 };
int64_t blockop_chunks(int64_t nnz);
void launch_blockop_check_classptr(hipStream_t s, int64_t d, int64_t nnz, const int64_t* classptr, unsigned long long* verdict);
void launch_blockop_check(hipStream_t s, int64_t nnz, const int32_t* blk, const int32_t* row, const int32_t* col, int base, int upper, int nb,
                          const uint32_t* pre, const int32_t* vs, unsigned long long* verdict, uint32_t* cnt, int64_t* off);  // cnt: chunks, off: chunks + 1
void launch_blockop_expand(hipStream_t s, int64_t nnz, int64_t d, const int64_t* classptr, const int32_t* blk, const int32_t* row,
                           const int32_t* col, const double* val, int base, int upper, int nb, const uint32_t* pre, const int32_t* vs,
                           const int64_t* off, void* rec, uint32_t* poskey);
void launch_blockop_gather(hipStream_t s, int64_t n, const uint32_t* sidx, const void* rec, void* out);
size_t blockop_carry_bytes(int64_t n);
void launch_blockop_keyed_sums(hipStream_t s, int64_t n, const void* rec, const double* v, int64_t nv, void* carry, double* out);
// blockop.cpp: the enqueue-only form of sdpsr_blockop_apply (adjoint = false: dv has d elements, dout sum s'_k^2) and
// sdpsr_blockop_adjoint (true: the other way round) on device arrays; carry: blockop_carry_bytes(op->nnz_full) of device scratch.
// Stream-ordered, no host wait; the public entries call it between their copies (sdp_solve.cpp: once each per iteration).
int blockop_map_enqueue(sdpsr_ctx* c, const sdpsr_blockop* op, bool adjoint, const double* dv, void* carry, double* dout);
// kernels_rowspace.hip / host_gram_jacobi.cpp: the row space of [newA | b] (rowspace.cpp, sdpsr_compress_constraints)
double rowspace_scale(double max_abs);
int rowspace_absmax_blocks(int64_t total);
size_t rowspace_gram_partial_doubles(int64_t m, int64_t ncols);
void rowspace_gram_shape(int64_t m, int64_t ncols, int* npairs, int* Z, int64_t* cps);
int rowspace_chunk(int64_t m, bool* j_lds);  // columns per workgroup of the rotation (j_lds given) resp. the write-out (nullptr)
void launch_rowspace_scale(hipStream_t s, int64_t total, int64_t md, const double* A, const double* b, double* pmax, uint32_t* flag,
                           double* W, double* info);
void launch_rowspace_gram(hipStream_t s, int64_t m, int64_t ncols, const double* W, double* P, double* G);
void launch_rowspace_rotate(hipStream_t s, int64_t m, int64_t ncols, const double* J, double* W);
void launch_rowspace_finish(hipStream_t s, int64_t m, int64_t ncols, int64_t r, const double* W, const int32_t* perm,
                            const double* sigma, double* sig, double droptol, double* out, unsigned long long* nnz);
int64_t host_gram_jacobi(int m, double* G, double* J, double tau, double floor2, int max_sweeps, int* sweeps_out, double* max_rel_out);
// complex.cpp, the complex path through the real embedding (the driver takes it for n > 64; any n >= 1 works).  cx_heev_general:
// eigenpairs of the Hermitian H (device planes, ld = n) into Vr, Vi (device) and vals (ascending, host); eigenvalues of the
// embedding within atol of each other are one cluster.  cx_block_norms_general: dnorms[sa * neig + sb] (device, zeroed by the
// caller) = max |(V^H H V)[a, b]| over space_of[a] == sa, space_of[b] == sb, as the bits of a double.
int cx_heev_general(sdpsr_ctx* c, int64_t n, const double* Hr, const double* Hi, double atol, double* Vr, double* Vi,
                    std::vector<double>& vals);
int cx_block_norms_general(sdpsr_ctx* c, int64_t n, const double* Hr, const double* Hi, const double* Vr, const double* Vi,
                           const int32_t* dspace, int neig, unsigned long long* dnorms);

}  // namespace sdpsr

#define CHECK_CTX(c) \
    if (!(c)) return SDPSR_BAD_ARGUMENT; \
    sdpsr::DeviceGuard _dg((c)->device); \
    (c)->err.clear();
