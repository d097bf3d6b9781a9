// blockDiagonalize (src/compat.jl:46-68): diagonalize + check_block_sizes (src/diagonalize.jl:1-40),
// then basis_image (:42-89).  Entry points sdpsr_block_diagonalize / _block_sizes / _q_hat / _block_images / sdpsr_basis_image.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_internal.h"

using namespace sdpsr;

namespace sdpsr {
// keep a device copy of the labels for phase 2 (or, in_place, the caller's device buffer itself)
// (narrow labels -- the public entry only; sdpsr_jordan_reduce hands over its own uint32 labels -- are widened into the ctx's copy)
static int keep_labels(sdpsr_ctx* c, int64_t n, const uint32_t* P, int mem, bool trusted_symmetric, bool in_place, bool labels_are_u32,
                       uint32_t*& L) {
    hipStream_t s = c->stream;
    const int64_t len = n * n;
    int st = SDPSR_OK;
    const bool narrow = !labels_are_u32 && c->label_width != 32;
    in_place = in_place && mem == SDPSR_MEM_DEVICE && !narrow;
    L = in_place ? const_cast<uint32_t*>(P) : (uint32_t*)ctx_buf(c, "bd_labels", len * 4);
    if (!L) return SDPSR_OUT_OF_MEMORY;
    c->bd_labels_ext = in_place ? P : nullptr;
    c->bd_sym_labels = nullptr;
    c->bd_sym_epoch = 0;
    c->bd_trusted_symmetric = (trusted_symmetric && mem == SDPSR_MEM_DEVICE && P == L) ? L : nullptr;
    if (narrow) {
        st = labels_fetch(c, L, P, (size_t)len, mem);
        if (st) return st;
    } else if (mem == SDPSR_MEM_DEVICE) {
        if (P != L) {
            // copy and symmetry check of the same tiles in one pass; the verdict ("bd_symflag"[0] ==
            // epoch <=> not symmetric) is read back by the driver with its first synchronisation
            const bool fresh = c->bufs.find("bd_symflag") == c->bufs.end();
            uint32_t* sf = (uint32_t*)ctx_buf(c, "bd_symflag", 64);
            if (!sf) return SDPSR_OUT_OF_MEMORY;
            if (fresh) HIP_TRY(c, hipMemsetAsync(sf, 0, 64, s));
            if (++c->epoch_counter == 0) ++c->epoch_counter;
            launch_copy_check_symmetric(s, n, P, L, sf, c->epoch_counter);
            c->bd_sym_epoch = c->epoch_counter;
            c->bd_sym_labels = L;
        }
    } else {
        HIP_TRY(c, hipMemcpyAsync(L, P, len * 4, hipMemcpyHostToDevice, s));
        c->h2d_bytes += (size_t)len * 4;
    }
    return SDPSR_OK;
}

// check_block_sizes (src/diagonalize.jl:1-11)
static int check_block_sizes(sdpsr_ctx* c, const std::vector<int32_t>& sizes, int64_t d) {
    int64_t final_dim = 0;
    for (int32_t sz : sizes) final_dim += (int64_t)sz * (sz + 1) / 2;
    if (final_dim == d) return SDPSR_OK;
    std::string szs;
    for (int32_t sz : sizes) szs += std::to_string(sz) + " ";
    return ctx_fail(c, SDPSR_DIMENSION_MISMATCH,
                    "final_dim=" + std::to_string(final_dim) + " block_sizes=[" + szs + "] expected dim(P)=" +
                        std::to_string(d) + " (rounding error: try another epsilon or try again; or the algebra is not block-diagonalizable over the reals)");
}

int block_diagonalize_impl(sdpsr_ctx* c, int64_t n, const uint32_t* P, int64_t d, double epsilon, int32_t* nblocks, int64_t* sum_sq,
                           int64_t* sum_s, double* phase_ms, int mem, bool trusted_symmetric, bool final_sync, bool in_place, bool labels_are_u32) {
    CHECK_CTX(c);
    if (!P || n < 1 || d < 0 || !(epsilon > 0)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const int64_t len = n * n;
    int st = check_len(c, len);
    if (st) return st;
    hipStream_t s = c->stream;
    c->bd_valid = false;
    c->bd_q_valid = false;
    c->bd_qrm_current = false;  // set again by the module lift, which stores the row-major copy itself
    PhaseTimer tm(c, phase_ms != nullptr);
    TotalEvents ev_total(phase_ms != nullptr, s);
    uint32_t* L = nullptr;
    st = keep_labels(c, n, P, mem, trusted_symmetric, in_place, labels_are_u32, L);
    if (st) return st;
    dbg_mark(c, "block_diagonalize: entered, labels copied");
    const double atol = epsilon;  // diagonalize(T, P; atol=epsilon), src/compat.jl:53
    EigInfo info;
    std::vector<int32_t> sizes;
    int64_t S1 = 0, S = 0;
    st = DRIVER_FALLBACK;
    if (compression_eligible(c, n, d)) st = compressed_diagonalize(c, n, L, d, atol, info, sizes, S1, S, tm);
    if (st == DRIVER_FALLBACK && c->opts.eig_driver == 6)
        return ctx_fail(c, SDPSR_SOLVER_ERROR, "requested driver not applicable to this partition (" + c->err + ")");
    if (st != SDPSR_OK && st != DRIVER_FALLBACK) return st;
    if (st == DRIVER_FALLBACK) {
        flush_deferred_tail(c);  // sdpsr_jordan_reduce: a pending deferred tail goes first, every host wait of the dense driver is for the stream
        st = dense_diagonalize(c, n, L, nullptr, atol, info, sizes, S1, S, tm, d);  // d: extra coupling elements on demand
        if (st) return st;
    }

    dbg_mark(c, "block_diagonalize: diagonalize done");
    c->bd_n = n;
    c->bd_d = d;
    c->bd_sizes = sizes;
    c->bd_sum_s = S1;
    c->bd_sum_sq = S;
    c->bd_q_valid = true;
    if (nblocks) *nblocks = (int32_t)sizes.size();
    if (sum_sq) *sum_sq = S;
    if (sum_s) *sum_s = S1;
    if (phase_ms) {
        const float ms = ev_total.stop(s);
        tm.collect();
        for (int i = 0; i < SDPSR_T_COUNT; ++i) phase_ms[i] = tm.acc[i];
        phase_ms[SDPSR_T_TOTAL] = ms;
    } else if (final_sync) {
        HIP_TRY(c, ctx_sync_stream(c, s));
    }
    st = check_block_sizes(c, sizes, d);
    if (st) return st;
    c->bd_valid = true;
    return SDPSR_OK;
}

// basis_image (src/diagonalize.jl:42-89) as routes over one state: two shortcuts that check themselves, then one of three
// kernels for the projection formula.  The state is built from explicit arguments -- the labels, Q_hat row-major, the block
// sizes, a window of classes, atol, the output -- so that sdpsr_block_images (the ctx's own Q_hat, the window (1, d)) and
// sdpsr_basis_image (a caller's Q_hat, any window) are two callers of the same routes.  Nothing below assumes anything about
// Q: the shortcuts' checks are exact about cross terms (kernels_blockdiag.hip), so a Q that is not invariant fails them.
struct BasisImage {
    enum Shortcut { FALL_THROUGH, DONE, DONE_SYNCED };  // DONE_SYNCED: the verdict's host wait was the last thing on the stream
    enum Route { TWO_STAGE, OUTER, CHUNK };
    sdpsr_ctx* c;
    hipStream_t s;
    int64_t n, d, S1, S, len;  // d: the number of classes of the window, i.e. of output slabs
    uint32_t first;            // the window's first class (1-based): labels are read as window_label(l, first, d)
    const uint32_t* L;
    const double* Qrm;
    double* out;  // the window's d * S doubles
    double atol;
    const std::vector<int32_t>& sizes;
    BlockLayout lay;
    bool own_labels = false;  // the ctx's own labels and the window (1, d): the shortcuts' class sums use the labels as they are
    int route_flags = 0;      // SDPSR_BI_ROUTE_*: what produced `out`
    // sources of asynchronous uploads (chunk)
    std::vector<int32_t> desc;
    std::vector<int64_t> chunk_ptr, cb, ce;

    BasisImage(sdpsr_ctx* ctx, int64_t n_, const uint32_t* labels, const double* Q_rowmajor, const std::vector<int32_t>& blk_sizes, int64_t sum_s,
               int64_t sum_sq, int64_t class_first, int64_t class_count, double atol_, double* out_)
        : c(ctx), s(ctx->stream), n(n_), d(class_count), S1(sum_s), S(sum_sq), len(n_ * n_), first((uint32_t)class_first), L(labels),
          Qrm(Q_rowmajor), out(out_), atol(atol_), sizes(blk_sizes), lay(block_layout(blk_sizes)) {}

    bool shortcuts_allowed() const { return c->opts.basis_image_kernel == 0 && !(c->opts.flags & SDPSR_FLAG_FULL_BASIS_IMAGE) && d >= 1 && n >= 64; }
    uint32_t* verdict_words(size_t count);
    int shortcut_commutative(Shortcut& r);
    int shortcut_blocks(Shortcut& r);
    Route route() const;
    int two_stage();
    int outer(const uint32_t* ent, const std::vector<int64_t>& class_ptr);
    int chunk(const uint32_t* ent, const std::vector<int64_t>& class_ptr);
    int run(bool& done_synced);
};

// per-column / per-block verdicts, stored by the check kernel straight into pinned host memory: its own words, behind
// (not inside) the fixed reports at the start of the buffer; [0] = number of failures, [1 + k] = failure of column / block k
uint32_t* BasisImage::verdict_words(size_t count) {
    uint32_t* hv = (uint32_t*)ctx_pinned(c, PINNED_BASIS_IMAGE_VERDICTS.first * 4 + (count + 1) * 4);
    return hv ? hv + PINNED_BASIS_IMAGE_VERDICTS.first : nullptr;
}

// commutative case (every block 1 x 1): the images are eigenvalues, lambda_ik = q_k'(1[P==i] x) for x = sum_k q_k
// -- one vector's class sums -- with a randomized self-check; the projection formula runs if the check
// fails (kernels_blockdiag.hip, launch_basis_image_commutative) and always under SDPSR_FLAG_FULL_BASIS_IMAGE
int BasisImage::shortcut_commutative(Shortcut& r) {
    r = FALL_THROUGH;
    if (S != S1 || !shortcuts_allowed()) return SDPSR_OK;
    double* ws = (double*)ctx_buf(c, "bi_comm_ws", basis_image_commutative_workspace_doubles(n, d) * 8);
    uint32_t* hv = verdict_words((size_t)S1);
    if (!ws || !hv) return SDPSR_OUT_OF_MEMORY;
    if (!launch_basis_image_commutative(s, n, d, first, S1, L, Qrm, next_key(c), atol, 2e-10, ws, out, hv, own_labels)) return SDPSR_OK;
    HIP_TRY(c, ctx_sync_stream(c, s));
    HIP_TRY(c, hipGetLastError());
    const uint32_t nbad = hv[0];
    if (nbad == 0) r = DONE_SYNCED;
    route_flags = nbad == 0 ? SDPSR_BI_ROUTE_COMMUTATIVE : SDPSR_BI_ROUTE_SHORTCUT_REFUSED;
    if (nbad == 0 || nbad > 8) {
        if (nbad && dbg_on()) fprintf(stderr, "[sdpsr] basis_image: invariance check failed for %u columns, projection formula instead\n", nbad);
        return SDPSR_OK;
    }
    // a few columns failed (the eigenvectors of a pair of close eigenvalues): the projection formula for
    // those columns only, two per extra class-sum pass
    std::vector<int> badk;
    for (int64_t k2 = 0; k2 < S1; ++k2)
        if (hv[1 + k2]) badk.push_back((int)k2);
    bool done = true;
    for (size_t q = 0; q < badk.size() && done; q += 2)
        done = launch_basis_image_fix_pair(s, n, d, first, S1, L, Qrm, badk[q], badk[q + 1 < badk.size() ? q + 1 : q], atol, ws, out, own_labels);
    if (dbg_on()) fprintf(stderr, "[sdpsr] basis_image: invariance check failed for %u column(s), projection formula for those\n", nbad);
    if (done) r = DONE, route_flags = SDPSR_BI_ROUTE_COMMUTATIVE | SDPSR_BI_ROUTE_REPAIRED;
    return SDPSR_OK;
}

// blocks up to 3 x 3 (non-commutative algebras with small blocks: ER(q) (x) K_k): the images from FOUR vectors' class
// sums with a per-block check (kernels_blockdiag.hip, launch_basis_image_blocks); blocks that fail get the projection
// formula, one block per extra pair of passes; many failures: the two-stage kernels for everything
int BasisImage::shortcut_blocks(Shortcut& r) {
    r = FALL_THROUGH;
    if (S == S1 || !shortcuts_allowed() || lay.nb > 4096 || lay.max_size > 3) return SDPSR_OK;
    const int nb = lay.nb;
    int32_t* d_cs = (int32_t*)ctx_buf(c, "bi_colsz", (size_t)2 * nb * 4);
    int64_t* d_off = (int64_t*)ctx_buf(c, "bi_off", (size_t)nb * 8);
    double* ws = (double*)ctx_buf(c, "bi_comm_ws", basis_image_blocks_workspace_doubles(n, d) * 8);
    uint32_t* hv = verdict_words((size_t)nb);
    if (!d_cs || !d_off || !ws || !hv) return SDPSR_OUT_OF_MEMORY;
    int st = h2d_sync(c, d_cs, lay.colsz.data(), (size_t)2 * nb * 4);
    if (!st) st = h2d_sync(c, d_off, lay.off.data(), (size_t)nb * 8);
    if (st) return st;
    if (!launch_basis_image_blocks(s, n, d, first, S1, S, nb, d_cs, d_cs + nb, d_off, L, Qrm, next_key(c), -1, atol, 2e-10, ws, out, hv, own_labels)) return SDPSR_OK;
    HIP_TRY(c, ctx_sync_stream(c, s));
    HIP_TRY(c, hipGetLastError());
    const uint32_t nbad = hv[0];
    route_flags = nbad == 0 ? SDPSR_BI_ROUTE_BLOCKS : SDPSR_BI_ROUTE_SHORTCUT_REFUSED;
    if (nbad == 0) {
        r = DONE_SYNCED;
        return SDPSR_OK;
    }
    bool done = nbad <= 4;
    for (int k2 = 0; k2 < nb && done; ++k2)
        if (hv[1 + k2]) done = launch_basis_image_blocks(s, n, d, first, S1, S, nb, d_cs, d_cs + nb, d_off, L, Qrm, 0, k2, atol, 2e-10, ws, out, nullptr, own_labels);
    if (dbg_on()) fprintf(stderr, "[sdpsr] basis_image: invariance check failed for %u block(s)%s\n", nbad, done ? ", projection formula for those" : ", two-stage kernels instead");
    if (done) r = DONE, route_flags = SDPSR_BI_ROUTE_BLOCKS | SDPSR_BI_ROUTE_REPAIRED;
    return SDPSR_OK;
}

// opts.basis_image_kernel = 1 two_stage | 2 outer | 3 chunk forces one of the three kernels (tests: the
// automatic choice reaches `outer` / `chunk` only for shapes far beyond the test sizes)
BasisImage::Route BasisImage::route() const {
    const int force = c->opts.basis_image_kernel;
    const bool f_outer = force == 2, f_chunk = force == 3;
    if (basis_image_two_stage_fits(n, d, S1) && !f_outer && !f_chunk) return TWO_STAGE;
    // many small classes (average class below 4096 entries) and blocks up to 256: outer-product
    // kernel, one workgroup per (class, block), every output written once, no partial sums
    if (lay.max_size <= 256 && d > 0 && (len / d < 4096 || f_outer) && !f_chunk && d <= 0x7FFFFFFF && lay.nb <= 65535) return OUTER;
    return CHUNK;
}

// two-stage form (class sums per row, then the s_k x s_k dots)
int BasisImage::two_stage() {
    desc = pair_descriptor(sizes, S);
    int32_t* d_desc = (int32_t*)ctx_buf(c, "bi_desc", (size_t)2 * S * 4);
    double* Tb = (double*)ctx_buf(c, "bi_T", (size_t)d * n * S1 * 8);
    if (!d_desc || !Tb) return SDPSR_OUT_OF_MEMORY;
    const int st = h2d_sync(c, d_desc, desc.data(), (size_t)2 * S * 4);
    if (st) return st;
    launch_basis_image_two_stage(s, n, d, first, S1, S, L, Qrm, Tb, d_desc, d_desc + S, atol, out);
    return SDPSR_OK;
}

int BasisImage::outer(const uint32_t* ent, const std::vector<int64_t>& class_ptr) {
    const int nb = lay.nb;
    int32_t* d_col = (int32_t*)ctx_buf(c, "bi_col", (size_t)nb * 4);
    int32_t* d_sz = (int32_t*)ctx_buf(c, "bi_sz", (size_t)nb * 4);
    int64_t* d_off = (int64_t*)ctx_buf(c, "bi_off", (size_t)nb * 8);
    int64_t* d_cls = (int64_t*)ctx_buf(c, "bi_cls_ptr", (size_t)(d + 2) * 8);
    if (!d_col || !d_sz || !d_off || !d_cls) return SDPSR_OUT_OF_MEMORY;
    int st = h2d_sync(c, d_col, lay.col(), (size_t)nb * 4);
    if (!st) st = h2d_sync(c, d_sz, lay.size(), (size_t)nb * 4);
    if (!st) st = h2d_sync(c, d_off, lay.off.data(), (size_t)nb * 8);
    if (!st) st = h2d_sync(c, d_cls, class_ptr.data(), (size_t)(d + 2) * 8);
    if (st) return st;
    launch_basis_image_outer(s, n, d, S1, S, nb, lay.max_size, Qrm, ent, d_cls, d_col, d_sz, d_off, atol, out);
    return SDPSR_OK;
}

// chunks of 4096 entries of a class + output descriptors; the uploads are asynchronous, from vectors of the state
int BasisImage::chunk(const uint32_t* ent, const std::vector<int64_t>& class_ptr) {
    cut_chunks(class_ptr, d, 4096, chunk_ptr, cb, ce);
    desc = pair_descriptor(sizes, S);
    const int64_t nch = (int64_t)cb.size();
    int64_t* d_chunk_ptr = (int64_t*)ctx_buf(c, "bi_chunk_ptr", (d + 1) * 8);
    int64_t* d_cb = (int64_t*)ctx_buf(c, "bi_cb", std::max<int64_t>(nch, 1) * 8);
    int64_t* d_ce = (int64_t*)ctx_buf(c, "bi_ce", std::max<int64_t>(nch, 1) * 8);
    int32_t* d_dA = (int32_t*)ctx_buf(c, "bi_da", std::max<int64_t>(S, 1) * 4);
    int32_t* d_dB = (int32_t*)ctx_buf(c, "bi_db", std::max<int64_t>(S, 1) * 4);
    double* partial = (double*)ctx_buf(c, "bi_partial", (size_t)std::max<int64_t>(nch * S, 1) * 8);
    if (!d_chunk_ptr || !d_cb || !d_ce || !d_dA || !d_dB || !partial) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(d_chunk_ptr, chunk_ptr.data(), (d + 1) * 8, hipMemcpyHostToDevice, s));
    if (nch) {
        HIP_TRY(c, hipMemcpyAsync(d_cb, cb.data(), nch * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(d_ce, ce.data(), nch * 8, hipMemcpyHostToDevice, s));
    }
    if (S) {
        HIP_TRY(c, hipMemcpyAsync(d_dA, desc.data(), S * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(d_dB, desc.data() + S, S * 4, hipMemcpyHostToDevice, s));
    }
    launch_basis_image(s, n, d, S1, S, Qrm, ent, nullptr, d_dA, d_dB, d_chunk_ptr, nch, nullptr, d_cb, d_ce,
                       partial, out, atol);
    return SDPSR_OK;
}

int BasisImage::run(bool& done_synced) {
    Shortcut r;
    int st = shortcut_commutative(r);
    if (!st && r == FALL_THROUGH) st = shortcut_blocks(r);
    done_synced = !st && r == DONE_SYNCED;
    if (st || r != FALL_THROUGH) return st;  // (out is complete)
    const Route kind = route();
    route_flags = (route_flags & SDPSR_BI_ROUTE_SHORTCUT_REFUSED) | (kind == TWO_STAGE ? SDPSR_BI_ROUTE_TWO_STAGE : kind == OUTER ? SDPSR_BI_ROUTE_OUTER : SDPSR_BI_ROUTE_CHUNK);
    if (kind == TWO_STAGE) return two_stage();
    // _constraints(P): entries grouped by class (src/diagonalize.jl:42-50); the keys are window-relative
    uint32_t* ent = nullptr;
    std::vector<int64_t> class_ptr;  // size d+2: class_ptr[l]..class_ptr[l+1] = class first + l - 1 (l = 0: everything outside the window)
    st = sort_entries_by_label(c, len, d, L, &ent, class_ptr, first);
    if (st) return st;
    return kind == OUTER ? outer(ent, class_ptr) : chunk(ent, class_ptr);
}
}  // namespace sdpsr

extern "C" {

int sdpsr_block_diagonalize(sdpsr_ctx* c, int64_t n, const uint32_t* P, int64_t d, double epsilon,
                            int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* phase_ms,
                            int mem) {
    return block_diagonalize_impl(c, n, P, d, epsilon, nblocks, sum_sq, sum_s, phase_ms, mem, false, true, false, /*labels_are_u32=*/false);
}

int sdpsr_block_sizes(sdpsr_ctx* c, int32_t* blk_sizes) {
    if (!c || !blk_sizes) return SDPSR_BAD_ARGUMENT;
    if (c->bd_sizes.empty()) return ctx_fail(c, SDPSR_BAD_STATE, "no block diagonalisation available");
    memcpy(blk_sizes, c->bd_sizes.data(), c->bd_sizes.size() * sizeof(int32_t));
    return SDPSR_OK;
}

int sdpsr_q_hat(sdpsr_ctx* c, double* Q_hat, int mem) {
    CHECK_CTX(c);
    if (!c->bd_q_valid) return ctx_fail(c, SDPSR_BAD_STATE, "no diagonalisation available on this ctx");
    if (!Q_hat) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    const size_t cnt = (size_t)c->bd_n * c->bd_sum_s;
    double* Qhat = (double*)ctx_buf(c, "bd_qhat", cnt * 8);
    if (!Qhat) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemcpyAsync(Q_hat, Qhat, cnt * 8, mem == SDPSR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    return SDPSR_OK;
}

int sdpsr_block_images(sdpsr_ctx* c, double* blks, double* Q_hat, double* phase_ms, int mem) {
    CHECK_CTX(c);
    if (!c->bd_valid) return ctx_fail(c, SDPSR_BAD_STATE, "sdpsr_block_diagonalize has not succeeded on this ctx");
    if (!blks) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    hipStream_t s = c->stream;
    TotalEvents ev_total(phase_ms != nullptr, s);
    const int64_t n = c->bd_n, d = c->bd_d, S1 = c->bd_sum_s, S = c->bd_sum_sq;
    int st = SDPSR_OK;
    const uint32_t* L = c->bd_labels_ext ? c->bd_labels_ext : (const uint32_t*)ctx_buf(c, "bd_labels", (size_t)n * n * 4);
    double* Qhat = (double*)ctx_buf(c, "bd_qhat", (size_t)n * S1 * 8);
    double* Qrm = (double*)ctx_buf(c, "bd_qrm", (size_t)n * S1 * 8);
    double* out = out_dev(c, "bd_blks", blks, (size_t)d * S, mem, &st);
    if (st || !L || !Qhat || !Qrm) return st ? st : SDPSR_OUT_OF_MEMORY;
    // the ctx's own state, every class, basis_image's default atol (src/diagonalize.jl:67); lives until the one host wait
    // below: its host vectors are the sources of asynchronous uploads
    BasisImage bi(c, n, L, Qrm, c->bd_sizes, S1, S, 1, d, 1e-12 * (double)n, out);
    bi.own_labels = true;
    if (!c->bd_qrm_current) launch_transpose_to_rowmajor(s, n, S1, Qhat, Qrm);  // (the module lift has written Qrm beside Q_hat)
    bool done_synced = false;  // the stream was synchronised by a shortcut's verdict and nothing was enqueued since
    st = bi.run(done_synced);
    if (st) return st;
    HIP_TRY(c, hipGetLastError());
    // ONE host wait for everything (the images, Q_hat, and the host vectors of `bi`, which must outlive their copies): the
    // copies are enqueued first.  (Three waits before: the second and third found an idle stream, ~3 us each.)
    if (mem != SDPSR_MEM_DEVICE) {
        HIP_TRY(c, hipMemcpyAsync(blks, bi.out, (size_t)d * S * 8, hipMemcpyDeviceToHost, s));
        c->d2h_bytes += (size_t)d * S * 8;
    }
    if (Q_hat) {
        HIP_TRY(c, hipMemcpyAsync(Q_hat, Qhat, (size_t)n * S1 * 8, mem == SDPSR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        if (mem != SDPSR_MEM_DEVICE) c->d2h_bytes += (size_t)n * S1 * 8;
    }
    if (!(done_synced && mem == SDPSR_MEM_DEVICE && !Q_hat)) HIP_TRY(c, ctx_sync_stream(c, s));
    if (phase_ms) {
        const float ms = ev_total.stop(s);
        for (int i = 0; i < SDPSR_T_COUNT; ++i) phase_ms[i] = 0;
        phase_ms[SDPSR_T_IMAGE] = ms;
        phase_ms[SDPSR_T_TOTAL] = ms;
    }
    return SDPSR_OK;
}

// basis_image(Q, P; atol) (src/diagonalize.jl:64-89) of a caller's Q_hat for a window of classes.  Buffers of its own for the
// labels ("bie_labels"), Q_hat and its row-major copy: the ctx's block diagonalisation is not touched.
int sdpsr_basis_image(sdpsr_ctx* c, int64_t n, const uint32_t* P, int64_t d, int32_t nblocks, const int32_t* blk_sizes, const double* Q_hat,
                      int64_t class_first, int64_t class_count, double atol, double* blks, int32_t* route, double* phase_ms, int mem) {
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
    const size_t out_count = (size_t)class_count * S;
    const uint64_t h2d0 = c->h2d_bytes, d2h0 = c->d2h_bytes;
    TotalEvents ev_total(phase_ms != nullptr, s);
    uint32_t* L = (uint32_t*)ctx_buf(c, "bie_labels", (size_t)len * 4);
    uint32_t* flag = (uint32_t*)ctx_buf(c, "bie_flag", 64);
    double* Qrm = (double*)ctx_buf(c, "bie_qrm", (size_t)n * S1 * 8);
    if (!L || !flag || !Qrm) return SDPSR_OUT_OF_MEMORY;
    const double* Qcm = in_dev(c, "bie_qhat", Q_hat, (size_t)n * S1, mem, &st);
    double* out = out_dev(c, "bie_blks", blks, out_count, mem, &st);
    if (st || !Qcm || !out) return st ? st : SDPSR_OUT_OF_MEMORY;
    // the labels come in and are judged in the same pass: symmetry (the routes read one triangle) and "a label exceeds d"
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
    launch_transpose_to_rowmajor(s, n, S1, Qcm, Qrm);
    const std::vector<int32_t> sizes(blk_sizes, blk_sizes + nblocks);
    BasisImage bi(c, n, L, Qrm, sizes, S1, S, class_first, class_count, atol < 0 ? 1e-12 * (double)n : atol, out);  // lives until the last host wait
    bool done_synced = false;
    st = bi.run(done_synced);
    if (st) return st;
    HIP_TRY(c, hipGetLastError());
    if (!done_synced) HIP_TRY(c, ctx_sync_stream(c, s));
    // what this entry moved: the arrays and the verdicts (the routes' descriptor words are not part of its account)
    c->h2d_bytes = h2d0 + (mem != SDPSR_MEM_DEVICE ? (uint64_t)len * (c->label_width / 8) + (uint64_t)n * S1 * 8 : 0);
    c->d2h_bytes = d2h0 + (mem != SDPSR_MEM_DEVICE ? 0 : 8);
    if (verdict[0]) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "basis_image: partition is not symmetric");
    if (verdict[1]) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "basis_image: a label exceeds d = dim(P)");
    if (mem != SDPSR_MEM_DEVICE) {
        HIP_TRY(c, hipMemcpyAsync(blks, out, out_count * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, ctx_sync_stream(c, s));
        c->d2h_bytes += out_count * 8;
    }
    if (route) *route = bi.route_flags;
    if (phase_ms) {
        const float ms = ev_total.stop(s);
        for (int i = 0; i < SDPSR_T_COUNT; ++i) phase_ms[i] = 0;
        phase_ms[SDPSR_T_IMAGE] = ms;
        phase_ms[SDPSR_T_TOTAL] = ms;
    }
    return SDPSR_OK;
}

}  // extern "C"
