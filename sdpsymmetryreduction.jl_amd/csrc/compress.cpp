// Module-compression driver of diagonalize (src/diagonalize.jl:25-40 on the restriction of the
// partition algebra to a cyclic module): see the block comment below and DESIGN.md.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>

#include "host_internal.h"
#include "module_select.h"

using namespace sdpsr;

namespace {

// device buffers of the speculative second element (Module::growth_round); have_t: T = A2 W was formed with the round's own product
struct Rider { double *dBs, *gps; bool have_t; };

// ===========================================================================
// Module-compression driver of diagonalize (DESIGN.md "module compression").
//
// For a random x the cyclic module M = <S> x (S = the partition subspace, <S> the associative
// algebra it generates) is invariant under every element of S and contains every irreducible
// constituent of the action with multiplicity min(s_k, m_k) >= 1, so Murota's algorithm run on
// the restriction S|_M (dimension w = sum_k s_k min(s_k, m_k) <= sum_k s_k^2 < 2 dim(P))
// finds the same blocks, and Q_hat = W * Q_hat_small (W an orthonormal basis of M) is a valid
// Q_hat of the full problem.  M is grown one vector at a time: y = A z for a fresh generic
// element A and a random z in the current span; y is appended if it leaves the span (CGS2);
// three consecutive misses end the growth.  Only first powers of well-scaled matrices are
// involved, so the rank decisions are sharp (eps vs O(1)).
// Cost: w passes over an n x n element + a dense w x w diagonalisation, against 4/3 n^3.
//
// Block growth.  The candidates of a round (class sums of x, then A_g W for G fresh generic
// elements) are written right behind the basis, Y = W[:, w : w+m), so that ONE split-K MFMA
// product [W Y]' Y delivers both C = W'Y and the Gram matrix Y'Y.  On the host the Gram matrix
// of the projected candidates is G - C'C (its cancellation error ~eps |Y|^2 sits four orders
// below the rank threshold), a pivoted Cholesky factorisation picks the new directions
// (rank gap: O(1) against eps^2, sharp because every candidate is a first power of a
// well-scaled matrix) and Q1 = [W Y] [-C X; X] forms them in one pass (module_select.h).  A second
// product [W Q1]' Q1 with the same structure re-orthonormalises (CholQR2).  A round that adds nothing
// (the module is complete) therefore costs one product.
// ===========================================================================
struct Module {
    sdpsr_ctx* c;
    int64_t n, ld, d;
    const uint32_t* L;
    int wmax;
    int64_t wcap, ycap, wtot;  // basis | candidates of one round | + padding of the last tile
    double *W = nullptr, *T = nullptr, *zy = nullptr, *dout = nullptr, *Cc = nullptr, *dSm = nullptr, *Q1 = nullptr;
    int w = 1;
    std::vector<double> hG;             // host copy of the last product [W V]'V ...
    int64_t saved_ld = 0;               // ... its leading dimension once the module is complete
    bool first_product_intact = false;  // Cc still holds the round's [W Y]'Y (no second product ran)
    bool have_saved = false;            // the top block of that product serves as the first compressed element
    bool spec_b2 = false;               // the second compressed element was formed behind the final round's product
    bool sym_pre = false, sym_trusted = false, sym_checked = false;  // the symmetric check's verdict: who made it, whether it was looked at
    bool forked = false;                // device tail: the fork point of the next prefetch is marked
    int window = 0;                     // which of the two host windows the step at hand opens (sdpsr_internal.h: 0 class sums, 1 growth rounds)
    // Scratch discipline (DESIGN.md "module scratch").  lean: the growth is on the small-module route -- small_on_host(), every
    // product the fused label product, the skinny Gram kernel or the row-owning tall product -- whose kernels read exact shapes:
    // only the padding rows n .. ld-1 of W are kept zero (seed_basis), nothing is filled per round and Q1 is not used.  The first
    // step that needs more (a padded split-K product, the device tail) calls restore_fills(), which brings W and Q1 to what the
    // whole-buffer fills would have left, and the growth goes on with those fills.  live: candidate columns behind the basis
    // that hold data of the round at hand.
    bool lean = false;
    int live = 0;
    bool parent_form() const { return (c->opts.flags & SDPSR_FLAG_MODULE_SCRATCH_FILLS) != 0; }
    int restore_fills();

    bool fused_product(int wcols) const { return wcols <= 64 && d <= 4000; }
    // small modules: Murota's steps on the host (small_eigen_host.cpp)
    bool small_on_host() const { return w <= 64 && !(c->opts.flags & SDPSR_FLAG_SMALL_EIGEN_ON_DEVICE) && (c->opts.eig_driver == 0 || c->opts.eig_driver >= 4); }
    // where the speculative B2 of a G = 1 round sits in the pinned buffer: behind that round's Gram matrix
    size_t spec_b2_offset() const { return ((size_t)round_up(2 * w, 128) * (size_t)round_up(w, 128) * 8 + 255) & ~size_t(255); }
    double* spec_b2_pinned() const { return (double*)((char*)c->pinned + spec_b2_offset()); }

    int setup();
    int seed_basis();
    int apply_generic(int wcols, double* dst);
    int ortho_step(int mc, double tol, bool take_ref, const Rider* rider, Selection& sel);
    int apply_stacked(int mc, const Selection& sel);
    int absorb(int m, const Rider* rider, int& got);
    int class_sum_round();
    int growth_round(int& got);
    int grow(PhaseTimer& tm);
    int small_host_tail(PhaseTimer& tm, double atol, std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, std::vector<double>& Qs);
    int make_element(double* dst);
    int prefetch_element(double* dst);
    int device_tail(PhaseTimer& tm, double atol, EigInfo& info, std::vector<int32_t>& sizes, int64_t& S1, int64_t& S);
    int lift(PhaseTimer& tm, const double* Qs_host, int64_t S1, double atol);
};

// buffers and the enqueue of the symmetric check
int Module::setup() {
    uint32_t* flag = (uint32_t*)ctx_buf(c, "bd_flag", 64);
    W = (double*)ctx_buf(c, "cm_w", (size_t)ld * wtot * 8);
    T = (double*)ctx_buf(c, "cm_t", (size_t)ld * wcap * 8);
    zy = (double*)ctx_buf(c, "cm_zy", (size_t)ld * 2 * 8);
    dout = (double*)ctx_buf(c, "cm_out", 64);
    if (!flag || !W || !T || !zy || !dout) return SDPSR_OUT_OF_MEMORY;
    // symmetric check: the verdict is copied back without a synchronisation of its own and is
    // looked at after the first read-back of the module growth (the kernels in between are
    // memory-safe for any labels, their results are simply discarded)
    if (!c->pinned_small) return SDPSR_OUT_OF_MEMORY;
    sym_pre = c->bd_sym_epoch != 0 && c->bd_sym_labels == L;  // checked by the copy pass of blockDiagonalize
    sym_trusted = c->bd_trusted_symmetric == L;               // labels of the library's own symmetric loop
    c->pinned_small[0] = 0;
    if (!sym_trusted) {
        if (!sym_pre) launch_check_symmetric(c->stream, n, L, flag);
        HIP_TRY(c, hipMemcpyAsync(c->pinned_small, sym_pre ? (const uint32_t*)ctx_buf(c, "bd_symflag", 64) : flag, 4,
                                  hipMemcpyDeviceToHost, c->stream));
    }
    sym_checked = sym_trusted;
    dbg_mark(c, "compressed: buffers + symmetric check done");
    return SDPSR_OK;
}

// leaving the lean route: everything but the basis and the live candidates zero, as the whole-buffer fills leave it
// (rows >= n of every column are zero already)
int Module::restore_fills() {
    if (!lean) return SDPSR_OK;
    lean = false;
    HIP_TRY(c, hipMemsetAsync(W + (size_t)(w + live) * ld, 0, (size_t)ld * (wtot - w - live) * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(Q1, 0, (size_t)ld * ycap * 8, c->stream));
    return SDPSR_OK;
}

// W = [x / |x|, 0, ...] for a random x, and the buffers of the growth
int Module::seed_basis() {
    lean = !parent_form() && small_on_host();  // (w == 1: what can still end it is the module's growth past 64 or a shape the exact-shape kernels refuse)
    if (lean) launch_pad_rows(c->stream, n, ld, wtot, W);  // nothing at all when ld == n
    else HIP_TRY(c, hipMemsetAsync(W, 0, (size_t)ld * wtot * 8, c->stream));
    if (parent_form()) {
        launch_random_vector(c->stream, n, next_key(c), zy);
        launch_normalize_columns(c->stream, n, ld, W, 0, zy, ld, 1, dout);  // W[:,0] = x / |x|
    } else {
        launch_seed_vector(c->stream, n, next_key(c), zy, W, dout);  // the same two steps in one launch
    }
    Cc = (double*)ctx_buf(c, "cm_c", (size_t)(wcap + ycap + 128) * ycap * 8);
    dSm = (double*)ctx_buf(c, "cm_sm", (size_t)(wcap + ycap) * ycap * 8);
    Q1 = (double*)ctx_buf(c, "cm_q1", (size_t)ld * ycap * 8);
    if (!Cc || !dSm || !Q1) return SDPSR_OUT_OF_MEMORY;
    if (!lean) HIP_TRY(c, hipMemsetAsync(Q1, 0, (size_t)ld * ycap * 8, c->stream));  // rows >= n stay zero for good
    return SDPSR_OK;
}

// Y <- A W for a fresh generic element A: fused label product when the shape allows it,
// gather + split-K MFMA GEMM otherwise.  Columns >= wcols of dst keep their old content.
int Module::apply_generic(int wcols, double* dst) {
    deferred_window_close(c);
    const uint64_t key = next_key(c);
    if (fused_product(wcols)) {
        double* part = (double*)ctx_buf(c, "cm_part", label_spmm_pair_partial_doubles(n) * 8);
        if (!part) return SDPSR_OUT_OF_MEMORY;
        if (launch_label_spmm(c->stream, n, L, key, d, W, ld, wcols, part, dst, ld)) return SDPSR_OK;
    }
    { int e0 = restore_fills(); if (e0) return e0; }  // the padded product: not the lean route
    double* Afull = (double*)ctx_buf(c, "cm_a", (size_t)ld * ld * 8);
    const int64_t wcp = round_up(wcols, 128);
    double* tmpo = (double*)ctx_buf(c, "cm_tmpo", (size_t)ld * wcp * 8);
    if (!Afull || !tmpo) return SDPSR_OUT_OF_MEMORY;
    launch_gather_f64_padded(c->stream, n, ld, L, key, Afull);
    int e3 = gemm_tn_splitk(c, ld, wcp, ld, Afull, ld, W, ld, tmpo, ld);
    if (e3) return e3;
    HIP_TRY(c, hipMemcpyAsync(dst, tmpo, (size_t)ld * wcols * 8, hipMemcpyDeviceToDevice, c->stream));
    return SDPSR_OK;
}

// One orthonormalisation step on the mc columns behind the basis, V = W[:, w : w+mc): product [W V]' V, then the
// selection on the host (sel.rank new directions, V_new = [W V] sel.coef).  rider: the speculative B2 = W'A2 W is
// enqueued between the product and its host wait and comes back with that wait.
int Module::ortho_step(int mc, double tol, bool take_ref, const Rider* rider, Selection& sel) {
    const int64_t ap = round_up(w + mc, 128), mp = round_up(mc, 128);
    deferred_window_close(c);
    // the exact-shape Gram kernel stores the product into pinned host memory as well: no copy launch before the read-back
    double* hpin = (double*)ctx_pinned(c, (size_t)ap * mp * 8);
    bool host_filled = false;
    // sdpsr_jordan_reduce, the loop's deferred tail pending (sdpsr_internal.h): the first step of a round whose product comes back in
    // pinned memory takes ONE segment along -- a stamp behind the product (and the rider), the segment behind the stamp, and the host
    // waits for the stamp: the segment's square and verify pass run while the host selects the directions (class sums) or solves the
    // compressed problem (invariance round); what the host enqueues next follows them in stream order.  The segments' buffers belong to
    // the loop (flush_deferred_tail names them); the growth works on "cm_*", "gram_partials", the labels and the pinned buffers only and
    // runs no refinement, so "ref_first" stays what the verify passes expect.  Any other step waits for the stream, or may request
    // buffers: everything pending is enqueued before its product.  (ctx_buf itself enqueues what is pending before it frees ANY buffer, the
    // growth's own "cm_*" / "gram_partials" included: on a ctx whose buffers still grow a segment that would have ridden is then
    // counted as enqueued outside a ride -- the first reductions of an order, never the steady state.)
    const bool ride = take_ref && hpin && deferred_tail_pending(c) && small_on_host() && gram_tn_is_skinny(w + mc, mc);
    // (Trade-off, off the benchmark's path: a step that does not ride -- the second orthogonalisation step of a non-commutative round --
    // puts the pending segment in front of its product, so its stream wait is ~100 us longer than the product alone; and an upload behind
    // a ride that finds the upload ring wrapped (h2d_sync) waits for the stream behind the segment.  Both cost what the segment would have
    // cost in the loop, never more, and keep the rule that a segment is always enqueued before anything that could disturb it.)
    if (!ride) flush_deferred_tail(c);
    if (lean && !gram_tn_is_skinny(w + mc, mc)) {  // the padded split-K product reads whole 128-column tiles
        const int e0 = restore_fills();
        if (e0) return e0;
    }
    int st = hpin ? gram_tn(c, w + mc, mc, ld, W, ld, W + (size_t)w * ld, ld, Cc, ap, mp, hpin, &host_filled) : SDPSR_OUT_OF_MEMORY;
    if (st) return st;
    if (rider && (rider->have_t || apply_generic(w, T) == SDPSR_OK)) {  // T[:, 0:w) = A2 W
        launch_gram_small(c->stream, n, w, w, W, ld, T, ld, rider->gps, rider->dBs, w, w, w, spec_b2_pinned());
        spec_b2 = true;
    }
    hG.resize((size_t)ap * mp);
    if (host_filled && ride) {
        uint32_t* stamp = c->pinned_small + PINNED_SMALL_GRAM_STAMP.first;
        const uint32_t seq = ++c->report_seq ? c->report_seq : ++c->report_seq;
        *(volatile uint32_t*)stamp = 0;
        launch_report_stamp(c->stream, stamp, seq);  // (a kernel of its own: a ticket inside gram_reduce_kernel, last workgroup stamps, measured 3 % slower, profiles/r15)
        flush_deferred_tail(c, 1, /*in_ride=*/true);
        if (ctx_wait_word(c, c->stream, stamp, seq) != hipSuccess) return ctx_fail(c, SDPSR_HIP_ERROR, "report wait (module growth)");
        deferred_window_open(c, window);
        memcpy(hG.data(), hpin, (size_t)ap * mc * 8);
    } else if (host_filled) {
        if (ctx_sync_stream(c, c->stream) != hipSuccess) return ctx_fail(c, SDPSR_HIP_ERROR, "hipStreamSynchronize (module growth)");
        if (take_ref) deferred_window_open(c, window);  // (the step a segment would ride with: the window is measured either way)
        memcpy(hG.data(), hpin, (size_t)ap * mc * 8);
    } else {
        st = d2h_sync(c, hG.data(), Cc, (size_t)ap * mc * 8);  // the mc columns the host looks at
        if (st) return st;
    }
    if (!sym_checked) {  // the product is in (stream or stamp), and the verdict of the symmetric check was copied before it in the stream
        sym_checked = true;
        if (sym_pre ? c->pinned_small[0] == c->bd_sym_epoch : c->pinned_small[0] != 0)
            return ctx_fail(c, SDPSR_INVALID_DECOMPOSITION_FIELD,
                            "partition is not symmetric: decomposition over Float64 requested but the generic element has a complex spectrum");
    }
    // The cancellation error of G - C'C and the projection error are both ~eps |candidate|^2 of the
    // round at hand: class sums have |.|^2 ~ class valency, growth candidates A_g W up to ~n^2/4.
    sel = select_directions(hG.data(), ap, w, mc, tol, take_ref);
    return SDPSR_OK;
}

// V_new = [W V] S written straight behind the basis: the row-owning product reads its 64 rows of [W V] before it stores any
// (the old V is dead by then).  More than 64 new columns, or SDPSR_FLAG_MODULE_SCRATCH_FILLS: into Q1, then copied back.
int Module::apply_stacked(int mc, const Selection& sel) {
    int e2 = h2d_sync(c, dSm, sel.coef.data(), (size_t)(w + mc) * sel.rank * 8);
    if (e2) return e2;
    double* V = W + (size_t)w * ld;
    const bool in_place = !parent_form() && launch_tall_times_small_rows(c->stream, n, ld, W, w + mc, dSm, w + mc, sel.rank, 1.0, 0.0, V, ld);
    if (!in_place) {
        live = mc;  // the old V is still read by the product
        e2 = restore_fills();  // Q1's padding rows travel with the copy
        if (e2) return e2;
        launch_tall_times_small(c->stream, n, ld, W, w + mc, dSm, w + mc, sel.rank, 1.0, 0.0, Q1, ld);
        HIP_TRY(c, hipMemcpyAsync(V, Q1, (size_t)ld * sel.rank * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    live = sel.rank;
    return SDPSR_OK;
}

// absorb m candidate columns W[:, w : w+m) into the basis; got = the number of new basis vectors (0 = nothing left the span)
int Module::absorb(int m, const Rider* rider, int& got) {
    got = 0;
    Selection s1, s2;
    // threshold 1e-10 |Y|^2: the projected Gram matrix comes from the cancellation G - C'C,
    // whose error is ~ w sqrt(n) eps |Y|^2 (~1e-13 at n = 4096: with 1e-12 about one
    // invariance round in ten let noise-level candidates through to the second step); a
    // genuine new direction of a generic element has an O(1) relative component
    int st = ortho_step(m, 1e-10, true, rider, s1);
    if (st) return st;
    if (dbg_on() && s1.rank > 0) fprintf(stderr, "[sdpsr] absorb(%d): rank %d, pivots %.3e .. %.3e (ratio %.1e)\n", m, s1.rank, s1.piv_max, s1.piv_min, s1.piv_max / s1.piv_min);
    first_product_intact = (s1.rank == 0);
    if (s1.rank == 0) return SDPSR_OK;
    if (w + s1.rank >= wmax) return driver_fallback(c, "module dimension exceeds " + std::to_string(wmax));
    st = apply_stacked(m, s1);
    if (st) return st;
    // One Cholesky-based step leaves an orthogonality error of ~eps * cond(projected Gram) (and
    // the projection against W one of ~eps * |candidate|^2 / smallest pivot): with both ratios
    // below 1e3 that is < 1e-12 and the second step (another product, another host round trip,
    // ~80 us at N = 4096) adds nothing.  Measured ratios: 2e2-5e2 for the class sums of a
    // commutative scheme, 1e4-1e5 for the non-commutative growth rounds (those keep the second step).
    const double worst = std::max(s1.piv_max, s1.ref) / s1.piv_min;
    got = s1.rank;
    if (!(worst <= 1e3) || (c->opts.flags & SDPSR_FLAG_ALWAYS_REORTHOGONALIZE)) {
        st = ortho_step(s1.rank, 1e-6, false, nullptr, s2);  // Q1 columns have unit scale
        got = s2.rank;
        if (st || got == 0) return st;
        st = apply_stacked(s1.rank, s2);
        if (st) return st;
    }
    w += got;
    live = 0;
    return SDPSR_OK;
}

// level 1: S x = span{P_i x}: all d class sums of x in ONE pass over the labels (the
// row-sum kernel of basis_image with a single column).  For a commutative algebra this
// already is the whole module.
int Module::class_sum_round() {
    if (!(class_sums_supports(n, d, ld) && basis_image_two_stage_fits(n, d, 1) && d <= ycap && d + 1 < wmax)) {
        flush_deferred_tail(c);  // no class-sum round: not the route with a host wait per segment (ortho_step)
        return SDPSR_OK;
    }
    launch_class_sums(c->stream, n, d, L, W, W + (size_t)w * ld, ld);  // W[:, w + i] = P_{i+1} x
    window = 0;
    int got;
    live = (int)d;
    return absorb((int)d, nullptr, got);
}

// One growth round: candidates W[:, w + g*w + (0:w)] = A_g W for G fresh generic elements A_g (rows >= n zero)
int Module::growth_round(int& got) {
    const bool fused = fused_product(w);
    int G = (fused && w <= 16) ? 4 : 2;  // generic elements per round
    while (G > 2 && (int64_t)G * w > ycap) --G;
    // dim <S> x <= dim S = d: once w has reached d the round is (almost surely) only the
    // invariance check, for which ONE generic element suffices (the elements that map the
    // module into itself form a subspace of S; it contains a generic point iff it is S)
    if ((int64_t)G * w > ycap || w >= d) G = 1;
    const int m = G * w;
    double* Y = W + (size_t)w * ld;
    live = 0;
    window = 1;
    deferred_window_close(c);
    if (lean && !(fused && small_on_host())) {  // the module has outgrown the small-module route
        const int e0 = restore_fills();
        if (e0) return e0;
    }
    // lean: the label products write rows < n of exactly the m columns the round's Gram product reads; rows >= n are zero
    if (!lean) HIP_TRY(c, hipMemsetAsync(Y, 0, (size_t)ld * round_up(m, 128) * 8, c->stream));
    bool batched = false;
    if (fused && G > 1 && G != 3 && G * w <= 64 && !(c->opts.flags & SDPSR_FLAG_SPMM_ONE_BY_ONE)) {
        // the G generic elements of the round in one pass over the labels
        double* part = (double*)ctx_buf(c, "cm_part", label_spmm_pair_partial_doubles(n) * 8);
        if (!part) return SDPSR_OUT_OF_MEMORY;
        uint64_t keys[4];
        const uint64_t save = c->stream_counter;
        for (int gidx = 0; gidx < G; ++gidx) keys[gidx] = next_key(c);
        batched = launch_label_spmm_multi(c->stream, n, L, keys, G, d, W, ld, w, part, Y, ld);
        if (!batched) c->stream_counter = save;
    }
    // A round with ONE element is the invariance check of a module that is (almost surely) complete, and the host path of
    // the small problem will then want the second compressed element B2 = W'A2 W right away: it is formed behind this
    // round's product and comes back with the same host wait (its pinned words sit behind the round's Gram matrix).
    // If the round does add a direction, the element is dropped.
    // A2 W has the same W, the same labels and another key: where the fused product takes the shape, both products are ONE pass
    // over the labels (launch_label_spmm_pair: Y = A1 W behind the basis, T = A2 W, each bit for bit what a launch of its own
    // gives), and the rider's part of ortho_step is the Gram product on T alone.  The keys are drawn in the order of the two
    // launches (nothing draws between them).  SDPSR_FLAG_SPMM_ONE_BY_ONE keeps the two launches.
    spec_b2 = false;
    Rider rider{};
    bool armed = false;
    if (G == 1 && small_on_host()) {
        // everything sized BEFORE the round's own requests (the largest the round's own product can make): no buffer moves,
        // and no pointer handed out here goes stale, between the product and the wait
        char* pinb = (char*)ctx_pinned(c, spec_b2_offset() + (size_t)w * w * 8);
        rider.dBs = (double*)ctx_buf(c, "cm_bsmall", (size_t)64 * 64 * 8);
        rider.gps = (double*)ctx_buf(c, "gram_partials", gram_small_partial_doubles(n, 128, 128) * 8);
        armed = pinb && rider.dBs && rider.gps;
    }
    if (armed && fused && !(c->opts.flags & SDPSR_FLAG_SPMM_ONE_BY_ONE)) {
        double* part = (double*)ctx_buf(c, "cm_part", label_spmm_pair_partial_doubles(n) * 8);
        if (!part) return SDPSR_OUT_OF_MEMORY;
        uint64_t keys[2];
        const uint64_t save = c->stream_counter;
        keys[0] = next_key(c);
        keys[1] = next_key(c);
        rider.have_t = launch_label_spmm_pair(c->stream, n, L, keys, d, W, ld, w, part, Y, ld, T, ld);
        if (!rider.have_t) c->stream_counter = save;
    }
    for (int gidx = 0; gidx < G && !batched && !rider.have_t; ++gidx) {
        live = gidx * w;
        int e2 = apply_generic(w, Y + (size_t)gidx * w * ld);
        if (e2) return e2;
    }
    live = m;
    int st = absorb(m, armed ? &rider : nullptr, got);
    if (st) return st;
    if (got != 0) spec_b2 = false;
    if (got == 0) {
        // the module is complete: the top block of this round's product, C = W' (A W), IS the
        // compressed generic element W' A W of the round's first element -- keep it for the
        // eigen stage instead of forming another one (one label product + one GEMM saved)
        saved_ld = round_up(w + m, 128);
        have_saved = first_product_intact;  // not if noise-level candidates went through the second step
    }
    return SDPSR_OK;
}

// the EIGEN phase: the seed vector, the class sums, then growth rounds until an invariance round adds nothing
int Module::grow(PhaseTimer& tm) {
    PhaseScope phase{tm, SDPSR_T_EIGEN, true};
    int st = seed_basis(), got = 1;
    if (!st) st = class_sum_round();
    for (int round = 0; round < 40 && !st && got != 0; ++round) {
        if (round >= 1) flush_deferred_tail(c);  // (more than two rounds: one segment per round was the class sums' and the first growth round's)
        st = growth_round(got);
    }
    flush_deferred_tail(c);  // the steps behind the growth wait for the stream
    if (st) return st;
    if (got != 0) return driver_fallback(c, "module growth did not close within 40 rounds");  // never diagonalise a module that no round has confirmed invariant
    // device tail: columns >= w must be zero for its padded products
    live = 0;
    if (!small_on_host()) {
        st = restore_fills();
        if (st) return st;
        HIP_TRY(c, hipMemsetAsync(W + (size_t)w * ld, 0, (size_t)ld * (wtot - w) * 8, c->stream));
    }
    return SDPSR_OK;
}

// ---- small modules (w <= 64): Murota's steps on the host (small_eigen_host.cpp) ----
// The first compressed generic element B1 = W'A1 W is the top block of the final invariance
// round's product, which the host already holds (hG); the device forms B2 = W'A2 W while the
// host diagonalises B1; after one w x w read-back everything up to Q_hat_small (w x S1) is host
// arithmetic on a few KiB, and one upload + one tall product lift it: Q_hat = W Q_hat_small.
int Module::small_host_tail(PhaseTimer& tm, double atol, std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, std::vector<double>& Qs) {
    PhaseScope phase{tm, SDPSR_T_ISO, false};
    const size_t bbytes = (size_t)w * w * 8;
    double* dB = (double*)ctx_buf(c, "cm_bsmall", bbytes);
    double* gp = (double*)ctx_buf(c, "gram_partials", gram_small_partial_doubles(n, w, w) * 8);
    double* pin = (double*)ctx_pinned(c, bbytes);
    if (!dB || !gp || !pin) return SDPSR_OUT_OF_MEMORY;
    // B = W'(A W) for a fresh generic element, compact w x w, copied towards the pinned buffer; no host wait
    auto enqueue_element = [&]() -> int {
        const int e2 = apply_generic(w, T);  // T[:, 0:w) = A W (rows < n)
        if (e2) return e2;
        launch_gram_small(c->stream, n, w, w, W, ld, T, ld, gp, dB, w, w, w, pin);  // product stored into the pinned buffer itself
        return SDPSR_OK;
    };
    auto fetch = [&](double* dst) -> int {  // waits for the enqueued element
        HIP_TRY(c, ctx_sync_stream(c, c->stream));
        symmetrize_copy(pin, w, w, dst);
        return SDPSR_OK;
    };
    std::vector<double> B1((size_t)w * w);
    if (have_saved) {
        symmetrize_copy(hG.data(), saved_ld, w, B1.data());
    } else {
        int e2 = enqueue_element();
        if (!e2) e2 = fetch(B1.data());
        if (e2) return e2;
    }
    bool spec_avail = spec_b2 && have_saved;  // B2 came back with the final round's product: no launch, no wait
    bool pending = spec_avail ? false : enqueue_element() == SDPSR_OK;  // else B2 is formed while the host diagonalises B1
    const std::function<int(double*)> next_element = [&](double* dst) -> int {
        if (spec_avail) {
            spec_avail = false;
            symmetrize_copy(spec_b2_pinned(), w, w, dst);
            return SDPSR_OK;
        }
        if (!pending) {
            const int e2 = enqueue_element();
            if (e2) return e2;
        }
        pending = false;
        return fetch(dst);
    };
    const int st = murota_small_host(c, w, B1.data(), next_element, atol, d, sizes, S1, S, Qs);
    if (pending) ctx_sync_stream(c, c->stream);  // never leave a copy into the pinned buffer in flight
    phase.collect = st != 0;
    return st;
}

// the next compressed element B = W'A W (w x w in wp x wp, zero padded, symmetric) for the dense driver
int Module::make_element(double* dst) {
    const int64_t wp = round_up(w, 128);
    if (have_saved) {  // first element: the product of the final invariance round (growth_round)
        have_saved = false;
        launch_extract_symmetric(c->stream, w, wp, Cc, saved_ld, dst);  // zero padding + copy + symmetrize in one launch
        return SDPSR_OK;
    }
    HIP_TRY(c, hipMemsetAsync(T, 0, (size_t)ld * wp * 8, c->stream));
    { int e2 = apply_generic(w, T); if (e2) return e2; }   // T = A W
    gram_tn(c, w, w, ld, W, ld, T, ld, dst, wp, wp);  // B = W' T
    launch_symmetrize(c->stream, w, wp, dst);
    return SDPSR_OK;
}

// make_element on the side stream, behind the fork point; ev_join marks its end
int Module::prefetch_element(double* dst) {
    if (!ctx_ensure_side(c)) return SDPSR_HIP_ERROR;
    if (have_saved) return SDPSR_BAD_STATE;  // the next element is the saved one: nothing to overlap
    hipStream_t main_stream = c->stream;
    if (!forked && hipEventRecord(c->ev_fork, main_stream) != hipSuccess) return SDPSR_HIP_ERROR;
    forked = false;
    if (hipStreamWaitEvent(c->side_stream, c->ev_fork, 0) != hipSuccess) return SDPSR_HIP_ERROR;
    c->stream = c->side_stream;  // every step and helper launches on c->stream
    c->main_shadow = main_stream;
    const int e2 = make_element(dst);
    const bool rec = hipEventRecord(c->ev_join, c->side_stream) == hipSuccess;
    c->stream = main_stream;
    c->main_shadow = nullptr;
    if (e2 || !rec) {
        ctx_sync_stream(c, c->side_stream);
        return e2 ? e2 : SDPSR_HIP_ERROR;
    }
    return SDPSR_OK;
}

// larger modules: the dense driver on the compressed elements, then the lift
int Module::device_tail(PhaseTimer& tm, double atol, EigInfo& info, std::vector<int32_t>& sizes, int64_t& S1, int64_t& S) {
    if (dbg_on()) fprintf(stderr, "[sdpsr] module compression: n=%lld dim(P)=%lld -> w=%d\n", (long long)n, (long long)d, w);
    dbg_mark(c, "compressed: module grown");
    ElemGen gen;
    gen.make = [this](double* dst) { return make_element(dst); };
    gen.prefetch = [this](double* dst) { return prefetch_element(dst); };
    gen.fork = [this]() -> int {
        forked = false;
        if (have_saved) return SDPSR_BAD_STATE;  // the next element is the saved one: nothing to overlap
        if (!ctx_ensure_side(c) || hipEventRecord(c->ev_fork, c->stream) != hipSuccess) return SDPSR_HIP_ERROR;
        forked = true;
        return SDPSR_OK;
    };
    gen.join = [this]() -> int {
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        return SDPSR_OK;
    };
    if (!ctx_buf(c, "bd_qhat", (size_t)n * wmax * 8)) return SDPSR_OUT_OF_MEMORY;  // final size now: no move later
    int st = dense_diagonalize(c, w, nullptr, &gen, atol, info, sizes, S1, S, tm, d);
    if (st) return st;
    dbg_mark(c, "compressed: small dense diagonalize done");
    st = lift(tm, nullptr, S1, atol);
    if (st) return st;
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    HIP_TRY(c, hipGetLastError());
    dbg_mark(c, "compressed: lifted");
    return SDPSR_OK;
}

// lift: Q_hat = W * Q_hat_small, clamped (src/diagonalize.jl:39).  Qs_host: Q_hat_small (w x S1) on the host; nullptr: it sits
// at the start of "bd_qhat", which was sized for n x wmax before the small problem ran (S1 <= w < wmax), so the buffer
// does not move here and stream order suffices
int Module::lift(PhaseTimer& tm, const double* Qs_host, int64_t S1, double atol) {
    PhaseScope phase{tm, SDPSR_T_IRRED, false};
    deferred_window_close(c);
    double* qs = (double*)ctx_buf(c, "cm_qsmall", (size_t)w * S1 * 8);
    double* Qhat = (double*)ctx_buf(c, "bd_qhat", (size_t)n * S1 * 8);
    if (!qs || !Qhat) return SDPSR_OUT_OF_MEMORY;
    if (Qs_host) {
        const int st = h2d_sync(c, qs, Qs_host, (size_t)w * S1 * 8);
        if (st) return st;
    } else {
        HIP_TRY(c, hipMemcpyAsync(qs, Qhat, (size_t)w * S1 * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    if (!parent_form() && tall_times_small_rows_supports((int)S1)) {
        // the product's store clamps and writes the row-major copy sdpsr_block_images reads: no clamp pass, no transpose pass
        double* Qrm = (double*)ctx_buf(c, "bd_qrm", (size_t)n * S1 * 8);
        if (!Qrm) return SDPSR_OUT_OF_MEMORY;
        launch_lift_clamped(c->stream, n, ld, W, w, qs, w, (int)S1, atol, Qhat, Qrm);
        c->bd_qrm_current = true;
        return SDPSR_OK;
    }
    launch_tall_times_small(c->stream, n, ld, W, w, qs, w, (int)S1, 1.0, 0.0, Qhat, n);
    launch_clamptol(c->stream, n * S1, Qhat, atol);
    return SDPSR_OK;
}

}  // namespace

namespace sdpsr {

int compressed_diagonalize(sdpsr_ctx* c, int64_t n, const uint32_t* L, int64_t d, double atol, EigInfo& info,
                           std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, PhaseTimer& tm) {
    const int wmax = (int)std::min<int64_t>(std::min<int64_t>(n / 2, 500), 2 * d + 8);
    if (wmax < 2) return driver_fallback(c, "module too small to compress");
    const int64_t wcap = round_up(wmax + 2, 128), ycap = 2 * wcap;  // candidate columns of one round: ycap
    Module m{c, n, round_up(n, 128), d, L, wmax, wcap, ycap, wcap + ycap + 128};
    int st = m.setup();
    if (!st) st = m.grow(tm);
    if (st) return st;
    if (!m.small_on_host()) return m.device_tail(tm, atol, info, sizes, S1, S);
    std::vector<double> Qs;
    st = m.small_host_tail(tm, atol, sizes, S1, S, Qs);
    if (!st) st = m.lift(tm, Qs.data(), S1, atol);
    if (st) return st;
    HIP_TRY(c, hipGetLastError());  // no host wait here: the caller synchronises (or keeps enqueueing: sdpsr_jordan_reduce)
    dbg_mark(c, "compressed: small problem solved on the host, lift enqueued");
    return SDPSR_OK;
}

// eig_driver: 0 auto (module compression when dim(P) is small against n, dense otherwise),
// 4 dense forced, 6 module compression forced, 1-3 rocSOLVER variants (comparison only).
bool compression_eligible(const sdpsr_ctx* c, int64_t n, int64_t d) {
    if (c->opts.eig_driver == 6) return true;
    if (c->opts.eig_driver != 0) return false;
    return n >= 512 && 2 * d + 8 <= std::min<int64_t>(n / 2, 500);
}

}  // namespace sdpsr
