// admissible_subspace (src/partitions.jl:109-190): the Jordan-reduction loop on the device, and desymmetrize (:197-223).
#include <algorithm>
#include <cmath>

#include "host_internal.h"

using namespace sdpsr;

namespace {  // ---- the admissible_subspace loop, src/partitions.jl:145-185 ----
// Which label array is current.  Symmetric labels live as the packed lower triangle Lp (column j at offset j n - j (j - 1) / 2) between the
// refinements of the int8 loop: every consumer there reads the packed form (the channel gather mirrors it tile by tile).  The full matrix L is
// formed by the channel gather of a round that is expected not to refine (a confirm round, the speculative square of a guess): that kernel holds
// every tile in both orientations anyway, and when the round's verdict is "unchanged" L is the call's output as it stands.  A refinement
// invalidates it; the unpack pass forms it where no such gather ran (no confirm rounds), or whenever a step needs it (non-symmetric basis, other
// square modes).  Only the methods below write the validity bits.
// The guessed-closed path also keeps Lp8, a byte copy of Lp (labels <= 255), valid from the guess that made or found it until anything
// refines: the streaming passes of that path read a quarter of the label bytes.  Lp stays the truth; the shadow never outlives it.
class LoopLabels {
public:
    uint32_t* L = nullptr;   // the full matrix (the call's output)
    uint32_t* Lp = nullptr;  // the packed lower triangle (integer modes)
    uint8_t* Lp8 = nullptr;  // its 8-bit shadow ("adm_lpacked8"; nullptr: this call keeps none)
    int sym = 0;             // the labels are symmetric: by construction, or by the verdict of the last refine_full
    void init(sdpsr_ctx* ctx, int64_t order, uint32_t* symflag_dev, bool keep, bool early) { c = ctx, n = order, symflag = symflag_dev, keep_packed = keep, early_ok = early; }
    bool packed() const { return packed_valid; }
    const uint32_t* current(bool from_packed) const { return from_packed ? Lp : L; }
    void need_full() {
        if (!full_valid) launch_unpack_symmetric_labels(c->stream, n, Lp, L);
        full_valid = true;
    }
    // where a gather of the packed labels should write the full matrix too (nullptr: it is current already); the caller enqueues that gather
    uint32_t* full_from_gather() {
        if (full_valid || !packed_valid) return nullptr;
        full_valid = true;
        return L;
    }
    void packed_refined() { packed_valid = true, full_valid = false, narrow_valid = false; }
    // the shadow holds the packed labels (made by this call's narrowing launch, or recorded by the last call): right after the guess
    void shadow_current() { narrow_valid = packed_valid && Lp8 != nullptr; }
    bool narrow() const { return narrow_valid; }
    const uint8_t* shadow(bool from_packed = true) const { return from_packed && packed_valid && narrow_valid ? Lp8 : nullptr; }
    // symmetric by construction: refine the n (n + 1) / 2 entries of the packed lower triangle (same relative order, same canonical numbering; in
    // place when the labels were packed); the full matrix is formed right away only where the loop does not keep packed labels (the joint iteration
    // runs with keep_packed alone: nothing to form there)
    int refine_packed(const SigSource& src, int64_t* d) {
        const int st = refine_signatures(c, n * (n + 1) / 2, src, Lp, d, 0, nullptr, nullptr, early_ok);  // (early report: what follows is stream-ordered)
        packed_refined();
        if (!st && !keep_packed) need_full();
        return st;
    }
    int refine_full(const SigSource& src, int64_t* d, bool with_symmetry_verdict) {
        if (with_symmetry_verdict) c->symflag_zero = false;  // (the check pass stores its verdict into symflag[0])
        const int st = with_symmetry_verdict ? refine_signatures(c, n * n, src, L, d, n, symflag, &sym) : refine_signatures(c, n * n, src, L, d);
        full_valid = true, packed_valid = false, narrow_valid = false;
        return st;
    }
private:
    sdpsr_ctx* c = nullptr;
    int64_t n = 0;
    uint32_t* symflag = nullptr;
    bool keep_packed = false, early_ok = false, full_valid = true, packed_valid = false, narrow_valid = false;
};

// Extra independent draws before a stall is believed: a round that did not refine spends one of the confirm rounds left and asks for another square
// (true).  A confirmed speculation is the confirm round just scheduled, made and looked at already -- it found nothing either and spends the next one.
bool another_confirm_round(bool refined, int& confirm_left, bool spec_confirmed = false) {
    if (refined || confirm_left <= 0) return false;
    --confirm_left;
    if (!spec_confirmed) return true;
    if (confirm_left == 0) return false;
    --confirm_left;
    return true;
}

struct Verdict {
    bool unchanged = false;       // no entry differs from the representative of its class: no refinement needed
    bool spec_confirmed = false;  // the confirm round ran speculatively behind this verify pass and found nothing either
};

// One call of the loop: its constants, its buffers, and the state the iterations share.
struct Loop {
    Loop(sdpsr_ctx* ctx, PhaseTimer& timer) : c(ctx), s(ctx->stream), tm(timer) {}
    sdpsr_ctx* c;
    hipStream_t s;
    PhaseTimer& tm;
    int64_t n, len, ld, r;
    double atol, scale;  // scale: src/utils.jl:37
    int mode, T, vmax = 0;
    bool int_mode, keep_packed, early_ok;
    const double* dU;
    uint64_t* sig;
    static constexpr int nblk = 2048;
    double *partial, *coef, *Y = nullptr;
    void *Xp = nullptr, *Cp = nullptr;
    uint32_t* symflag;          // [0] verdict of the last check, [8] constant 0
    const uint32_t* zero_flag;  // "symmetric" for the kernels that take a device flag
    LoopLabels lab;
    // --- state ---
    int64_t current = 0;
    int it = 0, confirm_left = 0;
    uint64_t key = 0;          // the projection's key of this iteration
    bool packed_proj = false;  // ... and whether it works on the lower triangle
    bool proj_dead = false;    // every U_k constant on the classes of S: the projection half cannot refine S any more
    // Projection on the lower triangle (half the bytes and hashes of the step) needs symmetric labels AND symmetric basis matrices U_k.  The caller
    // may vouch for the latter (sdpsr_hint_symmetric_basis); otherwise the first iteration's dot-product pass carries a randomized symmetry probe and
    // the following iterations use its verdict.
    bool basis_sym = false, probe_pending = false;
    // ---- signature sources (sdpsr_internal.h: SigSource) ----
    // integer modes: y = round(x - U coef) exists only inside the insert pass of the refinement
    SigSource proj_source(const uint32_t* labels, int packed, int lab_packed) {
        SigSource q;
        q.kind = SIG_PROJ, q.sig = sig, q.U = dU, q.coef = coef, q.r = (int)r, q.key = key, q.atol = atol, q.scale = scale, q.n = n;
        q.L = labels, q.packed = packed, q.lab_packed = lab_packed;
        return q;
    }
    // signatures of the squares: computed inside the insert pass of the refinement (integer modes; kind SIG_ARRAY: the fp64 mode's array)
    SigSource chan_source(int kind, const uint32_t* labels, int packed, int lab_packed) {
        SigSource q;
        q.kind = kind, q.sig = sig, q.n = n, q.ld = ld, q.T = T, q.C = Cp;
        q.L = labels, q.packed = packed, q.lab_packed = lab_packed;
        return q;
    }
    // (label, rounded projection, channel values) of the packed triangle; projection dead: the square's channel values alone
    SigSource joint_source(bool from_packed) {
        SigSource q = proj_source(lab.current(from_packed), 1, from_packed ? 1 : 0);
        q.kind = proj_dead ? SIG_CHAN_I32 : SIG_JOINT_I32, q.ld = ld, q.T = T, q.C = Cp;
        q.L8 = lab.shadow(from_packed);  // (the verify passes' label stream while the shadow is current; a refinement reads q.L)
        return q;
    }
    // The symmetric int8 square of a fresh random element of S: X from the packed or the full labels, X'X = X X on the lower-triangle tiles only (X
    // is symmetric, the product exact).
    // write_full (packed labels only): the gather forms the full label matrix as well, unless it is current (LoopLabels).
    // gather_only: the product itself is a segment of the ctx's deferred tail (verify_round), enqueued and counted by flush_deferred_tail.
    void launch_square(bool from_packed, uint64_t key, void* X, void* C, int64_t dim, bool write_full = false, bool gather_only = false) {
        if (from_packed) launch_gather_i8_sym_packed(s, n, ld, T, lab.Lp, key, (int8_t*)X, dim, write_full ? lab.full_from_gather() : nullptr, lab.shadow());
        else launch_gather_i8(s, n, ld, T, lab.L, key, (int8_t*)X, dim);
        if (gather_only) return;
        launch_gemm_tn_i8_sym(s, ld, ld, (const int8_t*)X, ld, (int32_t*)C, ld, T, ld * ld, ld * ld, zero_flag, c->num_cus, c->opts.square_kernel);
        ++c->squares_launched;
    }
    // Is the projection half still able to split a class?  Not once every U_k is constant on the classes of S (kernels_class_compare.hip,
    // launch_basis_constant_on_classes): x - U U'x of a class-constant x is then class-constant for every x, and a finer S keeps that.  Generically
    // this holds after the first projection refinement (entries of a class with different U_k get different projected values); it is CHECKED, once
    // per iteration until it holds, on the labels the last refinement made, and from then on the iteration is the square alone: no dot-product pass
    // over U, signatures from the channel values only.
    int check_projection_dead() {
        void* uref = ctx_buf(c, "adm_uref", uconst_ref_bytes(current, r));
        const uint32_t* first = (const uint32_t*)ctx_buf(c, "ref_first", (size_t)refine_first_cap() * 4);
        uint32_t* hv = pinned_report(c, PINNED_BASIS_CONSTANT);
        if (!uref || !first || !hv) return SDPSR_OUT_OF_MEMORY;
        if (launch_basis_constant_on_classes(s, n, r, dU, lab.Lp, current, first, atol, scale, uref, hv)) {
            HIP_TRY(c, ctx_sync_stream(c, s));
            HIP_TRY(c, hipGetLastError());
            proj_dead = hv[0] == 0;
        }
        return SDPSR_OK;
    }
    // Rounds that are expected NOT to refine -- a confirm round, and the first iteration (an input that is closed already) -- first ask the cheap
    // question "does any entry differ from the representative of its class?" (one streaming compare pass, kernels_class_compare.hip verify_*); only a yes
    // runs the insert / rank / label passes.  A confirm round re-checks the channels only: its projected element is the one the previous round has
    // cleared.
    bool verify_applies(bool confirming, bool from_packed) const {
        return (it == 1 || confirming) && from_packed && c->first_idx_labels == lab.Lp && current >= 1 && current <= (int64_t)refine_first_cap() &&
               !(c->opts.flags & SDPSR_FLAG_NO_VERIFY_SHORTCUT);
    }
    bool guess_applies(bool confirming) const { return it == 1 && !confirming && confirm_left > 0 && c->predict_closed && c->predict_n == n && early_ok; }
    // The guess inside sdpsr_jordan_reduce, both verdicts deferred: the round launches its two gathers only, and the two squares and
    // verify passes wait on the ctx as its deferred tail (sdpsr_internal.h) for the host waits of blockDiagonalize.  Decided before the
    // round's first launch, from everything verify_round would find out on its way: its buffers (asked for here, with its names and
    // sizes) and the verify pass's instances.  With phase timers the tail would be booked under blockDiagonalize's phases (event
    // pairs around a segment enqueued there would need a collect of their own behind another wait): a timed call launches everything here.
    // confirm_left == 1: the speculative square is the LAST confirm round, so the round that registers the tail is the loop's last launch
    // (another_confirm_round returns false on "confirmed").  With more confirm rounds the loop goes on: its next round gathers into
    // "adm_xi8" again, and a refinement behind a violated verdict rewrites "adm_lpacked" / "ref_first" and outgrows "adm_vref" -- all of
    // them the segments' operands (flush_deferred_tail).  Such a call launches everything here, in stream order, as before.
    bool tail_applies(const SigSource& qj, bool confirming, bool from_packed) {
        if (!verify_applies(confirming, from_packed) || !guess_applies(confirming) || confirm_left != 1 || !c->allow_deferred_verdict || !c->pinned_small || tm.enabled) return false;
        SigSource q2 = qj;
        q2.kind = SIG_CHAN_I32;
        if (!verify_no_split_supports(qj, current) || !verify_no_split_supports(q2, current)) return false;
        return ctx_buf(c, "adm_vref", verify_ref_bytes(current)) && ctx_buf(c, "ref_first", (size_t)refine_first_cap() * 4) &&
               pinned_report(c, PINNED_VERIFY) && ctx_buf(c, "adm_xi8_spec", (size_t)T * ld * ld) &&
               ctx_buf(c, "adm_ci32_spec", (size_t)T * ld * ld * 4) && ctx_buf(c, "adm_vref2", verify_ref_bytes(current));
    }
    // The guessed-closed first iteration without its two squares (kernels_square_check.hip, DESIGN section 2 dev. 15): both rounds are
    // expected to answer "no class splits" and nothing else, and that answer -- X_t^2 equals its class constants -- is checked with a
    // random vector in one pass over the labels.  Symmetric packed labels, int8 channels; the projection half of the joint verdict
    // needs the LDS form of the compare (or no live projection at all).
    bool check_applies(bool confirming, bool from_packed) const {
        return guess_applies(confirming) && verify_applies(confirming, from_packed) && lab.sym && mode == SDPSR_SQUARE_I8 &&
               square_check_supports(n, current, 2, T) && !(c->opts.flags & SDPSR_FLAG_SQUARE_EVERY_VERDICT) &&
               (proj_dead || r == 0 || current <= (int64_t)verify_lds_cap());
    }
    // The launches whose only product is a verdict word read in reduce.cpp -- the pair check of a guessed initial partition, the
    // projection's dot products and compare, the square check's verdict kernels -- go to the ctx's deferred tail as check segments
    // (sdpsr_internal.h) under the conditions that let check_round leave its verdicts unread, with the phase timers off (as in
    // tail_applies).  SDPSR_FLAG_CHECKS_IN_LOOP: everything is launched here.
    bool checks_deferrable() const {
        return c->allow_deferred_verdict && c->pinned_small != nullptr && !tm.enabled && !(c->opts.flags & SDPSR_FLAG_CHECKS_IN_LOOP);
    }
    // The checked rounds: key2 is the joint round's key, the confirm round's is drawn here, where verify_round draws it.  Stream order:
    // class constants, the pass (which writes the full labels: expected to be the call's last label pass), the projection compare into
    // the first verdict word, the verdicts.  The label write cannot wait unless blockDiagonalize reads the record's copy of the labels
    // (on_record below: then the class constants and the pass are a segment too).  tail (joint_iteration decides, and has then left the
    // projection's dot products to this round too): what follows the pass is registered as the round's check segment instead of
    // launched -- dot products, projection compare, verdict kernels, with the arguments they have here -- and both words read
    // "violated" until the segment is enqueued.
    // Both rounds count as squares examined.  A "violated" first verdict read here forms the real square of key2 for the refinement
    // that follows (not counted again).
    int check_round(const SigSource& qj, uint64_t key2, bool tail, Verdict* v) {
        SquareCheck q;
        q.n = n, q.d = current, q.G = 2, q.T = T;
        void* ws = ctx_buf(c, "adm_sqcheck", square_check_ws_bytes(n, current, 2, T));
        const uint32_t* first = (const uint32_t*)ctx_buf(c, "ref_first", (size_t)refine_first_cap() * 4);
        uint32_t* hv = pinned_report(c, PINNED_VERIFY);
        uint32_t* hv2 = pinned_report(c, PINNED_SPECULATIVE);
        if (!ws || !first || !hv || !hv2) return SDPSR_OUT_OF_MEMORY;
        const bool defer = c->allow_deferred_verdict && c->pinned_small != nullptr;
        if (defer) hv = c->pinned_small + PINNED_SMALL_DEFERRED_VERIFY.first, hv2 = c->pinned_small + PINNED_SMALL_DEFERRED_SPECULATIVE.first;
        square_check_ws_carve(q, ws);
        q.key[0] = key2, q.key[1] = next_key(c);
        q.Lp = lab.Lp, q.Lp8 = lab.shadow(), q.first_idx = first, q.Lfull = lab.full_from_gather();
        q.flag[0] = hv, q.flag[1] = hv2;
        const bool proj_verify = qj.kind == SIG_JOINT_I32 && r >= 1;
        // (joint_iteration has left the dot products to the segment: a round that cannot register one would compare against stale "proj_coef")
        if (tail && !defer) return ctx_fail(c, SDPSR_BAD_STATE, "admissible_subspace: check segment asked for where the verdicts are read in the loop");
        if (tail) {
            *(volatile uint32_t*)hv = DEFERRED_NEVER_RAN;  // (flush_deferred_tail clears both words from the host in front of the segment)
            *(volatile uint32_t*)hv2 = DEFERRED_NEVER_RAN;
            // The guessed initial partition is the record's, and the record holds its full labels (rec_full): nothing refines in this
            // call unless a verdict is violated, so blockDiagonalize starts on that copy (reduce.cpp) and the class constants and the
            // pass, whose label write was all that kept them here, go in front of everything else that is pending.
            const bool on_record = rec_full != nullptr && c->initial_guess_pending && q.Lfull == lab.L;
            if (!on_record) launch_square_check_ref_and_pass(s, q);
            DeferredTail& t = c->deferred_tail;
            if (t.next == t.count) t.next = t.count = 0;
            if (t.count >= DEFERRED_SEGMENTS) return ctx_fail(c, SDPSR_BAD_STATE, "admissible_subspace: no room for the round's check segment");
            DeferredSegment& g = t.seg[t.count++] = DeferredSegment{};
            g.kind = DEFERRED_CHECK, g.q = qj, g.n = n, g.d = current, g.first = first, g.flag = hv;
            g.Lp = lab.Lp, g.Lp8 = lab.shadow();
            g.proj_coef = !proj_dead, g.partial = partial, g.coef = coef, g.nblk = nblk;
            g.proj_verify = proj_verify;
            g.verdict = true, g.sq = q;
            ++c->check_stats.registered;
            if (on_record) {
                // Two segments as before.  The pending pair segment becomes {class constants, pass} and its compare moves into the
                // round's segment (same labels, same representatives): 51 us behind the class sums' product and 86 us behind the
                // growth round's at N = 4096.  The host's own work there is 14 and 58 us, so both overflow under any split and
                // the order is what matters: the pass before the block sums (profiles/r28_recorded_labels.txt).  No pair segment
                // pending: the round's own segment starts with the pass.
                DeferredSegment& g0 = t.seg[t.next];
                if (&g0 != &g && g0.pair && g0.n == g.n && g0.Lp == g.Lp && g0.Lp8 == g.Lp8 && g0.first == g.first) {
                    g.pair = true, g.a = g0.a, g.b = g0.b, g.pair_d = g0.pair_d, g.pair_flag = g0.pair_flag;
                    g0.pair = false;
                }
                g0.sq_pass = true, g0.sq = q;
                c->labels_on_record = rec_full;
            }
        } else {
            *(volatile uint32_t*)hv = 0u;  // (the kernels only ever store 1; the last verdicts on these words have been read)
            *(volatile uint32_t*)hv2 = 0u;
            launch_square_check_ref_and_pass(s, q);
            if (proj_verify) launch_verify_projection(s, qj, current, first, hv);
            launch_square_check_verdict(s, q);
        }
        c->squares_launched += 2, ++c->squares_speculative, ++c->square_checks;
        if (defer) {
            c->deferred_verdict = true;  // both words are read in reduce.cpp
            HIP_TRY(c, hipGetLastError());
            v->unchanged = v->spec_confirmed = true;
            return SDPSR_OK;
        }
        HIP_TRY(c, ctx_sync_stream(c, s));
        HIP_TRY(c, hipGetLastError());
        v->unchanged = hv[0] == 0;
        v->spec_confirmed = v->unchanged && hv2[0] == 0;
        if (!v->spec_confirmed) --c->stream_counter;  // (a confirm round that follows redraws this key)
        if (!v->unchanged) {
            ++c->square_check_fallbacks;
            --c->squares_launched;
            launch_square(true, key2, Xp, Cp, current);
        }
        return SDPSR_OK;
    }
    // tail (tail_applies): the round's square has not been launched
    int verify_round(const SigSource& qj, bool confirming, bool from_packed, bool tail, Verdict* v) {
        if (!verify_applies(confirming, from_packed)) return SDPSR_OK;
        SigSource qv = qj;
        if (confirming) qv.kind = SIG_CHAN_I32;
        void* vref = ctx_buf(c, "adm_vref", verify_ref_bytes(current));
        const uint32_t* first = (const uint32_t*)ctx_buf(c, "ref_first", (size_t)refine_first_cap() * 4);
        // the verdicts have their own pinned words (the refinement's counters live at the start of the buffer)
        uint32_t* hv = pinned_report(c, PINNED_VERIFY);
        uint32_t* hv2 = pinned_report(c, PINNED_SPECULATIVE);
        if (!vref || !first || !hv) return SDPSR_OUT_OF_MEMORY;
        // (inside sdpsr_jordan_reduce, on a guess that the input is closed: both verdicts go to words nobody else writes and are read by the
        // reduction behind its next host waits, not here) (no guess under SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT: the control flow of rounds 1-4)
        const bool guess = guess_applies(confirming);
        const bool defer = guess && c->allow_deferred_verdict && c->pinned_small != nullptr;
        if (defer) hv = c->pinned_small + PINNED_SMALL_DEFERRED_VERIFY.first, hv2 = c->pinned_small + PINNED_SMALL_DEFERRED_SPECULATIVE.first;
        if (tail) {
            // The speculative gather -- the key the confirm round would draw, the full labels for blockDiagonalize -- and then nothing:
            // first square -> joint verify and speculative square -> channel verify are registered with the arguments they would be
            // launched with here.  Until a segment is enqueued its verdict word reads as "violated".
            int8_t* Xs = (int8_t*)ctx_buf(c, "adm_xi8_spec", (size_t)T * ld * ld);
            int32_t* Cs = (int32_t*)ctx_buf(c, "adm_ci32_spec", (size_t)T * ld * ld * 4);
            void* vref2 = ctx_buf(c, "adm_vref2", verify_ref_bytes(current));
            if (!Xs || !Cs || !vref2) return SDPSR_OUT_OF_MEMORY;
            launch_square(true, next_key(c), Xs, Cs, current, /*write_full=*/true, /*gather_only=*/true);
            DeferredTail& t = c->deferred_tail;
            t.ld = ld, t.d = current, t.T = T, t.zero_flag = zero_flag, t.first = first;
            t.seg[0] = t.seg[1] = DeferredSegment{};  // (kind DEFERRED_SQUARE; nothing is pending here: joint_iteration)
            t.seg[0].X = (const int8_t*)Xp, t.seg[0].C = (int32_t*)Cp, t.seg[0].q = qv, t.seg[0].vref = vref, t.seg[0].flag = hv, t.seg[0].speculative = false;
            t.seg[1].X = Xs, t.seg[1].C = Cs, t.seg[1].q = qj, t.seg[1].vref = vref2, t.seg[1].flag = hv2, t.seg[1].speculative = true;
            t.seg[1].q.kind = SIG_CHAN_I32, t.seg[1].q.C = Cs;
            *(volatile uint32_t*)hv = DEFERRED_NEVER_RAN;
            *(volatile uint32_t*)hv2 = DEFERRED_NEVER_RAN;
            t.next = 0, t.count = DEFERRED_SEGMENTS;
            c->deferred_verdict = true;  // both words are read in reduce.cpp
            HIP_TRY(c, hipGetLastError());
            v->unchanged = v->spec_confirmed = true;
            return SDPSR_OK;
        }
        if (!launch_verify_no_split(s, qv, current, first, vref, hv)) return SDPSR_OK;  // the verdict is stored straight into pinned host memory
        // An input that was closed the last time (the restarts of ONE problem, the use this library is built for) will be closed again: the confirm
        // round -- a fresh square into its own buffers and its verify pass -- is enqueued behind the first verdict's kernels and both verdicts come
        // back with one host wait instead of two.  A wrong guess costs the discarded square; the result is the same either way (the first verdict
        // decides first, exactly as without the guess).  The speculative square draws the key the confirm round would draw; a square that does not
        // serve as a confirm round gives its key back, so that the call's later draws are those of a call that took no guess.
        bool spec = false;
        if (guess) {
            void* Xs = ctx_buf(c, "adm_xi8_spec", (size_t)T * ld * ld);
            void* Cs = ctx_buf(c, "adm_ci32_spec", (size_t)T * ld * ld * 4);
            void* vref2 = ctx_buf(c, "adm_vref2", verify_ref_bytes(current));
            if (Xs && Cs && vref2) {
                launch_square(true, next_key(c), Xs, Cs, current, /*write_full=*/true);  // (expected to be the call's last gather)
                ++c->squares_speculative;
                SigSource q2 = qj;
                q2.kind = SIG_CHAN_I32, q2.C = Cs;
                spec = launch_verify_no_split(s, q2, current, first, vref2, hv2);
            }
        }
        if (defer && spec) {
            c->deferred_verdict = true;  // both words are read in reduce.cpp
            HIP_TRY(c, hipGetLastError());
            v->unchanged = v->spec_confirmed = true;
        } else {
            HIP_TRY(c, ctx_sync_stream(c, s));
            HIP_TRY(c, hipGetLastError());
            v->unchanged = hv[0] == 0;
            v->spec_confirmed = spec && v->unchanged && hv2[0] == 0;
            if (spec && !v->spec_confirmed) --c->stream_counter;  // (a confirm round that follows redraws this key)
        }
        return SDPSR_OK;
    }
    // Joint iteration (int8, everything symmetric, few classes): the projected element and the square -- two independent random elements of the SAME
    // partition S -- refine S in ONE canonical relabel of the signature (label, rounded projection, channel values).  The reference refines twice per
    // iteration and draws the squared element from the already refined partition (:159-174); both loops stop at the same fixed point (the smallest
    // partition subspace containing C_L, X0 that is closed under the projection and under squaring), since a class is only ever split when generic
    // elements of the closure force it.  An "iteration" is then one joint step.  Returns the new dimension in *d_out.
    int joint_iteration(int64_t* d_out) {
        int st = SDPSR_OK;
        const bool jl = lab.packed();
        if (!jl) lab.need_full();
        // The guessed-closed first round as check segments (checks_deferrable, check_round): decided here, in front of the iteration's
        // first launch, because the dot products -- read only by that round's projection compare when nothing refines -- go with them.
        // Every other iteration first enqueues what is pending (the pair check of a guessed initial partition): in stream order again.
        const bool defer_checks = checks_deferrable() && check_applies(false, jl);
        if (!defer_checks) flush_deferred_tail(c);
        // (at most three attempts: a basis that is never class-constant must not pay the check in every iteration)
        if (!proj_dead && it >= 2 && it <= 4 && r >= 1 && jl && c->first_idx_labels == lab.Lp && current >= 1 &&
            current <= (int64_t)refine_first_cap() && !(c->opts.flags & SDPSR_FLAG_ALWAYS_PROJECT)) {
            st = check_projection_dead();
            if (st) return st;
        }
        // (Round 3 measured this dot-product pass on the side stream BESIDE the channel gather and the int8 square -- two independent readers of the
        // same labels: theta_c32xk128 477 against 480 reductions/s in sequence, closed_scheme 1016 against 1028.  The square slows by what the
        // overlapped pass takes from it; kept in sequence.)
        if (!proj_dead && !defer_checks) launch_proj_coef_lower(s, n, r, dU, lab.current(jl), jl ? 1 : 0, key, partial, nblk, coef, lab.shadow(jl));
        tm.end();
        int64_t dj = current;
        bool confirming = false;  // this round repeats the square after a round that did not refine
        for (;;) {
            // the loop goes into another round: its gathers and a refinement behind it touch the pending segments' operands.  (A square
            // tail is never pending here: the round that registers one is the loop's last, tail_applies)
            if (confirming) flush_deferred_tail(c);
            tm.begin(SDPSR_T_SQUARE);
            const uint64_t key2 = next_key(c);
            const bool jl2 = lab.packed();
            // a confirm round that the verify pass will judge is expected to leave the labels as they are: its gather writes the full matrix
            const SigSource qj = joint_source(jl2);
            const bool check = check_applies(confirming, jl2);             // this round and the speculative one are checked, not squared
            if (defer_checks && !confirming && !check)  // (the same predicate on the same state; the dot products were left to this round's segment)
                return ctx_fail(c, SDPSR_BAD_STATE, "admissible_subspace: the round that was to carry the dot products is not a checked round");
            const bool tail = !check && tail_applies(qj, confirming, jl2);  // this square and the speculative one go to the ctx's deferred tail
            if (!check) launch_square(jl2, key2, Xp, Cp, current, /*write_full=*/confirming && verify_applies(confirming, jl2), /*gather_only=*/tail);
            tm.end();
            tm.begin(SDPSR_T_REFINE);
            Verdict v;
            st = check ? check_round(qj, key2, defer_checks && !confirming, &v) : verify_round(qj, confirming, jl2, tail, &v);
            if (st) return st;
            if (v.unchanged) dj = current;  // labels (packed, and full where a gather has written them), class representatives and table hints stay as they are
            else if (!(st = initial_guess_settled())) st = lab.refine_packed(qj, &dj);  // (never a refinement of labels that were only guessed)
            tm.end();
            if (st) return st;
            tm.collect();
            if (!another_confirm_round(dj != current, confirm_left, v.spec_confirmed)) break;
            confirming = true;  // (same projected element, a fresh square: the projection did not refine either)
        }
        *d_out = dj;
        return SDPSR_OK;
    }
    // The random square of the separate path (:166-168) in every mode, and the source of its signatures. Integer modes.  Symmetric labels (the
    // Jordan-algebra case; the verdict came back with the counters of the last refinement): X is symmetric, X X = X'X is symmetric and exact, so only
    // the lower-triangle tiles are computed, only entries i >= j get a signature, and the strict upper triangle of the new labels is mirrored after
    // the refinement (first occurrences in column-major order always sit in the lower triangle: same canonical numbering).  Non-symmetric labels: X X
    // literally, with the K-contiguous left operand gathered from the transposed labels (same draw).
    int launch_separate_square(uint64_t key2, int64_t d1, int64_t d2, SigSource* qs) {
        const bool slab = keep_packed && lab.sym && lab.packed();  // the square step reads the packed labels
        if (!slab) lab.need_full();
        const uint32_t* L = lab.L;
        *qs = chan_source(SIG_ARRAY, lab.current(slab), lab.sym, slab ? 1 : 0);
        const uint32_t* Lleft = L;
        if (int_mode && !lab.sym) {
            uint32_t* Lt = (uint32_t*)ctx_buf(c, "des_lt", len * 4);
            if (!Lt) return SDPSR_OUT_OF_MEMORY;
            launch_transpose_labels(s, n, L, Lt);
            Lleft = Lt;
        }
        switch (mode) {
        case SDPSR_SQUARE_I8:
            qs->kind = SIG_CHAN_I32;
            if (lab.sym) return launch_square(slab, key2, Xp, Cp, d2), SDPSR_OK;  // d2 = current dimension
            launch_gather_i8(s, n, ld, T, L, key2, (int8_t*)Xp, d2);
            if (int8_t* Xl = (int8_t*)ctx_buf(c, "des_yi8", (size_t)T * ld * ld)) {
                launch_gather_i8(s, n, ld, T, Lleft, key2, Xl, d2);
                launch_gemm_tn_i8(s, ld, ld, ld, Xl, ld, (const int8_t*)Xp, ld, (int32_t*)Cp, ld, T, ld * ld, ld * ld, ld * ld);
                break;
            }
            return SDPSR_OUT_OF_MEMORY;
        case SDPSR_SQUARE_F32:
            qs->kind = SIG_CHAN_F32;
            launch_gather_f32(s, n, ld, T, vmax, L, key2, (float*)Xp);
            if (!lab.sym) {
                float* Xl = (float*)ctx_buf(c, "adm_xlf32", (size_t)T * ld * ld * 4);
                if (!Xl) return SDPSR_OUT_OF_MEMORY;
                launch_gather_f32(s, n, ld, T, vmax, Lleft, key2, Xl);
                launch_gemm_tn_f32(s, ld, ld, ld, Xl, ld, (const float*)Xp, ld, (float*)Cp, ld, T, ld * ld, ld * ld, ld * ld);
            } else {
                launch_gemm_tn_f32_sym(s, ld, ld, (const float*)Xp, ld, (float*)Cp, ld, T, ld * ld, ld * ld, zero_flag);
            }
            break;
        default:
            // reference-literal: the projected element is squared when the projection step did not refine S (X is overwritten in place at :160-163),
            // a fresh random element otherwise (:166-168)
            if (d1 != current || confirm_left != c->opts.confirm_rounds) launch_gather_f64_padded(s, n, ld, L, key2, (double*)Xp);
            else launch_pad_copy(s, n, ld, Y, Xp, 8);
            launch_gemm_tn_f64(s, ld, ld, ld, (const double*)Xp, ld, (const double*)Xp, ld, (double*)Cp, ld, 1, 0, 0, 0);
            launch_sig_f64_rounded(s, n, ld, L, (const double*)Cp, atol, scale, sig);
        }
        ++c->squares_launched;  // (one square of T channels, whichever mode)
        return SDPSR_OK;
    }
    // The reference's iteration: refine by the projected element (:159-164), then by the square of a fresh one (:166-174).
    int separate_iteration(int64_t* d_out) {
        int st = SDPSR_OK;
        double* probe_host = nullptr;  // set: the dot products carry the symmetry probe of the basis, copied towards here
        flush_deferred_tail(c);  // (a guessed initial partition's pair check: this iteration refines)
        const bool plab = packed_proj && lab.packed();  // the projection reads the packed labels
        if (!plab) lab.need_full();
        if (packed_proj) {
            launch_proj_coef_lower(s, n, r, dU, lab.current(plab), plab ? 1 : 0, key, partial, nblk, coef);
        } else if (probe_pending && int_mode && len < (int64_t(1) << 32)) {
            launch_proj_coef_probe(s, len, n, r, dU, lab.L, key, partial, nblk, coef);
            if (PINNED_FIXED_BYTES + (size_t)r * 8 <= c->pinned_bytes) {  // (behind the fixed pinned words: no other report reaches there)
                probe_host = (double*)((char*)c->pinned + PINNED_FIXED_BYTES);
                HIP_TRY(c, hipMemcpyAsync(probe_host, coef + r, (size_t)r * 8, hipMemcpyDeviceToHost, s));
            }
        } else {
            launch_proj_coef(s, len, r, dU, lab.L, key, nullptr, partial, nblk, coef);
        }
        SigSource qp;
        if (Y) {
            qp.sig = sig;
            launch_proj_apply(s, len, r, dU, lab.L, key, nullptr, coef, atol, scale, 1, Y, sig);
        } else {
            qp = proj_source(lab.current(plab), packed_proj ? 1 : 0, plab ? 1 : 0);
        }
        tm.end();
        tm.begin(SDPSR_T_REFINE);
        int64_t d1 = 0;
        st = packed_proj ? lab.refine_packed(qp, &d1) : lab.refine_full(qp, &d1, int_mode);
        tm.end();
        if (st) return st;
        if (probe_host) {  // the refinement has synchronised the stream: the probes are in
            probe_pending = false, basis_sym = true;
            for (int64_t k = 0; k < r; ++k)
                if (!(std::fabs(probe_host[k]) <= 1e-10)) basis_sym = false;  // |U_k| = 1 (orthonormal basis)
        }
        int64_t d2 = d1;
        for (;;) {
            tm.begin(SDPSR_T_SQUARE);
            SigSource qs;
            st = launch_separate_square(next_key(c), d1, d2, &qs);
            if (st) return st;
            tm.end();
            tm.begin(SDPSR_T_REFINE);
            // symmetric labels: the signatures exist for the packed lower triangle only
            st = (int_mode && lab.sym) ? lab.refine_packed(qs, &d2) : lab.refine_full(qs, &d2, false);
            tm.end();
            if (st) return st;
            tm.collect();
            if (!another_confirm_round(d2 != current, confirm_left)) break;
        }
        *d_out = d2;
        return SDPSR_OK;
    }
    // S = Part(CL); S = refine!(S, Part(X0L))   (:145-146): both refinements in one canonical relabel; the pair signature is computed inside the
    // insert pass
    // guess (admissible_subspace_impl decides): "adm_lpacked" / "ref_first" still hold the initial partition of the last call on this ctx, which
    // found its input closed -- the restarts of one problem hand in the same C_L, X0_L again.  Then the partition is not rebuilt but CHECKED: one
    // streaming compare of every entry's pair signature with its class representative's (launch_verify_pair: the word stays 0 exactly when the
    // refinement would write the same labels and representatives again), no table, no ranking, no label pass, no host wait.  The verdict goes to a
    // word of its own and is read with the loop's two deferred ones, behind the reduction's last wait (reduce.cpp); the loop goes on from the
    // state a rebuild would have left.  Before anything REFINES these labels the word is read here (initial_guess_settled).
    int initial_partition(const double* dCL, const double* dX0, int hint, const InitialRecord* guess, int64_t* d) {
        SigSource q;
        q.kind = SIG_PAIR, q.sig = sig, q.a = dCL, q.b = dX0;
        if (!((hint & 2) && lab.Lp && len < (int64_t(1) << 32))) return lab.refine_full(q, d, true);  // + symmetry verdict of the initial partition
        // the caller vouches for symmetric CL / X0L (the reference symmetrises both, src/partitions.jl:128-141): the initial partition from the lower
        // triangle, mirrored
        q.n = n, q.packed = 1, lab.sym = 1;
        initial_packed = true;
        // The labels' 8-bit shadow (lab.Lp8 set: this call keeps one) is made here once, in front of the first pass that streams it, unless
        // the record says that it is there already.  Its overflow word is nobody's to wait for -- d0 <= 255 says that every label fits --
        // and is read with the guess's verdict (initial_guess_violated), as "violated".
        const uint8_t* Lp8 = guess ? lab.Lp8 : nullptr;
        if (guess) {
            uint32_t* over = c->pinned_small + PINNED_SMALL_DEFERRED_NARROW.first;
            *(volatile uint32_t*)over = 0u;
            if (Lp8 && !(guess->narrow && guess->Lp8 == Lp8)) {
                launch_labels_narrow(s, n * (n + 1) / 2, lab.Lp, lab.Lp8, 8, over, c->num_cus);
                ++c->label_narrowings;
            }
        }
        // The pair check's only product is its word: where the round's checks can be deferred (checks_deferrable; not beside a square
        // tail, which fills the ctx's two segments itself) it is registered as the first check segment instead of launched -- dCL / dX0
        // are the caller's device arrays or their staging copies "adm_cl" / "adm_x0", both outlive the reduction -- and the word
        // reads "violated" until the segment is enqueued.  The shadow's narrowing launch above stays: the loop's passes stream it.
        bool pair_registered = false;
        if (guess && checks_deferrable() && !(c->opts.flags & SDPSR_FLAG_SQUARE_EVERY_VERDICT) && n < (int64_t(1) << 31) && guess->d0 >= 1 &&
            guess->d0 <= (int64_t)verify_lds_cap()) {  // (the shapes launch_verify_pair takes)
            flush_deferred_tail(c);  // (nothing is pending at the start of a loop call)
            DeferredTail& t = c->deferred_tail;
            DeferredSegment& g = t.seg[0] = DeferredSegment{};
            g.kind = DEFERRED_CHECK, g.pair = true, g.n = n, g.a = dCL, g.b = dX0, g.Lp = lab.Lp, g.Lp8 = Lp8, g.pair_d = guess->d0, g.first = guess->first;
            g.pair_flag = c->pinned_small + PINNED_SMALL_DEFERRED_INITIAL.first;
            *(volatile uint32_t*)g.pair_flag = DEFERRED_NEVER_RAN;
            t.next = 0, t.count = 1;
            ++c->check_stats.registered;
            pair_registered = true;
        }
        if (guess && (pair_registered || launch_verify_pair(s, n, dCL, dX0, lab.Lp, guess->d0, guess->first, c->pinned_small + PINNED_SMALL_DEFERRED_INITIAL.first, Lp8))) {
            c->initial_guess_pending = true;
            ++c->initial_guesses;
            HIP_TRY(c, hipGetLastError());
            *d = guess->d0;
            lab.packed_refined();
            lab.shadow_current();
            // (the hint a refinement that found d0 classes leaves, primitives.cpp; first_idx_labels is Lp already)
            c->table_log2_hint = refine_table_hint(n * (n + 1) / 2, (uint64_t)guess->d0);
            return SDPSR_OK;
        }
        return lab.refine_packed(q, d);
    }
    // The guessed initial partition's verdict, where the loop cannot go on without it: waits for the stream.  Violated: the loop ends with
    // STATUS_REPEAT_REDUCTION (the word stays pending: reduce.cpp reads it again and repeats the reduction).
    int initial_guess_settled() {
        if (!c->initial_guess_pending) return SDPSR_OK;
        flush_deferred_tail(c);  // (the word is read: its pair check must have been enqueued; and what follows refines)
        HIP_TRY(c, ctx_sync_stream(c, s));
        HIP_TRY(c, hipGetLastError());
        if (initial_guess_violated(c) != 0) return STATUS_REPEAT_REDUCTION;
        c->initial_guess_pending = false;
        return SDPSR_OK;
    }
    bool initial_packed = false;  // the initial partition was formed (or guessed) on the packed lower triangle
    const uint32_t* rec_full = nullptr;  // the guessed record's full labels, where this call may leave blockDiagonalize to them (check_round)
    // The square mode's buffers (same names and sizes for every call of a mode; T = 1 in the fp64 mode)
    int square_buffers() {
        static const struct { const char *x, *c; size_t xb, cb; } B[] = {{"adm_xi8", "adm_ci32", 1, 4}, {"adm_xf32", "adm_cf32", 4, 4}, {"adm_xf64", "adm_cf64", 8, 8}};
        if (mode < SDPSR_SQUARE_I8 || mode > SDPSR_SQUARE_F64) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "unknown square_mode");
        const size_t e = (size_t)T * ld * ld;
        Xp = ctx_buf(c, B[mode - SDPSR_SQUARE_I8].x, e * B[mode - SDPSR_SQUARE_I8].xb);
        Cp = ctx_buf(c, B[mode - SDPSR_SQUARE_I8].c, e * B[mode - SDPSR_SQUARE_I8].cb);
        if (mode == SDPSR_SQUARE_F32) {
            vmax = std::min(127, (int)std::floor(std::sqrt(16777216.0 / (double)n)));
            if (vmax < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "n too large for the exact fp32 square");
        }
        if (mode == SDPSR_SQUARE_F64 && !(Y = (double*)ctx_buf(c, "adm_y", (size_t)len * 8))) return SDPSR_OUT_OF_MEMORY;
        return (Xp && Cp) ? SDPSR_OK : SDPSR_OUT_OF_MEMORY;
    }
};
}  // namespace

namespace sdpsr {
// The deferred tail's segments, in order, on the ctx's stream; squares are counted here, where they are enqueued.  A segment reads
// "adm_xi8" / "adm_xi8_spec" (its gathered element), "adm_lpacked" or its shadow "adm_lpacked8" and "ref_first" (labels and class representatives), "proj_coef" and
// the caller's U (joint verify), "adm_symflag" (the constant zero); it writes "adm_ci32" / "adm_ci32_spec", "adm_vref" / "adm_vref2"
// and its verdict word.  A check segment (DEFERRED_CHECK) reads "adm_lpacked" or "adm_lpacked8" and "ref_first" as well; the pair check reads the
// caller's C_L / X0_L (or "adm_cl" / "adm_x0"); the round's segment reads the caller's U (or "adm_u") and the square check's partial sums in
// "adm_sqcheck" (written by the pass, which ran in the loop), and writes "proj_partial", "proj_coef", the rest of "adm_sqcheck" and its two
// verdict words, which the host clears here, in front of the segment's first launch (the kernels only ever store 1).
// Where blockDiagonalize reads the record's labels "adm_lfull_rec" (check_round), the pass is a segment too: it reads "adm_lpacked" or
// "adm_lpacked8" and "ref_first", writes all of "adm_sqcheck" and the caller's label matrix, which nothing reads before the call's last
// flush; "adm_lfull_rec" itself is read by blockDiagonalize's kernels between the segments and written by nobody while a record lives.
// Whoever enqueues work of its own while segments are pending must touch none of these -- in particular run no refinement
// (refine_signatures rewrites "ref_first") and request none of these buffers with another size (ctx_buf enqueues what is pending before
// it frees any buffer).  Whoever waits for the stream in order to read a deferred word enqueues what is pending first.
void flush_deferred_tail(sdpsr_ctx* c, int max_segments, bool in_ride) {
    DeferredTail& t = c->deferred_tail;
    if (!in_ride && t.next < t.count) deferred_window_close(c);
    for (; max_segments > 0 && t.next < t.count; --max_segments, ++t.next) {
        const DeferredSegment& g = t.seg[t.next];
        if (g.kind == DEFERRED_CHECK) {
            if (g.sq_pass) launch_square_check_ref_and_pass(c->stream, g.sq);
            if (g.pair) launch_verify_pair(c->stream, g.n, g.a, g.b, g.Lp, g.pair_d, g.first, g.pair_flag, g.Lp8);  // (clears the word from the host)
            if (g.verdict) {
                *(volatile uint32_t*)g.sq.flag[0] = 0u;
                *(volatile uint32_t*)g.sq.flag[1] = 0u;
                if (g.proj_coef) launch_proj_coef_lower(c->stream, g.n, g.q.r, g.q.U, g.Lp, 1, g.q.key, g.partial, g.nblk, g.coef, g.Lp8);
                if (g.proj_verify) launch_verify_projection(c->stream, g.q, g.d, g.first, g.flag);
                launch_square_check_verdict(c->stream, g.sq);
            }
            ++(in_ride ? c->check_stats.in_ride : c->check_stats.outside_ride);
            continue;
        }
        launch_gemm_tn_i8_sym(c->stream, t.ld, t.ld, g.X, t.ld, g.C, t.ld, t.T, t.ld * t.ld, t.ld * t.ld, t.zero_flag, c->num_cus, c->opts.square_kernel);
        ++c->squares_launched;
        if (g.speculative) ++c->squares_speculative;
        launch_verify_no_split(c->stream, g.q, t.d, t.first, g.vref, g.flag);  // (clears the word from the host where it is one launch)
    }
}

// mem_in: where CL / X0L / U live; mem_out: where P_out lives.  final_sync = false (sdpsr_jordan_reduce): return with the last launches (the
// gather or the unpack that forms the full labels) still in flight on ctx's stream -- the caller keeps enqueueing; *labels_sym_out = 1 if the labels written are symmetric by
// construction.
int admissible_subspace_impl(sdpsr_ctx* c, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r, double atol,
                             uint32_t* P_out, int64_t* dim_out, int32_t* iters_out, double* phase_ms, int mem, int mem_out,
                             bool final_sync, int* labels_sym_out) {
    CHECK_CTX(c);
    const int hint = c->hint_symmetric_basis;  // one call only, whatever happens below
    c->hint_symmetric_basis = 0;
    c->hint_used = hint;
    c->adm_dims.clear();
    const InitialRecord rec = c->initial_record;  // whatever this call does, it ends with its own record or with none
    c->initial_record = InitialRecord{};
    if (!CL || !X0L || !P_out || !dim_out || n < 1 || r < 0 || (r > 0 && !U) || !(atol > 0))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const int64_t len = n * n;
    int st = check_len(c, len);
    if (st) return st;
    hipStream_t s = c->stream;
    PhaseTimer tm(c, phase_ms != nullptr);
    TotalEvents ev_total(phase_ms != nullptr, s);

    // the table-size hint left by the previous call describes ITS final partition; this call starts from the few classes of (C_L, X0) again (a stale
    // "many classes" hint would send the first refinements down the bucketed path)
    c->table_log2_hint = 12;
    Loop lp(c, tm);
    lp.n = n, lp.len = len, lp.ld = round_up(n, 128), lp.r = r, lp.atol = atol;
    lp.early_ok = !(c->opts.flags & SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT);  // refinements return on their label pass's report (ctx_wait_word)
    const double* dCL = in_dev(c, "adm_cl", CL, len, mem, &st);
    const double* dX0 = in_dev(c, "adm_x0", X0L, len, mem, &st);
    lp.dU = in_dev(c, "adm_u", U, (size_t)len * std::max<int64_t>(r, 1), mem, &st);
    lp.lab.L = out_dev(c, "adm_labels", P_out, len, mem_out, &st);
    lp.sig = (uint64_t*)ctx_buf(c, "sig", len * 8);
    lp.partial = (double*)ctx_buf(c, "proj_partial", (size_t)2 * std::max<int64_t>(r, 1) * lp.nblk * 8);  // + the symmetry probes
    lp.coef = (double*)ctx_buf(c, "proj_coef", (size_t)2 * std::max<int64_t>(r, 1) * 8);
    lp.symflag = (uint32_t*)ctx_buf(c, "adm_symflag", 64);
    if (st || !lp.sig || !lp.partial || !lp.coef || !lp.symflag) return st ? st : SDPSR_OUT_OF_MEMORY;
    // (the words are zero already when the last call on this ctx wrote none of them: one fill launch less)
    if (!c->symflag_zero) HIP_TRY(c, hipMemsetAsync(lp.symflag, 0, 64, s));
    c->symflag_zero = true;  // until somebody writes a verdict there (LoopLabels::refine_full) or the buffer is replaced (ctx_buf)
    lp.zero_flag = lp.symflag + 8;
    lp.mode = c->opts.square_mode, lp.T = (lp.mode == SDPSR_SQUARE_F64) ? 1 : c->opts.channels;
    st = lp.square_buffers();
    if (st) return st;
    lp.scale = round_scale(c, atol);
    lp.int_mode = (lp.mode == SDPSR_SQUARE_I8 || lp.mode == SDPSR_SQUARE_F32);
    lp.lab.Lp = lp.int_mode ? (uint32_t*)ctx_buf(c, "adm_lpacked", (size_t)(n * (n + 1) / 2) * 4) : nullptr;
    if (lp.int_mode && !lp.lab.Lp) return SDPSR_OUT_OF_MEMORY;
    lp.keep_packed = lp.mode == SDPSR_SQUARE_I8 && (lp.T == 1 || lp.T == 2 || lp.T == 4) && !(c->opts.flags & SDPSR_FLAG_UNPACK_EVERY_STEP);
    lp.lab.init(c, n, lp.symflag, lp.keep_packed, lp.early_ok);

    // The initial partition is guessed (Loop::initial_partition) inside sdpsr_jordan_reduce only, where a wrong guess repeats the reduction, for
    // an input predicted closed whose record is this call's: same order, same buffers, the packed route -- and only where the first iteration is
    // the joint one with its verify pass, which looks at the guessed labels before anything refines them.
    const bool first_joint = !(c->opts.flags & (SDPSR_FLAG_SEPARATE_REFINEMENTS | SDPSR_FLAG_NO_VERIFY_SHORTCUT)) && lp.keep_packed && (lp.T == 2 || lp.T == 4) &&
                             (r == 0 || (hint & 1)) && r <= 4 && len < (int64_t(1) << 32) && c->opts.max_iters >= 1;
    const bool guess_initial = c->allow_deferred_verdict && c->pinned_small && lp.early_ok && c->predict_closed && c->predict_n == n && (hint & 2) && first_joint &&
                               rec.valid && rec.n == n && rec.Lp == lp.lab.Lp && rec.sym == 1 && rec.d0 >= 1 && rec.d0 <= (int64_t)verify_lds_cap() &&
                               c->first_idx_labels == lp.lab.Lp && rec.first == (const uint32_t*)ctx_buf(c, "ref_first", (size_t)refine_first_cap() * 4);
    if (dbg_on() && c->allow_deferred_verdict && !guess_initial)
        fprintf(stderr, "[sdpsr] loop: initial partition not guessed (predicted closed %d at n %lld, hint %d, joint first iteration %d, record %d: n %lld, d0 %lld, "
                        "labels %d, representatives of them %d)\n", (int)c->predict_closed, (long long)c->predict_n, hint, (int)first_joint, (int)rec.valid,
                (long long)rec.n, (long long)rec.d0, (int)(rec.Lp == lp.lab.Lp), (int)(c->first_idx_labels == lp.lab.Lp));
    // ... and such a call streams the labels' 8-bit shadow where every label fits a byte (a record of 256 classes takes the guess with the wide
    // labels; SDPSR_FLAG_WIDE_LOOP_LABELS: never).  No buffer: the wide labels.
    if (guess_initial && rec.d0 <= 255 && !(c->opts.flags & SDPSR_FLAG_WIDE_LOOP_LABELS))
        lp.lab.Lp8 = (uint8_t*)ctx_buf(c, "adm_lpacked8", (size_t)(n * (n + 1) / 2));
    // The record's full labels ("adm_lfull_rec", InitialRecord::Lfull) serve a guessed call of sdpsr_jordan_reduce whose first round is the
    // checked one with its segments (check_applies, checks_deferrable: the conditions known here; check_round looks at the rest), and
    // are made for the next call, under the same conditions, by a call that ends with a record and finds no copy (below).
    const bool record_labels = c->record_labels_allowed && c->allow_deferred_verdict && c->pinned_small && !tm.enabled && first_joint && (hint & 2) &&
                               lp.mode == SDPSR_SQUARE_I8 && !(c->opts.flags & (SDPSR_FLAG_CHECKS_IN_LOOP | SDPSR_FLAG_SQUARE_EVERY_VERDICT));
    if (guess_initial && record_labels && rec.Lfull && rec.Lfull == (const uint32_t*)ctx_buf(c, "adm_lfull_rec", (size_t)len * 4)) lp.rec_full = rec.Lfull;
    int64_t d = 0;
    tm.begin(SDPSR_T_REFINE);
    st = lp.initial_partition(dCL, dX0, hint, guess_initial ? &rec : nullptr, &d);
    tm.end();
    if (st) return st;
    tm.collect();  // (intervals whose end has not passed yet stay pending: the refinement may have returned on its label pass's report)
    c->adm_dims.assign(1, d);
    if (label_overflows(c, (uint64_t)d)) return label_overflow_fail(c, "admissible_subspace: dim(S)", (uint64_t)d);
    lp.basis_sym = (r == 0) || (hint & 1) != 0, lp.probe_pending = !lp.basis_sym;

    const int64_t maximal = (len + n) / 2;  // :148
    lp.current = d, lp.confirm_left = c->opts.confirm_rounds;
    bool converged = lp.current >= maximal;
    const bool separate = (c->opts.flags & SDPSR_FLAG_SEPARATE_REFINEMENTS) != 0;
    while (lp.current < maximal) {  // :154
        if (lp.it >= c->opts.max_iters) break;
        ++lp.it;
        // --- random projection (:159-164) ---
        tm.begin(SDPSR_T_PROJECT);
        lp.key = next_key(c);
        lp.packed_proj = lp.int_mode && lp.lab.sym && lp.basis_sym && r <= 4 && len < (int64_t(1) << 32);
        const bool joint = !separate && lp.packed_proj && lp.keep_packed && (lp.T == 2 || lp.T == 4) && c->table_log2_hint < 21;
        int64_t dn = lp.current;
        st = joint ? lp.joint_iteration(&dn) : lp.separate_iteration(&dn);
        if (st) return st;
        c->adm_dims.push_back(dn);
        if (label_overflows(c, (uint64_t)dn)) return label_overflow_fail(c, "admissible_subspace: dim(S)", (uint64_t)dn);
        if (dn == lp.current) {  // :180-182
            converged = true;
            break;
        }
        lp.confirm_left = c->opts.confirm_rounds;
        lp.current = dn;  // :184
        if (lp.current >= maximal) converged = true;
    }
    lp.lab.need_full();
    HIP_TRY(c, hipGetLastError());
    c->predict_closed = converged && lp.it == 1 && c->adm_dims.size() == 2 && c->adm_dims[0] == c->adm_dims[1];
    c->predict_n = n;
    // a call that refined nothing after its initial partition leaves that partition, and its representatives, where the next call looks for them
    if (converged && lp.initial_packed && c->first_idx_labels == lp.lab.Lp && c->adm_dims[0] >= 1 && c->adm_dims[0] <= (int64_t)verify_lds_cap() &&
        std::all_of(c->adm_dims.begin(), c->adm_dims.end(), [&](int64_t x) { return x == c->adm_dims[0]; })) {
        // The full labels that belong to it: a guessed call leaves the record's copy as it found it.  A call that finds none -- an
        // unguessed one, or one that guessed on a record made where no copy was wanted (a timed call, a flag since cleared) and so
        // wrote its labels in the loop -- copies its output (complete in stream order: need_full above) where the next call could
        // start blockDiagonalize on the copy.  A wrong guess drops the record, and the copy with it, before anybody reads either.
        const uint32_t* lfull = guess_initial ? rec.Lfull : nullptr;
        if (!lfull && record_labels && lp.lab.sym && square_check_supports(n, c->adm_dims[0], 2, lp.T)) {
            uint32_t* copy = (uint32_t*)ctx_buf(c, "adm_lfull_rec", (size_t)len * 4);
            if (copy && hipMemcpyAsync(copy, lp.lab.L, (size_t)len * 4, hipMemcpyDeviceToDevice, s) == hipSuccess) lfull = copy;
            else (void)hipGetLastError();  // (no copy: the next call keeps the old order)
        }
        InitialRecord& ir = c->initial_record;
        ir.first = (const uint32_t*)ctx_buf(c, "ref_first", (size_t)refine_first_cap() * 4);  // (before `valid`: ctx_buf drops the record of a buffer it replaces)
        ir.Lfull = lfull;
        ir.n = n, ir.d0 = c->adm_dims[0], ir.Lp = lp.lab.Lp, ir.sym = lp.lab.sym;
        ir.narrow = lp.lab.narrow(), ir.Lp8 = ir.narrow ? lp.lab.Lp8 : nullptr;  // (the shadow, where the call ends with a current one)
        ir.valid = ir.first != nullptr;
    } else {
        c->labels_on_record = nullptr;  // (something refined behind a settled guess: the call's labels are its own, formed by need_full above)
    }
    *dim_out = lp.current;
    if (iters_out) *iters_out = lp.it;
    if (labels_sym_out) *labels_sym_out = lp.lab.sym;
    if (final_sync || mem_out != SDPSR_MEM_DEVICE) {
        st = out_finish(c, P_out, lp.lab.L, len, mem_out);
        if (st) return st;
    }
    if (phase_ms) {
        const float ms = ev_total.stop(s);
        tm.collect();
        for (int i = 0; i < SDPSR_T_COUNT; ++i) phase_ms[i] = tm.acc[i];
        phase_ms[SDPSR_T_TOTAL] = ms;
    }
    if (!converged) return ctx_fail(c, SDPSR_NOT_CONVERGED, "max_iters reached");
    return SDPSR_OK;
}
}  // namespace sdpsr

extern "C" {
int sdpsr_admissible_subspace(sdpsr_ctx* c, int64_t n, const double* CL, const double* X0L,
                              const double* U, int64_t r, double atol, uint32_t* P_out,
                              int64_t* dim_out, int32_t* iters_out, double* phase_ms, int mem) {
    if (!c || c->label_width == 32 || !P_out || !dim_out || n < 1)
        return admissible_subspace_impl(c, n, CL, X0L, U, r, atol, P_out, dim_out, iters_out, phase_ms, mem, mem, true, nullptr);
    // narrow labels: the loop works on the ctx's uint32 buffer; the result is narrowed into the caller's array once dim(S) is known to fit
    CHECK_CTX(c);
    uint32_t* L = (uint32_t*)ctx_buf(c, "adm_labels", (size_t)n * n * 4);
    if (!L) return SDPSR_OUT_OF_MEMORY;
    const int st = admissible_subspace_impl(c, n, CL, X0L, U, r, atol, L, dim_out, iters_out, phase_ms, mem, SDPSR_MEM_DEVICE, true, nullptr);
    if (st && st != SDPSR_NOT_CONVERGED) return st;
    if (label_width_overflows(c, (uint64_t)*dim_out)) return label_width_fail(c, "admissible_subspace", (uint64_t)*dim_out);  // (P_out untouched)
    const int st_out = labels_out_finish(c, P_out, L, (size_t)n * n, mem);
    return st_out ? st_out : st;
}

// desymmetrize, src/partitions.jl:197-223
int sdpsr_desymmetrize(sdpsr_ctx* c, int64_t n, uint32_t* P, int64_t* dim, int32_t* iters, int mem) {
    CHECK_CTX(c);
    if (!P || !dim || n < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    const int64_t len = n * n;
    int st = check_len(c, len);
    if (st) return st;
    // (device memory at width 32: refined in place; a narrow P is widened into the ctx's buffer and receives the result from there)
    uint32_t* L = (mem == SDPSR_MEM_DEVICE && c->label_width == 32) ? P : (uint32_t*)labels_in_dev(c, "adm_labels", (const uint32_t*)P, len, mem, &st);
    if (st) return st;
    st = desymmetrize_device(c, n, L, dim, iters);
    if (st) return st;
    if (label_width_overflows(c, (uint64_t)*dim)) return label_width_fail(c, "desymmetrize", (uint64_t)*dim);  // (P untouched)
    return labels_out_finish(c, P, L, len, mem);
}
}  // extern "C"

// the rounds of desymmetrize on uint32 device labels, in place; returns with the stream waited for (the last refinement's verdict)
int sdpsr::desymmetrize_device(sdpsr_ctx* c, int64_t n, uint32_t* L, int64_t* dim, int32_t* iters) {
    const int64_t len = n * n;
    int st = SDPSR_OK;
    hipStream_t s = c->stream;
    const int T = c->opts.channels;
    const int64_t ld = round_up(n, 128);
    uint32_t* Lt = (uint32_t*)ctx_buf(c, "des_lt", len * 4);
    int8_t* X = (int8_t*)ctx_buf(c, "adm_xi8", (size_t)T * ld * ld);
    int8_t* Y = (int8_t*)ctx_buf(c, "des_yi8", (size_t)T * ld * ld);
    int32_t* Cp = (int32_t*)ctx_buf(c, "adm_ci32", (size_t)T * ld * ld * 4);
    uint64_t* sig = (uint64_t*)ctx_buf(c, "sig", len * 8);
    if (!Lt || !X || !Y || !Cp || !sig) return SDPSR_OUT_OF_MEMORY;
    int64_t current = *dim;
    int it = 0;
    int confirm_left = c->opts.confirm_rounds;  // extra independent products before a stall is believed (as in the loop above)
    for (;;) {  // :208-220
        if (it >= c->opts.max_iters) return ctx_fail(c, SDPSR_NOT_CONVERGED, "max_iters reached");
        ++it;
        launch_transpose_labels(s, n, L, Lt);
        launch_gather_i8(s, n, ld, T, Lt, next_key(c), X);  // X' as the K-contiguous operand
        launch_gather_i8(s, n, ld, T, L, next_key(c), Y);
        launch_gemm_tn_i8(s, ld, ld, ld, X, ld, Y, ld, Cp, ld, T, ld * ld, ld * ld, ld * ld);  // (X')' Y = X Y
        launch_sig_i32(s, n, ld, T, L, Cp, sig);
        int64_t d2 = 0;
        st = refine_signatures(c, len, sig, L, &d2);
        if (st) return st;
        if (d2 == current) {
            if (!another_confirm_round(false, confirm_left)) break;
            --it;  // a confirm round is not an iteration of the reference's loop
            continue;
        }
        confirm_left = c->opts.confirm_rounds;
        current = d2;
    }
    *dim = current;
    if (iters) *iters = it;
    return SDPSR_OK;
}
