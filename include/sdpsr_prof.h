/*
 * sdpsr_prof.h -- measurement entry points of libsdpsr_prof.so.  NOT part of the product ABI
 * (include/sdpsr.h, libsdpsr_hip.so): bench.py's roofline leg and the scripts under tools/ time
 * single kernels of the product library through these.  libsdpsr_prof.so links against
 * libsdpsr_hip.so and works on the same sdpsr_ctx.
 */
#ifndef SDPSR_PROF_H
#define SDPSR_PROF_H

#include "sdpsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Times `reps` back-to-back launches of one hot kernel on ctx's stream with HIP events, on
   resident synthetic data of order n (n is rounded up to the kernel's tile).  kind:
   0 = square int8 MFMA (one channel), 1 = square fp32 MFMA, 2 = square / Q'AQ fp64 MFMA,
   3 = partition refine of n*n signatures with `aux` distinct classes,
   4 = fused gather+projection+signature pass with r = aux basis vectors,
   5 = the tridiagonalisation's symmetric-product (symv) kernel, one launch per column j = 0..n-2
       (average over the n-1 launches), 6 = one whole tridiagonalisation of order n,
   8 = the one-workgroup Jacobi eigensolver on a random symmetric matrix of order n <= 128,
   9 = the label product Y = A(v) W of the module-compression driver (n x n labels with d classes,
       W n x w, G elements per pass): aux = w | G << 8 | d << 12; with bit 30 of aux set the call
       returns in ms_per_launch[0] the largest absolute deviation of sampled rows of Y from a host
       evaluation in extended precision instead of the time.
   10 = the HOST eigensolver of the compressed problem (order n <= 512, one host core, no device work);
   11 = kind 3 as the FIRST refinement of a call meets it: the class-count prediction is reset before every
       repetition (a many-classes input pays the overflowing first pass, the sample and the path it selects);
   ms_per_launch[0] = average milliseconds per launch. */
int sdpsr_profile_kernel(sdpsr_ctx* ctx, int kind, int64_t n, int64_t aux, int reps,
                         double* ms_per_launch);
/* The same measurement with the shader clock sampled meanwhile by a one-wave kernel on a side
   stream (clock64 against the 100 MHz wall_clock64, ~20 us intervals): out[0] = ms per launch,
   out[1] = median shader clock in MHz while the timed launches ran, out[2] = intervals used.
   The int8 squares run power-limited (the clock drops under the kernel); the roofline of
   bench.py reports the fraction of the peak both at the nominal and at this measured clock. */
int sdpsr_profile_clock(sdpsr_ctx* ctx, int kind, int64_t n, int64_t aux, int reps, double* out);
/* Host waits for a stream of ctx since its creation (every wait of the library goes through one function): the host round
   trips of a reduction = the difference around it. */
int sdpsr_profile_host_waits(sdpsr_ctx* ctx, uint64_t* out);
/* Counters of ctx (restart 0) or of batch restart `restart` (as sdpsr_batch_block_sizes): out[0] = random draws so far
   (the ctx's stream position, reset by sdpsr_set_seed), out[1] = square rounds the loop has examined, out[2] = of those, rounds
   examined speculatively -- a round is one int8 square, or one round of the square check that stands in for it (a square formed
   behind a check's "violated" verdict belongs to the round already counted) --, out[3] = the symmetric-basis hint bits the last
   admissible_subspace run used. */
int sdpsr_profile_loop_counts(sdpsr_ctx* ctx, int32_t restart, uint64_t* out);
/* Stage 2 of a two-stage tridiagonalisation (band -> tridiagonal by Householder bulge chasing, one workgroup per sweep,
   hand-offs through progress words), built to be measured: A_host n x n dense symmetric with bandwidth b (16, 32 or 64),
   d_host (n), e_host (n - 1) the tridiagonal result, out[0] = kernel milliseconds, out[1] = 1 if the chase gave up. */
int sdpsr_profile_band_chase(sdpsr_ctx* ctx, int64_t n, int b, const double* A_host, double* d_host, double* e_host, double* out);
/* Stage 1 of the two-stage form, measured with library kernels (rocSOLVER panel QR + rocBLAS level-3 updates): dense
   symmetric A (n x n, column-major, host, n a multiple of b) -> band of width b, in place (lower triangle);
   out[0] = ms of the stage (second of two runs), out[1] = ms of its panel factorisations. */
int sdpsr_profile_band_reduce(sdpsr_ctx* ctx, int64_t n, int b, double* A_host, double* out);
/* What the hipGraph cache of the tridiagonalisation (one graph per problem shape and buffer set, kept in ctx) has done
   so far: out[0] = replays of a cached graph, out[1] = misses (a graph of ~2 n nodes built and instantiated on the
   host), out[2] = milliseconds spent building.  A caller that alternates between a few orders pays the build once per
   order. */
int sdpsr_profile_sytrd_graphs(sdpsr_ctx* ctx, double* out);
/* The loop's label passes on caller-made inputs (tests).  The packed lower triangle Lp_host of symmetric labels <= d of order n (column j at
   offset j n - j (j - 1) / 2) goes through the packed channel gather in its plain and in its label-writing form, Lfull_host (the mirrored n x n
   labels) through the full-matrix gather, all with the same key.  X_plain, X_writing, X_full: T * ld * ld bytes each (T = 1, 2 or 4, ld = n
   rounded up to 128), padding included; every byte no kernel wrote is 0x5A.  L_inout: n * n + guard words, uploaded as given, written by the
   writing form (leading dimension n), downloaded again. */
int sdpsr_profile_gather_packed(sdpsr_ctx* ctx, int64_t n, int T, int64_t d, uint64_t key, const uint32_t* Lp_host, const uint32_t* Lfull_host,
                                int8_t* X_plain, int8_t* X_writing, int8_t* X_full, uint32_t* L_inout, int64_t guard);
/* The verify pass "does any entry of the packed triangle differ from the representative of its class?".  first_idx_host: the packed index of
   the representative of class l at [l - 1]; C_host: T (2 or 4) int32 channels of ld x ld.  mode 0: channels alone; 1: joint with one basis
   matrix U_host (n x n) and its coefficient coef; 2: "is U_host constant on the classes" (C_host unused).  out[0] = verdict word (0: no entry
   differs), out[1] = the class count up to which the pass is a single launch. */
int sdpsr_profile_verify(sdpsr_ctx* ctx, int64_t n, int T, int64_t d, int mode, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                         const int32_t* C_host, const double* U_host, double coef, uint64_t key, double atol, uint32_t* out);
/* The basis check of mode 2 for r = 1 .. 4 basis matrices U_host (r * n * n): "is every one of them constant on the classes, and 0 on label
   0?"  Wide labels; out as above. */
int sdpsr_profile_basis_constant(sdpsr_ctx* ctx, int64_t n, int r, int64_t d, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                                 const double* U_host, double atol, uint32_t* out);
/* The pair check of the loop's guessed initial partition: "would the refinement of the value pairs (a, b) over the packed lower triangle write
   the labels Lp_host and the representatives first_idx_host (d of them, packed indices) again?"  a_host, b_host: n x n, column-major, the
   lower triangle is read.  out[0] = verdict word (0: it would, bit for bit), out[1] = the largest d the pass takes; a larger d is refused
   with SDPSR_BAD_ARGUMENT. */
int sdpsr_profile_verify_pair(sdpsr_ctx* ctx, int64_t n, int64_t d, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                              const double* a_host, const double* b_host, uint32_t* out);
/* Guessed initial partitions of ctx (restart 0) or of batch restart `restart` (as sdpsr_profile_loop_counts): out[0] = reductions that checked
   the recorded initial partition instead of rebuilding it, out[1] = of those, the ones whose check failed (reduction repeated). */
int sdpsr_profile_initial_guess(sdpsr_ctx* ctx, int32_t restart, uint64_t* out);
/* ... out[0] = launches that made the 8-bit shadow of the packed labels behind such a guess (once per recorded partition of <= 255 classes). */
int sdpsr_profile_narrow_labels(sdpsr_ctx* ctx, int32_t restart, uint64_t* out);
/* The four consumers of the loop's packed labels at either label width (tests/test_gpu_narrow_loop_labels.py).  width 32: the kernels stream
   Lp_host as uploaded; width 8: the library's narrowing pass makes the byte copy on the device (a label > 255: SDPSR_BAD_ARGUMENT) and the
   kernels stream that.  Everything else as the entries above: each pass has one body, and the entries without a width are its width-32 form,
   so every entry refuses what either refuses (a representative outside the triangle, d above its cap, width 8 with more than 255 classes).
   gather_packed_w: plain and label-writing form of the packed channel gather (X_plain, X_writing: T * ld * ld bytes, 0x5A where no kernel
   wrote; L_inout: n * n + guard words).
   verify_w: r = -1 the channels alone, r = 0 .. 4 joint with the r basis matrices U_host (r * n * n) and coefficients coef_host (r).
   proj_coef_lower: the dot-product pass <U_k, x> over the packed triangle, x drawn from the labels and key: partial_out (r * 2048, the
   per-workgroup sums as stored) and coef_out (r), 1 <= r <= 4. */
int sdpsr_profile_gather_packed_w(sdpsr_ctx* ctx, int64_t n, int T, int64_t d, uint64_t key, int width, const uint32_t* Lp_host, int8_t* X_plain,
                                  int8_t* X_writing, uint32_t* L_inout, int64_t guard);
int sdpsr_profile_verify_w(sdpsr_ctx* ctx, int64_t n, int T, int64_t d, int r, int width, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                           const int32_t* C_host, const double* U_host, const double* coef_host, uint64_t key, double atol, uint32_t* out);
int sdpsr_profile_verify_pair_w(sdpsr_ctx* ctx, int64_t n, int64_t d, int width, const uint32_t* Lp_host, const uint32_t* first_idx_host,
                                const double* a_host, const double* b_host, uint32_t* out);
int sdpsr_profile_proj_coef_lower(sdpsr_ctx* ctx, int64_t n, int64_t r, uint64_t key, int width, const uint32_t* Lp_host, const double* U_host,
                                  double* partial_out, double* coef_out);
/* The full-matrix channel gathers of the square step on caller-made labels (tests/test_gpu_primitives.py).  kind 0: launch_gather_i8
   (T = 1 .. 8 int8 channels; dmax as the loop passes it: 0 = unknown, 1 .. 2048 = the LDS table of class bits, beyond = hashed per entry),
   kind 1: launch_gather_f32 (T float channels in [-vmax, vmax]), kind 2: launch_gather_f64_padded (T = 1).  L_host: any n x n labels
   (with dmax > 0: none above it); X_inout: T * ld * ld + guard elements of the kind's type, ld = n rounded up to 128, uploaded as they are
   and downloaded after the kernel.  out[0] = the kernel's work items, out[1] = the threads of its launch. */
int sdpsr_profile_gather_full(sdpsr_ctx* ctx, int kind, int64_t n, int T, int vmax, int64_t dmax, uint64_t key, const uint32_t* L_host,
                              void* X_inout, int64_t guard, uint64_t* out);
/* The dot products <U_k, x> of the projection, x drawn from the labels and key, in 2048 workgroups as the library launches them.  form 0:
   launch_proj_coef, coef_out[0 .. r); form 1: launch_proj_coef_probe (len == n * n), coef_out[0 .. 2r): the dot products, then the symmetry
   probes <U_k, W - W'>.  U_host: r * len, 1 <= r <= 4. */
int sdpsr_profile_proj_coef(sdpsr_ctx* ctx, int form, int64_t len, int64_t n, int64_t r, uint64_t key, const uint32_t* L_host,
                            const double* U_host, double* coef_out);
/* One refinement over a COMPUTED signature source on caller-made inputs (tests/test_gpu_refine_sources.py): the source is put together as the
   loop does it and handed to the product's own refine_signatures, which refines through it in the form the ctx's flags and refine_path
   choose (insert kernel of the source's functor, materialised array, sort, bucket, the mid kernel).  Conventions of the module-kernel entries
   below: host arrays, every *_inout array uploaded as filled and downloaded whole (guard included), SDPSR_BAD_ARGUMENT before any upload.
   kind: 0 = value pairs (a_host, b_host: n * n doubles; packed: column-major, the lower triangle is read; else flat), 1 = rounded projection
   y = x(l) - sum_k U_k coef_k (U_host: r * n * n, coef_host: r, x drawn from the old label and key), 2 / 3 = T int32 / float channels
   (C_host: T * ld * ld, ld a multiple of 128), 4 = projection and int32 channels together.  1 <= n <= 2048, ld <= 2048, T <= 8, r <= 8.
   packed: the source runs over the lower triangle column by column (n (n + 1) / 2 entries), else over all n * n; lab_packed: the old labels
   are that packed triangle themselves.  L_inout: the old labels, n (n + 1) / 2 or n * n words by lab_packed, + guard; the refinement runs IN
   PLACE on its device copy -- except packed without lab_packed, where the loop reads the full labels and writes the packed ones: then the
   new labels go to Lnew_inout (n (n + 1) / 2 + guard words; null otherwise) and L_inout comes back as it was.  kind 0 has no old labels:
   L_inout (sized by packed) receives the result.
   what 0: refine through the source.  what 1: the stand-alone kernel of run-time shape (sig_channels_kernel, proj_apply_kernel) writes the
   signature array and that is refined; refused where no such kernel exists (kind 0 and 4, a packed projection).  A source that has neither
   a functor instance nor a stand-alone kernel is refused (a packed projection with r > 4, kind 4 not packed or with T other than 2, 4).
   sig_out (optional, one word per entry): the signatures as launch_sig_materialize (what 0) resp. the stand-alone kernel (what 1) writes
   them, by a launch of its own before the refinement.  prev_classes: the ctx's class-count prediction is set to what a refinement that
   ended with this many classes leaves.  sym != 0 (not packed): the symmetry verdict of the new n x n labels is asked for as well.
   *nparts = the class count; first_out (optional, min(*nparts, 65536) words are written) = the head of "ref_first"; report[0] = relabel
   passes the driver ran (repeats included), report[1] = symmetry verdict (1 symmetric, 0 not, -1 not asked for), report[2] = 1 when the
   ctx records "ref_first" as describing the new labels. */
int sdpsr_profile_refine_source(sdpsr_ctx* ctx, int kind, int what, int64_t n, int64_t ld, int T, int r, int packed, int lab_packed, uint64_t key,
                                double atol, const double* a_host, const double* b_host, const double* U_host, const double* coef_host,
                                const void* C_host, uint32_t* L_inout, uint32_t* Lnew_inout, int64_t guard, int64_t prev_classes, int sym,
                                uint64_t* sig_out, int64_t* nparts, uint32_t* first_out, int32_t* report);
/* Guessed-closed first iterations of ctx (restart 0) or of batch restart `restart` whose two rounds were judged by the square check instead of
   two int8 squares (out[0]), and those of them that formed a real square behind a "violated" verdict read inside the loop (out[1]). */
int sdpsr_profile_square_checks(sdpsr_ctx* ctx, int32_t restart, uint64_t* out);
/* The check segments of the guessed-closed path (include/sdpsr.h: SDPSR_FLAG_CHECKS_IN_LOOP) on ctx (restart 0) or on batch restart
   `restart`, since the ctx was created: out[0] = segments registered instead of launched in the loop, out[1] = of those, enqueued inside
   a ride (behind a product of the module growth, in front of the host's wait for it), out[2] = enqueued anywhere else.  And the two
   host windows the rides fill, measured on every reduction that takes the module-compression route, whatever it defers: the
   steady-clock time from the return of the wait for a growth step's product to the next thing the host enqueues -- out[3] nanoseconds
   and out[4] windows behind the class-sum step, out[5] and out[6] behind the growth rounds (the last of them holds the compressed
   eigenproblem).  out[7..9] = the three deferred verdict words as the last voided reduction read them behind its last wait (the
   first round's, the speculative round's, the initial partition's; 0 = not violated or not deferred, 1 = stored by a kernel that
   ran, 0xDEFE44ED = its segment was never enqueued).  out: 10 words. */
int sdpsr_profile_deferred_checks(sdpsr_ctx* ctx, int32_t restart, uint64_t* out);
/* The same ten words with one appended: out[10] = reductions of sdpsr_jordan_reduce on that ctx whose blockDiagonalize read the
   ctx's copy of the recorded labels while the pass that writes P_out waited among the check segments (include/sdpsr.h:
   SDPSR_FLAG_LABELS_BEFORE_BLOCKDIAG); a voided reduction counts, its repeat does not.  out: 11 words.  (An entry of its own:
   callers of sdpsr_profile_deferred_checks hand in 10 words.) */
int sdpsr_profile_recorded_labels(sdpsr_ctx* ctx, int32_t restart, uint64_t* out);
/* The square check (csrc/kernels_square_check.hip) on caller-made inputs: "does X_t^2 take its class representative's value on every entry,
   0 on label 0?" for G (1 or 2) rounds with keys[g], T (2 or 4) channels each, on the packed labels Lp_host (<= d <= 255, width 8 or 32 as
   above) of order n <= 8192 with the representatives first_idx_host.  layout[0..6] = byte offsets of c (int32 [G T][d]), part_x (int32
   [G T][nb][64 nb], nb = ceil(n / 64)), part_c (int64, same shape), y, w (int64 [G T][64 nb]), the 128-bit block sums (uint64 [G T][nb][2])
   and the equality bits (uint32 [G T], 1: |X_t v|^2 == v'C_t v) inside the workspace, layout[7] = its bytes; 64 bytes in front of every
   array and behind the last belong to nobody.  ws_inout == NULL: only layout is filled.  Otherwise ws_inout (layout[7] bytes) is uploaded as
   the caller filled it, the kernels run as the loop launches them, and it is downloaded whole; verdicts_out[g] = round g's verdict word
   (cleared by the host, 1 when a channel differs); write_full != 0: L_inout (n * n + guard words, uploaded, downloaded) receives the full
   label matrix. */
int sdpsr_profile_square_check(sdpsr_ctx* ctx, int64_t n, int64_t d, int G, int T, const uint64_t* keys, int width, int write_full,
                               const uint32_t* Lp_host, const uint32_t* first_idx_host, uint8_t* ws_inout, uint64_t* layout,
                               uint32_t* verdicts_out, uint32_t* L_inout, int64_t guard);

/* ---- The kernels of the module-compression driver on caller-made inputs (tests/test_gpu_module_kernels.py). ----
   All matrices are column-major host arrays of doubles; labels are n x n uint32, column-major.  Every *_inout array is uploaded as the caller
   filled it, handed to the product's own launcher the way the driver calls it, and downloaded WHOLE -- padding and the `guard` elements behind
   it included -- so that what no kernel wrote comes back as it went in.  Nothing is measured.  SDPSR_BAD_ARGUMENT, before anything is uploaded
   or launched, for: a null pointer, a dimension < 1 or above its cap (n, k <= 8192; leading dimensions <= 16384; guard <= 2^20), a leading
   dimension smaller than the rows it strides, a label > d. */

/* C = A' B.  A_host: lda x mp (k rows and ma columns used), B_host: ldb x np (k rows, nb columns), C_inout: mp * np + guard, leading
   dimension mp; ma <= mp <= 256, nb <= np <= 256.  mode 0: gram_tn as Module::ortho_step / make_element call it, result padded to mp x np;
   when the shape takes the split-K route, mp, np, k, lda and ldb must be multiples of 128 and the route multiplies ALL mp, np columns.
   mode 1: launch_gram_small itself with ldc = mp (the exact-shape result ldc = mp = ma, np = nb of the small host tail); refused for a
   shape the exact-shape kernel does not take.  pinned_inout (optional, like C_inout): goes through the ctx's pinned host memory, which the
   exact-shape kernel stores the result into as well.  report[0] = 1: the exact-shape (skinny) kernel ran, 0: split-K; report[1] = 1 when the
   pinned copy was filled. */
int sdpsr_profile_gram(sdpsr_ctx* ctx, int mode, int64_t k, int64_t ma, int64_t nb, int64_t lda, int64_t ldb, int64_t mp, int64_t np,
                       const double* A_host, const double* B_host, double* C_inout, double* pinned_inout, int64_t guard, int32_t* report);
/* out[:, c] = beta out[:, c] + alpha In S[:, c] through launch_tall_times_small.  In_host: ldi x kk (n rows used), S_host: lds x ncols
   (kk rows used), out_inout: ldo * ncols + guard; kk, ncols <= 512, lds <= 1024. */
int sdpsr_profile_tall_times_small(sdpsr_ctx* ctx, int64_t n, int64_t ldi, int64_t kk, int64_t lds, int64_t ncols, double alpha, double beta,
                                   int64_t ldo, const double* In_host, const double* S_host, double* out_inout, int64_t guard);
/* The label product Y[:, g w + j] = A(keys[g]) W[:, j] through launch_label_spmm_multi (launch_label_spmm when G == 1).  L_host: labels
   <= d; W_host: ldw x 64 (w columns used); Y_inout: ldy * G * w + guard.  SDPSR_BAD_ARGUMENT where the launcher refuses the shape (G = 3, G w > 64, d > 4000,
   a class table too large for LDS).  report = the form that ran, from the function the launcher itself asks: [0] = 1 matrix cores
   (label_spmm_mfma_kernel<JT, G>) or 0 VALU (label_spmm_sload_kernel<WMAX, G>), [1] = JT resp. WMAX, [2] = the column split z,
   [3] = columns per workgroup. */
int sdpsr_profile_label_product(sdpsr_ctx* ctx, int64_t n, int64_t d, int G, int64_t w, int64_t ldw, int64_t ldy, const uint64_t* keys,
                                const uint32_t* L_host, const double* W_host, double* Y_inout, int64_t guard, int32_t* report);
/* Two label products on one W in ONE pass over the labels, through launch_label_spmm_pair (the invariance round of the module growth and
   its rider): Y0 = A(keys[0]) W, Y1 = A(keys[1]) W, each Y_inout: ldy * w + guard.  The form is the one-element matrix-core form of
   (n, d, w), run with two class tables: each block is bit for bit what sdpsr_profile_label_product gives with G = 1 and that key.
   SDPSR_BAD_ARGUMENT where the pair launch refuses: w > 64, n < 64 (no matrix-core form), class tables that do not fit in LDS.
   report as above: [0] = 1, [1] = JT, [2] = the column split z, [3] = columns per workgroup. */
int sdpsr_profile_label_product_pair(sdpsr_ctx* ctx, int64_t n, int64_t d, int64_t w, int64_t ldw, int64_t ldy, const uint64_t* keys,
                                     const uint32_t* L_host, const double* W_host, double* Y0_inout, double* Y1_inout, int64_t guard,
                                     int32_t* report);
/* Class sums of a PAIR of vectors over the window of d classes that starts at class `first`, through the class-sum pass of the
   basis_image shortcuts (class_sums2_kernel): Y[((i - 1) n + r)] = sum over c with L[c + r n] == first + i - 1 of X[c], X_host: n
   pairs (x, y interleaved), Y_inout: 2 n d + guard doubles.  plain = 1 (first = 1, every label <= d): the labels index the tables as
   they are; plain = 0: any labels, mapped through the window.  report[0] = waves per workgroup (4, 2 or 1, by d).  Summation order:
   lane q of a wave adds the columns c = q, q + 64, ... of its class ascending, from +0.0; the 64 lane sums are added in lane order. */
int sdpsr_profile_class_sums2(sdpsr_ctx* ctx, int64_t n, int64_t d, uint32_t first, int plain, const uint32_t* L_host, const double* X_host,
                              double* Y_inout, int64_t guard, int32_t* report);
/* Class sums of one vector, out[(i - 1) ldo + r] = sum over c with L[c + r n] == i of x[c], through launch_class_sums with first = 1;
   d <= 4000, out_inout: ldo * d + guard.  report[0] = class_sums_supports(n, d, ldo) -- when 0, nothing ran (as in the driver) --,
   report[1] = 1: the kernel with per-lane tables in LDS, 0: the row-sort fallback (ldo == n only). */
int sdpsr_profile_class_sums(sdpsr_ctx* ctx, int64_t n, int64_t d, int64_t ldo, const uint32_t* L_host, const double* x_host,
                             double* out_inout, int64_t guard, int32_t* report);
/* The glue kernels.  symmetrize: B <- (B + B') / 2 on the leading m x m of B_inout (ld * m + guard; m <= 1024, ld <= 2048).
   extract_symmetric: dst_inout (mp * mp + guard, dense mp x mp, mp <= 1024) <- the symmetric part of the leading m x m of src_host
   (lds x m), zero elsewhere.  normalize_columns: H[r hstride + i] = X[i + r ldx] / |X[:, r]|, norm[r] = |X[:, r]| for nruns <= 64 runs
   (H_inout: hstride (nruns - 1) + n + guard, norm_inout: nruns + guard).  random_vector: x[i] = 2 u(key, i + 1) - 1 (x_inout: n + guard). */
int sdpsr_profile_symmetrize(sdpsr_ctx* ctx, int64_t m, int64_t ld, double* B_inout, int64_t guard);
int sdpsr_profile_extract_symmetric(sdpsr_ctx* ctx, int64_t m, int64_t mp, int64_t lds, const double* src_host, double* dst_inout, int64_t guard);
int sdpsr_profile_normalize_columns(sdpsr_ctx* ctx, int64_t n, int64_t ldx, int64_t hstride, int64_t nruns, const double* X_host,
                                    double* H_inout, double* norm_inout, int64_t guard);
int sdpsr_profile_random_vector(sdpsr_ctx* ctx, int64_t n, uint64_t key, double* x_inout, int64_t guard);

/* ---- The module growth's scratch discipline (tests/test_gpu_module_scratch.py). ----
   Each of the three kernel entries runs the form the ctx's flags choose: by default the one-launch form, under
   SDPSR_FLAG_MODULE_SCRATCH_FILLS the separate launches it replaced.  Conventions of the module-kernel entries above. */

/* Every device buffer of the ctx whose name starts with "cm_" (the module growth's scratch), and "bd_qrm", is filled with the
   NaN pattern 0x7FF85A5ADEADBEEF after a stream synchronisation: whatever a later call reads of them without writing it first
   shows in its results. */
int sdpsr_profile_poison_scratch(sdpsr_ctx* ctx);
/* The stacked product written in place: M[:, w + c] = sum_{t < kk} M[:, t] S[t + c lds], c < ncols -- out = In + w ldi, ldo = ldi,
   alpha = 1, beta = 0, as Module::apply_stacked calls it.  M_inout: ldi * mcols + guard with mcols >= max(kk, w + ncols); kk <= 512,
   ncols <= 512, 1 <= w.  Default form: launch_tall_times_small_rows, report[0] = 1; where it refuses (ncols > 64) or under the flag:
   launch_tall_times_small into a scratch matrix and a copy of rows < n back, report[0] = 0. */
int sdpsr_profile_stacked_in_place(sdpsr_ctx* ctx, int64_t n, int64_t ldi, int64_t kk, int64_t lds, int64_t ncols, int64_t w, int64_t mcols,
                                   double* M_inout, const double* S_host, int64_t guard, int32_t* report);
/* The lift Qcm = clamptol(In S, atol) (n x S1, ld n) and its row-major copy Qrm[i S1 + c]; Qcm_inout, Qrm_inout: n * S1 + guard each.
   Default: launch_lift_clamped (S1 <= 64, else SDPSR_BAD_ARGUMENT); under the flag: launch_tall_times_small, launch_clamptol,
   launch_transpose_to_rowmajor. */
int sdpsr_profile_lift(sdpsr_ctx* ctx, int64_t n, int64_t ldi, int64_t kk, int64_t lds, int64_t S1, double atol, const double* In_host,
                       const double* S_host, double* Qcm_inout, double* Qrm_inout, int64_t guard);
/* The seed: x[i] = 2 u(key, i + 1) - 1, h = x / |x|, norm[0] = |x|; x_inout, h_inout: n + guard, norm_inout: 1 + guard.  Default:
   launch_seed_vector; under the flag: launch_random_vector, then launch_normalize_columns with one run. */
int sdpsr_profile_seed_vector(sdpsr_ctx* ctx, int64_t n, uint64_t key, double* x_inout, double* h_inout, double* norm_inout, int64_t guard);
/* *current = 1 when the ctx holds "bd_qrm" as the row-major copy of the Q_hat in "bd_qhat" (sdpsr_block_images then skips its transpose) */
int sdpsr_profile_qrm_current(sdpsr_ctx* ctx, int32_t* current);

/* ---- The steps of blockDiagonalize(P; complex = true) on caller-made inputs (tests/test_gpu_complex_steps.py). ----
   Conventions of the module-kernel entries above.  A complex matrix is two column-major planes of doubles (real, imaginary) with leading
   dimension n.  `route` 0 = the one-workgroup kernels the driver takes for n <= 64 (refused above 64), 1 = the route through the real symmetric
   embedding that it takes for n > 64 (here for any n >= 1: cx_embed, the real eigensolver, cx_zero_pad, cx_rot, cx_stack, cx_combine and the
   host's pivoted Cholesky all run inside a route-1 call).  SDPSR_BAD_ARGUMENT, before anything is uploaded, for: a null pointer, n < 1 or
   n > 4096, guard outside [0, 2^20], a route other than 0 / 1, a space_of or a descriptor that points outside its arrays. */

/* H = A + A^H, A[r, c] = the complex class value of L[r + c n] under `key` (real part from sdpsr_class_uniform(key, l), imaginary part from
   sdpsr_class_uniform(key ^ 0xA5A5A5A55A5A5A5A, l), label 0 -> 0), through launch_cx_gather_herm.  L_host: n * n labels, any values;
   Hr_inout, Hi_inout: n * n + guard. */
int sdpsr_profile_cx_gather_herm(sdpsr_ctx* ctx, int64_t n, const uint32_t* L_host, uint64_t key, double* Hr_inout, double* Hi_inout, int64_t guard);
/* Eigenpairs of the Hermitian H: w ascending (w_inout: n + guard), orthonormal eigenvectors in the columns of V (Vr_inout, Vi_inout:
   n * n + guard).  Route 0: launch_cx_heev; info_out[0] = 1 when the Jacobi iteration did not converge, info_out[1] = sweeps; `atol` unused.
   Route 1: cx_heev_general with the cluster tolerance `atol` (eigenvalues of the embedding within atol of their neighbour share one
   eigenspace, and the eigenvectors of one cluster span it without being matched to its single eigenvalues); the eigenvalues come back
   through the host, so the guard of w_inout is left as the caller filled it; info_out = {0, 0}; the route's own status (e.g.
   SDPSR_NUMERICAL_INCONSISTENCY for a cluster of odd size) is returned as it is. */
int sdpsr_profile_cx_heev(sdpsr_ctx* ctx, int route, int64_t n, const double* Hr_host, const double* Hi_host, double atol, double* w_inout,
                          double* Vr_inout, double* Vi_inout, int64_t guard, int32_t* info_out);
/* norms[sa * neig + sb] = max |(V^H H V)[a, b]| over space_of[a] == sa, space_of[b] == sb, as doubles, from a zero fill of the neig * neig
   results as in the driver (a pair with an empty space stays 0).  V: n x n, any columns; space_of: n entries in [0, neig), 1 <= neig <= n;
   norms_inout: neig * neig + guard.  Route 0: launch_cx_block_norms; route 1: cx_block_norms_general. */
int sdpsr_profile_cx_block_norms(sdpsr_ctx* ctx, int route, int64_t n, const double* Hr_host, const double* Hi_host, const double* Vr_host,
                                 const double* Vi_host, const int32_t* space_of, int32_t neig, double* norms_inout, int64_t guard);
/* The columns of Q-hat (irreducible_decomposition).  V: n x vcols (vcols <= 4096, leading dimension n); desc: ncols x {kind, i0, mi, j0, mj,
   col}.  kind 0: column col = V[:, i0], entries of magnitude < atol set to +0; kind 1: column col = Q_j (Q_j^H H q_i1) / |Q_i^H H q_j1|
   with Q_i = V[:, i0 .. i0 + mi), Q_j = V[:, j0 .. j0 + mj), q_x1 their first columns, then the same clamp; i0 + mi, j0 + mj <= vcols,
   1 <= mi, mj <= n, 0 <= col < ncols.  Only the columns of V that desc names are read.  Qhat_inout: 2 n ncols + guard, column col at
   2 n col, (re, im) interleaved.  Route 0: launch_cx_irreducible; route 1: launch_cx_irreducible_general, which takes every n <= 4096
   (4 n doubles of dynamic LDS). */
int sdpsr_profile_cx_irreducible(sdpsr_ctx* ctx, int route, int64_t n, int64_t vcols, const double* Hr_host, const double* Hi_host,
                                 const double* Vr_host, const double* Vi_host, const int32_t* desc, int32_t ncols, double atol,
                                 double* Qhat_inout, int64_t guard);

/* ---- The steps of the real dense blockDiagonalize on caller-made inputs (tests/test_gpu_dense_steps.py). ----
   Conventions of the module-kernel entries above: column-major host arrays of doubles, every *_inout array uploaded as the caller filled it,
   handed to the launcher or step eigdec.cpp itself calls, and downloaded whole, the `guard` elements (8 bytes each) behind it included.
   SDPSR_BAD_ARGUMENT, before anything is uploaded, for: a null pointer (where none is allowed), a dimension < 1 or above its cap (orders,
   leading dimensions, column and pair counts <= 4096; guard <= 2^20), a leading dimension smaller than its rows, a space_of entry outside
   [0, neig), a descriptor or a column index that points outside its arrays. */

/* The coupling matrix: norms[sa * neig + sb] = max(what was there, max |M[a, b]| over space_of[a] == sa, space_of[b] == sb), M = Q' A Q, as
   bit patterns of non-negative doubles (norms_inout: neig * neig + guard, 1 <= neig <= n); an entry of M that is +-0 writes nothing.
   Route 0: launch_small_qtaq_block_norms, n <= 64; A_host, Q_host: ld x n; M_inout, T_inout (ld * n + guard each; either may be null):
   rows < n of the n columns receive M resp. T = A Q.  Route 1: EigDec::couple() on the driver's padded squares: ld a multiple of 128,
   A_host, Q_host: ld x ld with whatever padding the caller made (the driver's is zero), M_inout, T_inout (ld * ld + guard, both needed):
   all ld x ld of each are written.  Route 2: launch_block_norms alone on M_inout (ld x n, read only; A_host, Q_host, T_inout unused). */
int sdpsr_profile_dense_block_norms(sdpsr_ctx* ctx, int route, int64_t n, int64_t ld, const double* A_host, const double* Q_host,
                                    const int32_t* space_of, int32_t neig, double* norms_inout, double* M_inout, double* T_inout, int64_t guard);
/* launch_small_cluster_qtaq_block_norms (n <= 64): the eigenvalues evals_host (n) are clustered -- a new eigenspace where !(|dv| <= atol) --
   and the coupling matrix of Q' A Q over those eigenspaces is formed from a zero fill.  pack_inout: small_cluster_pack_bytes(n) bytes =
   [einfo[0], einfo[1], 2 int32 untouched, neig, 11 int32 untouched][space_of: n int32, padded to a multiple of 64 bytes, padding untouched]
   [evals: n doubles][norms: neig * neig written of n * n], then guard * 8 bytes.  T_inout: ld * n + guard or null. */
int sdpsr_profile_dense_cluster_norms(sdpsr_ctx* ctx, int64_t n, int64_t ld, const double* A_host, const double* Q_host,
                                      const double* evals_host, double atol, const int32_t* einfo, void* pack_inout, double* T_inout, int64_t guard);
/* isomorphism_classes_device on the raw coupling matrix norms_inout (neig * neig + guard, [i * neig + j]; the upper triangle i <= j is read)
   and the eigenspace dimensions dims_host (neig, each >= 1), for any 1 <= neig <= 4096.  Back come: the matrix symmetrised under the dimension
   rule; stat_out[20]: [0] = ~bits(min), [1] = bits(max), [2 + c] = entries with exactly c edges <= them; edges_out[17] and *thr_out as the
   host formed them; bits_inout (neig * W + guard words, W = ceil(neig / 64)): bit b of word [i * W + w] = pair (i, j = 64 w + b), j > i,
   coupling >= threshold, every other bit of the neig * W words 0; kpart_out[neig]: the root of every eigenspace.  The step's own status,
   SDPSR_OK or SDPSR_NUMERICAL_INCONSISTENCY, is returned with all outputs filled. */
int sdpsr_profile_dense_classes(sdpsr_ctx* ctx, int32_t neig, double* norms_inout, const int32_t* dims_host, double atol, uint64_t* stat_out,
                                double* edges_out, double* thr_out, uint64_t* bits_inout, int32_t* kpart_out, int64_t guard);
/* The columns of Q-hat of npairs pair descriptors desc = {c_i, m_i, c_j, m_j, f_i, f_j, col} (the driver's 7 ints): column col of Qhat
   (leading dimension n; Qhat_inout: n * ncols + guard) = Q_j (Q_j' b_i) / |Q_i' b_j|, Q_x = Q[:, c_x .. c_x + m_x), b_x = Bf[:, f_x];
   Q_host: ldq x vcols, Bf_host: ldq x nf, n rows of each used; 1 <= m_x <= n.  Through Irreducible::launch_pairs(): route 0 = launch_irreducible_pairs
   (refused when max (m_i + m_j) + 2 doubles exceed the 60 KiB of LDS the driver's rule allows), route 1 = the four launches per pair
   (gemv_t twice, inv_norm, gemv_n_scaled), route -1 = the driver's rule chooses.  report[0] = the route that ran. */
int sdpsr_profile_dense_irreducible(sdpsr_ctx* ctx, int route, int64_t n, int64_t ldq, int64_t vcols, const double* Q_host, const double* Bf_host,
                                    int64_t nf, const int32_t* desc, int32_t npairs, double* Qhat_inout, int64_t ncols, int64_t guard,
                                    int32_t* report);
/* launch_copy_cols: dst[:, dst_cols[k]] = src[:, src_cols[k]] (n rows) for k < count, in launches of 128 columns.  src_host: ld_src x scols,
   dst_inout: ld_dst * dcols + guard.  launch_clamptol: a[e] = +0.0 where |a[e]| < atol, e < len <= 4096^2 (a_inout: len + guard). */
int sdpsr_profile_copy_cols(sdpsr_ctx* ctx, int64_t n, int64_t count, const int32_t* src_cols, const int32_t* dst_cols, const double* src_host,
                            int64_t ld_src, int64_t scols, double* dst_inout, int64_t ld_dst, int64_t dcols, int64_t guard);
int sdpsr_profile_clamptol(sdpsr_ctx* ctx, int64_t len, double* a_inout, double atol, int64_t guard);

/* ---- The stages of the dense symmetric eigensolver on caller-made inputs (tests/test_gpu_eigen_stages.py). ----
   Conventions of the dense-step entries above.  2 <= n <= ld <= 4096, ld a multiple of 128: the padded column-major square that
   sdpsr_syev_f64 makes (padding rows and columns n .. ld-1 zero).  Anything else: SDPSR_BAD_ARGUMENT before any upload. */

/* launch_sytrd (A = Q T Q', Q = H_0 ... H_{n-2}, H_j = I - tau_j v_j v_j', v_j = [0 .. 0, 1 in row j+1, A[j+2 .., j]]: LAPACK dsytrd,
   uplo = 'L') on the ctx's own buffers, in the form the ctx's flags choose (default: row form up to 2048 and the panel / row hybrid
   beyond; SDPSR_FLAG_SYTRD_PANELS; SDPSR_FLAG_SYTRD_ONE_LAUNCH); a second call of the same shape in one ctx replays the cached graph.
   A_inout: ld * ld + guard, lower triangle referenced; d_inout, e_inout, tau_inout: n + guard each.
   May write: the leading n x n of A (the row form mirrors the lower triangle into the upper one; the reflectors go below the
   subdiagonal, the diagonal and subdiagonal are NOT kept up to date), d[0 .. n), e[0 .. n-1), tau[0 .. n-1).
   Never written: rows and columns n .. ld-1 of A, e[n-1], tau[n-1], the guards. */
int sdpsr_profile_sytrd(sdpsr_ctx* ctx, int64_t n, int64_t ld, double* A_inout, double* d_inout, double* e_inout, double* tau_inout,
                        int64_t guard);
/* backtransform_prepare, then backtransform_apply, both on the ctx's main stream: Z <- H_0 ... H_{n-2} Z in compact-WY blocks of 128
   reflectors, last block first.  A_host: ld x ld, only the reflector entries (rows j+2 .. n-1 of column j <= n-3) are read;
   tau_host: n - 1.  Z_inout: ld * ld + guard, uploaded as the caller filled it; the products run over all ld x ld of it.  What may
   CHANGE is rows 1 .. n-1: row 0, rows n .. ld-1 and -- zero on entry -- columns n .. ld-1 come back as they were.  Never the guards. */
int sdpsr_profile_backtransform(sdpsr_ctx* ctx, int64_t n, int64_t ld, const double* A_host, const double* tau_host, double* Z_inout,
                                int64_t guard);
/* The tridiagonal problem d_host (n), e_host (n - 1) as syev_device issues it: zero fill of Z, descriptor upload, launch_stedc_check,
   launch_stedc, launch_stedc_check.  w_inout: n + guard, w[0 .. n) written (ascending).  Z_inout: ld * ld + guard, all ld x ld
   written: eigenvectors in the leading n x n, exact zeros in rows and columns n .. ld-1.  Never the guards.
   SDPSR_SOLVER_ERROR, with the outputs filled, when a check raises its flag. */
int sdpsr_profile_stedc(sdpsr_ctx* ctx, int64_t n, int64_t ld, const double* d_host, const double* e_host, double* w_inout, double* Z_inout,
                        int64_t guard);

/* ---- The row-space kernels of sdpsr_compress_constraints on caller-made inputs (tests/test_gpu_rowspace_kernels.py). ----
   Conventions of the module-kernel entries above.  M, W and out are m x ncols, column-major with leading dimension m.
   SDPSR_BAD_ARGUMENT, before anything is uploaded, for: a null pointer (where none is allowed), m < 1 or m > 1024, ncols < 1,
   m * ncols > 2^26, guard outside [0, 2^20], r outside [0, m], a perm entry outside [0, m), a droptol that is not >= 0. */

/* launch_rowspace_scale on M = [A | b] (A_host: m x d, b_host: m or NULL; ncols = d + (b_host != NULL)), after zeroing the flag word
   as the driver does.  W_inout (m * ncols + guard) = M * 2^-e, e the exponent of max |M| (the scale is capped at 2^1000, and 1 for
   max |M| = 0); info_out[0] = max |M| over the finite entries, info_out[1] = 1.0 when an entry is Inf or NaN -- and then no element
   of W_inout is written. */
int sdpsr_profile_rowspace_scale(sdpsr_ctx* ctx, int64_t m, int64_t d, const double* A_host, const double* b_host, double* W_inout,
                                 double* info_out, int64_t guard);
/* G = W W' through launch_rowspace_gram: both triangles of the m x m G_inout (m * m + guard) are written, G[p, q] and G[q, p] with
   one value.  The partial sums are filled with NaN bytes before the launch, so one the Gram kernel left out shows.  report = {npairs,
   Z, cps} from rowspace_gram_shape, which the launcher asks: block pairs of 64 x 64, K splits, columns per split.  Order of summation:
   within a split four columns per matrix-core step, ascending; the splits' partial sums are added in ascending order from +0.0. */
int sdpsr_profile_rowspace_gram(sdpsr_ctx* ctx, int64_t m, int64_t ncols, const double* W_host, double* G_inout, int64_t guard,
                                int32_t* report);
/* W <- J W in place through launch_rowspace_rotate; J_host: m x m, column-major (J[i + k m]); W_inout: m * ncols + guard.  Each entry
   is the sum over k ascending from +0.0, a multiply and an add (or one FMA) per term.  report = {cc, j_lds} from rowspace_chunk, which
   the launcher asks: columns per workgroup, and 1 when J is staged in LDS beside them. */
int sdpsr_profile_rowspace_rotate(sdpsr_ctx* ctx, int64_t m, int64_t ncols, const double* J_host, double* W_inout, int64_t guard,
                                  int32_t* report);
/* launch_rowspace_finish.  perm_host, sigma_host: m entries, the first r used.  sig[k] = sigma[k] with the sign of the first entry of
   largest magnitude of row perm[k] of W, k < r (sig_inout: m + guard; entries >= r are not written).  out[k, c] = W[perm[k], c] / sig[k],
   values of magnitude <= droptol and the rows >= r as +0.0; *nnz_out = the non-zeros written.  in_place != 0: out is W, as in the driver
   (out_inout unused, may be NULL; the result comes back in W_inout); otherwise out_inout (m * ncols + guard) receives it and W_inout
   (m * ncols + guard) comes back as it went in. */
int sdpsr_profile_rowspace_finish(sdpsr_ctx* ctx, int64_t m, int64_t ncols, int64_t r, const int32_t* perm_host, const double* sigma_host,
                                  double droptol, int in_place, double* W_inout, double* out_inout, double* sig_inout, int64_t* nnz_out,
                                  int64_t guard);

#ifdef __cplusplus
}
#endif
#endif /* SDPSR_PROF_H */
