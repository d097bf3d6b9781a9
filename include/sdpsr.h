/*
 * sdpsr.h -- C ABI of libsdpsr_hip.so: the MI355X (gfx950) implementation of the
 * Jordan-reduction hot path of SDPSymmetryReduction.jl.
 *
 * The reference is pure Julia and has no FFI; its seam is dispatch on the
 * partition type (AbstractPartition contract, src/abstract_part.jl:7-16, exercised
 * by the alternate backend in test/partitions_set.jl:6-92,102-105).  A Julia
 * backend type `HIPPartition` binds these entry points with `ccall`
 * (INTEGRATION.md shows the stub).  Every entry point cites the reference lines it
 * replaces (paths relative to the reference repo root).
 *
 * Conventions
 *  - all matrices column-major, n x n unless stated; "len" = number of entries
 *    scanned in column-major linear order (the only order the reference uses);
 *  - labels are uint32: 0 = structurally-zero class (not counted), 1..dim; a ctx told so with
 *    sdpsr_set_label_width reads and writes them as uint16 / uint8 instead (the reference's Partition{T});
 *  - every array argument lives in the memory space named by `mem`
 *    (SDPSR_MEM_HOST: caller-owned host memory, copied by the library;
 *     SDPSR_MEM_DEVICE: device pointers on ctx's device, used in place);
 *  - scalar outputs (int64_t* etc.) are always host pointers;
 *  - calls on one ctx are serialised on ctx's HIP stream; distinct ctxs (on the same or on
 *    different devices) may be used from distinct host threads; no global state (but the function table of RCCL, filled
 *    once on the first sdpsr_comm_* call); no callbacks;
 *  - ordering of SDPSR_MEM_DEVICE arguments: inputs must be complete when the call is made, or
 *    be produced on a stream that ctx has been told about (sdpsr_set_stream, or
 *    sdpsr_wait_stream right before the call); on return from EVERY entry point the outputs
 *    are complete (the call synchronises ctx's stream before it returns);
 *  - return value: sdpsr_status; details via sdpsr_last_error(ctx).
 */
#ifndef SDPSR_H
#define SDPSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDPSR_VERSION_MAJOR 0
#define SDPSR_VERSION_MINOR 5

typedef struct sdpsr_ctx sdpsr_ctx;
typedef struct sdpsr_problem sdpsr_problem; /* device-resident inputs of the loop, sdpsr_problem_create */

typedef enum sdpsr_status {
    SDPSR_OK = 0,
    /* InvalidDecompositionField, src/eigen_decomposition.jl:140-150,247-253 */
    SDPSR_INVALID_DECOMPOSITION_FIELD = 1,
    /* NumericalInconsistency, src/eigen_decomposition.jl:152-161,264-270 */
    SDPSR_NUMERICAL_INCONSISTENCY = 2,
    /* DimensionMismatch from check_block_sizes, src/diagonalize.jl:1-11 */
    SDPSR_DIMENSION_MISMATCH = 3,
    /* Julia's InexactError on label overflow (src/partitions.jl:29,63).  At the interface: a partition that does not fit the
       width set with sdpsr_set_label_width, sdpsr_labels_convert (see there).  Inside the algorithms only with sdpsr_opts.label_bits = 8 / 16 / 32
       (the width of the reference's label type T): sdpsr_partition_from_* when the class count exceeds typemax(T);
       sdpsr_refine when the largest pair code l1 + l2 (dim(P1) + 1) does (exactly the reference's condition);
       sdpsr_admissible_subspace when dim(S) after a refinement does -- a NECESSARY condition of the reference's
       error there (its intermediate pair code may overflow although the refined dimension fits: the loop never
       forms Part(X) on its own, so that case is not reproduced).  label_bits = 0 (default): never returned,
       labels are uint32 with 64-bit signatures. */
    SDPSR_LABEL_OVERFLOW = 4,
    /* @assert n^2 == length(C) (src/partitions.jl:118), length(values)==dim(P) (:69) ... */
    SDPSR_BAD_ARGUMENT = 5,
    SDPSR_HIP_ERROR = 6,
    SDPSR_SOLVER_ERROR = 7,
    SDPSR_OUT_OF_MEMORY = 8,
    SDPSR_NOT_CONVERGED = 9,
    SDPSR_BAD_STATE = 10
} sdpsr_status;

typedef enum sdpsr_mem { SDPSR_MEM_HOST = 0, SDPSR_MEM_DEVICE = 1 } sdpsr_mem;

/* How the random square of src/partitions.jl:172 is evaluated. */
typedef enum sdpsr_square_mode {
    SDPSR_SQUARE_AUTO = 0, /* = I8 */
    /* exact integers: `channels` independent draws of int8 class values, int8 MFMA,
       int32 accumulate; classes compared by exact equality (no rounding involved) */
    SDPSR_SQUARE_I8 = 1,
    /* exact integers on the fp32 MFMA (|v| <= floor(sqrt(2^24/n)) so every partial sum
       is an exactly representable integer) */
    SDPSR_SQUARE_F32 = 2,
    /* reference-literal: uniform [0,1) doubles, fp64 MFMA, 7-digit rounding
       (src/utils.jl:34-53) */
    SDPSR_SQUARE_F64 = 3
} sdpsr_square_mode;

/* How _clamp_round! / unsafe_round (src/utils.jl:34-53) treats the 7-digit decimal mantissa. */
typedef enum sdpsr_round_mode {
    SDPSR_ROUND_NEAREST = 0, /* default: round to nearest (see sdpsr_clamp_round) */
    SDPSR_ROUND_TRUNC = 1    /* reference-literal: unsafe_trunc(Int, scale * x) / scale */
} sdpsr_round_mode;

/* Behaviour switches (sdpsr_opts.flags).  They replace the environment variables of ABI 0.2: the
   library reads no environment variable that changes results (SDPSR_DEBUG only adds stderr traces). */
enum {
    /* admissible_subspace: two refinements per iteration, as src/partitions.jl:159-174 is written,
       instead of the joint one (see sdpsr_admissible_subspace) */
    SDPSR_FLAG_SEPARATE_REFINEMENTS = 1u << 0,
    /* irreducible_decomposition draws its own generic element (src/eigen_decomposition.jl:306)
       instead of reusing the products T = A2 Q of the isomorphism step */
    SDPSR_FLAG_FRESH_IRREDUCIBLE_ELEMENT = 1u << 1,
    /* module-compression driver: always run the second orthonormalisation step of an absorb */
    SDPSR_FLAG_ALWAYS_REORTHOGONALIZE = 1u << 2,
    /* refinement: signatures always through an array in HBM (no fusion into the insert pass) */
    SDPSR_FLAG_REFINE_NO_FUSE = 1u << 3,
    /* int8 loop: unpack the lower-triangle labels to the full matrix after every refinement */
    SDPSR_FLAG_UNPACK_EVERY_STEP = 1u << 4,
    /* module growth: one label product per generic element instead of one pass for all of a round */
    SDPSR_FLAG_SPMM_ONE_BY_ONE = 1u << 5,
    /* dense driver: never raise the coupling matrix by extra generic elements (reference-literal
       single element, src/eigen_decomposition.jl:259-262) */
    SDPSR_FLAG_SINGLE_COUPLING_ELEMENT = 1u << 6,
    /* compressed problems (order <= 64): eigensolver and Murota's steps in one-workgroup kernels on
       the device instead of on the host inside the read-back the driver makes anyway */
    SDPSR_FLAG_SMALL_EIGEN_ON_DEVICE = 1u << 7,
    /* dense driver: launch the kernels of the tridiagonalisation one by one instead of replaying
       their hipGraph (per-kernel profiles) */
    SDPSR_FLAG_NO_GRAPH = 1u << 8,
    /* admissible_subspace: every round runs the full refinement (insert / rank / label passes); by
       default a round that is expected not to refine -- a confirm round, the first iteration -- first
       compares every entry with the representative of its class and skips the relabel when none differs */
    SDPSR_FLAG_NO_VERIFY_SHORTCUT = 1u << 9,
    /* basis_image: always the projection formula Q_k' 1[P==i] Q_k (src/diagonalize.jl:64-89); by default, when every
       block is 1 x 1, the images are read off as eigenvalues, blks[i][k] = q_k'(1[P==i] x) with x = sum_k q_k, under
       a randomized self-check that falls back to the projection formula (see sdpsr_block_images) */
    SDPSR_FLAG_FULL_BASIS_IMAGE = 1u << 10,
    /* admissible_subspace: run the projection half of every iteration (src/partitions.jl:159-164).  By default, once every
       basis matrix U_k is found constant on the classes of S (checked on the device after a refinement), that half is
       skipped for the rest of the call: x - U U'x of a class-constant x is then class-constant for every x, it cannot
       refine S any more (see sdpsr_admissible_subspace) */
    SDPSR_FLAG_ALWAYS_PROJECT = 1u << 11,
    /* dense driver: the panel form of the tridiagonalisation (two launches per column, rank-64 trailing updates on
       the matrix cores) at every order; by default orders <= 2048 take the one-launch-per-column row form */
    SDPSR_FLAG_SYTRD_PANELS = 1u << 12,
    /* eigen_decomposition: the coupling matrix of the eigenspaces (block norms, src/eigen_decomposition.jl:177-217) is
       always read back and thresholded on the host; by default, from 256 eigenspaces on, its extrema, the histogram
       counts of the Otsu threshold and one bit per pair are formed on the device (same classes) */
    SDPSR_FLAG_COUPLING_ON_HOST = 1u << 13,
    /* dense driver, orders in (2048, 8192]: the panel columns of the tridiagonalisation with ONE launch per column -- the
       product is taken with the unnormalised column, the reflector is finished by the next launch, redundantly in every
       tile (csrc/kernels_sytrd_look.hip).  Same results to rounding; measured slower than the two-launch form on MI355X
       (DESIGN.md 4.1), kept for comparison */
    SDPSR_FLAG_SYTRD_ONE_LAUNCH = 1u << 14,
    /* A/B: every host wait of the loop is a wait for the stream and every verdict is read where it arises (rounds 1-4) --
       no return on the label pass's report, no speculated confirm round, no verdicts deferred to the reduction's later
       waits (round 5).  Same partition, iterations, dimension trajectory and random draws either way. */
    SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT = 1u << 15,
    /* A/B: the guessed-closed path of sdpsr_jordan_reduce never makes or reads the 8-bit shadow of its packed labels: every
       pass streams the 32-bit labels.  By default a reduction that checks the recorded initial partition (<= 255 classes)
       instead of rebuilding it narrows the packed labels to bytes once, and the pair check, the dot-product pass, the
       channel gathers and the verify passes of that and the following restarts stream the bytes.  Same results bit for bit. */
    SDPSR_FLAG_WIDE_LOOP_LABELS = 1u << 16,
    /* A/B: the module growth of blockDiagonalize keeps its scratch the way it did before the small-module route stopped
       needing it: whole-buffer zero fills of the basis, the candidate block and the scratch matrix, the stacked product into
       the scratch matrix and a device copy back behind the basis, the seed vector and its normalisation as two launches, the
       lift's clamp as a pass of its own, and the row-major copy of Q_hat made by sdpsr_block_images.  By default (small
       modules, w <= 64, solved on the host) only the padding rows n .. ld-1 are zeroed, the stacked product is written in
       place, the seed is one launch, and the lift stores Q_hat clamped in both layouts.  Same results bit for bit. */
    SDPSR_FLAG_MODULE_SCRATCH_FILLS = 1u << 17,
    /* A/B: the guessed-closed rounds of the loop (first iteration of an input predicted closed: the joint round and the
       speculated confirm round) form their int8 squares and compare every entry with its class representative, as every
       other round does.  By default those two rounds, which are expected to report "no class splits" and nothing else,
       check X_t^2 against its class constants with a random vector (v'X_t^2 v = v'C_t v, exact integers, one pass over the
       labels, no product; a difference is missed w.p. <= 2^-15 per channel) and form the square only when the check of a
       verdict read inside the loop says "violated".  Same results. */
    SDPSR_FLAG_SQUARE_EVERY_VERDICT = 1u << 18,
    /* A/B: the guessed-closed path of sdpsr_jordan_reduce launches every check whose only product is a verdict word inside the
       loop, in front of blockDiagonalize: the compare of the guessed initial partition, the projection's dot products and
       compare, and the square check's verdict kernels.  By default (no phase timers) they are registered on the ctx and
       enqueued inside blockDiagonalize, behind the two products of the module growth whose read-backs the host waits for, so
       that they run while the host selects directions and solves the compressed problem; every other route enqueues them
       before its own first launch.  Same kernels, keys, stream and order among themselves; same results bit for bit, same
       host waits. */
    SDPSR_FLAG_CHECKS_IN_LOOP = 1u << 19,
    /* A/B: a guessed reduction of sdpsr_jordan_reduce writes the caller's full labels in the loop, in front of blockDiagonalize,
       which reads them there.  By default (device P_out at label width 32, no phase timers, none of SDPSR_FLAG_CHECKS_IN_LOOP /
       _SQUARE_EVERY_VERDICT / _WAIT_FOR_EVERY_VERDICT) the ctx keeps a full copy of the recorded initial partition's labels
       (n^2 * 4 bytes, made once by the unguessed call that makes the record); blockDiagonalize of a guessed reduction, which
       refines nothing, reads that copy, and the square check's class constants and its pass -- the launches that write P_out --
       are enqueued with the other checks inside blockDiagonalize.  With this flag no copy is made.  Same kernels, keys and
       stream; same results bit for bit, same host waits. */
    SDPSR_FLAG_LABELS_BEFORE_BLOCKDIAG = 1u << 20
};

typedef struct sdpsr_opts {
    uint32_t struct_size;   /* = sizeof(sdpsr_opts) */
    int32_t square_mode;    /* sdpsr_square_mode */
    int32_t channels;       /* independent int8 / f32 draws per square step (1..8).  0 = default: 2 channels AND
                               confirm_rounds >= 1 (a false stop needs confirm_rounds + 1 consecutive squares that
                               miss every needed split, each w.p. <= (2/256)^channels: the (2/256)^4 of four
                               channels, at 2 (I + 1) instead of 4 I channel squares for I iterations; the two rounds of
                               a guessed-closed first iteration are judged by the square check, which adds at most
                               2^-15 to a channel's 2/256: <= (2^-7 + 2^-15)^channels per round) */
    int32_t max_iters;      /* 0 = default (10000) */
    int32_t confirm_rounds; /* extra no-change square rounds demanded before stopping (default with channels = 0: 1) */
    int32_t eig_driver;     /* driver of diagonalize: 0 = default (module compression when dim(P) is small against n, else
                               the dense eigensolver: own tridiagonalisation, own tridiagonal divide and conquer, own
                               back-transformation); 4 = dense forced; 5 = dense with rocSOLVER's stedc for the tridiagonal
                               problem; 6 = module compression forced; 1, 2, 3 = rocSOLVER syevd / sytrd + stedc + ormtr /
                               sytrd + steqr + ormtr (comparison only) */
    /* ---- ABI 0.3 (reserved, zero, in 0.2) ---- */
    uint32_t flags;             /* SDPSR_FLAG_* */
    int32_t round_mode;         /* sdpsr_round_mode */
    int32_t basis_image_kernel; /* 0 = by shape, 1 = two-stage (class sums per row), 2 = outer products per class,
                                   3 = sorted chunks with partial sums */
    int32_t refine_path;        /* 0 = by class count (hash tables; beyond 2^18 classes the bucketed grouping), 1 = hash tables
                                   only, 2 = hipCUB radix-sort relabel forced (comparison), 3 = bucketed grouping forced,
                                   4 = as 0 without the one-workgroup-per-CU insert kernel of array sources (comparison), 6 = that kernel
                                   without the workgroups that go first (comparison) */
    int32_t label_bits;         /* 0 = no emulation; 8 / 16 / 32: width of the reference's label type T in
                                   Partition{T} (admissible_subspace defaults to UInt16, src/partitions.jl:84):
                                   SDPSR_LABEL_OVERFLOW where the reference throws InexactError (see below) */
    int32_t insert_wgs_per_cu;  /* measurement knob: resident workgroups per CU of the refinement's insert pass (0 = default) */
    int32_t square_kernel;      /* int8 square of symmetric labels (src/partitions.jl:172): 0 = default (one persistent launch
                                   of 256 x 256 macro-tiles once they fill the chip, 128 x 128 tiles below that), 1 = always
                                   128 x 128 tiles (the launch of ABI 0.3), 64 = always the persistent launch (64-byte K
                                   stages in a ring of four).  Same integers every way. */
    int32_t reserved[3];
} sdpsr_opts;

/* phase_ms slots filled by sdpsr_admissible_subspace / sdpsr_block_diagonalize
   (the reference only prints @timed per phase: src/diagonalize.jl:32-37,
   src/compat.jl:63-65) */
enum {
    SDPSR_T_TOTAL = 0,
    SDPSR_T_PROJECT = 1,   /* randomize + projection + signature */
    SDPSR_T_SQUARE = 2,    /* randomize + N x N square(s) */
    SDPSR_T_REFINE = 3,    /* partition refinement + canonical relabel */
    SDPSR_T_EIGEN = 4,     /* symmetric eigendecomposition */
    SDPSR_T_ISO = 5,       /* Q'AQ, block norms, isomorphism classes */
    SDPSR_T_IRRED = 6,     /* irreducible_decomposition */
    SDPSR_T_IMAGE = 7,     /* basis_image */
    SDPSR_T_COUNT = 8
};

/* ---- lifecycle ------------------------------------------------------------ */
/* opts may be NULL (defaults).  seed drives every random draw of the ctx. */
int sdpsr_create(int device_id, uint64_t seed, const sdpsr_opts* opts, sdpsr_ctx** out);
void sdpsr_destroy(sdpsr_ctx* ctx);
const char* sdpsr_last_error(const sdpsr_ctx* ctx);
const char* sdpsr_status_string(int status);
int sdpsr_version(void);
/* Use an existing HIP stream (hipStream_t) for all work of ctx; NULL = ctx's own. */
int sdpsr_set_stream(sdpsr_ctx* ctx, void* hip_stream);
int sdpsr_synchronize(sdpsr_ctx* ctx);
/* Make all later work of ctx wait for what has been submitted to `hip_stream` (hipStream_t,
   NULL = the legacy default stream) so far: event record + hipStreamWaitEvent, no host wait.
   For device-resident arguments produced by the caller's own kernels. */
int sdpsr_wait_stream(sdpsr_ctx* ctx, void* hip_stream);
/* Hints for the NEXT sdpsr_admissible_subspace call on this ctx (bit mask `yes`):
   bit 0: the columns of U, read as n x n matrices, are symmetric (true whenever the constraint
          matrices A_i are; a host-side setup knows).  With symmetric labels the projection step then
          works on the lower triangle only (half the bytes).  Without it the first iteration's
          dot-product pass carries a randomized symmetry probe (<U_k, W - W'> for a pseudo-random W)
          and later iterations use its verdict.
   bit 1: CL and X0L are symmetric (the reference symmetrises both, src/partitions.jl:128-141): the
          initial partition is formed from the lower triangle.
   A wrong hint is the caller's error (the result is then the partition of the mirrored lower triangle). */
int sdpsr_hint_symmetric_basis(sdpsr_ctx* ctx, int yes);
/* Reseed (tests; independent restarts use distinct seeds per rank).  A call's random draws depend only on the seed
   position (the seed and the draws made since sdpsr_set_seed), the inputs and the opts -- never on earlier calls on
   the ctx: a guess the library takes from its history (the speculated confirm round) changes the work done, not the
   draws, and a reduction repeated after a wrong guess starts again from the seed position of its entry. */
int sdpsr_set_seed(sdpsr_ctx* ctx, uint64_t seed);
/* Dimension trajectory of the last sdpsr_admissible_subspace call on ctx -- what the reference logs under
   verbose (src/partitions.jl:150,156,187-188): dims[0] = dim(S) after S = refine!(Part(CL), Part(X0L)),
   dims[k] = dim(S) at the end of iteration k; *count = iterations + 1 (also when capacity is smaller; at most
   `capacity` entries are written).  Host arrays. */
int sdpsr_dimension_trajectory(sdpsr_ctx* ctx, int64_t* dims, int32_t capacity, int32_t* count);

/* ---- label width: Partition{T <: Integer}, src/partitions.jl:6-11 (admissible_subspace defaults to UInt16, :84) ----
   width, in bits, of every label array this ctx's entry points read or write, in EITHER memory space:
   32 (default) | 16 | 8.  The prototypes keep uint32_t*; with 16 / 8 the caller passes uint16_t* / uint8_t* cast.
   Applies to calls made after it; restarts of a batch call inherit it.  Governed: `labels` of sdpsr_partition_from_f64 / _u32 /
   _u64 (their `in` stays as declared: keys, not labels), sdpsr_partition_checksum, sdpsr_fill, sdpsr_randomize,
   sdpsr_reduce_constraints / _csr; p1, p2 of sdpsr_refine; P of sdpsr_desymmetrize, sdpsr_block_diagonalize / _complex (and its
   P_desym), sdpsr_eigen_decomposition / _batched; P_out of sdpsr_admissible_subspace / _dense / _csr, sdpsr_jordan_reduce /
   _batch, sdpsr_problem_reduce / _batch.
   The label VALUES are those of the 32-bit interface: an array at width B equals the 32-bit array cast to B (same checksum).
   OUTPUT OVERFLOW: an entry point that would deliver a partition of more than 2^B - 1 classes -- the reference's InexactError
   of Partition{T} -- returns SDPSR_LABEL_OVERFLOW with the class count (*nparts, *d1, *dim, *dim_out, *d_desym) set and the
   label output untouched; sdpsr_jordan_reduce / sdpsr_problem_reduce stop behind the loop then, the batch entries report it
   in status[i].  The count is known on the host before any label is delivered: no kernel decides this.
   DEVICE MEMORY at 16 / 8: the work runs on the ctx's own uint32 buffer and the result is narrowed into the caller's array by
   one streaming pass; the in-place arrangements of width 32 (P_out serving blockDiagonalize directly, desymmetrize and refine
   on the caller's buffer) do not apply.  sdpsr_transfer_bytes counts what crosses: len * B / 8 per label array.
   Independent of sdpsr_opts.label_bits, which emulates the reference's overflow INSIDE the algorithms. */
int sdpsr_set_label_width(sdpsr_ctx* ctx, int bits); /* other values: SDPSR_BAD_ARGUMENT, width unchanged */
int sdpsr_label_width(sdpsr_ctx* ctx);               /* 8 / 16 / 32 */
/* element-wise conversion of a label array between two widths (8 / 16 / 32 each), on the device; `in` and `out` in memory space
   mem, must not overlap.  Narrowing a value that does not fit: SDPSR_LABEL_OVERFLOW (contents of out then unspecified, nothing
   outside out[0, len) written).  Independent of the ctx's own width. */
int sdpsr_labels_convert(sdpsr_ctx* ctx, int64_t len, const void* in, int in_bits, void* out, int out_bits, int mem);

/* ---- AbstractPartition contract (primitives) ------------------------------- */
/* Partition{T}(M::AbstractMatrix) float ctor, src/partitions.jl:24-35: classes of
   bit-equal values, labelled by first occurrence in column-major order, +0.0 -> 0. */
int sdpsr_partition_from_f64(sdpsr_ctx* ctx, int64_t len, const double* M,
                             uint32_t* labels, int64_t* nparts, int mem);
/* Integer ctor + __sort_unique!, src/partitions.jl:37-60. in == out allowed. */
int sdpsr_partition_from_u32(sdpsr_ctx* ctx, int64_t len, const uint32_t* in,
                             uint32_t* labels, int64_t* nparts, int mem);
/* The same for 64-bit integer entries (Partition{T}(M::AbstractMatrix{<:Integer}) is generic in the
   entry type; also the canonical relabel of the hash-combined labels of several restarts):
   0 stays 0, every other key is a class of its own value (told apart by a 64-bit mixing hash,
   collision bound as for sdpsr_refine). */
int sdpsr_partition_from_u64(sdpsr_ctx* ctx, int64_t len, const uint64_t* in,
                             uint32_t* labels, int64_t* nparts, int mem);
/* refine!(P1, P2), src/partitions.jl:62-66: p1 <- canonical relabel of the pairs
   (p1, p2); label 0 only where both are 0.  *d1 is updated.
   Classes are told apart by a 64-bit mixing hash of the pair (the reference's exact pair code
   l1 + l2 * (d1 + 1) overflows its label type, src/partitions.jl:63): two distinct pairs collide
   -- and are merged -- with probability ~ d^2 / 2^65 per call (2e-6 at 8M classes, 3e-17 at 34). */
int sdpsr_refine(sdpsr_ctx* ctx, int64_t len, uint32_t* p1, int64_t* d1,
                 const uint32_t* p2, int64_t d2, int mem);
/* Base.:(==)(p::Partition, q::Partition), src/partitions.jl:16-17 (same matrix), as a 128-bit
   position-weighted checksum of the canonical label matrix: equal partitions have equal
   checksums, different ones collide with probability ~2^-64 per word.  Used to agree the result
   of independent restarts across GPUs without moving the n x n labels.
   out[0..1] is host memory; `mem` says where `labels` lives. */
int sdpsr_partition_checksum(sdpsr_ctx* ctx, int64_t len, const uint32_t* labels, uint64_t* out, int mem);
/* fill!(M, P; values), src/partitions.jl:68-75: M[idx] = values[label-1], 0 -> 0.0.
   `values` has d entries. */
int sdpsr_fill(sdpsr_ctx* ctx, int64_t len, const uint32_t* labels, const double* values,
               int64_t d, double* M, int mem);
/* randomize!(M, P), src/abstract_part.jl:107-110: one uniform [0,1) draw per class from
   the ctx's counter-based generator (a fresh stream per call). */
int sdpsr_randomize(sdpsr_ctx* ctx, int64_t len, const uint32_t* labels, double* M, int mem);
/* _clamp_round!, src/utils.jl:34-53; in place.  BEHAVIOURAL DIFFERENCE a Julia caller will see with
   the default round_mode: the reference TRUNCATES the 7-digit decimal mantissa (unsafe_trunc,
   src/utils.jl:49-53), SDPSR_ROUND_NEAREST rounds it to nearest -- the 7th digit differs on about every
   second input.  What the path outputs are the CLASSES of equal rounded values, and those only differ
   for values that sit on an edge of the rule in use: a truncation edge such as 0.0625 = 0.5 * 2^-3 is
   split into two classes by last-bit noise (esc16j: 10712 classes instead of the pinned 150 with
   NumPy's projection arithmetic); nearest rounding keeps them together, hence the default.
   sdpsr_opts.round_mode = SDPSR_ROUND_TRUNC is the reference's rule bit for bit (this primitive, the
   projection step and the fp64 square of the loop, the setup stage of sdpsr_admissible_subspace_dense). */
int sdpsr_clamp_round(sdpsr_ctx* ctx, int64_t len, double* a, double atol, int mem);
/* x .-= projL(x), src/partitions.jl:161 + src/utils.jl:62-66, with qr(A') folded into an
   orthonormal basis U (len x r, column-major) of rowspace(A). */
int sdpsr_project_out(sdpsr_ctx* ctx, int64_t len, double* x, const double* U, int64_t r,
                      int mem);

/* ---- the N x N square, mul!(X2, X, X) src/partitions.jl:172 ----------------- */
/* X symmetric, column-major, leading dimension n. */
int sdpsr_square_f64(sdpsr_ctx* ctx, int64_t n, const double* X, double* X2, int mem);
int sdpsr_square_f32(sdpsr_ctx* ctx, int64_t n, const float* X, float* X2, int mem);
int sdpsr_square_i8(sdpsr_ctx* ctx, int64_t n, const int8_t* X, int32_t* X2, int mem);
/* The square step as the int8 loop runs it: `batch` (1..8) SYMMETRIC n x n int8 matrices (the channel matrices of one
   draw, batch-major; symmetry is the caller's word, as the loop has it from the labels), squared exactly in one launch
   that computes the lower-triangle tiles only (sdpsr_opts.square_kernel picks the kernel); X2 receives the full
   matrices, the upper triangles mirrored.  mul!(X2, X, X), src/partitions.jl:172, for symmetric X. */
int sdpsr_square_i8_symmetric(sdpsr_ctx* ctx, int64_t n, int64_t batch, const int8_t* X, int32_t* X2, int mem);
/* C = A' * B, all column-major fp64: A is k x m (lda), B is k x n (ldb), C m x n (ldc).
   The Q'AQ products of src/eigen_decomposition.jl:203 and the block products of :70. */
int sdpsr_gemm_tn_f64(sdpsr_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* A,
                      int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                      int mem);

/* ---- admissible_subspace, src/partitions.jl:109-190 ------------------------- */
/* Loop :145-185 on the device.  The setup stage (:117-142: qr(A'), C_L, CRAIG x0) stays
   with the caller, which passes
     CL   n x n  reshape(_symmetrize!(_clamp_round!(c - projL(c))), n, n)      (:129-134)
     X0L  n x n  reshape(_clamp_round!(projL(_symmetrize!(craig(A,b)))), n, n) (:137-142)
     U    n^2 x r orthonormal basis of rowspace(A)                              (:124)
   Outputs: P_out (n x n labels), *dim_out, *iters_out, phase_ms[SDPSR_T_COUNT] (may be
   NULL).
   BEHAVIOURAL DIFFERENCE (int8 mode, symmetric labels and basis, <= 4 basis matrices): an
   iteration refines the partition ONCE, by the projected random element and the square of a second
   random element of the same partition together; the reference refines after the projection and
   draws the squared element from the refined partition (:159-174).  Both loops end at the same
   partition (the smallest partition subspace containing C_L and X0 that is closed under the
   projection and under squaring; P_out is canonical, so it is the same matrix); *iters_out counts
   joint steps (equal to the reference-structured count on every test problem).
   sdpsr_opts.flags & SDPSR_FLAG_SEPARATE_REFINEMENTS restores two refinements per iteration.
   In that joint form the projection half of an iteration is SKIPPED once it can no longer refine anything: when every
   basis matrix U_k is constant on every class of the current partition S (compared on the device through the rounding of
   _clamp_round!, :159-164), x - U U'x of any x that is constant on the classes of S is constant on them too -- U_k in
   span(S) implies U U'x in span(S) -- and every finer partition inherits that; generically it holds right after the first
   projection refinement.  TOLERANCE CAVEAT: "constant" is decided on the per-entry rounded codes of U_k (atol, 7 digits: an
   entry |U_k| < atol counts as 0), while the reference rounds x - U U'x AFTER multiplying those differences by the
   coefficients U_k'x (of the order of |x|): differences of U_k inside a class that are below the rounding resolution can
   still split it there.  So the partition returned is the same up to that rounding -- exactly the same whenever the U_k
   take exactly representable values on the classes (constraint matrices with integer entries: every test problem and
   BASELINE config) --, and SDPSR_FLAG_ALWAYS_PROJECT keeps the projection in every iteration.  The check is made at most
   three times per call. */
int sdpsr_admissible_subspace(sdpsr_ctx* ctx, int64_t n, const double* CL, const double* X0L,
                              const double* U, int64_t r, double atol, uint32_t* P_out,
                              int64_t* dim_out, int32_t* iters_out, double* phase_ms, int mem);
/* Convenience for dense problems: the setup stage (:117-142) runs on the DEVICE as well
   (pivoted modified Gram-Schmidt with re-orthogonalisation on the rows of A in place of qr(A'),
   C_L, min-norm x0 = U R^-T b), then the loop.  C: n^2, A: m x n^2 column-major, b: m;
   host pointers (copied by the library).  P_out is in `mem_out`. */
int sdpsr_admissible_subspace_dense(sdpsr_ctx* ctx, int64_t n, int64_t m, const double* C,
                                    const double* A, const double* b, double atol,
                                    uint32_t* P_out, int64_t* dim_out, int32_t* iters_out,
                                    double* phase_ms, int mem_out);

/* ---- setup from a sparse constraint matrix, src/partitions.jl:117-142, src/utils.jl:58-66 ------------------
   The setup stage of admissible_subspace (qr(A') at :124, C_L at :129-134, Krylov.craig's min-norm x0 and X0_L at
   :137-142, projL of src/utils.jl:58-66) for an A given as CSR -- the form of every SDP a user builds (the reference's
   own QAP relaxation, test/sd_problems.jl:63-92, is (2n+1) x n^4 with 2n + 1 + n^4 + 2 n^3 nonzeros).
     rowptr[m + 1], colind[nnz], val[nnz], b[m], C[n^2]: host memory.  colind = the column-major linear index into the
       n x n matrix (the reference's vec), index_base 0 or 1: with 1 a Julia caller passes sparse(A')'s colptr / rowval /
       nzval unchanged (the CSC arrays of A' are the CSR arrays of A).  Unsorted columns, duplicates (summed, in input
       order) and explicit zeros are accepted.  m = 0: L is the whole space.
     A bad rowptr[0], a non-monotone rowptr, an index outside [0, n^2) after the base is subtracted or a non-finite
     value: SDPSR_BAD_ARGUMENT before any kernel runs; n^2 x m doubles that do not fit the device: SDPSR_OUT_OF_MEMORY.
     The ctx stays usable after either.
   On the device: A's rows are densified into the columns of one n^2 x m buffer that becomes U in place; G = A A' (one
   tall-skinny Gram kernel, any m) decides by a pivoted Cholesky on the host: every pivot's residual norm >= 1e-4 of
   the largest row norm -> CholeskyQR2 (two Gram passes, two in-place triangular right-multiplications, two host
   waits), else the pivoted MGS of sdpsr_admissible_subspace_dense (rank decided at 1e-12 of the largest row norm).
   sdpsr_admissible_setup_csr: CL, X0L (n^2, column-major) and U (n^2 x r, column-major; capacity n^2 x m) in memory
     space mem_out; *r_out = r; *hint_out = the bits of sdpsr_hint_symmetric_basis the library has proved (3 when every
     row of A is a symmetric n x n matrix bit for bit -- every kernel of the stage does the same arithmetic for entry
     (i, j) as for (j, i) --, else 0); *info_out = sdpsr_setup_path (may be NULL).
   sdpsr_admissible_subspace_csr: the same stage, then the loop of sdpsr_admissible_subspace with those hint bits --
     the CSR twin of sdpsr_admissible_subspace_dense.  P_out is in mem_out. */
typedef enum sdpsr_setup_path {
    SDPSR_SETUP_NO_CONSTRAINTS = 0, /* m = 0 */
    SDPSR_SETUP_CHOLESKY_QR2 = 1,   /* rows clearly independent: CholeskyQR2 */
    SDPSR_SETUP_MGS = 2             /* otherwise: pivoted modified Gram-Schmidt */
} sdpsr_setup_path;
int sdpsr_admissible_setup_csr(sdpsr_ctx* ctx, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* colind,
                               const double* val, int index_base, const double* b, const double* C, double atol,
                               double* CL, double* X0L, double* U, int64_t* r_out, int* hint_out, int32_t* info_out,
                               int mem_out);
int sdpsr_admissible_subspace_csr(sdpsr_ctx* ctx, int64_t n, int64_t m, const int64_t* rowptr, const int64_t* colind,
                                  const double* val, int index_base, const double* b, const double* C, double atol,
                                  uint32_t* P_out, int64_t* dim_out, int32_t* iters_out, double* phase_ms, int mem_out);

/* ---- desymmetrize(P) / unSymmetrize, src/partitions.jl:197-223, src/compat.jl:70 -------------- */
/* WL-type refinement with products X*Y of two independent random elements until the dimension
   stalls: P (n x n labels) is refined in place, *dim updated, *iters (may be NULL) = rounds.
   The products are evaluated exactly (int8 channels), like the squares of admissible_subspace. */
int sdpsr_desymmetrize(sdpsr_ctx* ctx, int64_t n, uint32_t* P, int64_t* dim, int32_t* iters, int mem);

/* ---- reduced-SDP assembly, README.md:57-60, test/sd_problems.jl:32-37 ------------------------- */
/* out = A * PMat with PMat = hcat(vec(P.matrix .== i) for i = 1:d): the columns of A summed per
   class.  A: m x len column-major (dense), labels: len, out: m x d column-major.  C' * PMat is the
   m = 1 case.  The accumulators live in LDS: (d + 1) * min(m, 64) doubles must fit 60 KiB, else SDPSR_BAD_ARGUMENT; a
   sparse A, or a larger d, goes to sdpsr_reduce_constraints_csr. */
int sdpsr_reduce_constraints(sdpsr_ctx* ctx, int64_t len, const uint32_t* labels, int64_t d, int64_t m,
                             const double* A, double* out, int mem);
/* The same product for a sparse A given as CSR and any d: newA = A * PMat, newC = C' * PMat (README.md:57-60,
   test/sd_problems.jl:32-37,113-118, docs/src/examples/ReduceAndSolveJuMP.jl:42-51) without a dense copy of A anywhere.
     rowptr[m + 1], colind[nnz], val[nnz]: host memory, exactly the conventions of sdpsr_admissible_setup_csr (colind =
       column-major linear index into [0, len), index_base 0 or 1 -- with 1 a Julia caller passes sparse(A')'s colptr /
       rowval / nzval unchanged; unsorted columns, duplicates (summed, in input order) and explicit zeros are accepted)
       and the same validation: malformed CSR is SDPSR_BAD_ARGUMENT before any kernel runs.
     labels[len] with values 0 .. d (0: no column) and out (m x d column-major) live in the memory space `mem`.
   out[r, i - 1] = the sum of val over the entries of row r whose column carries label i; a pair (r, i) without such an
   entry gets exactly 0.0 -- every element of out is written.  C' * PMat is the m = 1 case; m = 0 and nnz = 0 are legal.
   Any 1 <= d <= len: nothing but out itself grows with d.  An output or workspace (28 bytes per non-zero) that does not
   fit the device: SDPSR_OUT_OF_MEMORY.  The entries are indexed with 32 bits: nnz >= 2^32 is SDPSR_BAD_ARGUMENT.  A label
   > d: SDPSR_BAD_ARGUMENT ("a label exceeds d"), found by a flag -- such a label never indexes anything.  The ctx stays
   usable after each of these.
   REPRODUCIBLE BITS: the entries of a (row, class) pair are added in an order that depends on the inputs alone (no
   floating-point atomics; DESIGN.md "A * PMat from a sparse A"), so equal calls return equal bits on any ctx. */
int sdpsr_reduce_constraints_csr(sdpsr_ctx* ctx, int64_t len, const uint32_t* labels, int64_t d, int64_t m,
                                 const int64_t* rowptr, const int64_t* colind, const double* val, int index_base,
                                 double* out, int mem);

/* ---- a device-resident sparse A: canonicalise once, on the device; use it for the setup stage and for A * PMat ------
   The constraint matrix enters a work flow twice -- the setup stage (src/partitions.jl:117-142, projL of
   src/utils.jl:58-66) and newA = A * PMat (README.md:57-60, docs/src/examples/ReduceAndSolveJuMP.jl:42-51) -- and each
   _csr entry above validates and canonicalises it on one host thread and uploads it again.  A sdpsr_sparse handle holds
   the canonical CSR form in device memory (upload once, use many times: the idiom of sdpsr_problem), made by a canonical
   pass that runs ON THE DEVICE from host or device arrays.
   sdpsr_sparse_create (src/partitions.jl:117-142, README.md:57-60): rowptr[m + 1], colind[nnz], val[nnz] live in `mem`;
     device arrays are read where they lie and never modified, the handle aliases none of them.  Exactly the conventions
     of sdpsr_admissible_setup_csr (colind = column-major linear index, index_base 0 or 1, unsorted columns, duplicates
     and explicit zeros accepted, m = 0 and nnz = 0 legal).  nnz is passed explicitly (the host cannot read a device
     rowptr[m]); rowptr[m] - index_base != nnz is SDPSR_BAD_ARGUMENT.
     The canonical form is the host pass's, bit for bit on every input: rows sorted by column, duplicates summed in input
     order (s = v0; s += v1; ...), every v == 0.0 of either sign dropped, uint32 columns.  The verdicts and messages are
     the host pass's too, all SDPSR_BAD_ARGUMENT: "rowptr[0] != index_base", "rowptr is not monotone at row i" (the lowest
     i), "column index out of [0, n^2) at entry p" / "non-finite value at entry p" (the lowest offending p of either kind,
     the column message at equal p), "duplicate entries sum to a non-finite value", index_base outside {0, 1}, a NULL
     array with nnz > 0, nnz >= 2^32, m >= 2^31, a len outside [1, 2^32 - 16).  *out stays NULL then, nothing is leaked,
     the ctx stays usable.  The handle owns (m + 1) * 8 + nnz_canonical * 12 bytes of device memory (SDPSR_OUT_OF_MEMORY
     when they do not fit); the workspace (7 bytes per raw entry, 51 when some row needs the sort, 16 more for the raw copies of
     host arrays) belongs to the ctx.  Three host
     waits.  sdpsr_transfer_bytes, host arrays: (m + 1) * 8 + nnz * 16 bytes up and 216 bytes of verdict words down; device
     arrays: nothing up.  Like sdpsr_problem the handle is read-only after creation, any ctx of that device may use it,
     and the caller destroys it after the last call that names it.
   sdpsr_sparse_info: len, m, the canonical entry count, and rows_symmetric = 1 when len is a perfect square n^2 and
     every canonical row is a symmetric n x n matrix bit for bit (the predicate behind hint_out = 3 of the setup entries).
   sdpsr_sparse_export: the canonical arrays as int64 / int64 / double with index_base, rowptr[m + 1], colind / val
     [nnz_canonical] in `mem` -- they go into the _csr entries, or into sdpsr_sparse_create again, as they are.
   sdpsr_admissible_setup_sparse / sdpsr_admissible_subspace_sparse (src/partitions.jl:117-142, src/utils.jl:58-66): the
     stage of sdpsr_admissible_setup_csr / _subspace_csr on the handle's arrays; n * n must equal the handle's len, its m
     is the row count; b and C are host memory.  Every kernel of the stage sees the same inputs with the same launch
     geometry as behind the host pass: the outputs equal those of the _csr entry on the same raw arrays bit for bit.
   sdpsr_reduce_constraints_sparse (README.md:57-60, docs/src/examples/ReduceAndSolveJuMP.jl:42-51): the assembly of
     sdpsr_reduce_constraints_csr on the handle's arrays, labels[len] and out (m x d) in `mem`; equal bits likewise. */
typedef struct sdpsr_sparse sdpsr_sparse; /* canonical CSR of an m x len matrix, resident on ctx's device */
int sdpsr_sparse_create(sdpsr_ctx* ctx, int64_t len, int64_t m, int64_t nnz, const int64_t* rowptr, const int64_t* colind,
                        const double* val, int index_base, int mem, sdpsr_sparse** out);
int sdpsr_sparse_destroy(sdpsr_sparse* A);
int sdpsr_sparse_info(const sdpsr_sparse* A, int64_t* len, int64_t* m, int64_t* nnz_canonical, int* rows_symmetric);
int sdpsr_sparse_export(sdpsr_ctx* ctx, const sdpsr_sparse* A, int index_base, int64_t* rowptr, int64_t* colind, double* val,
                        int mem);
int sdpsr_admissible_setup_sparse(sdpsr_ctx* ctx, int64_t n, const sdpsr_sparse* A, const double* b, const double* C,
                                  double atol, double* CL, double* X0L, double* U, int64_t* r_out, int* hint_out,
                                  int32_t* info_out, int mem_out);
int sdpsr_admissible_subspace_sparse(sdpsr_ctx* ctx, int64_t n, const sdpsr_sparse* A, const double* b, const double* C,
                                     double atol, uint32_t* P_out, int64_t* dim_out, int32_t* iters_out, double* phase_ms,
                                     int mem_out);
int sdpsr_reduce_constraints_sparse(sdpsr_ctx* ctx, const sdpsr_sparse* A, const uint32_t* labels, int64_t d, double* out,
                                    int mem);

/* ---- removing the linearly dependent reduced constraints, docs/src/examples/ReduceAndSolveJuMP.jl:44-50 ----
   ("Removing linearly dependent constraints", docs/src/examples/QuadraticAssignmentProblems.jl:116-122)
     newConstraints = hcat(A * PMat, b)
     newConstraints = sparse(svd(Matrix(newConstraints)').U[:, 1:rank(newConstraints)]');  droptol!(newConstraints, 1e-8)
   M = [newA | b] is m x ncols, ncols = d + 1 (d when b == NULL: newA alone).  newA: m x d, column-major -- what the three
   sdpsr_reduce_constraints* entries write -- in `mem`; b: m doubles, HOST memory, may be NULL; out: m x ncols, column-major
   with leading dimension m, in `mem`, never aliasing newA.  1 <= m <= 1024 (m = 0: nothing to do, rank 0); m > ncols is fine.
     rows 0 .. r-1 of out   an orthonormal basis of rowspace(M): row k is the right singular vector of M for its k-th largest
                            singular value (the rows of svd(M').U[:, 1:r]'; within a repeated singular value any orthonormal
                            basis of its space), normalised, its sign fixed so that its first entry of largest magnitude is
                            positive, and every entry with |v| <= droptol set to exactly 0.0 afterwards (droptol!; 0 keeps all)
     rows r .. m-1 of out   exactly 0.0 -- every element of out is written
     *rank_out = r          the number of singular values > rtol * sigma_1; rtol = 0: Julia's dense rank(M) default
                            min(m, ncols) * eps.  rtol < 0, NaN or Inf, droptol < 0 or NaN: SDPSR_BAD_ARGUMENT
     sv                     m doubles, host memory, may be NULL: all computed singular values, descending
     *nnz_out               may be NULL: the non-zeros left in rows 0 .. r-1 after the drop (sizes a sparse copy)
     *passes_out            may be NULL: outer passes made (Gram matrix on the device, Jacobi rotations of it on the host, rows
                            rotated on the device; DESIGN.md "Dependent reduced constraints"); host waits: passes + 1, and for m > 64
                            one more per rotating pass (the upload of the rotations)
   A non-finite entry of newA or b: SDPSR_BAD_ARGUMENT ("non-finite value"), out untouched.  An all-zero M: r = 0, SDPSR_OK.
   Pass limit (16) reached: SDPSR_NOT_CONVERGED, every output written as it stands.  Every sum has an order fixed by
   (m, ncols) and there are no floating-point atomics: equal inputs give equal bytes, on any ctx.  The ctx stays usable
   after every error. */
int sdpsr_compress_constraints(sdpsr_ctx* ctx, int64_t m, int64_t d, const double* newA, const double* b, double rtol,
                               double droptol, double* out, int64_t* rank_out, double* sv, int64_t* nnz_out,
                               int32_t* passes_out, int mem);

/* ---- blockDiagonalize, src/compat.jl:46-68 ---------------------------------- */
/* Phase 1 = diagonalize(Float64, P; atol=epsilon) (src/diagonalize.jl:25-40) +
   check_block_sizes (:1-11).  Keeps Q_hat on the device inside ctx.
   Outputs: *nblocks, *sum_sq = sum_k s_k^2, *sum_s = sum_k s_k. */
int sdpsr_block_diagonalize(sdpsr_ctx* ctx, int64_t n, const uint32_t* P, int64_t d,
                            double epsilon, int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s,
                            double* phase_ms, int mem);
/* blkSizes of the last phase 1 that got as far as check_block_sizes (host array of nblocks ints). */
int sdpsr_block_sizes(sdpsr_ctx* ctx, int32_t* blk_sizes);
/* Q_hat = diagonalize(Float64, P; atol) itself (src/diagonalize.jl:25-40), n x sum_s column-major,
   blocks side by side: available after sdpsr_block_diagonalize returned OK or
   SDPSR_DIMENSION_MISMATCH (diagonalize does not run check_block_sizes, src/compat.jl:60 does). */
int sdpsr_q_hat(sdpsr_ctx* ctx, double* Q_hat, int mem);
/* Phase 2 = basis_image(Q_hat, P) (src/diagonalize.jl:64-89).
   BEHAVIOURAL NOTE (commutative algebras, every block 1 x 1): Q_hat from Murota's decomposition spans invariant
   subspaces, 1[P==i] q_k = blks[i][k] q_k, so the images are obtained from the class sums of ONE vector x = sum_k q_k
   (n^2 label reads) instead of all sum_k s_k columns; a second vector with random signs goes through the same pass and
   the two answers must agree to 2e-10, else -- and always with SDPSR_FLAG_FULL_BASIS_IMAGE -- the projection formula
   Q_k' 1[P==i] Q_k is evaluated as the reference does.  Both give Q_k' 1[P==i] Q_k up to rounding (tests: 1e-9).
   blks: d * sum_sq doubles, class-major, then block, each block column-major s_k x s_k.
   Q_hat (optional, may be NULL): n x sum_s column-major, blocks side by side. */
int sdpsr_block_images(sdpsr_ctx* ctx, double* blks, double* Q_hat, double* phase_ms, int mem);
/* basis_image(Q, P; atol), src/diagonalize.jl:64-89 (_constraints :42-50), for a caller's Q_hat and the classes
   class_first .. class_first + class_count - 1 (1-based): blks[i][k] = Q_k' 1[P==i] Q_k for the classes i of that window.
   The Q_hat that sdpsr_comm_broadcast delivered to every rank becomes images here, each rank taking its own window; a large
   output is taken window by window.
     P            n x n labels at the ctx's label width (sdpsr_set_label_width), in `mem`; must be symmetric;
     d            dim(P);
     blk_sizes    host array of nblocks sizes s_k >= 1, sum s_k <= n;
     Q_hat        n x sum s_k column-major, blocks side by side, in `mem`.  ARBITRARY: neither orthonormal columns nor
                  invariant subspaces are assumed.  The shortcuts of sdpsr_block_images still run, because their checks
                  are exact about cross terms: a Q they do not hold for fails the check and gets the projection formula;
     blks         class_count * sum s_k^2 doubles in `mem`: class-major starting at class_first, then block, each block
                  column-major (the layout of sdpsr_block_images).  Nothing outside those elements is written;
     atol         entries below it in absolute value become 0; atol < 0: the reference's default 1e-12 * n; 0: no clamp;
     route        (may be NULL) what produced the output: SDPSR_BI_ROUTE_COMMUTATIVE .. _CHUNK, or-ed with
                  SDPSR_BI_ROUTE_REPAIRED when a shortcut recomputed some columns / blocks by the projection formula, with
                  SDPSR_BI_ROUTE_SHORTCUT_REFUSED when a shortcut ran, failed its check and a kernel route produced everything;
     phase_ms     (may be NULL) as sdpsr_block_images fills it.
   opts.basis_image_kernel and SDPSR_FLAG_FULL_BASIS_IMAGE apply as they do to sdpsr_block_images.  On the three kernel routes a
   window's output equals, bit for bit, the same slice of the full call (every class is summed on its own, in a fixed order);
   the shortcuts draw a fresh key per call and agree to rounding (their checks accept 2e-10 absolute, as in sdpsr_block_images:
   meant for columns of norm <= 1; SDPSR_FLAG_FULL_BASIS_IMAGE evaluates the projection formula for everything).
   The ctx's block diagonalisation (sdpsr_block_sizes / sdpsr_q_hat / sdpsr_block_images) is neither needed nor disturbed.
   SDPSR_BAD_ARGUMENT, before any kernel and with the ctx usable afterwards: a NULL pointer, n < 1, d < 0, nblocks < 1, some
   s_k < 1, sum s_k > n, class_count < 0, class_first < 1 or a window that ends beyond d.  class_count == 0 is legal: SDPSR_OK,
   nothing written, no kernel launched (a split over more ranks than classes).  Found on the device, in the pass that brings
   the labels in: "partition is not symmetric" and "a label exceeds d" (SDPSR_BAD_ARGUMENT; host blks: nothing is delivered,
   device blks: the window's contents are unspecified).  Labels outside the window -- of any value -- are read as the skipped
   class 0 where they are loaded and index nothing.
   sdpsr_transfer_bytes, host arrays: n^2 * B / 8 + n * sum s_k * 8 bytes up at label width B, class_count * sum s_k^2 * 8 down
   (the routes' descriptor words are not counted by this entry); device arrays: nothing up, the 8 bytes of the two verdicts down. */
enum {
    SDPSR_BI_ROUTE_COMMUTATIVE = 1,
    SDPSR_BI_ROUTE_BLOCKS = 2,
    SDPSR_BI_ROUTE_TWO_STAGE = 3,
    SDPSR_BI_ROUTE_OUTER = 4,
    SDPSR_BI_ROUTE_CHUNK = 5,
    SDPSR_BI_ROUTE_REPAIRED = 0x100,
    SDPSR_BI_ROUTE_SHORTCUT_REFUSED = 0x200
};
int sdpsr_basis_image(sdpsr_ctx* ctx, int64_t n, const uint32_t* P, int64_t d, int32_t nblocks, const int32_t* blk_sizes,
                      const double* Q_hat, int64_t class_first, int64_t class_count, double atol, double* blks, int32_t* route,
                      double* phase_ms, int mem);
/* ---- one reduction in one call ---------------------------------------------------------------------
   sdpsr_admissible_subspace followed by sdpsr_block_diagonalize on its result and -- when the images fit the
   caller's buffer -- sdpsr_block_images, with the partition staying on the device and no host synchronisation
   between the stages (the separate entry points each return with their outputs complete).  Same arguments and
   meaning as those three; `mem` names the memory space of CL / X0L / U / P_out / blks / Q_hat.
     P_out           n x n labels, may be NULL (the partition is then only kept inside ctx for sdpsr_block_images);
     blks            d * sum_sq doubles if that is <= blks_capacity (in doubles), else untouched: the caller reads
                     *dim_out * *sum_sq, allocates and calls sdpsr_block_images; blks_capacity = 0: sizes only;
     Q_hat           n * sum_s doubles under the same rule with qhat_capacity; may be NULL.
   With device-resident P_out the partition is formed in the caller's buffer (no copy).  A reduction that guesses its input
   closed may write P_out late, inside blockDiagonalize, which then reads the ctx's own copy of the same labels
   (SDPSR_FLAG_LABELS_BEFORE_BLOCKDIAG); whenever the call returns -- successfully, with an error, or after a voided guess
   and its repeat -- everything it registered has been enqueued and waited for, and P_out holds the complete labels of the
   partition the call reports.  Once this call has
   delivered the images itself, a further sdpsr_block_images needs a new sdpsr_block_diagonalize (sizes and Q_hat stay
   available through sdpsr_block_sizes / sdpsr_q_hat).
   Status: that of the first stage that fails.  After SDPSR_NUMERICAL_INCONSISTENCY / SDPSR_DIMENSION_MISMATCH
   (the randomized failures of blockDiagonalize, "try again" in the reference) the partition outputs are valid and
   the caller retries with sdpsr_block_diagonalize on them; SDPSR_NOT_CONVERGED is reported after the other stages ran. */
int sdpsr_jordan_reduce(sdpsr_ctx* ctx, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r,
                        double atol, double epsilon, uint32_t* P_out, int64_t* dim_out, int32_t* iters_out,
                        int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* blks, int64_t blks_capacity,
                        double* Q_hat, int64_t qhat_capacity, double* phase_ms, int mem);

/* R independent random restarts of the same reduction in ONE call on ONE host thread (1 <= R <= 64): restart i runs
   sdpsr_jordan_reduce with its own random streams (seeds[i]; seeds == NULL: the ctx's own stream for restart 0, derived
   seeds for the others), its own HIP stream and its own workspace inside ctx.  While one restart's host side waits for a
   verdict from the device (the reference's loop has one per refinement, src/partitions.jl:154-185), the calling thread
   submits the other restarts' work: on one MI355X two restarts in flight finish 1.4-1.5 x the reductions per second of
   one at a time.  These are the "independent random restarts" of the multi-GPU north-star on the per-GPU side, and the
   reference's own answer to the randomized failures of blockDiagonalize ("try again", src/eigen_decomposition.jl:264-270,
   src/diagonalize.jl:4-9): the caller takes the first restart whose status[i] is SDPSR_OK.
     CL, X0L, U      shared by all restarts (same problem), in memory space `mem`;
     P_out, blks     arrays of R pointers (each as in sdpsr_jordan_reduce; P_out or blks or single entries may be NULL),
                     blks_capacity[R] in doubles; Q_hat is not delivered here (sdpsr_q_hat of a single-restart call);
     dim_out .. sum_s  arrays of R entries (iters_out, nblocks, sum_sq, sum_s may be NULL);
     status[R]       per restart, the status sdpsr_jordan_reduce would have returned.
   Returns SDPSR_OK if every restart did, else the first restart's failure.  A hint given with
   sdpsr_hint_symmetric_basis applies to all R restarts, and so does the ordering of ctx's stream (sdpsr_wait_stream,
   sdpsr_set_stream): every restart's stream starts behind what ctx's stream has been ordered behind.  No threads are created; do not call it from two host threads
   on one ctx. */
int sdpsr_jordan_reduce_batch(sdpsr_ctx* ctx, int32_t R, const uint64_t* seeds, int64_t n, const double* CL, const double* X0L,
                              const double* U, int64_t r, double atol, double epsilon, uint32_t* const* P_out, int64_t* dim_out,
                              int32_t* iters_out, int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* const* blks,
                              const int64_t* blks_capacity, int32_t* status, int mem);
/* (With host arrays, mem = SDPSR_MEM_HOST, C_L / X0_L / U are uploaded ONCE for all R restarts -- into ctx's own input
   buffers -- not once per restart.) */
/* blkSizes (nblocks[restart] ints) of restart `restart` of the last batch call on ctx whose status[restart] was SDPSR_OK or
   SDPSR_DIMENSION_MISMATCH -- sdpsr_block_sizes for a restart. */
int sdpsr_batch_block_sizes(sdpsr_ctx* ctx, int32_t restart, int32_t* blk_sizes);

/* ---- upload once, reduce many times ----------------------------------------------------------------
   The reference's seam hands host arrays to admissible_subspace on every call (src/partitions.jl:109-116); a caller
   who restarts the randomized reduction of ONE problem many times (the reference's "try again",
   src/eigen_decomposition.jl:264-270, the multi-GPU restarts) pays the upload of C_L, X0_L and U -- 3 x 134 MB at
   N = 4096, ~9 ms against a 0.8 ms reduction -- on each of them.  A problem handle holds the three arrays on ctx's
   device: created once (mem names where CL / X0L / U live; device-resident inputs are COPIED, the caller's buffers are
   free on return), used by any number of sdpsr_problem_reduce / sdpsr_problem_reduce_batch calls of ctxs on that
   device, read-only, destroyed by the caller (after the last call that names it has returned).
     hint    bits of sdpsr_hint_symmetric_basis that hold for these inputs (they then apply to every reduction);
     mem_out where P_out / blks / Q_hat live; everything else as in sdpsr_jordan_reduce / sdpsr_jordan_reduce_batch.
   A Julia caller holding AMDGPU.jl arrays passes their device pointers with SDPSR_MEM_DEVICE. */
int sdpsr_problem_create(sdpsr_ctx* ctx, int64_t n, const double* CL, const double* X0L, const double* U, int64_t r, int hint,
                         int mem, sdpsr_problem** out);
int sdpsr_problem_destroy(sdpsr_problem* problem);
int sdpsr_problem_reduce(sdpsr_ctx* ctx, const sdpsr_problem* problem, double atol, double epsilon, uint32_t* P_out,
                         int64_t* dim_out, int32_t* iters_out, int32_t* nblocks, int64_t* sum_sq, int64_t* sum_s, double* blks,
                         int64_t blks_capacity, double* Q_hat, int64_t qhat_capacity, double* phase_ms, int mem_out);
int sdpsr_problem_reduce_batch(sdpsr_ctx* ctx, const sdpsr_problem* problem, int32_t R, const uint64_t* seeds, double atol,
                               double epsilon, uint32_t* const* P_out, int64_t* dim_out, int32_t* iters_out, int32_t* nblocks,
                               int64_t* sum_sq, int64_t* sum_s, double* const* blks, const int64_t* blks_capacity,
                               int32_t* status, int mem_out);
/* Bytes ctx (and the restarts' ctxs inside it) has moved host -> device / device -> host since its creation: what a
   caller of the host-array interface pays on PCIe (tests: a 4-restart batch uploads what one call uploads).  A label array
   counts len * B / 8 bytes at label width B (sdpsr_set_label_width).  Since the label widths were added the host label upload
   of sdpsr_block_diagonalize and the label upload / P_desym download of sdpsr_block_diagonalize_complex are counted too, at
   every width (they crossed uncounted before). */
int sdpsr_transfer_bytes(sdpsr_ctx* ctx, uint64_t* h2d, uint64_t* d2h);

/* ---- blockDiagonalize(P; complex = true), src/compat.jl:26-32,46-68 with T = ComplexF64 ---------
   diagonalize(ComplexF64, P) = desymmetrize (src/diagonalize.jl:26-28) + Murota's decomposition
   over C + check_block_sizes with sum s_k^2 == dim(P) (:13-23); the partition handed to
   basis_image is the desymmetrized one (src/compat.jl:54-57).
   n <= 64: every step in single-workgroup kernels (the reference's own complex tests are 3 x 3
   and 4 x 4, test/runtests.jl:43-57).  64 < n <= 4096: the Hermitian elements go through their real
   symmetric embedding (2n x 2n: the real dense eigensolver and the fp64 MFMA GEMMs; eigenspaces
   are extracted per eigenvalue cluster, SDPSR_NUMERICAL_INCONSISTENCY if a cluster does not
   split evenly).  Larger n: SDPSR_BAD_ARGUMENT.
   BEHAVIOURAL DIFFERENCE: the generic elements are Hermitian (A + A^H with complex class
   coefficients) and the eigensolver is a Hermitian Jacobi iteration, where the reference hands a
   general complex element to eigen(); block sizes and block spectra are the same.
   P_desym (optional, n x n labels in `mem`) / *d_desym: the desymmetrized partition whose classes
   index the block images. */
int sdpsr_block_diagonalize_complex(sdpsr_ctx* ctx, int64_t n, const uint32_t* P, int64_t d, double epsilon,
                                    uint32_t* P_desym, int64_t* d_desym, int32_t* nblocks, int64_t* sum_sq,
                                    int64_t* sum_s, int mem);
int sdpsr_block_sizes_complex(sdpsr_ctx* ctx, int32_t* blk_sizes);
/* blks: d_desym * sum_sq complex numbers as (re, im) pairs, class-major, then block, each block
   column-major s_k x s_k.  Q_hat (optional): n x sum_s complex, (re, im) pairs, column-major. */
int sdpsr_block_images_complex(sdpsr_ctx* ctx, double* blks, double* Q_hat, int mem);
/* basis_image(Q, P; atol) over ComplexF64, src/diagonalize.jl:64-89 (_constraints :42-50) as blockDiagonalize(P; complex = true)
   calls it with the desymmetrized partition (src/compat.jl:54-57), for a caller's Q_hat and the classes class_first ..
   class_first + class_count - 1 (1-based): blks[i][k] = Q_k^H 1[P==i] Q_k, i.e.
   blks[i][k][a,b] = sum over the entries (r,c) with P[r,c] == i of conj(Q_k[r,a]) * Q_k[c,b].
   The complex counterpart of sdpsr_basis_image: the complex Q_hat that sdpsr_comm_broadcast delivered to every rank becomes
   images here, each rank taking its own window; a large output is taken window by window.
     P            n x n labels at the ctx's label width (sdpsr_set_label_width), column-major, in `mem`.  NOT required to be
                  symmetric (desymmetrized partitions are not); label 0 is skipped;
     d            dim(P);
     blk_sizes    host array of nblocks sizes s_k >= 1, sum s_k <= n;
     Q_hat        n x sum s_k complex numbers as (re, im) pairs, column-major, blocks side by side, in `mem` (the layout
                  sdpsr_block_images_complex writes).  ARBITRARY: neither orthonormal columns nor invariant subspaces are assumed;
     blks         class_count * sum s_k^2 complex numbers as (re, im) pairs in `mem`: class-major starting at class_first, then
                  block, each block column-major (the layout of sdpsr_block_images_complex).  Nothing outside those elements
                  is written;
     atol         entries with |z| < atol (the complex magnitude, strict <, as clamptol does with abs, src/utils.jl:14-16) become
                  0 + 0i; atol < 0: the reference's default 1e-12 * n; 0: no clamp;
     route        (may be NULL) SDPSR_BI_ROUTE_OUTER or SDPSR_BI_ROUTE_CHUNK: the kernels that produced the output;
     phase_ms     (may be NULL) as sdpsr_block_images fills it.
   Routes.  There are no shortcuts over C, so SDPSR_FLAG_FULL_BASIS_IMAGE has no effect here.  opts.basis_image_kernel = outer or
   chunk forces that route (outer covers blocks up to 128 x 128; with a larger block a forced `outer` runs `chunk` and *route
   says so); two_stage is treated as auto (the real two-stage kernels rely on a symmetric partition).  The automatic choice is
   a function of (n, d, the block sizes) alone, never of the window: an average class below 4096 entries and every block within
   what the outer kernel supports gives outer, else chunk.
   A window's output equals, bit for bit, the same slice of the full call, on both routes and under auto; equal inputs give
   equal bits on any ctx and any seed (no random numbers, no floating-point atomics, every class summed on its own in a fixed
   order).  The ctx's block diagonalisations and what sdpsr_basis_image keeps are neither needed nor disturbed:
   sdpsr_block_images_complex, sdpsr_block_images and sdpsr_basis_image behave after this call exactly as before it.
   SDPSR_BAD_ARGUMENT, before any kernel, with nothing written and the ctx usable afterwards: a NULL pointer, n < 1, d < 0,
   nblocks < 1, some s_k < 1, sum s_k > n, class_count < 0, class_first < 1 or a window that ends beyond d.  class_count == 0 is
   legal: SDPSR_OK, nothing written, no kernel launched.  Found on the device, in the pass that brings the labels in: "a label
   exceeds d" (SDPSR_BAD_ARGUMENT; host blks: nothing is delivered, device blks: the window's contents are unspecified).
   Labels outside the window -- of any value -- are read as the skipped class 0 where they are loaded and index nothing.
   sdpsr_transfer_bytes, host arrays: n^2 * B / 8 + n * sum s_k * 16 bytes up at label width B, class_count * sum s_k^2 * 16 down
   (the routes' descriptor words are not counted by this entry); device arrays: nothing up, the 8 bytes of the two label
   verdicts down. */
int sdpsr_basis_image_complex(sdpsr_ctx* ctx, int64_t n, const uint32_t* P, int64_t d, int32_t nblocks, const int32_t* blk_sizes,
                              const double* Q_hat, int64_t class_first, int64_t class_count, double atol, double* blks,
                              int32_t* route, double* phase_ms, int mem);

/* ---- block images as solver triplets, README.md:72-79, test/sd_problems.jl:46-52,
        docs/src/examples/ReduceAndSolveJuMP.jl:56-84 ---------------------------------------------------------
   Every consumer of the reduced SDP takes its PSD part as sparse per-variable, per-block entries (variable i, block k, row, col,
   value) -- JuMP's PSDCone expressions sum_i x_i blks[i][k], SDPA-sparse files, a first-order method's operator.  This entry
   compacts a window of dense block images into those entries on the device, in order, so that a large d * sum s_k^2 output
   leaves the device as what it holds and not as its zeros: take sdpsr_basis_image window by window and compact each slab.
     blk_sizes    host array of nblocks sizes s_k >= 1;
     blks         class_count * sum s_k^2 elements in `mem`, in exactly the layout sdpsr_basis_image{,_complex} and
                  sdpsr_block_images{,_complex} write: class-major, then block, each block column-major s_k x s_k; doubles, or
                  complex numbers as (re, im) pairs when is_complex != 0.  The pointer needs 8-byte alignment only: a window that
                  starts at an odd element of a larger buffer is a supported input;
     the VIRTUAL block k of a class is the block itself (real input, order s'_k = s_k) or its real embedding [Re -Im; Im Re] of
                  order s'_k = 2 s_k (complex input; ReduceAndSolveJuMP.jl:59-76).  Negation is the only arithmetic on values;
     kept         an element v of a virtual block is kept iff !(|v| <= tol): zeros of either sign never, a NaN always;
     triangle     SDPSR_TRI_UPPER keeps row <= col only, SDPSR_TRI_FULL every position;
     order        the scan order of the virtual blocks: class, then block, then column-major inside the block;
     classptr     class_count + 1 offsets (0-based, `mem`): the entries of window class i are [classptr[i], classptr[i+1]);
     blk row col  int32 in `mem`, 0-based plus index_base (0 or 1); val: the kept values;
     nnz          (host) = classptr[class_count].  classptr and *nnz are ALWAYS written.  If *nnz > capacity the four entry
                  arrays are not touched and the status is still SDPSR_OK (the capacity rule of sdpsr_jordan_reduce);
                  capacity = 0 with NULL entry arrays is the sizing call;
     max_asym     (host, may be NULL: the pass is skipped) the maximum over all virtual blocks and row < col of
                  |M[row,col] - M[col,row]| -- what SDPSR_TRI_UPPER gives up.  0.0 for an empty window, unspecified when a NaN
                  is involved.
   The output is a function of the inputs alone: positions come from an exclusive scan over fixed chunks of the element range,
   no atomics decide one and nothing is sorted, so two calls -- on any ctx -- give equal bytes.
   SDPSR_BAD_ARGUMENT, before any kernel, with the ctx usable afterwards: a NULL blk_sizes, classptr or nnz; NULL blks with
   class_count > 0; a NULL entry array with capacity > 0; capacity < 0; nblocks < 1, some s_k < 1, class_count < 0; tol < 0 or NaN;
   index_base or triangle outside their values; an element count that does not fit int64.  class_count == 0: SDPSR_OK,
   classptr[0] = 0, *nnz = 0, no kernel.  Workspace that does not fit: SDPSR_OUT_OF_MEMORY.
   sdpsr_transfer_bytes, host arrays: the window up; 16 bytes of result words, (class_count + 1) * 8 bytes of classptr and -- when
   delivered -- *nnz * 20 bytes of entries down (never `capacity` of them).  Device arrays: nothing up, the 16 bytes down. */
enum { SDPSR_TRI_UPPER = 0, SDPSR_TRI_FULL = 1 };
int sdpsr_block_images_sparse(sdpsr_ctx* ctx, int32_t nblocks, const int32_t* blk_sizes, int64_t class_count, const void* blks,
                              int is_complex, int triangle, double tol, int index_base, int64_t capacity, int64_t* classptr,
                              int32_t* blk, int32_t* row, int32_t* col, double* val, int64_t* nnz, double* max_asym, int mem);

/* eigen_decomposition(P, A; atol), src/eigen_decomposition.jl:236-273: status only
   (test/numerical_issues.jl:91-94), *neig = number of eigenspaces, *nclasses = number of
   isomorphism classes. */
int sdpsr_eigen_decomposition(sdpsr_ctx* ctx, int64_t n, const uint32_t* P, int64_t d,
                              double atol, int32_t* neig, int32_t* nclasses, int mem);
/* Batched small-N mode: `count` independent runs of eigen_decomposition(P, A; atol) on ONE
   partition, each with its own pair of generic elements -- the shape of the reference's
   robustness pin (test/numerical_issues.jl:85-94: 10 000 runs on a 64 x 64 partition, none may
   throw).  For n <= 64 one workgroup handles one run (Jacobi eigensolver, Q'AQ, block norms,
   Otsu threshold, union-find and __isconsistent all inside the workgroup) and all CUs work in
   parallel; larger n goes through the single-problem path run by run.
   values: NULL (fresh draws from ctx's generator) or 2*count*d doubles in `mem` -- run r uses
           values[(2r)*d ...] as the class values of element #1 and values[(2r+1)*d ...] of #2
           (n <= 64 only; lets a caller replay given elements);
   status/neig/nclasses: host arrays of `count` ints, each may be NULL.
   Returns SDPSR_OK when every run is OK, else the status of the first failing run. */
int sdpsr_eigen_decomposition_batched(sdpsr_ctx* ctx, int64_t n, const uint32_t* P, int64_t d, double atol,
                                      int64_t count, const double* values, int32_t* status, int32_t* neig,
                                      int32_t* nclasses, int mem);
/* Symmetric eigendecomposition used by the path (eigen(A), :246): ascending values,
   orthonormal vectors (column-major n x n, overwrites nothing of A).  Only the lower triangle of A is referenced.
   Range: the solver's norms are sums of squares, so the copy the entry point makes of A is multiplied by a power of two -- exact --
   when max |a| over the lower triangle lies outside [2^-400, 2^400], and the eigenvalues are multiplied back (on the device, no host
   wait): every finite input whose eigenvalues are representable is solved to the same relative accuracy, subnormal entries
   included; inside the window no bit of the result differs from a solver without the scaling.  A NaN or Inf entry
   is not scaled away: the solver's own checks see it (n > 128: SDPSR_SOLVER_ERROR from the check of the tridiagonal matrix). */
int sdpsr_syev_f64(sdpsr_ctx* ctx, int64_t n, const double* A, double* values, double* vectors,
                   int mem);

/* ---- agreement of independent restarts ---------------------------------------------------
   The reference's answer to its randomized steps is "try again" (src/eigen_decomposition.jl:264-270, src/diagonalize.jl:4-9);
   here the tries run side by side -- R restarts per ctx (sdpsr_jordan_reduce_batch, sdpsr_problem_reduce_batch), one process
   per GPU -- and return partitions that are equal (Base.:(==), src/partitions.jl:16-17) with probability 1 - eps.  These entry
   points reconcile them: when they differ every restart receives their MEET, the coarsest common refinement -- refine!
   (src/partitions.jl:62-66) folded over the restarts, a restart whose draws missed a split is refined by the others.

   A restart is a SLOT, numbered rank * R + i over all ranks.  The meet's keys are
       keys[e] = sum over i < R with valid[i] of labels_i[e] * m(first_slot + i)   mod 2^64,
       m(k) = ODD[k mod 8] * (2 floor(k / 8) + 1) mod 2^64,
       ODD = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD6E8FEB86659FD93,
             0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5, 0x85EBCA77C2B2AE63,
   summed over the ranks mod 2^64; their canonical relabel (sdpsr_partition_from_u64: first occurrence, 0 stays 0) is the meet.
   A key is 0 where every valid array is 0 -- and, like two entries of different label tuples receiving equal keys, elsewhere
   only by a collision of the universal hash: probability ~ d^2 / 2^64 for a meet of d classes, on top of the ~ d^2 / 2^65 of
   the relabel's own mixing hash (sdpsr_refine). */
typedef struct sdpsr_comm sdpsr_comm; /* one rank's handle of a communicator, sdpsr_comm_create */

/* The key pass alone, one streaming kernel ((R * B / 8 + 8) bytes per entry at label width B): for a caller with a transport
   of its own (MPI.jl, a thread pool), who sums the ranks' keys itself and hands the sum to sdpsr_partition_from_u64.
     labels   host array of R pointers (1 <= R <= 64) to label arrays of len entries at the ctx's label width, in `mem`;
              device arrays are read where they lie, aligned to their element only (sub-arrays);
     valid    host array of R ints, NULL = all: a restart with valid[i] == 0 is not read;
     first_slot >= 0: the slot of labels[0] (rank * R);
     keys     len words in `mem` (8-byte aligned); every word is written. */
int sdpsr_meet_keys(sdpsr_ctx* ctx, int32_t R, const uint32_t* const* labels, const int32_t* valid, int64_t len,
                    int64_t first_slot, uint64_t* keys, int mem);

/* The agreement of the partitions of R restarts on every rank of comm (NULL: this process alone).  COLLECTIVE.
     1. sdpsr_partition_checksum of every valid array; the ranks' records (len, R, label width, valid and checksum per
        restart) are all-gathered and every rank takes the same decision from the same table:
     2. some rank's len, R or label width differs: SDPSR_BAD_ARGUMENT on every rank; no valid restart anywhere:
        SDPSR_BAD_STATE; every restart of every rank valid and all checksums equal: *met = 0, nothing is written, *dim_out is
        untouched;
     3. anything else: the key pass over the valid restarts, with a comm ONE sum all-reduce of the len keys, the canonical
        relabel; the result is written into ALL R arrays, the invalid ones included, *met = 1, *dim_out = its class count.
        After an OK return every array of every rank holds the same canonical partition, the meet of the valid restarts.
   valid[i] (NULL = all): restart i's labels are a partition -- its status was SDPSR_OK, SDPSR_NUMERICAL_INCONSISTENCY or
   SDPSR_DIMENSION_MISMATCH (the loop ended; blockDiagonalize's randomized failure does not touch P_out).  An invalid restart's
   array is never read: whatever it holds cannot refine the others.
   SDPSR_LABEL_OVERFLOW: the meet has more than 2^B - 1 classes at label width B; *dim_out is set, every array is untouched
   (decided on the host from the count, which is the same on every rank).
   R outside 1 .. 64, a NULL pointer, len out of range: SDPSR_BAD_ARGUMENT before any kernel or collective.  The ctx stays
   usable after every error.
   Host arrays (SDPSR_MEM_HOST): the valid arrays are uploaded once (len * B / 8 bytes each) for the checksums and the key
   pass, and all R arrays are delivered back only after a meet; sdpsr_transfer_bytes counts both, and 16 bytes of checksum
   read back per restart in either memory space. */
int sdpsr_agree_partitions(sdpsr_ctx* ctx, sdpsr_comm* comm, int32_t R, uint32_t* const* labels, const int32_t* valid,
                           int64_t len, int64_t* dim_out, int32_t* met, int mem);

/* blockDiagonalize's side of the agreement: the tries have run side by side, the LOWEST rank whose status is SDPSR_OK wins
   and every rank receives its blkSizes (the reference retries after NumericalInconsistency / DimensionMismatch,
   src/eigen_decomposition.jl:264-270, src/diagonalize.jl:4-9).  COLLECTIVE: one all-gather of (status, nblocks), one broadcast
   of the winner's sizes.  comm == NULL: the winner is this process or nobody.
     status, nblocks, blk_sizes   this rank's result (blk_sizes is read only with status == SDPSR_OK);
     *winner       the winning rank, -1 when every rank failed (SDPSR_OK is returned: the caller retries with fresh draws);
     *nblocks_out  the winner's block count (0 without a winner); sizes_out[capacity]: its sizes.  capacity < *nblocks_out:
                   sizes_out is untouched and SDPSR_BAD_ARGUMENT is returned -- after the collectives have completed, so the
                   ranks stay in step.  Q_hat of the winner travels with sdpsr_comm_broadcast. */
int sdpsr_agree_block_diagonalization(sdpsr_ctx* ctx, sdpsr_comm* comm, int32_t status, int32_t nblocks,
                                      const int32_t* blk_sizes, int32_t* winner, int32_t* nblocks_out, int32_t* sizes_out,
                                      int32_t capacity);

/* ---- the communicator: RCCL behind the C ABI -------------------------------------------------------------
   One process per GPU.  RCCL is opened lazily on the first sdpsr_comm_* call, with dlopen("librccl.so.1") -- by SONAME, not
   by path: libsdpsr_hip.so does not link against it (a process that never calls these loads what it loaded before), and a
   process that has imported torch shares the RCCL torch has already mapped.  A library that cannot be opened or lacks a
   symbol: SDPSR_BAD_STATE (dlerror() in sdpsr_last_error); an RCCL call that fails: SDPSR_SOLVER_ERROR (ncclGetErrorString
   in sdpsr_last_error).
   EVERY RANK MUST MAKE THE SAME SEQUENCE OF COLLECTIVE CALLS (sdpsr_comm_create, sdpsr_comm_broadcast,
   sdpsr_agree_partitions and sdpsr_agree_block_diagonalization with a comm), with arguments that pass the checks made before
   the first collective of a call: a rank that returns early, or never arrives, leaves the others waiting.  THE LIBRARY ADDS
   NO TIME-OUT OF ITS OWN.  All collectives run on the ctx's stream; the calls return with their outputs complete. */
/* 128 bytes of host memory (ncclUniqueId): any one rank calls it, the caller distributes the bytes to the others */
int sdpsr_comm_unique_id(void* id128);
/* collective over the `world` ranks holding the same id; the communicator lives on ctx's device */
int sdpsr_comm_create(sdpsr_ctx* ctx, int32_t world, int32_t rank, const void* id128, sdpsr_comm** out);
int sdpsr_comm_rank(const sdpsr_comm* comm); /* -1 for a NULL comm, as sdpsr_comm_world */
int sdpsr_comm_world(const sdpsr_comm* comm);
/* `bytes` bytes of buf (in `mem`) of rank `root` to every rank's buf: the winner's Q_hat (sdpsr_q_hat) */
int sdpsr_comm_broadcast(sdpsr_ctx* ctx, sdpsr_comm* comm, void* buf, int64_t bytes, int32_t root, int mem);
/* before the ctx it was created on is destroyed */
int sdpsr_comm_destroy(sdpsr_comm* comm);

/* ---- the reduced PSD blocks as an operator: Z(x), its adjoint, block spectra -------------------------------
   The reduced PSD constraint is the pencil  Z_k(x) = sum_i x_i blks[i][k],  k = 1 .. nblocks  --
   sum(blkD.blks[i] .* x[i] for i = 1:dim(P)), docs/src/examples/ErdosRenyiThetaFunction.jl:83, QuadraticAssignmentProblems.jl:136,
   test/sd_problems.jl:46-52,127-134.  These entries evaluate it, its adjoint  g_i = sum_k <blks[i][k], S_k>  and the spectra of
   all blocks on the device, from the triplets sdpsr_block_images_sparse writes: what one iteration of a first-order method over
   the reduced SDP needs, and the certificate (lambda_min of every block) of a solved one.  No SDP is solved here
   (sdpsr_sdp_solve, below, is the solver built on these entries).

   sdpsr_blockop: a device-resident handle, read-only after creation; any ctx of its device may use it; the caller destroys it
   (before the device is reset; a ctx is not needed for that).
     nblocks, blk_sizes  host array of the VIRTUAL orders s'_k >= 1 (s_k for real images, 2 s_k for the real embedding of complex
                  ones), sum s'_k^2 < 2^32;
     d            the number of classes (x has d elements), 0 <= d < 2^31;
     classptr blk row col val   exactly what sdpsr_block_images_sparse writes (classptr: d + 1 offsets, 0-based; blk / row / col:
                  int32, 0-based plus index_base), windows concatenated by the caller included; in `mem`.  Host arrays are
                  uploaded once; device arrays are read where they lie, never modified, and the handle keeps no pointer into
                  them.  The entries of a class need not be sorted, duplicates are legal and are summed, a NaN value is legal
                  and propagates.  classptr may be NULL when nnz == 0;
     triangle     SDPSR_TRI_FULL: every entry is one position; SDPSR_TRI_UPPER: an entry with row != col stands for (row, col)
                  and (col, row).  The handle stores the FULL entry list, nnz_full <= 2 nnz entries, < 2^32.
   A POSITION is the flat index of (k, row, col) in the layout of one class of sdpsr_block_images: blocks side by side, each
   column-major s'_k x s'_k.  The handle keeps the full list twice, 16 bytes per entry each (32 * nnz_full bytes of device
   memory in all): sorted by class (input order, a mirror right behind its entry) for the adjoint, and sorted by position with
   the library's stable radix sort (ties in class-major order) for the forward map.
   Validation runs on the device in the pass that reads the arrays; its verdict comes back on the ONE host wait a creation makes
   in front of the allocation (a second wait ends it, the handle is complete on return).  SDPSR_BAD_ARGUMENT with a message that
   names the lowest offending index: classptr[0] != 0, a non-monotone classptr, classptr[d] != nnz; a block index outside
   [0, nblocks) after the base; a row or column outside [0, s'_k); row > col under SDPSR_TRI_UPPER.  SDPSR_BAD_ARGUMENT before
   any kernel: sum s'_k^2 >= 2^32, nnz >= 2^32, nblocks < 1, some s'_k < 1, d < 0, a NULL array with nnz > 0, a bad triangle or
   index_base (a full entry count >= 2^32 with nnz below it: after the first wait).  nnz == 0 and d == 0 are legal.  After every
   refusal *op is NULL, nothing is leaked and the ctx stays usable.
   sdpsr_transfer_bytes of a creation: host arrays (d + 1) * 8 + nnz * 20 bytes up; 56 bytes of verdict words down in either
   memory space. */
typedef struct sdpsr_blockop sdpsr_blockop;
int sdpsr_blockop_create(sdpsr_ctx* ctx, int32_t nblocks, const int32_t* blk_sizes, int64_t d, int64_t nnz, const int64_t* classptr,
                         const int32_t* blk, const int32_t* row, const int32_t* col, const double* val, int triangle, int index_base,
                         int mem, sdpsr_blockop** op);
int sdpsr_blockop_destroy(sdpsr_blockop* op);
/* every pointer may be NULL; *sum_sq = sum s'_k^2, the length of Z and S */
int sdpsr_blockop_info(const sdpsr_blockop* op, int64_t* d, int32_t* nblocks, int64_t* sum_sq, int64_t* nnz_full);
/* The forward map  Z[p] = sum over the full entries e at position p of x[class(e)] * val(e):  x has d elements, Z sum s'_k^2, both
   in `mem`.  EVERY element of Z is written; a position without an entry gets exactly +0.0; blocks come out as full
   matrices in the one-class layout of sdpsr_block_images (what sdpsr_blocks_syev reads) -- under SDPSR_TRI_UPPER symmetric up to the
   rounding of the two sums, which hold the same terms.
   The adjoint  g[i] = sum over the full entries e of class i of val(e) * S[position(e)]:  for symmetric S this is
   sum_k <blks[i][k], S_k>; S has sum s'_k^2 elements, g d; an empty class gets +0.0.
   Both are sums with an order fixed by the inputs alone (the position in the stored arrangement; DESIGN.md "The reduced PSD
   blocks as an operator"), without floating-point atomics: equal inputs give equal bytes, on any ctx.  An element with one term
   is exactly x_i * val.  One host wait each (the outputs are complete on return).
   The complex route needs nothing of its own: its triplets carry the real embedding [Re -Im; Im Re] of order 2 s_k, the operator
   acts on those virtual blocks, and their spectra are the Hermitian blocks' spectra with every value doubled. */
int sdpsr_blockop_apply(sdpsr_ctx* ctx, const sdpsr_blockop* op, const double* x, double* Z, int mem);
int sdpsr_blockop_adjoint(sdpsr_ctx* ctx, const sdpsr_blockop* op, const double* S, double* g, int mem);
/* The spectra of all blocks in one call.  Z: symmetric blocks in the layout sdpsr_blockop_apply writes (sum s_k^2 elements, in
   `mem`); only the lower triangle of a block is referenced, as in sdpsr_syev_f64, and Z is not modified.
     w   sum s_k values: ascending inside a block, the blocks in order;
     V   NULL (values only: the same w bits), or sum s_k^2 elements in the layout of Z: orthonormal eigenvectors as the columns of
         block k, column j belonging to the j-th value of the block; the sign is unspecified.
   The blocks of order <= 64 are solved in ONE launch, one workgroup per block, by the Jacobi solver sdpsr_syev_f64 uses for one
   matrix of that order (blocks of order 1 are copied); the larger ones go one by one through sdpsr_syev_f64 itself.  Range: as
   sdpsr_syev_f64 -- a block whose max |a| over the lower triangle lies outside [2^-400, 2^400] is solved on an exact
   power-of-two multiple and its values are multiplied back.  A block that reaches the Jacobi sweep limit (40): SDPSR_NOT_CONVERGED,
   every output written as it stands.  nblocks < 1, some s_k < 1, sum s_k^2 >= 2^32, NULL Z or w: SDPSR_BAD_ARGUMENT. */
int sdpsr_blocks_syev(sdpsr_ctx* ctx, int32_t nblocks, const int32_t* blk_sizes, const double* Z, double* w, double* V, int mem);

/* ---- Solving the reduced SDP: PSD projection and a first-order (ADMM) driver ---------------------------------
   The last step of the reference's work flow, reduceAndSolve (docs/src/examples/ReduceAndSolveJuMP.jl:40-91; the models of
   test/sd_problems.jl:29-55,107-137; the pinned optima of test/lovasz.jl:16,32,48 and test/qap.jl:31):
       max / min  c'x   s.t.   A x = b,   x >= 0,   Z_k(x) = sum_i x_i blks[i][k] in PSDCone() for all k.
   The reference hands this model to CSDP (an interior-point method) through JuMP.  The library solves it on the device with a
   first-order method over the operator handle above.  It is NOT an interior-point replacement: the theta' pins of the
   reference are reached to their printed 8 digits, a degenerate instance (esc16j) to about 1e-4 relative in 20 000 iterations
   (DESIGN.md "Deviations", README "Solving the reduced SDP").

   sdpsr_psd_project: P_k = V max(w, 0) V' for every block, the projection onto the PSD cone in the Frobenius norm.  Z and P: the
   one-class layout sdpsr_blockop_apply writes (sum s_k^2 elements, in `mem`); only the lower triangle of a block is referenced,
   as in sdpsr_blocks_syev; P is written as a full matrix that is symmetric bit for bit (one triangle is computed and mirrored)
   and may alias Z.  lambda_min: NULL, or nblocks values: the smallest eigenvalue of each block.  A block of order 1 is a clamp;
   a block without a positive eigenvalue (an all-zero or negative semidefinite one) gives +0.0 everywhere.  ONE launch for all
   blocks, one workgroup per block on the Jacobi solver of sdpsr_blocks_syev (one wave per block while every order is <= 16);
   the sum runs over the eigenvalues w > 0, or over those < 0 subtracted from Z when these are fewer.  Range: the rule of
   sdpsr_syev_f64 -- a block whose max |a| lies outside [2^-400, 2^400] is projected as an exact power-of-two multiple and
   multiplied back: the result scales exactly.  A NaN or Inf in a block's lower triangle: that block's outputs are NaN, the
   others are intact, SDPSR_SOLVER_ERROR.  The Jacobi sweep limit (40): SDPSR_NOT_CONVERGED, outputs written as they stand.
   An order above the ctx's psd_max_order (64 unless set, below): SDPSR_BAD_ARGUMENT with a message that names the cap; also
   nblocks < 1, some s_k < 1, sum s_k^2 >= 2^32, NULL Z or P.  One host wait.  Equal inputs give equal bytes, on any ctx.

   sdpsr_set_psd_max_order(ctx, 128) opts a ctx into blocks of order 65 .. 128, for sdpsr_psd_project and sdpsr_sdp_solve
   alike (the solver's final lambda_min included).  Those blocks run in a SECOND launch behind the first, one workgroup of
   1024 threads per block on the one-workgroup Jacobi sdpsr_syev_f64 uses at these orders: A in LDS, the eigenvectors behind it
   up to order 97 and in a per-block slice of a ctx scratch (128 KB a block) beyond.  The contract above holds word for word
   (lower triangle, scaling, +0.0, NaN, sweep limit, aliasing, bitwise symmetry, equal bytes); the blocks of order <= 64 of a
   mixed call get the bytes a default ctx gives them.  A call without such blocks makes no second launch, a call with only such
   blocks no first one; still one job table and one host wait.  A ctx that is never told runs exactly what it ran before. */
int sdpsr_set_psd_max_order(sdpsr_ctx* ctx, int order); /* 64 (default) or 128; other values: SDPSR_BAD_ARGUMENT, setting unchanged */
int sdpsr_psd_max_order(sdpsr_ctx* ctx);
/*

   sdpsr_sdp_solve.  B: R^d -> (+)_k Sym(s'_k) is sdpsr_blockop_apply, B' sdpsr_blockop_adjoint (both on full entries, so
   <Bx, S> = x'B'S as stored).  A: r x d, column-major, with INDEPENDENT rows (the output of sdpsr_compress_constraints), b: r,
   c: d, all in `mem`.  Split x = u (u >= 0) and Bx = S (S PSD) with scaled duals lam, Lam; chat = -+c / |c|_2 (minus for max);
       M = I + B'B (d x d),   G = A M^-1 A',   Kt = M^-1 - M^-1 A' G^-1 A M^-1,   x0 = M^-1 A' G^-1 b
   are built once and do not depend on rho.  One iteration:
       g    = (u - lam) + B'(S - Lam) - chat / rho
       x    = Kt g + x0                                   (A x = b up to the rounding of one d-length sum)
       u+   = max(0, x + lam)            S+   = proj_PSD(Bx + Lam)      (sdpsr_psd_project's kernel, fused with the next line)
       lam+ = (x + lam) - u+             Lam+ = (Bx + Lam) - S+
       r_p^2 = |x - u+|^2 + |Bx - S+|^2,   r_d^2 = rho^2 (|u+ - u|^2 + |S+ - S|^2)
   from u = lam = 0, S = Lam = 0.  Every check_every iterations (and at the last one) the host reads r_p^2, r_d^2 and a
   non-finite flag from pinned memory and stops when r_p <= eps and r_d <= eps.  adapt_rho (residual balancing, at a check that
   does not stop): r_p > 10 r_d doubles rho, r_d > 10 r_p halves it, lam and Lam are multiplied by rho_old / rho_new; Kt and x0
   stay.  It is an option, not the default: on ER(7) it changed rho 105 times and was slower than rho = 1.
     opts   NULL or a zeroed struct: rho = 1, eps = 1e-9, max_iters = 20000, check_every = 50, no adaptation, sense = +1 (max),
            x >= 0 enforced.  A zero field selects its default; nonneg = -1 drops x >= 0 (u+ = x + lam); reserved stays 0;
     x      d values: the last iterate of the affine step;   S: NULL or sum s'_k^2 values, the PSD split variable;
     Y      NULL or sum s'_k^2 values: rho Lam, the multiplier of Bx = S;
     info   NULL or the report, computed on the host from the returned x itself: objective = c'x (the unscaled c), eq_residual =
            |A x - b|_inf, min_x, lambda_min = min_k lambda_min(Z_k(x)) through the projection kernel; r_primal, r_dual and rho
            as of the last check, iters, rho_changes.
   Setup (not the hot path): M by a Gram kernel over the handle's entries sorted by (class, position) -- entries sharing a
   position contribute val_i val_j to M_ij, positions ascending, one thread per element, no floating-point atomics; M^-1 through
   sdpsr_syev_f64; G goes to the host (Cholesky).  The loop is six kernels and two fills per iteration and makes no host wait
   between two checks: host waits of a call = ceil(iters / check_every) + a constant that depends on the setup path (d, r, mem),
   not on the iteration count -- 5 for host arrays with d <= 64 and r > 0 (tests/test_gpu_sdp_solve.py holds the count).
   Every sum has an order fixed by the inputs alone: equal inputs give equal bytes, on any ctx.
   SDPSR_BAD_ARGUMENT, nothing written: d < 1 or d > 4096 (Kt is 134 MB at the cap; checked before any allocation); a virtual
   block order above the ctx's psd_max_order (64, or 128 after sdpsr_set_psd_max_order); r outside [0, min(d, 1024)]; a non-finite value in A, b or c; bad options; G numerically singular
   ("rows of A are dependent: compress_constraints first").  r = 0 is legal.  The iteration limit: SDPSR_NOT_CONVERGED with every
   output and the report written as they stand.  A non-finite value met on the way (a NaN in the operator): SDPSR_SOLVER_ERROR.
   The ctx and the handle stay usable after every refusal.  The complex route needs nothing of its own (real embedding). */
int sdpsr_psd_project(sdpsr_ctx* ctx, int32_t nblocks, const int32_t* blk_sizes, const double* Z, double* P, double* lambda_min,
                      int mem);
typedef struct {
    double rho, eps;
    int32_t max_iters, check_every, adapt_rho, sense /* +1 max, -1 min */, nonneg /* 0, 1: x >= 0; -1: free */;
    int32_t reserved[5];
} sdpsr_sdp_opts;
typedef struct {
    double objective, r_primal, r_dual, rho, eq_residual, min_x, lambda_min;
    int32_t iters, rho_changes;
} sdpsr_sdp_info;
int sdpsr_sdp_solve(sdpsr_ctx* ctx, const sdpsr_blockop* op, int64_t r, const double* A, const double* b, const double* c,
                    const sdpsr_sdp_opts* opts, double* x, double* S, double* Y, sdpsr_sdp_info* info, int mem);

#ifdef __cplusplus
}
#endif
#endif /* SDPSR_H */
