// The class-compare checks for gfx950: "does any entry differ from the representative of its class?" -- one table kernel,
// one compare kernel, and the checks (Chk*) that say what an entry loads, keeps per class and compares.
#include <type_traits>
#include "sdpsr_internal.h"
#include "kernel_util.h"
#include "sig_sources.h"
#include "refine_table.h"

namespace sdpsr {

// ---------------------------------------------------------------------------
// "Does this step split any class?" without a relabel.  A refinement that ends with the dimension it
// started with (every confirm round; the first iteration on an already closed partition) leaves the
// labels as they are, so the insert / rank / label passes only establish that nothing changed.  That
// question needs no hash table: with the first-occurrence index of every class at hand (first_idx,
// written by the ranking pass of the refinement that made the labels) a tiny kernel evaluates the
// step's values at the class representatives, and one streaming pass compares every entry with the
// representative of its class -- raw values (rounded projection, channel products), no signature
// hashing, no atomics; flag[0] = 1 as soon as some entry differs (the caller then runs the full
// refinement).  Packed lower triangle, int32 channels (the default loop).
// The same pass answers two more questions, with other values per entry and per class: "is every basis
// matrix constant on the classes?" (ChkBasis) and "would Part(a) ^ Part(b) write these labels again?"
// (ChkPair).  There is ONE table kernel and ONE compare kernel (class_ref_kernel, class_compare_kernel);
// what a question loads, keeps per class and compares is its check, a functor like the Src* sources (sig_sources.h):
//   Raw                    what one entry loads;            Ref   what the table holds per class
//   ref_of(cls, first_idx) the record of class cls, taken at its representative
//   zero_ref()             the record that label 0 and the slots past a column compare with
//   fetch(i, j, e, ok)     the loads of entry (i, j), packed number e (ok = 0: past the column, zeros)
//   differs(raw, ref)      THE comparison
//   load_uniforms()        what differs reads for every entry alike, into registers once
//   order()                n;   kUntrusted: labels and representatives are a guess (see ChkPair)
// ---------------------------------------------------------------------------
struct VerifyRef {  // one per class: the step's values at the class representative
    double x;        // the class's uniform draw (depends on the label only)
    uint64_t ybits;  // code of the rounded projected value there (sdpsr_round_key)
    int32_t c[4];    // channel products there
};
// Up to this many classes the compare pass builds the table of representatives itself, in LDS, in a prologue of every workgroup (8 KiB: the
// kernel's occupancy stays where it is): no launch of its own for the table, no gather from global memory per entry.  More classes: the table
// kernel and the compare pass as two launches.  The same cap serves the basis check (<= 4 codes of 8 bytes per class) and the pair check.
constexpr int VERIFY_LDS_CAP = 256;
int verify_lds_cap() { return VERIFY_LDS_CAP; }

// "Does this step split a class?": the T int32 channels and, JOINT, the rounded projection x - sum_k coef[k] U_k of the class draws x.
// The zero record is all zero bits (ybits = 0 is what sdpsr_round_key gives below atol, not a code of its own).
template <int R, int T, bool JOINT>
struct ChkStep {
    using Ref = VerifyRef;
    static constexpr bool kUntrusted = false;
    struct Raw {
        int32_t c[T];
        double u[R > 0 ? R : 1];
    };
    int n;
    int64_t ld;
    const double* __restrict__ U;
    const double* __restrict__ coef;
    double atol, scale;
    const int32_t* __restrict__ C;  // T channels, ld x ld each
    uint64_t key;
    double cf[R > 0 ? R : 1];  // coef, once load_uniforms() has run
    __host__ __device__ __forceinline__ int order() const { return n; }
    __device__ __forceinline__ void load_uniforms() {
#pragma unroll
        for (int k = 0; k < R; ++k) cf[k] = coef[k];
    }
    __device__ __forceinline__ Ref ref_of(int cls, const uint32_t* __restrict__ first_idx) const {
        uint32_t i, j;
        packed_lower_ij(n, (int64_t)first_idx[cls], i, j);
        const int64_t ef = (int64_t)i + (int64_t)j * n;
        Ref r;
        r.x = 0;
        r.ybits = 0;
        if (JOINT) {
            r.x = sdpsr_class_uniform(key, (uint32_t)cls + 1u);
            double p = 0;
#pragma unroll
            for (int k = 0; k < R; ++k) p = fma(U[(int64_t)k * n * n + ef], coef[k], p);
            r.ybits = sdpsr_round_key(r.x - p, atol, scale);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) r.c[t] = t < T ? C[(int64_t)t * ld * ld + (int64_t)j * ld + i] : 0;
        return r;
    }
    __device__ __forceinline__ Ref zero_ref() const { return Ref{0.0, 0ull, {0, 0, 0, 0}}; }
    __device__ __forceinline__ Raw fetch(int i, int j, int64_t, bool ok) const {
        Raw v;
        const int32_t* Cij = C + (int64_t)j * ld + i;
#pragma unroll
        for (int t = 0; t < T; ++t) v.c[t] = ok ? __builtin_nontemporal_load(&Cij[(int64_t)t * ld * ld]) : 0;
        if (JOINT) {
            const double* Uij = U + (int64_t)j * n + i;
#pragma unroll
            for (int k = 0; k < R; ++k) v.u[k] = ok ? __builtin_nontemporal_load(&Uij[(int64_t)k * n * n]) : 0.0;
        }
        return v;
    }
    __device__ __forceinline__ bool differs(const Raw& v, const Ref& r) const {
        bool bad = false;
        if (JOINT) {
            double p = 0;
#pragma unroll
            for (int k = 0; k < R; ++k) p = fma(v.u[k], cf[k], p);
            bad = sdpsr_round_key(r.x - p, atol, scale) != r.ybits;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) bad = bad || v.c[t] != r.c[t];
        return bad;
    }
};
size_t verify_ref_bytes(int64_t d) { return (size_t)(d > 0 ? d : 1) * sizeof(VerifyRef); }

// The projection half of ChkStep<R, T, true> alone, the same ybits rule: the channel half of such a round is settled without the
// product (kernels_square_check.hip), so nothing of C is read here.
template <int R>
struct ChkProj {
    struct Ref {
        double x;
        uint64_t ybits;
    };
    static constexpr bool kUntrusted = false;
    struct Raw {
        double u[R];
    };
    int n;
    const double* __restrict__ U;
    const double* __restrict__ coef;
    double atol, scale;
    uint64_t key;
    double cf[R];  // coef, once load_uniforms() has run
    __host__ __device__ __forceinline__ int order() const { return n; }
    __device__ __forceinline__ void load_uniforms() {
#pragma unroll
        for (int k = 0; k < R; ++k) cf[k] = coef[k];
    }
    __device__ __forceinline__ Ref ref_of(int cls, const uint32_t* __restrict__ first_idx) const {
        uint32_t i, j;
        packed_lower_ij(n, (int64_t)first_idx[cls], i, j);
        const int64_t ef = (int64_t)i + (int64_t)j * n;
        Ref r;
        r.x = sdpsr_class_uniform(key, (uint32_t)cls + 1u);
        double p = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) p = fma(U[(int64_t)k * n * n + ef], coef[k], p);
        r.ybits = sdpsr_round_key(r.x - p, atol, scale);
        return r;
    }
    __device__ __forceinline__ Ref zero_ref() const { return Ref{0.0, 0ull}; }
    __device__ __forceinline__ Raw fetch(int i, int j, int64_t, bool ok) const {
        Raw v;
        const double* Uij = U + (int64_t)j * n + i;
#pragma unroll
        for (int k = 0; k < R; ++k) v.u[k] = ok ? __builtin_nontemporal_load(&Uij[(int64_t)k * n * n]) : 0.0;
        return v;
    }
    __device__ __forceinline__ bool differs(const Raw& v, const Ref& r) const {
        double p = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) p = fma(v.u[k], cf[k], p);
        return sdpsr_round_key(r.x - p, atol, scale) != r.ybits;
    }
};

// "Can the projection step still split a class?"  x - U U'x of an x that is constant on the classes of S is constant on
// them for EVERY x exactly when every basis matrix U_k is (U_k in span(S) => U U'x in span(S)), and a finer S keeps the
// property: once it holds, the projection half of the loop (src/partitions.jl:159-164) cannot refine S any more.  The
// check compares the rounded codes of U_k (the rounding of the projection's own signatures, sdpsr_round_key) at every
// entry of the packed lower triangle with those at the class representative; label 0 (structural zeros) needs U_k = 0:
// the zero record holds the code of 0.0.  flag[0] = 1 <=> some U_k is NOT constant on some class.
template <int R>
struct ChkBasis {
    struct Ref {
        uint64_t code[R];  // (8 R bytes per class: uconst_ref_bytes)
    };
    static constexpr bool kUntrusted = false;
    struct Raw {
        double u[R];
    };
    int n;
    const double* __restrict__ U;  // symmetric basis matrices U_k, n x n, column-major
    double atol, scale;
    __host__ __device__ __forceinline__ int order() const { return n; }
    __device__ __forceinline__ void load_uniforms() {}
    __device__ __forceinline__ Ref ref_of(int cls, const uint32_t* __restrict__ first_idx) const {
        uint32_t i, j;
        packed_lower_ij(n, (int64_t)first_idx[cls], i, j);
        const int64_t ef = (int64_t)i + (int64_t)j * n;
        Ref r;
#pragma unroll
        for (int k = 0; k < R; ++k) r.code[k] = sdpsr_round_key(U[(int64_t)k * n * n + ef], atol, scale);
        return r;
    }
    __device__ __forceinline__ Ref zero_ref() const {
        Ref r;
#pragma unroll
        for (int k = 0; k < R; ++k) r.code[k] = sdpsr_round_key(0.0, atol, scale);
        return r;
    }
    __device__ __forceinline__ Raw fetch(int i, int j, int64_t, bool ok) const {
        Raw v;
        const double* Uij = U + (int64_t)j * n + i;
#pragma unroll
        for (int k = 0; k < R; ++k) v.u[k] = ok ? __builtin_nontemporal_load(&Uij[(int64_t)k * n * n]) : 0.0;
        return v;
    }
    __device__ __forceinline__ bool differs(const Raw& v, const Ref& r) const {
        bool bad = false;
#pragma unroll
        for (int k = 0; k < R; ++k) bad = bad || sdpsr_round_key(v.u[k], atol, scale) != r.code[k];
        return bad;
    }
};
size_t uconst_ref_bytes(int64_t d, int64_t r) { return (size_t)(d > 0 ? d : 1) * (size_t)(r > 0 ? r : 1) * 8; }

// "Is the initial partition S = Part(a) ^ Part(b) of this call the one that Lp and first_idx already describe?"  (the restarts of one
// problem: a, b are what they were, and a call that found its input closed has left the initial partition in place).  Lp, first_idx: the
// canonical labels of a refinement and the first occurrences of its d <= VERIFY_LDS_CAP classes.  flag[0] stays 0 exactly when the
// refinement of SrcPair{a, b, n, packed} would write the same labels and representatives again:
//   every entry of label l >= 1 has the signature of first_idx[l - 1]; no representative has the zero signature (its class would be
//   label 0); the representatives' signatures are pairwise distinct; every entry of label 0 has the zero signature
// -- then the classes of the signatures ARE the classes of Lp, and the canonical numbering depends on the partition alone.  The signature
// is the refinement's own (SrcPair::fetch / sig): -0.0, NaN payloads and equal hashes count as they do in the insert pass.
// kUntrusted: labels and representatives are a guess, so the compare kernel adds what the list above needs beyond the entry compare: a
// representative outside the triangle (ref_of gives it the zero signature) or with the zero signature, two classes of one signature,
// a label > d: violated.  The table is checked where it is built, in LDS: one launch, d <= VERIFY_LDS_CAP.
struct ChkPair {
    using Ref = uint64_t;
    using Raw = SrcPair::Raw;
    static constexpr bool kUntrusted = true;
    SrcPair src;
    __host__ __device__ __forceinline__ int order() const { return src.n; }
    __device__ __forceinline__ void load_uniforms() {}
    __device__ __forceinline__ Ref ref_of(int cls, const uint32_t* __restrict__ first_idx) const {
        const int64_t e = (int64_t)first_idx[cls];
        uint64_t sg = 0;
        if (e < (int64_t)src.n * (src.n + 1) / 2) {
            uint32_t i, j;
            packed_lower_ij(src.n, e, i, j);
            sg = src.sig(src.fetch(i, j, e));
        }
        return sg;
    }
    __device__ __forceinline__ Ref zero_ref() const { return 0; }
    __device__ __forceinline__ Raw fetch(int i, int j, int64_t e, bool ok) const {
        return ok ? src.fetch((uint32_t)i, (uint32_t)j, e) : Raw{0.0, 0.0};
    }
    __device__ __forceinline__ bool differs(const Raw& v, const Ref& r) const { return src.sig(v) != r; }
};

// The table of the two-launch form: one record per class, and the verdict word of the compare pass that follows in stream order cleared.
template <class CHK>
__global__ void class_ref_kernel(CHK chk, int d, const uint32_t* __restrict__ first_idx, typename CHK::Ref* __restrict__ ref,
                                 uint32_t* __restrict__ flag) {
    const int cls = blockIdx.x * blockDim.x + threadIdx.x;
    if (cls == 0) flag[0] = 0u;
    if (cls >= d) return;
    ref[cls] = chk.ref_of(cls, first_idx);
}
// Column j over the workgroups, rows over the threads; flag[0] = 1 when some entry differs from the record of its class.
// LDSREF (d <= VERIFY_LDS_CAP): the table is built here from first_idx (ref unused) and nobody zeroes flag[0] on the device -- a workgroup
// could set the word before another one clears it: the launcher stores the 0 from the host before it enqueues the pass.
// LT: the element type of Lp (uint8_t: the loop's 8-bit shadow of labels <= 255, LDSREF only); the loads and the widening differ, nothing else.
template <class CHK, bool LDSREF, typename LT>
__global__ void __launch_bounds__(256)
class_compare_kernel(CHK chk, const LT* __restrict__ Lp, const typename CHK::Ref* __restrict__ ref, uint32_t* __restrict__ flag, int d,
                     const uint32_t* __restrict__ first_idx) {
    using Ref = typename CHK::Ref;
    static_assert(LDSREF || !CHK::kUntrusted, "an untrusted table is checked in LDS");
    __shared__ Ref sref[LDSREF ? VERIFY_LDS_CAP : 1];
    const int n = chk.order();
    const Ref zero = chk.zero_ref();
    bool bad = false;
    if (LDSREF) {
        for (int cls = threadIdx.x; cls < d; cls += blockDim.x) {
            sref[cls] = chk.ref_of(cls, first_idx);
            if constexpr (CHK::kUntrusted) bad = bad || sref[cls] == zero;
        }
        __syncthreads();
        if constexpr (CHK::kUntrusted) {
            if (blockIdx.x == 0) {  // pairwise distinct: one workgroup's finding is enough (every lane reads the same word: a broadcast)
                for (int cls = threadIdx.x; cls < d; cls += blockDim.x) {
                    const Ref mine = sref[cls];
                    for (int k = 0; k < cls; ++k) bad = bad || sref[k] == mine;
                }
            }
        }
    }
    chk.load_uniforms();
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const int64_t poff = (int64_t)j * n - (int64_t)j * (j - 1) / 2 - j;
        const LT* Lj = Lp + poff;
        // VB entries of a thread per trip: their labels and values in one batch of loads, then the records of their
        // classes in a second one (entry by entry it was two dependent memory round trips per entry, round 4)
        constexpr int VB = 4;
        for (int i0 = j + threadIdx.x; i0 < n; i0 += 256 * VB) {
            uint32_t l[VB];
            typename CHK::Raw v[VB];
#pragma unroll
            for (int b = 0; b < VB; ++b) {
                const int i = i0 + 256 * b;
                const bool ok = i < n;
                l[b] = ok ? (uint32_t)__builtin_nontemporal_load(&Lj[i]) : 0u;
                v[b] = chk.fetch(i, j, poff + i, ok);
            }
            Ref r[VB];
#pragma unroll
            for (int b = 0; b < VB; ++b) {
                // label 0 (and the slots past the column): the zero class stays together only while every value is the zero record's
                r[b] = zero;
                if (CHK::kUntrusted && l[b] > (uint32_t)d) bad = true;
                else if (l[b]) {
                    if (LDSREF) r[b] = sref[l[b] - 1];
                    else r[b] = ref[l[b] - 1];
                }
            }
#pragma unroll
            for (int b = 0; b < VB; ++b) bad = bad || chk.differs(v[b], r[b]);
        }
    }
    if (bad) flag[0] = 1u;
}
// THE launcher of the three checks.  Up to VERIFY_LDS_CAP classes: one launch, flag[0] cleared from the host (flag: a word of pinned host
// memory whose last verdict has been read).  More: the table kernel, which clears the word, and the compare pass; that form exists for wide
// labels and trusted tables only, and the callers ask for no other.
template <class CHK, typename LT>
static void launch_class_compare(hipStream_t s, const CHK& chk, const LT* Lp, int64_t d, const uint32_t* first_idx, void* ref, uint32_t* flag) {
    const int n = chk.order();
    const int g = n < 256 * 8 ? n : 256 * 8;
    if (d <= VERIFY_LDS_CAP) {
        *(volatile uint32_t*)flag = 0u;
        class_compare_kernel<CHK, true, LT><<<g, 256, 0, s>>>(chk, Lp, nullptr, flag, (int)d, first_idx);
    } else if constexpr (std::is_same_v<LT, uint32_t> && !CHK::kUntrusted) {
        class_ref_kernel<CHK><<<(unsigned)((d + 255) / 256), 256, 0, s>>>(chk, (int)d, first_idx, (typename CHK::Ref*)ref, flag);
        class_compare_kernel<CHK, false, LT><<<g, 256, 0, s>>>(chk, Lp, (const typename CHK::Ref*)ref, flag, (int)d, first_idx);
    }
}

// symmetric basis matrices U_k (n x n, column-major, r <= 4 of them), packed labels Lp of d <= REFINE_FIRST_CAP classes
// with their representatives first_idx.  Wide labels only.
bool launch_basis_constant_on_classes(hipStream_t s, int64_t n, int64_t r, const double* U, const uint32_t* Lp, int64_t d,
                                      const uint32_t* first_idx, double atol, double scale, void* ref, uint32_t* flag) {
    if (d < 1 || d > (int64_t)REFINE_FIRST_CAP) return false;
    return with_constant<1, 2, 3, 4>((int)r, [&](auto R) {
        launch_class_compare(s, ChkBasis<decltype(R)::value>{(int)n, U, atol, scale}, Lp, d, first_idx, ref, flag);
    });
}
// a, b: symmetric n x n, column-major (the lower triangle is read); Lp, first_idx: as above (Lp8: the labels' 8-bit shadow, or null).
// false: more classes than the one-launch form holds (nothing is enqueued)
bool launch_verify_pair(hipStream_t s, int64_t n, const double* a, const double* b, const uint32_t* Lp, int64_t d, const uint32_t* first_idx,
                        uint32_t* flag, const uint8_t* Lp8) {
    if (n < 1 || n >= (int64_t(1) << 31) || d < 1 || d > VERIFY_LDS_CAP) return false;
    const ChkPair chk{SrcPair{a, b, (int)n, 1}};
    if (Lp8 && d <= 255) launch_class_compare(s, chk, Lp8, d, first_idx, nullptr, flag);
    else launch_class_compare(s, chk, Lp, d, first_idx, nullptr, flag);
    return true;
}

// q: SIG_JOINT_I32 or SIG_CHAN_I32 on the packed lower triangle with packed labels (q.L = Lp); flag[0] = verdict.
// Returns false when there is no instance for the shape (the caller runs the refinement).
bool verify_no_split_supports(const SigSource& q, int64_t d) {
    if (!q.packed || !q.lab_packed || d < 1 || d > (int64_t)REFINE_FIRST_CAP || (q.T != 2 && q.T != 4)) return false;
    return q.kind == SIG_CHAN_I32 || (q.kind == SIG_JOINT_I32 && q.r >= 0 && q.r <= 4);
}
template <int R, int T, bool JOINT>
static void launch_verify_rt(hipStream_t s, const SigSource& q, int64_t d, const uint32_t* first_idx, void* ref, uint32_t* flag) {
    const ChkStep<R, T, JOINT> chk{(int)q.n, q.ld, q.U, q.coef, q.atol, q.scale, (const int32_t*)q.C, q.key, {}};
    // the labels' 8-bit shadow -- except in the two joint instances whose byte form needs 4 more VGPRs than a wave per SIMD allows
    // (74 against 70, 97 against 93: occupancy 6 against 7 and 4 against 5): those keep the wide labels
    constexpr bool byte_form = !(JOINT && T == 2 && (R == 2 || R == 4));
    if constexpr (byte_form) {
        if (q.L8 && d <= 255) {
            launch_class_compare(s, chk, q.L8, d, first_idx, ref, flag);
            return;
        }
    }
    launch_class_compare(s, chk, q.L, d, first_idx, ref, flag);
}
bool launch_verify_projection(hipStream_t s, const SigSource& q, int64_t d, const uint32_t* first_idx, uint32_t* flag) {
    if (q.kind != SIG_JOINT_I32 || !q.packed || !q.lab_packed || d < 1 || d > VERIFY_LDS_CAP) return false;
    return with_constant<1, 2, 3, 4>(q.r, [&](auto R) {
        const ChkProj<decltype(R)::value> chk{(int)q.n, q.U, q.coef, q.atol, q.scale, q.key, {}};
        if (q.L8 && d <= 255) launch_class_compare(s, chk, q.L8, d, first_idx, nullptr, flag);
        else launch_class_compare(s, chk, q.L, d, first_idx, nullptr, flag);
    });
}
bool launch_verify_no_split(hipStream_t s, const SigSource& q, int64_t d, const uint32_t* first_idx, void* ref, uint32_t* flag) {
    if (!verify_no_split_supports(q, d)) return false;
    with_constant<2, 4>(q.T, [&](auto T) {
        if (q.kind == SIG_CHAN_I32) launch_verify_rt<0, decltype(T)::value, false>(s, q, d, first_idx, ref, flag);
        else with_constant<0, 1, 2, 3, 4>(q.r, [&](auto R) { launch_verify_rt<decltype(R)::value, decltype(T)::value, true>(s, q, d, first_idx, ref, flag); });
    });
    return true;
}

}  // namespace sdpsr
