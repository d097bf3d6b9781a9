// eigen_decomposition + irreducible_decomposition (src/eigen_decomposition.jl:14-41,83-139,163-348)
// with the dense eigensolver: the device orchestration as steps over one state each (EigDec, Irreducible); the host
// arithmetic is iso_classes.h.  Entry points sdpsr_eigen_decomposition(_batched), sdpsr_syev_f64.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "host_internal.h"

using namespace sdpsr;

namespace sdpsr {

constexpr const char* NOT_SYMMETRIC =
    "partition is not symmetric: decomposition over Float64 requested but the generic element has a complex spectrum";

static int kpartition_status(sdpsr_ctx* c, DisjointSets& K, std::vector<int>& kpart) {
    return kpartition(K, kpart) ? SDPSR_OK : ctx_fail(c, SDPSR_NUMERICAL_INCONSISTENCY, KPARTITION_INCONSISTENT);
}

// Otsu threshold + union-find + __isconsistent on a symmetric neig x neig coupling matrix
// (src/eigen_decomposition.jl:205-217, :163-167, :264-270)
int isomorphism_classes(sdpsr_ctx* c, const std::vector<double>& norms, int neig, double atol,
                        std::vector<int>& kpart) {
    const double thr = otsu_threshold(norms, atol);
    DisjointSets K(neig);
    unite_coupled(K, norms, neig, thr);
    return kpartition_status(c, K, kpart);
}

// The same with the coupling matrix on the device (kernels_blockdiag.hip coupling_*): the matrix is symmetrised with the
// dimension rule there, the host sees its extrema, the 18 counts and one bit per pair.  The union-find visits the
// pairs in the reference's order (i, then j > i); a pair whose ends already share a root is a no-op there too.
// `trace` (tests): the edges and the threshold the host formed on the way.
int isomorphism_classes_device(sdpsr_ctx* c, unsigned long long* dnorms, int neig, const std::vector<int32_t>& dims, double atol,
                               std::vector<int>& kpart, CouplingTrace* trace) {
    hipStream_t s = c->stream;
    const int W = (neig + 63) / 64;
    int32_t* ddims = (int32_t*)ctx_buf(c, "bd_dims", (size_t)neig * 4);
    unsigned long long* stat = (unsigned long long*)ctx_buf(c, "bd_cstat", 32 * 8);
    unsigned long long* dbits = (unsigned long long*)ctx_buf(c, "bd_cbits", (size_t)neig * W * 8);
    if (!ddims || !stat || !dbits) return SDPSR_OUT_OF_MEMORY;
    int st = h2d_sync(c, ddims, dims.data(), (size_t)neig * 4);
    if (st) return st;
    HIP_TRY(c, hipMemsetAsync(stat, 0, 32 * 8, s));
    launch_coupling_symmetrize_minmax(s, neig, dnorms, ddims, stat);
    unsigned long long hs[32];
    st = d2h_sync(c, hs, stat, 16);
    if (st) return st;
    double mn = INFINITY, mx;
    const unsigned long long mn_bits = ~hs[0];
    if (hs[0]) memcpy(&mn, &mn_bits, 8);
    memcpy(&mx, &hs[1], 8);
    double edges[OTSU_NB + 1];
    otsu_edges(mn, mx, atol, edges);
    launch_coupling_count(s, neig, dnorms, edges, stat);
    st = d2h_sync(c, hs, stat, 20 * 8);
    if (st) return st;
    int64_t cnt[OTSU_NB + 2];
    for (int q = 0; q <= 17; ++q) cnt[q] = (int64_t)hs[2 + q];
    const double thr = otsu_pick(edges, cnt);
    if (trace) {
        memcpy(trace->edges, edges, sizeof(edges));
        trace->thr = thr;
    }
    launch_coupling_bits(s, neig, dnorms, thr, dbits);
    const unsigned long long* hb = (const unsigned long long*)ctx_pinned(c, (size_t)neig * W * 8);
    if (!hb) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "pinned staging");
    HIP_TRY(c, hipMemcpyAsync((void*)hb, dbits, (size_t)neig * W * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, ctx_sync_stream(c, s));
    DisjointSets K(neig);
    unite_pair_bits(K, hb, neig, W);
    return kpartition_status(c, K, kpart);
}

int make_element(sdpsr_ctx* c, const ElemGen* gen, int64_t n, int64_t ld, const uint32_t* L, double* dst) {
    if (gen) return gen->make(dst);
    launch_gather_f64_padded(c->stream, n, ld, L, next_key(c), dst);
    return SDPSR_OK;
}

// eigen_decomposition (src/eigen_decomposition.jl:236-273) on the device, step by step
struct EigDec {
    sdpsr_ctx* c;
    int64_t n, ld;
    const uint32_t* L;
    const ElemGen* gen;
    double atol;
    int64_t expect_dim;
    EigInfo& info;
    PhaseTimer& tm;
    hipStream_t s;
    uint32_t* flag = nullptr;
    double *Q = nullptr, *Ap = nullptr, *Tp = nullptr, *w = nullptr;  // "bd_q", "bd_a", "bd_t", "bd_w"
    int32_t* dspace = nullptr;                                        // "bd_space", or its words inside "bd_pack"
    unsigned long long* dnorms = nullptr;                             // "bd_norms", or its words inside "bd_pack"
    bool prefetched = false;  // the second generic element is being formed on the side stream and is not joined yet
    bool one_readback = false;
    int neig = 0;
    std::vector<double> norms;  // host copy of the coupling matrix
    bool have_norms = false;    // ... filled by the one read-back

    EigDec(sdpsr_ctx* ctx, int64_t n_, const uint32_t* L_, const ElemGen* g, double atol_, int64_t expect, EigInfo& i, PhaseTimer& t)
        : c(ctx), n(n_), ld(round_up(n_, 128)), L(L_), gen(g), atol(atol_), expect_dim(expect), info(i), tm(t), s(ctx->stream) {}
    ~EigDec() {  // every return: never leave side-stream work behind, nor a phase open
        if (prefetched) gen->join();
        tm.end();
    }
    int dimof(int b) const { return info.ptrs[b + 1] - info.ptrs[b]; }

    int buffers();
    int symmetry_verdict();
    int first_element_and_eigensolver();
    int second_element();
    int cluster_one_readback();
    int cluster_on_host();
    void couple();
    int raise_coupling();
    int classes_on_device();
    int classes_on_host(bool reuse_norms);
    int classes();
    int run();
};

int EigDec::buffers() {
    flag = (uint32_t*)ctx_buf(c, "bd_flag", 64);
    Q = (double*)ctx_buf(c, "bd_q", (size_t)ld * ld * 8);
    Ap = (double*)ctx_buf(c, "bd_a", (size_t)ld * ld * 8);
    Tp = (double*)ctx_buf(c, "bd_t", (size_t)ld * ld * 8);
    w = (double*)ctx_buf(c, "bd_w", (size_t)n * 8);
    return (!flag || !Q || !Ap || !Tp || !w) ? SDPSR_OUT_OF_MEMORY : SDPSR_OK;
}

// a non-symmetric partition has a non-symmetric generic element: eigen() leaves the reals
// (src/eigen_decomposition.jl:247-253)
int EigDec::symmetry_verdict() {
    if (gen || c->bd_trusted_symmetric == L) return SDPSR_OK;
    const bool pre = c->bd_sym_epoch != 0 && c->bd_sym_labels == L;  // checked by the copy pass of blockDiagonalize
    const uint32_t* fsrc = flag;
    if (pre) fsrc = (const uint32_t*)ctx_buf(c, "bd_symflag", 64);
    else launch_check_symmetric(s, n, L, flag);
    uint32_t* hflag = (uint32_t*)c->pinned;
    HIP_TRY(c, hipMemcpyAsync(hflag, fsrc, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, ctx_sync_stream(c, s));
    if (pre ? hflag[0] == c->bd_sym_epoch : hflag[0] != 0) return ctx_fail(c, SDPSR_INVALID_DECOMPOSITION_FIELD, NOT_SYMMETRIC);
    return SDPSR_OK;
}

// Step 1-2: generic element and its eigendecomposition (:242-254)
int EigDec::first_element_and_eigensolver() {
    tm.begin(SDPSR_T_EIGEN);
    int st = make_element(c, gen, n, ld, L, Q);
    if (st) return st;
    dbg_mark(c, "eigen_decomposition: element made");
    info.vals.resize(n);
    // Small compressed problems (one-workgroup eigensolver, one-workgroup Q'AQ): the eigenvalues are
    // clustered on the device, so the status and values of the eigensolver, the eigenspaces and the block
    // norms come back in ONE read-back (SDPSR_SMALL_TWO_READBACKS=1: one after the eigensolver for the
    // clustering on the host, one after the norms)
    one_readback = gen && n <= 64 && (c->opts.eig_driver == 0 || c->opts.eig_driver >= 4);
    double* host_w = one_readback ? nullptr : info.vals.data();
    // the second generic element does not depend on the eigendecomposition of the first: when
    // the generator can, it is formed on a side stream while the (one-workgroup) eigensolver runs
    if (gen && gen->prefetch && gen->join && gen->fork && gen->fork() == SDPSR_OK) {
        const std::function<void()> after = [&]() { prefetched = gen->prefetch(Ap) == SDPSR_OK; };
        st = syev_device(c, n, Q, ld, w, host_w, &after, one_readback);
    } else {
        prefetched = gen && gen->prefetch && gen->join && gen->prefetch(Ap) == SDPSR_OK;
        st = syev_device(c, n, Q, ld, w, host_w, nullptr, one_readback);
    }
    dbg_mark(c, "eigen_decomposition: syev returned");
    tm.end();
    return st;
}

// the second generic element into Ap: the prefetched one, or a fresh one
int EigDec::second_element() {
    const bool join = prefetched;
    prefetched = false;
    const int st = join ? gen->join() : make_element(c, gen, n, ld, L, Ap);
    if (st == SDPSR_OK) info.t_valid = true;
    return st;
}

// Step 3 enqueued behind the eigensolver: second generic element, clustering + Q'AQ + block norms, one read-back
int EigDec::cluster_one_readback() {
    tm.begin(SDPSR_T_ISO);
    const size_t o_space = 64, o_vals = o_space + (((size_t)n * 4 + 63) / 64) * 64, o_norms = o_vals + (size_t)n * 8;
    const size_t pack_bytes = small_cluster_pack_bytes(n);
    char* dpack = (char*)ctx_buf(c, "bd_pack", pack_bytes);
    int* dinfo = (int*)ctx_buf(c, "eig_info", 64);
    char* hp = (char*)ctx_pinned(c, pack_bytes);
    if (!dpack || !dinfo || !hp) return SDPSR_OUT_OF_MEMORY;
    dspace = (int32_t*)(dpack + o_space);  // stay valid for the launches of a retry
    dnorms = (unsigned long long*)(dpack + o_norms);
    int st = second_element();
    if (st) return st;
    launch_small_cluster_qtaq_block_norms(s, n, ld, Ap, Q, w, atol, dinfo, dpack, Tp);
    tm.end();
    HIP_TRY(c, hipMemcpyAsync(hp, dpack, pack_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, ctx_sync_stream(c, s));
    tm.collect();
    const int hinfo = ((const int*)hp)[0];
    if (dbg_on()) fprintf(stderr, "[sdpsr] small syev n=%lld: %d sweeps\n", (long long)n, ((const int*)hp)[1]);
    if (hinfo != 0) return ctx_fail(c, SDPSR_SOLVER_ERROR, "eigensolver did not converge, info=" + std::to_string(hinfo));
    neig = ((const int*)hp)[4];
    if (neig < 1 || neig > n) return ctx_fail(c, SDPSR_SOLVER_ERROR, "eigenvalue clustering on the device returned nonsense");
    memcpy(info.vals.data(), hp + o_vals, (size_t)n * 8);
    const int32_t* hs = (const int32_t*)(hp + o_space);
    info.ptrs.assign(1, 0);
    for (int64_t i = 1; i < n; ++i)
        if (hs[i] != hs[i - 1]) info.ptrs.push_back((int)i);
    info.ptrs.push_back((int)n);
    if ((int)info.ptrs.size() - 1 != neig) return ctx_fail(c, SDPSR_SOLVER_ERROR, "eigenvalue clustering on the device is inconsistent");
    norms.resize((size_t)neig * neig);
    memcpy(norms.data(), hp + o_norms, (size_t)neig * neig * 8);
    have_norms = true;
    return SDPSR_OK;
}

// the eigenvalues are on the host: clustering there, then Step 3: second generic element, Q'AQ, block norms (:259-262, :201-205)
int EigDec::cluster_on_host() {
    tm.collect();
    info.ptrs = eigenspace_ptrs(info.vals.data(), n, atol);
    neig = (int)info.ptrs.size() - 1;
    const std::vector<int32_t> space_of = space_of_ptrs(info.ptrs);
    tm.begin(SDPSR_T_ISO);
    dnorms = (unsigned long long*)ctx_buf(c, "bd_norms", (size_t)neig * neig * 8);
    if (!dnorms) return SDPSR_OUT_OF_MEMORY;
    int st = h2d_sync(c, dspace, space_of.data(), n * 4);
    if (st) return st;
    HIP_TRY(c, hipMemsetAsync(dnorms, 0, (size_t)neig * neig * 8, s));
    st = second_element();
    if (st) return st;
    // small (compressed) problems: one workgroup does Q'AQ and the block maxima (T = A Q goes to Tp)
    if (n <= 64) launch_small_qtaq_block_norms(s, n, ld, Ap, Q, dspace, neig, dnorms, nullptr, Tp);
    else couple();
    tm.end();
    return SDPSR_OK;
}

// the coupling matrix of the element in Ap: block_norms accumulates maxima, so a further element can only raise it
void couple_block_norms(hipStream_t s, int64_t n, int64_t ld, double* Ap, const double* Q, double* Tp, const int32_t* dspace, int neig,
                        unsigned long long* dnorms) {
    launch_gemm_tn_f64(s, ld, ld, ld, Ap, ld, Q, ld, Tp, ld, 1, 0, 0, 0);  // T = A Q (A symmetric)
    launch_gemm_tn_f64(s, ld, ld, ld, Q, ld, Tp, ld, Ap, ld, 1, 0, 0, 0);  // M = Q' T  (into Ap)
    launch_block_norms(s, n, ld, Ap, dspace, neig, dnorms);
}
void EigDec::couple() { couple_block_norms(s, n, ld, Ap, Q, Tp, dspace, neig, dnorms); }

// one more independent generic element raises the coupling matrix
int EigDec::raise_coupling() {
    info.t_valid = false;  // the classes now rest on several coupling elements
    const int st = make_element(c, gen, n, ld, L, Ap);
    if (st == SDPSR_OK) couple();
    return st;
}

// many eigenspaces: the coupling matrix stays on the device
// (a raised matrix of a later pass is symmetric already: maxima of symmetric blocks were added to both halves)
int EigDec::classes_on_device() {
    std::vector<int32_t> dims(neig);
    for (int i = 0; i < neig; ++i) dims[i] = dimof(i);
    const int st = isomorphism_classes_device(c, dnorms, neig, dims, atol, info.kpart);
    tm.collect();
    dbg_mark(c, "eigen_decomposition: Otsu + union-find done (coupling matrix on the device)");
    return st;
}

int EigDec::classes_on_host(bool reuse_norms) {
    if (!reuse_norms) {
        norms.resize((size_t)neig * neig);
        const int st = d2h_sync(c, norms.data(), dnorms, (size_t)neig * neig * 8);
        if (st) return st;
        tm.collect();
    }
    // the kernel computes the (bi, bj) max with bi = row space
    symmetrize_coupling(info.ptrs, norms.data(), norms.data());
    dbg_mark(c, "eigen_decomposition: block norms on the host");
    const int st = isomorphism_classes(c, norms, neig, atol, info.kpart);
    dbg_mark(c, "eigen_decomposition: Otsu + union-find done");
    return st;
}

// The coupling of an isomorphic pair of eigenspaces under ONE generic element is the maximum over
// an m_i x m_j block of random numbers -- a single one when the eigenspaces are 1-dimensional
// (always so in compressed problems, often in QAP- and theta'-type partitions) -- and falls below
// the Otsu threshold in ~0.1-0.5 % of the draws (measured round 2: 6 DimensionMismatch in 1000
// compressed reductions of ER(7) (x) K_72, 4 in 2000 dense ones at N = 456, against 0 in 1000 for
// the reference-literal oracle).  When the caller knows dim(P) (blockDiagonalize does) and the
// classes found do not add up to it -- the check the reference makes right afterwards,
// src/diagonalize.jl:1-11 -- or are inconsistent, the coupling matrix is raised by another
// independent generic element and the classes are formed again, up to twice (coupling_settled).
// The common case pays nothing; SDPSR_FLAG_SINGLE_COUPLING_ELEMENT keeps the reference's single element (:259-262).
int EigDec::classes() {
    const bool on_device = !have_norms && neig >= 256 && !(c->opts.flags & SDPSR_FLAG_COUPLING_ON_HOST);
    const bool single = (c->opts.flags & SDPSR_FLAG_SINGLE_COUPLING_ELEMENT) != 0;
    const auto verdict = [](int st) { return st == SDPSR_OK || st == SDPSR_NUMERICAL_INCONSISTENCY; };
    int extra = 0;
    int st = on_device ? classes_on_device() : classes_on_host(have_norms);
    while (verdict(st) && !coupling_settled(extra, expect_dim, single, st == SDPSR_OK, info.kpart)) {
        ++extra;
        st = raise_coupling();
        if (st == SDPSR_OK) st = on_device ? classes_on_device() : classes_on_host(false);
    }
    if (st == SDPSR_OK) c->err.clear();  // (the message of an inconsistent earlier pass)
    return st;
}

int EigDec::run() {
    int st = buffers();
    if (!st) st = symmetry_verdict();
    if (!st) st = first_element_and_eigensolver();
    if (st) return st;
    dspace = (int32_t*)ctx_buf(c, "bd_space", (size_t)n * 4 + 64);
    if (!dspace) return SDPSR_OUT_OF_MEMORY;
    st = one_readback ? cluster_one_readback() : cluster_on_host();
    if (st) return st;
    return classes();
}

// On success the padded buffers "bd_q" (eigenvectors, ld x ld) stay valid in ctx.
int eigen_decomposition_device(sdpsr_ctx* c, int64_t n, const uint32_t* L, double atol, EigInfo& info,
                               PhaseTimer& tm, const ElemGen* gen, int64_t expect_dim) {
    EigDec ed(c, n, L, gen, atol, expect_dim, info, tm);
    return ed.run();
}

// status used internally when a driver of diagonalize hands over to the dense one
int driver_fallback(sdpsr_ctx* c, const std::string& why) {
    c->err = "driver fell back to the dense eigensolver: " + why;
    if (dbg_on()) fprintf(stderr, "[sdpsr] %s\n", c->err.c_str());
    return DRIVER_FALLBACK;
}

// irreducible_decomposition (src/eigen_decomposition.jl:295-348) on the device, step by step
struct Irreducible {
    sdpsr_ctx* c;
    int64_t n, ld;
    const uint32_t* L;
    const ElemGen* gen;
    double atol;
    const EigInfo& info;
    hipStream_t s;
    int neig;
    std::vector<int> roots;  // unique(Kpartition) in first-occurrence order (:303)
    std::vector<std::vector<int>> members;
    std::vector<int> fcol;  // column of F / B of every eigenspace that sits in a merged class (-1: none)
    int nf = 0;
    double *Q = nullptr, *Qhat = nullptr, *Bf = nullptr;
    std::vector<int32_t> cp_src, cp_dst;  // first members, copied in one launch
    std::vector<int32_t> pairs;           // the other members: one workgroup each, one launch
    int64_t max_m2 = 0;

    int layout(std::vector<int32_t>& sizes, int64_t& S1, int64_t& S);
    int source_of_b();
    int fresh_b(double* A3, double* F, int64_t nfp);
    void describe_pairs();
    int launch_pairs();
};

// classes -> block sizes, Q_hat's buffer, and the first eigenvector of every eigenspace that sits in a merged class -> F
int Irreducible::layout(std::vector<int32_t>& sizes, int64_t& S1, int64_t& S) {
    class_structure(info.kpart, roots, members);
    block_sizes(members, sizes, S1, S);
    Q = (double*)ctx_buf(c, "bd_q", (size_t)ld * ld * 8);
    Qhat = (double*)ctx_buf(c, "bd_qhat", (size_t)n * S1 * 8);
    if (!Q || !Qhat) return SDPSR_OUT_OF_MEMORY;
    c->bd_qrm_current = false;  // Q_hat is rewritten here: "bd_qrm" no longer is its row-major copy
    fcol.assign(neig, -1);
    for (size_t p = 0; p < roots.size(); ++p)
        if (members[p].size() > 1)
            for (int j : members[p]) fcol[j] = nf++;
    return SDPSR_OK;
}

// B = A F: columns of the saved T = A2 Q, or the product with a fresh third element
int Irreducible::source_of_b() {
    if (nf == 0) return SDPSR_OK;
    const int64_t nfp = round_up(nf, 128);
    double* A3 = (double*)ctx_buf(c, "bd_a", (size_t)ld * ld * 8);
    double* F = (double*)ctx_buf(c, "bd_f", (size_t)ld * nfp * 8);
    Bf = (double*)ctx_buf(c, "bd_bf", (size_t)ld * nfp * 8);
    if (!A3 || !F || !Bf) return SDPSR_OUT_OF_MEMORY;
    const bool fresh = (c->opts.flags & SDPSR_FLAG_FRESH_IRREDUCIBLE_ELEMENT) != 0;
    double* Tq = (double*)ctx_buf(c, "bd_t", (size_t)ld * ld * 8);
    if (!(info.t_valid && Tq && !fresh)) return fresh_b(A3, F, nfp);
    // B = A F needs A q for the first eigenvector q of every merged eigenspace: those are
    // columns of T = A2 Q, which the isomorphism step has just formed.  The reference draws
    // a third generic element here (:306); any generic element of the algebra serves, and
    // A2 is the one whose blocks between the merged eigenspaces are known to be large
    // (they passed the Otsu threshold).  Saves an element, its products and ~neig copies.
    std::vector<int32_t> bsrc, bdst;
    for (int j = 0; j < neig; ++j)
        if (fcol[j] >= 0) {
            bsrc.push_back((int32_t)info.ptrs[j]);
            bdst.push_back((int32_t)fcol[j]);
        }
    launch_copy_cols(s, n, (int64_t)bsrc.size(), bsrc.data(), bdst.data(), Tq, ld, Bf, ld);
    return SDPSR_OK;
}

int Irreducible::fresh_b(double* A3, double* F, int64_t nfp) {
    const int st = make_element(c, gen, n, ld, L, A3);  // generic element #3 (:306)
    if (st) return st;
    HIP_TRY(c, hipMemsetAsync(F, 0, (size_t)ld * nfp * 8, s));
    for (int j = 0; j < neig; ++j)
        if (fcol[j] >= 0)
            HIP_TRY(c, hipMemcpyAsync(F + (size_t)fcol[j] * ld, Q + (size_t)info.ptrs[j] * ld, n * 8,
                                      hipMemcpyDeviceToDevice, s));
    launch_gemm_tn_f64(s, ld, nfp, ld, A3, ld, F, ld, Bf, ld, 1, 0, 0, 0);  // B = A3' F = A3 F
    return SDPSR_OK;
}

void Irreducible::describe_pairs() {
    int64_t col = 0;
    for (size_t p = 0; p < roots.size(); ++p) {
        const int i = roots[p];
        const int64_t mi = info.ptrs[i + 1] - info.ptrs[i];
        // first member: P1 = I -> first eigenvector of Ei (:311-313, :326)
        cp_src.push_back((int32_t)info.ptrs[i]);
        cp_dst.push_back((int32_t)col);
        ++col;
        for (size_t q = 1; q < members[p].size(); ++q) {
            const int j = members[p][q];
            const int64_t mj = info.ptrs[j + 1] - info.ptrs[j];
            // first column of P_blk = block(A,Ei,Ej)' is Qj' (A q_i1)  (:333); its norm is
            // || Qi' (A q_j1) ||  (:335); column of P_hat = Qj * that column, normalised (:338-344)
            const int32_t dsc[7] = {(int32_t)info.ptrs[i], (int32_t)mi, (int32_t)info.ptrs[j], (int32_t)mj,
                                    (int32_t)fcol[i], (int32_t)fcol[j], (int32_t)col};
            pairs.insert(pairs.end(), dsc, dsc + 7);
            max_m2 = std::max(max_m2, mi + mj);
            ++col;
        }
    }
}

// the pair kernel keeps w (m_j), c (m_i) and one scalar in LDS: it takes the pairs whose m_i + m_j + 2 doubles fit in 60 KiB
bool irreducible_pairs_fit_lds(int64_t max_m2) { return !((size_t)(max_m2 + 2) * 8 > 60 * 1024); }

int Irreducible::launch_pairs() { return irreducible_pairs(c, n, ld, Q, Bf, pairs, max_m2, Qhat, -1, nullptr); }

// route -1: the pair kernel where its LDS allows, else one by one; 0 / 1 (tests) ask for one of the two; *ran = the route taken
int irreducible_pairs(sdpsr_ctx* c, int64_t n, int64_t ld, const double* Q, const double* Bf, const std::vector<int32_t>& pairs,
                      int64_t max_m2, double* Qhat, int route, int* ran) {
    if (pairs.empty()) return SDPSR_OK;
    int32_t* d_pairs = (int32_t*)ctx_buf(c, "bd_pairs", pairs.size() * 4);
    if (!d_pairs) return SDPSR_OUT_OF_MEMORY;
    const int st = h2d_sync(c, d_pairs, pairs.data(), pairs.size() * 4);
    if (st) return st;
    const bool one_by_one = route < 0 ? !irreducible_pairs_fit_lds(max_m2) : route == 1;
    if (ran) *ran = one_by_one ? 1 : 0;
    if (one_by_one) return irreducible_pairs_one_by_one(c, n, ld, Q, Bf, pairs, Qhat);
    if (!irreducible_pairs_fit_lds(max_m2)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "irreducible pairs: eigenspaces too large for the pair kernel");
    launch_irreducible_pairs(c->stream, n, ld, Q, Bf, (int)(pairs.size() / 7), (int)max_m2, d_pairs, Qhat);
    return SDPSR_OK;
}

// eigenspaces too large for the LDS of the pair kernel: four small launches per pair
int irreducible_pairs_one_by_one(sdpsr_ctx* c, int64_t n, int64_t ld, const double* Q, const double* Bf, const std::vector<int32_t>& pairs,
                                 double* Qhat) {
    hipStream_t s = c->stream;
    double* wv = (double*)ctx_buf(c, "bd_wv", (size_t)n * 8);
    double* cv = (double*)ctx_buf(c, "bd_cv", (size_t)n * 8);
    double* inv = (double*)ctx_buf(c, "bd_inv", 64);
    if (!wv || !cv || !inv) return SDPSR_OUT_OF_MEMORY;
    for (size_t q = 0; q + 7 <= pairs.size(); q += 7) {
        const int32_t* dsc = pairs.data() + q;
        launch_gemv_t(s, n, ld, Q, dsc[2], dsc[3], Bf + (size_t)dsc[4] * ld, wv);
        launch_gemv_t(s, n, ld, Q, dsc[0], dsc[1], Bf + (size_t)dsc[5] * ld, cv);
        launch_inv_norm(s, dsc[1], cv, inv);
        launch_gemv_n_scaled(s, n, ld, Q, dsc[2], dsc[3], wv, inv, Qhat + (size_t)dsc[6] * n);
    }
    return SDPSR_OK;
}

// diagonalize(Float64, P) with the dense eigensolver (src/diagonalize.jl:25-40): on success the
// device buffer "bd_qhat" holds Q_hat (n x S1 column-major, classes side by side).
int dense_diagonalize(sdpsr_ctx* c, int64_t n, const uint32_t* L, const ElemGen* gen, double atol, EigInfo& info,
                      std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, PhaseTimer& tm, int64_t expect_dim) {
    int st = eigen_decomposition_device(c, n, L, atol, info, tm, gen, expect_dim);
    if (st) return st;
    PhaseScope phase(tm, SDPSR_T_IRRED, false);
    Irreducible ir{c, n, round_up(n, 128), L, gen, atol, info, c->stream, (int)info.ptrs.size() - 1};
    st = ir.layout(sizes, S1, S);
    if (!st) st = ir.source_of_b();
    if (st) return st;
    ir.describe_pairs();
    st = ir.launch_pairs();
    if (st) return st;
    launch_copy_cols(ir.s, n, (int64_t)ir.cp_src.size(), ir.cp_src.data(), ir.cp_dst.data(), ir.Q, ir.ld, ir.Qhat, n);
    launch_clamptol(ir.s, n * S1, ir.Qhat, atol);  // src/diagonalize.jl:39
    tm.end();
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

// the labels of a stand-alone eigen_decomposition entry on the device; whatever sdpsr_block_diagonalize left behind is void
static const uint32_t* fresh_labels(sdpsr_ctx* c, int64_t n, const uint32_t* P, int mem, int* st) {
    c->bd_sym_epoch = 0;  // the verdict cached by sdpsr_block_diagonalize belongs to the labels it copied, not to these
    c->bd_sym_labels = nullptr;
    c->bd_trusted_symmetric = nullptr;
    c->bd_labels_ext = nullptr;
    const uint32_t* L = labels_in_dev(c, "bd_labels", P, (size_t)n * n, mem, st);
    if (!*st) c->bd_valid = false;
    return L;
}

// n <= 64: one workgroup per run, matrices in LDS (kernels_batched.hip); out: count statuses, then neig, then nclasses
static int eigdec_batched_small(sdpsr_ctx* c, int64_t n, const uint32_t* L, int64_t d, double atol, int64_t count, const double* values,
                                int mem, int32_t* out) {
    hipStream_t s = c->stream;
    int st = SDPSR_OK;
    uint32_t* flag = (uint32_t*)ctx_buf(c, "bd_flag", 64);
    int32_t* dout = (int32_t*)ctx_buf(c, "be_out", (size_t)count * 3 * 4);
    if (!flag || !dout) return SDPSR_OUT_OF_MEMORY;
    const double* dvals = nullptr;
    if (values) {
        dvals = in_dev(c, "be_values", values, (size_t)2 * count * std::max<int64_t>(d, 1), mem, &st);
        if (st) return st;
    }
    launch_check_symmetric(s, n, L, flag);
    launch_eigdec_batched64(s, n, d, count, L, dvals, c->seed, c->stream_counter, atol, dout, dout + count,
                            dout + 2 * count, c->num_cus);
    c->stream_counter += 2 * (uint64_t)count;
    HIP_TRY(c, hipGetLastError());
    int32_t* hp = (int32_t*)ctx_pinned(c, (size_t)count * 3 * 4 + 64);
    if (!hp) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "pinned staging");
    HIP_TRY(c, hipMemcpyAsync(hp, flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hp + 16, dout, (size_t)count * 3 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, ctx_sync_stream(c, s));
    if (hp[0]) return ctx_fail(c, SDPSR_INVALID_DECOMPOSITION_FIELD, NOT_SYMMETRIC);
    memcpy(out, hp + 16, (size_t)count * 3 * 4);
    return SDPSR_OK;
}

// larger orders: the runs go through the single-problem path one after the other
static int eigdec_batched_serial(sdpsr_ctx* c, int64_t n, const uint32_t* L, double atol, int64_t count, int32_t* out) {
    for (int64_t r = 0; r < count; ++r) {
        EigInfo info;
        PhaseTimer tm(c, false);
        const int e = eigen_decomposition_device(c, n, L, atol, info, tm);
        if (e != SDPSR_OK && e != SDPSR_NUMERICAL_INCONSISTENCY && e != SDPSR_SOLVER_ERROR) return e;
        out[r] = e;
        if (e == SDPSR_OK) {
            out[count + r] = (int32_t)info.ptrs.size() - 1;
            out[2 * count + r] = count_classes(info.kpart);
        }
    }
    return SDPSR_OK;
}

}  // namespace sdpsr

extern "C" {

int sdpsr_eigen_decomposition(sdpsr_ctx* c, int64_t n, const uint32_t* P, int64_t d, double atol,
                              int32_t* neig, int32_t* nclasses, int mem) {
    CHECK_CTX(c);
    (void)d;
    if (!P || n < 1 || !(atol > 0)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = check_len(c, n * n);
    if (st) return st;
    const uint32_t* L = fresh_labels(c, n, P, mem, &st);
    if (st) return st;
    EigInfo info;
    PhaseTimer tm(c, false);
    st = eigen_decomposition_device(c, n, L, atol, info, tm);
    if (st) return st;
    if (neig) *neig = (int32_t)info.ptrs.size() - 1;
    if (nclasses) *nclasses = count_classes(info.kpart);
    return SDPSR_OK;
}

int sdpsr_eigen_decomposition_batched(sdpsr_ctx* c, int64_t n, const uint32_t* P, int64_t d, double atol,
                                      int64_t count, const double* values, int32_t* status, int32_t* neig,
                                      int32_t* nclasses, int mem) {
    CHECK_CTX(c);
    if (!P || n < 1 || d < 0 || count < 1 || count > (int64_t)1 << 24 || !(atol > 0))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = check_len(c, n * n);
    if (st) return st;
    const uint32_t* L = fresh_labels(c, n, P, mem, &st);
    if (st) return st;
    std::vector<int32_t> h(3 * (size_t)count, 0);  // statuses, neig, nclasses
    if (n > 64 && values) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "explicit class values are supported for n <= 64 only");
    st = n <= 64 ? eigdec_batched_small(c, n, L, d, atol, count, values, mem, h.data()) : eigdec_batched_serial(c, n, L, atol, count, h.data());
    if (st) return st;
    if (status) memcpy(status, h.data(), (size_t)count * 4);
    if (neig) memcpy(neig, h.data() + count, (size_t)count * 4);
    if (nclasses) memcpy(nclasses, h.data() + 2 * count, (size_t)count * 4);
    for (int64_t r = 0; r < count; ++r)
        if (h[r] != SDPSR_OK) {
            const char* what = h[r] == SDPSR_NUMERICAL_INCONSISTENCY ? KPARTITION_INCONSISTENT : "eigensolver did not converge";
            return ctx_fail(c, h[r], "run " + std::to_string(r) + ": " + what);
        }
    return SDPSR_OK;
}

int sdpsr_syev_f64(sdpsr_ctx* c, int64_t n, const double* A, double* values, double* vectors, int mem) {
    CHECK_CTX(c);
    if (!A || !values || !vectors || n < 1) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = SDPSR_OK;
    const double* dA = in_dev(c, "ev_in", A, (size_t)n * n, mem, &st);
    double* dV = out_dev(c, "ev_vec", vectors, (size_t)n * n, mem, &st);
    double* dW = out_dev(c, "ev_val", values, (size_t)n, mem, &st);
    if (st) return st;
    const int64_t ld = round_up(n, 128);
    double* Ap = (double*)ctx_buf(c, "ev_pad", (size_t)ld * ld * 8);
    void* scale = ctx_buf(c, "ev_scale", 64);
    if (!Ap || !scale) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemsetAsync(Ap, 0, (size_t)ld * ld * 8, c->stream));
    // the copy into the padded buffer brings max |a| into [2^-400, 2^400] by a power of two (kernels_sytrd.hip: the solver's
    // norms are sums of squares); the factor stays on the device and is 1 for every input inside the window
    launch_syev_scaled_copy(c->stream, n, dA, ld, Ap, scale);
    HIP_TRY(c, hipGetLastError());
    st = syev_device(c, n, Ap, ld, dW);
    if (st) return st;
    launch_syev_unscale_values(c->stream, n, dW, scale);
    HIP_TRY(c, hipMemcpy2DAsync(dV, n * 8, Ap, ld * 8, n * 8, n, hipMemcpyDeviceToDevice, c->stream));
    st = out_finish(c, vectors, dV, (size_t)n * n, mem);
    if (st) return st;
    return out_finish(c, values, dW, (size_t)n, mem);
}

}  // extern "C"
