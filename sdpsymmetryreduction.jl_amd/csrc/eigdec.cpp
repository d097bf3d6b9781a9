// eigen_decomposition + irreducible_decomposition (src/eigen_decomposition.jl:14-41,83-139,163-348)
// with the dense eigensolver: host pieces (clustering, Otsu threshold, union-find, consistency check)
// and the device orchestration; entry points sdpsr_eigen_decomposition(_batched), sdpsr_syev_f64.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <functional>
#include <numeric>

#include "host_internal.h"

using namespace sdpsr;

namespace sdpsr {


// DataStructures.jl IntDisjointSets (union by rank, path compression) as used at
// src/eigen_decomposition.jl:208-217
struct DisjointSets {
    std::vector<int> parent, rank;
    explicit DisjointSets(int n) : parent(n), rank(n, 0) { std::iota(parent.begin(), parent.end(), 0); }
    int find(int x) {
        int r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) {
            int nx = parent[x];
            parent[x] = r;
            x = nx;
        }
        return r;
    }
    void unite(int x, int y) {
        x = find(x);
        y = find(y);
        if (x == y) return;
        if (rank[x] < rank[y]) std::swap(x, y);
        else if (rank[x] == rank[y]) ++rank[x];
        parent[y] = x;
    }
};

// otsu_threshold + log_histogram, src/eigen_decomposition.jl:83-139, in three steps so that the values may stay on
// the device (isomorphism_classes_device): extrema -> edges, counts per number of edges below a value -> threshold
constexpr int OTSU_NB = 16;  // max(ceil(-log10(eps(Float64))), 4)
static void otsu_edges(double mn, double mx, double atol, double (&edges)[OTSU_NB + 1]) {
    if (mn < atol) mn = atol;
    const double l0 = std::log(mn), l1 = std::log(mx);
    for (int i = 0; i <= OTSU_NB; ++i) {
        // Julia range(a, b, length=n): a + i*(b-a)/(n-1), endpoints exact
        double t = (i == OTSU_NB) ? l1 : l0 + (l1 - l0) * (double)i / (double)OTSU_NB;
        edges[i] = std::exp(t);
    }
}
// cnt[c], c = 0..17: number of values with exactly c edges <= them (a NaN: 17)
static double otsu_pick(const double (&edges)[OTSU_NB + 1], const int64_t (&cnt)[OTSU_NB + 2]) {
    const int nb = OTSU_NB;
    std::vector<double> counts(nb, 0.0);
    {
        // something(findfirst(b -> b > x, edges), nb + 1) (1-based) = 1 + #{edges <= x} for ascending edges;
        // f = min(c + 1, nb + 1): no edge above x (c = 17: x >= the last edge, or a NaN) is the default nb + 1
        std::vector<int64_t> hist(nb + 2, 0);
        for (int cidx = 0; cidx <= 17; ++cidx) hist[cidx + 1 < nb + 1 ? cidx + 1 : nb + 1] += cnt[cidx];
        for (int f = 1; f <= nb + 1; ++f) {
            const int bin = std::min(std::max(f - 1, 1), nb);
            counts[bin - 1] += (double)hist[f];
        }
    }
    double total = 0;
    for (double v : counts) total += v;
    std::vector<double> w(nb), mu(nb);
    double cw = 0, cm = 0;
    for (int i = 0; i < nb; ++i) {
        double p = counts[i] / total;
        cw += p;
        cm += std::log(edges[i]) * p;
        w[i] = cw;
        mu[i] = cm;
    }
    const double muT = mu[nb - 1];
    int best = 0;
    double bestv = -INFINITY;
    bool have_nan = false;
    for (int i = 0; i < nb - 1; ++i) {
        double num = muT * w[i] - mu[i];
        double s2 = num * num / (w[i] * (1 - w[i]));
        if (std::isnan(s2)) {  // Julia argmax returns the first NaN
            if (!have_nan) {
                best = i;
                have_nan = true;
            }
        } else if (!have_nan && s2 > bestv) {
            bestv = s2;
            best = i;
        }
    }
    return edges[best + 1];
}
double otsu_threshold(const std::vector<double>& X, double atol) {
    double mn = INFINITY, mx = 0;
    {  // eight independent running minima / maxima (one chain is bound by the latency of min / max: 2 x 4 clocks per value)
        double mns[8], mxs[8];
        for (int q = 0; q < 8; ++q) mns[q] = INFINITY, mxs[q] = 0;
        const size_t nx = X.size(), n8 = nx & ~size_t(7);
        const double* xp = X.data();
        for (size_t e = 0; e < n8; e += 8)
            for (int q = 0; q < 8; ++q) {
                const double a = std::fabs(xp[e + q]);
                mns[q] = std::min(mns[q], a);  // std::min(a, b) = (b < a) ? b : a: a NaN in b never replaces a, as in the scalar loop
                mxs[q] = std::max(mxs[q], a);
            }
        for (size_t e = n8; e < nx; ++e) {
            const double a = std::fabs(xp[e]);
            mns[0] = std::min(mns[0], a);
            mxs[0] = std::max(mxs[0], a);
        }
        for (int q = 0; q < 8; ++q) mn = std::min(mn, mns[q]), mx = std::max(mx, mxs[q]);
    }
    double edges[OTSU_NB + 1];
    otsu_edges(mn, mx, atol, edges);
    // counted without branches (the loop vectorises; neig^2 values go through it)
    int64_t cnt[OTSU_NB + 2];
    host_count_edges17(X.data(), X.size(), edges, cnt);  // cnt[c]: c edges <= x
    return otsu_pick(edges, cnt);
}


// Otsu threshold + union-find + __isconsistent on a symmetric neig x neig coupling matrix
// (src/eigen_decomposition.jl:205-217, :163-167, :264-270)
int isomorphism_classes(sdpsr_ctx* c, const std::vector<double>& norms, int neig, double atol,
                        std::vector<int>& kpart) {
    const double thr = otsu_threshold(norms, atol);
    DisjointSets K(neig);
    for (int i = 0; i < neig; ++i)
        for (int j = i + 1; j < neig; ++j)
            if (norms[(size_t)i * neig + j] >= thr) K.unite(i, j);
    kpart.resize(neig);
    for (int i = 0; i < neig; ++i) kpart[i] = K.find(i);
    std::vector<int> first(neig, -1);
    for (int i = 0; i < neig; ++i)
        if (first[kpart[i]] < 0) first[kpart[i]] = i;
    for (int i = 0; i < neig; ++i)
        if (first[kpart[i]] != kpart[i])
            return ctx_fail(c, SDPSR_NUMERICAL_INCONSISTENCY,
                            "eigen_decomposition: the K-partition seems inconsistent with eigenspaces. Decrease atol, or simply try again.");
    return SDPSR_OK;
}

// The same with the coupling matrix on the device (kernels_blockdiag.hip coupling_*): the matrix is symmetrised with the
// dimension rule there, the host sees its extrema, the 18 counts and one bit per pair.  The union-find visits the
// pairs in the reference's order (i, then j > i); a pair whose ends already share a root is a no-op there too.
int isomorphism_classes_device(sdpsr_ctx* c, unsigned long long* dnorms, int neig, const std::vector<int32_t>& dims, double atol,
                               std::vector<int>& kpart) {
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
    auto as_double = [](unsigned long long b) {
        double x;
        memcpy(&x, &b, 8);
        return x;
    };
    const double mn = hs[0] ? as_double(~hs[0]) : INFINITY, mx = as_double(hs[1]);
    double edges[OTSU_NB + 1];
    otsu_edges(mn, mx, atol, edges);
    launch_coupling_count(s, neig, dnorms, edges, stat);
    st = d2h_sync(c, hs, stat, 20 * 8);
    if (st) return st;
    int64_t cnt[OTSU_NB + 2];
    for (int q = 0; q <= 17; ++q) cnt[q] = (int64_t)hs[2 + q];
    const double thr = otsu_pick(edges, cnt);
    launch_coupling_bits(s, neig, dnorms, thr, dbits);
    const unsigned long long* hb = (const unsigned long long*)ctx_pinned(c, (size_t)neig * W * 8);
    if (!hb) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "pinned staging");
    HIP_TRY(c, hipMemcpyAsync((void*)hb, dbits, (size_t)neig * W * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, ctx_sync_stream(c, s));
    DisjointSets K(neig);
    for (int i = 0; i < neig; ++i) {
        const unsigned long long* row = hb + (size_t)i * W;
        for (int w = i / 64; w < W; ++w) {
            unsigned long long m = row[w];
            while (m) {
                const int j = 64 * w + __builtin_ctzll(m);
                m &= m - 1;
                K.unite(i, j);
            }
        }
    }
    kpart.resize(neig);
    for (int i = 0; i < neig; ++i) kpart[i] = K.find(i);
    std::vector<int> first(neig, -1);
    for (int i = 0; i < neig; ++i)
        if (first[kpart[i]] < 0) first[kpart[i]] = i;
    for (int i = 0; i < neig; ++i)
        if (first[kpart[i]] != kpart[i])
            return ctx_fail(c, SDPSR_NUMERICAL_INCONSISTENCY,
                            "eigen_decomposition: the K-partition seems inconsistent with eigenspaces. Decrease atol, or simply try again.");
    return SDPSR_OK;
}

// roots (first-occurrence order, src/eigen_decomposition.jl:303) and members of every class
void class_structure(const std::vector<int>& kpart, std::vector<int>& roots, std::vector<std::vector<int>>& members) {
    const int neig = (int)kpart.size();
    roots.clear();
    std::vector<char> seen(neig, 0);
    for (int i = 0; i < neig; ++i)
        if (!seen[kpart[i]]) {
            seen[kpart[i]] = 1;
            roots.push_back(kpart[i]);
        }
    members.assign(roots.size(), {});
    std::vector<int> root_pos(neig, -1);
    for (size_t p = 0; p < roots.size(); ++p) root_pos[roots[p]] = (int)p;
    for (int i = 0; i < neig; ++i) members[root_pos[kpart[i]]].push_back(i);
}
int make_element(sdpsr_ctx* c, const ElemGen* gen, int64_t n, int64_t ld, const uint32_t* L, double* dst) {
    if (gen) return gen->make(dst);
    launch_gather_f64_padded(c->stream, n, ld, L, next_key(c), dst);
    return SDPSR_OK;
}

// eigen_decomposition (src/eigen_decomposition.jl:236-273) on the device.  On success the
// padded buffers "bd_q" (eigenvectors, ld x ld) stay valid in ctx.
int eigen_decomposition_device(sdpsr_ctx* c, int64_t n, const uint32_t* L, double atol, EigInfo& info,
                               PhaseTimer& tm, const ElemGen* gen, int64_t expect_dim) {
    hipStream_t s = c->stream;
    const int64_t ld = round_up(n, 128);
    uint32_t* flag = (uint32_t*)ctx_buf(c, "bd_flag", 64);
    double* Q = (double*)ctx_buf(c, "bd_q", (size_t)ld * ld * 8);
    double* Ap = (double*)ctx_buf(c, "bd_a", (size_t)ld * ld * 8);
    double* Tp = (double*)ctx_buf(c, "bd_t", (size_t)ld * ld * 8);
    double* w = (double*)ctx_buf(c, "bd_w", (size_t)n * 8);
    if (!flag || !Q || !Ap || !Tp || !w) return SDPSR_OUT_OF_MEMORY;
    // a non-symmetric partition has a non-symmetric generic element: eigen() leaves the reals
    // (src/eigen_decomposition.jl:247-253)
    if (!gen && c->bd_trusted_symmetric != L) {
        const bool pre = c->bd_sym_epoch != 0 && c->bd_sym_labels == L;  // checked by the copy pass of blockDiagonalize
        const uint32_t* fsrc = flag;
        if (pre) fsrc = (const uint32_t*)ctx_buf(c, "bd_symflag", 64);
        else launch_check_symmetric(s, n, L, flag);
        uint32_t* hflag = (uint32_t*)c->pinned;
        HIP_TRY(c, hipMemcpyAsync(hflag, fsrc, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, ctx_sync_stream(c, s));
        if (pre ? hflag[0] == c->bd_sym_epoch : hflag[0] != 0) return ctx_fail(c, SDPSR_INVALID_DECOMPOSITION_FIELD,
                                      "partition is not symmetric: decomposition over Float64 requested but the generic element has a complex spectrum");
    }
    // Step 1-2: generic element and its eigendecomposition (:242-254)
    tm.begin(SDPSR_T_EIGEN);
    int st = make_element(c, gen, n, ld, L, Q);
    if (st) return st;
    dbg_mark(c, "eigen_decomposition: element made");
    // the second generic element does not depend on the eigendecomposition of the first: when
    // the generator can, it is formed on a side stream while the (one-workgroup) eigensolver runs
    bool prefetched = false;
    info.vals.resize(n);
    // Small compressed problems (one-workgroup eigensolver, one-workgroup Q'AQ): the eigenvalues are
    // clustered on the device, so the status and values of the eigensolver, the eigenspaces and the block
    // norms come back in ONE read-back (SDPSR_SMALL_TWO_READBACKS=1: one after the eigensolver for the
    // clustering on the host, one after the norms)
    const bool one_readback = gen && n <= 64 && (c->opts.eig_driver == 0 || c->opts.eig_driver >= 4);
    if (gen && gen->prefetch && gen->join && gen->fork && gen->fork() == SDPSR_OK) {
        const std::function<void()> after = [&]() { prefetched = gen->prefetch(Ap) == SDPSR_OK; };
        st = syev_device(c, n, Q, ld, w, one_readback ? nullptr : info.vals.data(), &after, one_readback);
    } else {
        prefetched = gen && gen->prefetch && gen->join && gen->prefetch(Ap) == SDPSR_OK;
        st = syev_device(c, n, Q, ld, w, one_readback ? nullptr : info.vals.data(), nullptr, one_readback);
    }
    dbg_mark(c, "eigen_decomposition: syev returned");
    tm.end();
    if (st) {
        if (prefetched) gen->join();  // never leave side-stream work behind
        return st;
    }
    int neig = 0;
    int32_t* dspace = (int32_t*)ctx_buf(c, "bd_space", (size_t)n * 4 + 64);
    if (!dspace) return SDPSR_OUT_OF_MEMORY;
    unsigned long long* dnorms = nullptr;
    std::vector<double> norms;
    bool have_norms = false;
    if (one_readback) {
        // Step 3 enqueued behind the eigensolver: second generic element, clustering + Q'AQ + block norms
        tm.begin(SDPSR_T_ISO);
        const size_t o_space = 64, o_vals = o_space + (((size_t)n * 4 + 63) / 64) * 64, o_norms = o_vals + (size_t)n * 8;
        const size_t pack_bytes = small_cluster_pack_bytes(n);
        char* dpack = (char*)ctx_buf(c, "bd_pack", pack_bytes);
        int* dinfo = (int*)ctx_buf(c, "eig_info", 64);
        char* hp = (char*)ctx_pinned(c, pack_bytes);
        if (!dpack || !dinfo || !hp) return SDPSR_OUT_OF_MEMORY;
        dspace = (int32_t*)(dpack + o_space);  // stay valid for the launches of a retry
        dnorms = (unsigned long long*)(dpack + o_norms);
        st = prefetched ? gen->join() : make_element(c, gen, n, ld, L, Ap);
        if (st) return st;
        info.t_valid = true;
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
    } else {
        tm.collect();
        // EigenDecomposition ctor (:19-40): new eigenspace where |dv| > atol
        info.ptrs.assign(1, 0);
        for (int64_t i = 0; i < n; ++i) {
            if (i == n - 1) {
                info.ptrs.push_back((int)n);
                break;
            }
            if (!(std::fabs(info.vals[i + 1] - info.vals[i]) <= atol)) info.ptrs.push_back((int)i + 1);
        }
        neig = (int)info.ptrs.size() - 1;
        std::vector<int32_t> space_of(n);
        for (int b2 = 0; b2 < neig; ++b2)
            for (int i = info.ptrs[b2]; i < info.ptrs[b2 + 1]; ++i) space_of[i] = b2;
        // Step 3: second generic element, Q'AQ, block norms (:259-262, :201-205)
        tm.begin(SDPSR_T_ISO);
        dnorms = (unsigned long long*)ctx_buf(c, "bd_norms", (size_t)neig * neig * 8);
        if (!dnorms) return SDPSR_OUT_OF_MEMORY;
        st = h2d_sync(c, dspace, space_of.data(), n * 4);
        if (st) return st;
        HIP_TRY(c, hipMemsetAsync(dnorms, 0, (size_t)neig * neig * 8, s));
        st = prefetched ? gen->join() : make_element(c, gen, n, ld, L, Ap);
        if (st) return st;
        info.t_valid = true;
        if (n <= 64) {  // small (compressed) problems: one workgroup does Q'AQ and the block maxima (T = A Q goes to Tp)
            launch_small_qtaq_block_norms(s, n, ld, Ap, Q, dspace, neig, dnorms, nullptr, Tp);
        } else {
            launch_gemm_tn_f64(s, ld, ld, ld, Ap, ld, Q, ld, Tp, ld, 1, 0, 0, 0);   // T = A Q (A symmetric)
            launch_gemm_tn_f64(s, ld, ld, ld, Q, ld, Tp, ld, Ap, ld, 1, 0, 0, 0);   // M = Q' T  (into Ap)
            launch_block_norms(s, n, ld, Ap, dspace, neig, dnorms);
        }
        tm.end();
    }
    auto dimof = [&](int b) { return info.ptrs[b + 1] - info.ptrs[b]; };
    // The coupling of an isomorphic pair of eigenspaces under ONE generic element is the maximum over
    // an m_i x m_j block of random numbers -- a single one when the eigenspaces are 1-dimensional
    // (always so in compressed problems, often in QAP- and theta'-type partitions) -- and falls below
    // the Otsu threshold in ~0.1-0.5 % of the draws (measured round 2: 6 DimensionMismatch in 1000
    // compressed reductions of ER(7) (x) K_72, 4 in 2000 dense ones at N = 456, against 0 in 1000 for
    // the reference-literal oracle).  When the caller knows dim(P) (blockDiagonalize does) and the
    // classes found do not add up to it -- the check the reference makes right afterwards,
    // src/diagonalize.jl:1-11 -- or are inconsistent, the coupling matrix is raised by another
    // independent generic element (block_norms accumulates maxima: a coupling can only grow) and
    // the classes are formed again, up to twice.  The common case pays nothing;
    // SDPSR_FLAG_SINGLE_COUPLING_ELEMENT keeps the reference's single element (:259-262).
    // many eigenspaces: the coupling matrix stays on the device (isomorphism_classes_device)
    const bool classes_on_device = !have_norms && neig >= 256 && !(c->opts.flags & SDPSR_FLAG_COUPLING_ON_HOST);
    for (int extra = 0;; ++extra) {
        if (classes_on_device) {
            std::vector<int32_t> dims(neig);
            for (int i = 0; i < neig; ++i) dims[i] = dimof(i);
            // (a raised matrix of a later pass is symmetric already: maxima of symmetric blocks were added to both halves)
            st = isomorphism_classes_device(c, dnorms, neig, dims, atol, info.kpart);
            tm.collect();
            dbg_mark(c, "eigen_decomposition: Otsu + union-find done (coupling matrix on the device)");
        } else {
        if (!(have_norms && extra == 0)) {
            norms.resize((size_t)neig * neig);
            st = d2h_sync(c, norms.data(), dnorms, (size_t)neig * neig * 8);
            if (st) return st;
            tm.collect();
        }
        // blocks between eigenspaces of different dimension count as zero (:185-186); the kernel
        // computes the (bi, bj) max with bi = row space, symmetrise like end_norm[i,j] = end_norm[j,i]
        for (int i = 0; i < neig; ++i)
            for (int j = i; j < neig; ++j) {
                double v = (dimof(i) != dimof(j)) ? 0.0 : norms[(size_t)i * neig + j];  // block rows Ei, cols Ej
                norms[(size_t)i * neig + j] = norms[(size_t)j * neig + i] = v;
            }
        dbg_mark(c, "eigen_decomposition: block norms on the host");
        st = isomorphism_classes(c, norms, neig, atol, info.kpart);
        dbg_mark(c, "eigen_decomposition: Otsu + union-find done");
        }
        if (expect_dim < 0 || extra >= 2 || (c->opts.flags & SDPSR_FLAG_SINGLE_COUPLING_ELEMENT)) return st;
        if (st != SDPSR_OK && st != SDPSR_NUMERICAL_INCONSISTENCY) return st;
        if (st == SDPSR_OK) {
            std::vector<int> cnt(neig, 0);
            for (int i = 0; i < neig; ++i) ++cnt[info.kpart[i]];
            int64_t fd = 0;
            for (int i = 0; i < neig; ++i) fd += (int64_t)cnt[i] * (cnt[i] + 1) / 2;
            if (fd == expect_dim) {
                c->err.clear();
                return st;
            }
        }
        info.t_valid = false;  // the classes now rest on several coupling elements
        int e2 = make_element(c, gen, n, ld, L, Ap);
        if (e2) return e2;
        launch_gemm_tn_f64(s, ld, ld, ld, Ap, ld, Q, ld, Tp, ld, 1, 0, 0, 0);
        launch_gemm_tn_f64(s, ld, ld, ld, Q, ld, Tp, ld, Ap, ld, 1, 0, 0, 0);
        launch_block_norms(s, n, ld, Ap, dspace, neig, dnorms);
    }
}



// status used internally when a driver of diagonalize hands over to the dense one

int driver_fallback(sdpsr_ctx* c, const std::string& why) {
    c->err = "driver fell back to the dense eigensolver: " + why;
    if (dbg_on()) fprintf(stderr, "[sdpsr] %s\n", c->err.c_str());
    return DRIVER_FALLBACK;
}



// diagonalize(Float64, P) with the dense eigensolver (src/diagonalize.jl:25-40): on success the
// device buffer "bd_qhat" holds Q_hat (n x S1 column-major, classes side by side).
int dense_diagonalize(sdpsr_ctx* c, int64_t n, const uint32_t* L, const ElemGen* gen, double atol, EigInfo& info,
                      std::vector<int32_t>& sizes, int64_t& S1, int64_t& S, PhaseTimer& tm, int64_t expect_dim) {
    hipStream_t s = c->stream;
    int st = eigen_decomposition_device(c, n, L, atol, info, tm, gen, expect_dim);
    if (st) return st;

    // irreducible_decomposition (src/eigen_decomposition.jl:295-348)
    tm.begin(SDPSR_T_IRRED);
    const int64_t ld = round_up(n, 128);
    const int neig = (int)info.ptrs.size() - 1;
    std::vector<int> roots;  // unique(Kpartition) in first-occurrence order (:303)
    std::vector<std::vector<int>> members;
    class_structure(info.kpart, roots, members);
    sizes.assign(roots.size(), 0);
    S1 = 0;
    S = 0;
    for (size_t p = 0; p < roots.size(); ++p) {
        sizes[p] = (int32_t)members[p].size();
        S1 += sizes[p];
        S += (int64_t)sizes[p] * sizes[p];
    }
    double* Q = (double*)ctx_buf(c, "bd_q", (size_t)ld * ld * 8);
    double* Qhat = (double*)ctx_buf(c, "bd_qhat", (size_t)n * S1 * 8);
    if (!Q || !Qhat) return SDPSR_OUT_OF_MEMORY;
    // first eigenvector of every eigenspace that sits in a merged class -> F; B = A3 * F
    std::vector<int> fcol(neig, -1);
    int nf = 0;
    for (size_t p = 0; p < roots.size(); ++p)
        if (members[p].size() > 1)
            for (int j : members[p]) fcol[j] = nf++;
    double* Bf = nullptr;
    if (nf > 0) {
        const int64_t nfp = round_up(nf, 128);
        double* A3 = (double*)ctx_buf(c, "bd_a", (size_t)ld * ld * 8);
        double* F = (double*)ctx_buf(c, "bd_f", (size_t)ld * nfp * 8);
        Bf = (double*)ctx_buf(c, "bd_bf", (size_t)ld * nfp * 8);
        if (!A3 || !F || !Bf) return SDPSR_OUT_OF_MEMORY;
        const bool fresh = (c->opts.flags & SDPSR_FLAG_FRESH_IRREDUCIBLE_ELEMENT) != 0;
        double* Tq = (double*)ctx_buf(c, "bd_t", (size_t)ld * ld * 8);
        if (info.t_valid && Tq && !fresh) {
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
        } else {
        st = make_element(c, gen, n, ld, L, A3);  // generic element #3 (:306)
        if (st) return st;
        HIP_TRY(c, hipMemsetAsync(F, 0, (size_t)ld * nfp * 8, s));
        for (int j = 0; j < neig; ++j)
            if (fcol[j] >= 0)
                HIP_TRY(c, hipMemcpyAsync(F + (size_t)fcol[j] * ld, Q + (size_t)info.ptrs[j] * ld, n * 8,
                                          hipMemcpyDeviceToDevice, s));
        launch_gemm_tn_f64(s, ld, nfp, ld, A3, ld, F, ld, Bf, ld, 1, 0, 0, 0);  // B = A3' F = A3 F
        }
    }
    int64_t col = 0;
    std::vector<int32_t> cp_src, cp_dst;  // first members, copied in one launch after the loop
    std::vector<int32_t> pairs;           // the other members: one workgroup each, one launch
    int64_t max_m2 = 0;
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
    if (!pairs.empty()) {
        int32_t* d_pairs = (int32_t*)ctx_buf(c, "bd_pairs", pairs.size() * 4);
        if (!d_pairs) return SDPSR_OUT_OF_MEMORY;
        st = h2d_sync(c, d_pairs, pairs.data(), pairs.size() * 4);
        if (st) return st;
        if ((size_t)(max_m2 + 2) * 8 <= 60 * 1024) {
            launch_irreducible_pairs(s, n, ld, Q, Bf, (int)(pairs.size() / 7), (int)max_m2, d_pairs, Qhat);
        } else {
            // eigenspaces too large for the LDS of the pair kernel: four small launches per pair
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
        }
    }
    launch_copy_cols(s, n, (int64_t)cp_src.size(), cp_src.data(), cp_dst.data(), Q, ld, Qhat, n);
    launch_clamptol(s, n * S1, Qhat, atol);  // src/diagonalize.jl:39
    tm.end();
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}



// C = A' B for skinny outputs: the 128 x 128 output tiling alone would occupy a handful of
// CUs, so K is split over the batch dimension of the same MFMA kernel and the partial tiles are
// summed in fixed order.  Requires ldc == m (dense C) -- true for every caller.  `partials` names the ctx buffer of
// the partial tiles: a caller whose products run on the side stream beside the main stream's passes its own.
int gemm_tn_splitk(sdpsr_ctx* c, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B,
                   int64_t ldb, double* C, int64_t ldc, const char* partials) {
    const int64_t tiles = (m / 128) * (n / 128);
    // K is split over Z workgroups per output tile: the largest divisor of the K-tile count that keeps
    // >= 128 of K per workgroup and the launch within ~one workgroup per CU (any divisor, not only
    // powers of two: ld = 4224 = 33 * 128 at N = 4104 has 264 = 8 * 33 K-tiles)
    int Z = 1;
    {
        const int64_t kt = k / 16;
        for (int64_t z = 1; z <= kt && tiles * z <= 256; ++z)
            if (kt % z == 0 && k / z >= 128) Z = (int)z;
    }
    if (Z == 1 || ldc != m) {
        launch_gemm_tn_f64(c->stream, m, n, k, A, lda, B, ldb, C, ldc, 1, 0, 0, 0);
        return SDPSR_OK;
    }
    double* P = (double*)ctx_buf(c, partials, (size_t)Z * m * n * 8);
    if (!P) return SDPSR_OUT_OF_MEMORY;
    const int64_t kz = k / Z;
    launch_gemm_tn_f64(c->stream, m, n, kz, A, lda, B, ldb, P, m, Z, kz, kz, m * n);
    launch_splitk_reduce(c->stream, m * n, Z, m * n, P, C);
    return SDPSR_OK;
}

// C = A' B of the exact shape ma x nb (A: k x ma, B: k x nb) into the mp x np padded result (zero
// outside ma x nb): the skinny Gram kernel when both operands fit its LDS stage, the padded split-K
// MFMA product otherwise.
int gram_tn(sdpsr_ctx* c, int64_t ma, int64_t nb, int64_t k, const double* A, int64_t lda, const double* B, int64_t ldb,
            double* C, int64_t mp, int64_t np, double* host_C, bool* host_filled) {
    if (host_filled) *host_filled = false;
    const int64_t pa = (ma + 15) / 16 * 16 + 1, pb = (nb + 15) / 16 * 16 + 1;
    if (ma >= 1 && nb >= 1 && ma <= 128 && nb <= 128 && 32 * (pa + pb) * 8 <= 64 * 1024) {
        double* P = (double*)ctx_buf(c, "gram_partials", gram_small_partial_doubles(k, (int)ma, (int)nb) * 8);
        if (!P) return SDPSR_OUT_OF_MEMORY;
        launch_gram_small(c->stream, k, (int)ma, (int)nb, A, lda, B, ldb, P, C, mp, (int)mp, (int)np, host_C);
        if (host_filled) *host_filled = host_C != nullptr;
        return SDPSR_OK;
    }
    return gemm_tn_splitk(c, mp, np, k, A, lda, B, ldb, C, mp);
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
    c->bd_sym_epoch = 0;  // the verdict cached by sdpsr_block_diagonalize belongs to the labels it copied, not to these
    c->bd_sym_labels = nullptr;
    c->bd_trusted_symmetric = nullptr;
    c->bd_labels_ext = nullptr;
    const uint32_t* L = labels_in_dev(c, "bd_labels", P, (size_t)n * n, mem, &st);
    if (st) return st;
    c->bd_valid = false;
    EigInfo info;
    PhaseTimer tm(c, false);
    st = eigen_decomposition_device(c, n, L, atol, info, tm);
    if (st) return st;
    if (neig) *neig = (int32_t)info.ptrs.size() - 1;
    if (nclasses) {
        std::vector<int> roots(info.kpart);
        std::sort(roots.begin(), roots.end());
        *nclasses = (int32_t)(std::unique(roots.begin(), roots.end()) - roots.begin());
    }
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
    c->bd_sym_epoch = 0;  // the verdict cached by sdpsr_block_diagonalize belongs to the labels it copied, not to these
    c->bd_sym_labels = nullptr;
    c->bd_trusted_symmetric = nullptr;
    c->bd_labels_ext = nullptr;
    const uint32_t* L = labels_in_dev(c, "bd_labels", P, (size_t)n * n, mem, &st);
    if (st) return st;
    c->bd_valid = false;
    std::vector<int32_t> h_st(count, 0), h_ne(count, 0), h_nc(count, 0);
    if (n <= 64) {
        // one workgroup per run, matrices in LDS (kernels_batched.hip)
        hipStream_t s = c->stream;
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
        if (hp[0])
            return ctx_fail(c, SDPSR_INVALID_DECOMPOSITION_FIELD,
                            "partition is not symmetric: decomposition over Float64 requested but the generic element has a complex spectrum");
        memcpy(h_st.data(), hp + 16, (size_t)count * 4);
        memcpy(h_ne.data(), hp + 16 + count, (size_t)count * 4);
        memcpy(h_nc.data(), hp + 16 + 2 * count, (size_t)count * 4);
    } else {
        // larger orders: the runs go through the single-problem path one after the other
        if (values) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "explicit class values are supported for n <= 64 only");
        for (int64_t r = 0; r < count; ++r) {
            EigInfo info;
            PhaseTimer tm(c, false);
            const int e = eigen_decomposition_device(c, n, L, atol, info, tm);
            if (e != SDPSR_OK && e != SDPSR_NUMERICAL_INCONSISTENCY && e != SDPSR_SOLVER_ERROR) return e;
            h_st[r] = e;
            if (e == SDPSR_OK) {
                h_ne[r] = (int32_t)info.ptrs.size() - 1;
                std::vector<int> roots(info.kpart);
                std::sort(roots.begin(), roots.end());
                h_nc[r] = (int32_t)(std::unique(roots.begin(), roots.end()) - roots.begin());
            }
        }
    }
    if (status) memcpy(status, h_st.data(), (size_t)count * 4);
    if (neig) memcpy(neig, h_ne.data(), (size_t)count * 4);
    if (nclasses) memcpy(nclasses, h_nc.data(), (size_t)count * 4);
    for (int64_t r = 0; r < count; ++r)
        if (h_st[r] != SDPSR_OK) {
            const char* what = h_st[r] == SDPSR_NUMERICAL_INCONSISTENCY
                                   ? "eigen_decomposition: the K-partition seems inconsistent with eigenspaces. Decrease atol, or simply try again."
                                   : "eigensolver did not converge";
            return ctx_fail(c, h_st[r], "run " + std::to_string(r) + ": " + what);
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
    if (!Ap) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemsetAsync(Ap, 0, (size_t)ld * ld * 8, c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(Ap, ld * 8, dA, n * 8, n * 8, n, hipMemcpyDeviceToDevice, c->stream));
    st = syev_device(c, n, Ap, ld, dW);
    if (st) return st;
    HIP_TRY(c, hipMemcpy2DAsync(dV, n * 8, Ap, ld * 8, n * 8, n, hipMemcpyDeviceToDevice, c->stream));
    st = out_finish(c, vectors, dV, (size_t)n * n, mem);
    if (st) return st;
    return out_finish(c, values, dW, (size_t)n, mem);
}

}  // extern "C"
