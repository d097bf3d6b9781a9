// The host arithmetic between the eigensolver and the block images, once: eigenspace boundaries, the coupling matrix's dimension
// rule, the Otsu threshold, the union-find with its consistency verdict, the class structure and the column layouts derived
// from the block sizes (src/eigen_decomposition.jl:19-40,83-139,163-217,301-303).  Plain C++17, no HIP, no ctx, tested alone
// (tests/test_iso_classes_cpu.py).  Used by eigdec.cpp, small_eigen_host.cpp, blockdiag.cpp and complex.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

namespace sdpsr {

void host_count_edges17(const double* x, size_t n, const double* ed, int64_t* hist);  // host_syev.cpp

// EigenDecomposition ctor (:19-40): 0-based boundaries of the eigenspaces of ascending values, a new one where |dv| > atol
inline std::vector<int> eigenspace_ptrs(const double* vals, int64_t n, double atol) {
    std::vector<int> ptrs(1, 0);
    for (int64_t i = 0; i + 1 < n; ++i)
        if (!(std::fabs(vals[i + 1] - vals[i]) <= atol)) ptrs.push_back((int)i + 1);
    ptrs.push_back((int)n);
    return ptrs;
}
// the eigenspace of every eigenvector
inline std::vector<int32_t> space_of_ptrs(const std::vector<int>& ptrs) {
    std::vector<int32_t> space_of(ptrs.back());
    for (int b = 0; b + 1 < (int)ptrs.size(); ++b)
        for (int i = ptrs[b]; i < ptrs[b + 1]; ++i) space_of[i] = b;
    return space_of;
}

// blocks between eigenspaces of different dimension count as zero (:185-186); the upper triangle decides, like
// end_norm[i,j] = end_norm[j,i].  sym may be norms itself.
inline void symmetrize_coupling(const std::vector<int>& ptrs, const double* norms, double* sym) {
    const int neig = (int)ptrs.size() - 1;
    for (int i = 0; i < neig; ++i)
        for (int j = i; j < neig; ++j) {
            const bool same_dim = ptrs[i + 1] - ptrs[i] == ptrs[j + 1] - ptrs[j];
            const double v = same_dim ? norms[(size_t)i * neig + j] : 0.0;  // block rows Ei, cols Ej
            sym[(size_t)i * neig + j] = sym[(size_t)j * neig + i] = v;
        }
}

// otsu_threshold + log_histogram, src/eigen_decomposition.jl:83-139, in steps so that the values may stay on the device:
// extrema -> edges, counts per number of edges below a value -> counts per bin -> the chosen bin -> threshold
constexpr int OTSU_NB = 16;  // max(ceil(-log10(eps(Float64))), 4)
inline void otsu_edges(double mn, double mx, double atol, double (&edges)[OTSU_NB + 1]) {
    if (mn < atol) mn = atol;
    const double l0 = std::log(mn), l1 = std::log(mx);
    for (int i = 0; i <= OTSU_NB; ++i) {
        // Julia range(a, b, length=n): a + i*(b-a)/(n-1), endpoints exact
        double t = (i == OTSU_NB) ? l1 : l0 + (l1 - l0) * (double)i / (double)OTSU_NB;
        edges[i] = std::exp(t);
    }
}
// cnt[c], c = 0..17: number of values with exactly c edges <= them (a NaN: 17) -> the histogram's counts per bin
inline void otsu_bins(const int64_t (&cnt)[OTSU_NB + 2], double (&counts)[OTSU_NB]) {
    const int nb = OTSU_NB;
    // something(findfirst(b -> b > x, edges), nb + 1) (1-based) = 1 + #{edges <= x} for ascending edges;
    // f = min(c + 1, nb + 1): no edge above x (c = 17: x >= the last edge, or a NaN) is the default nb + 1
    int64_t hist[nb + 2] = {};
    for (int cidx = 0; cidx <= 17; ++cidx) hist[cidx + 1 < nb + 1 ? cidx + 1 : nb + 1] += cnt[cidx];
    for (int i = 0; i < nb; ++i) counts[i] = 0.0;
    for (int f = 1; f <= nb + 1; ++f) {
        const int bin = std::min(std::max(f - 1, 1), nb);
        counts[bin - 1] += (double)hist[f];
    }
}
// the bin whose upper edge is the threshold (0-based): argmax of the between-class variance (:112-139)
inline int otsu_best_bin(const double (&edges)[OTSU_NB + 1], const double (&counts)[OTSU_NB]) {
    const int nb = OTSU_NB;
    double total = 0;
    for (double v : counts) total += v;
    double w[nb], mu[nb];
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
    return best;
}
inline double otsu_pick(const double (&edges)[OTSU_NB + 1], const int64_t (&cnt)[OTSU_NB + 2]) {
    double counts[OTSU_NB];
    otsu_bins(cnt, counts);
    return edges[otsu_best_bin(edges, counts) + 1];
}
// min and max of |x| (min = INFINITY, max = 0 for no values)
inline void abs_extrema(const double* xp, size_t nx, double& mn, double& mx) {
    mn = INFINITY, mx = 0;
    // eight independent running minima / maxima (one chain is bound by the latency of min / max: 2 x 4 clocks per value)
    double mns[8], mxs[8];
    for (int q = 0; q < 8; ++q) mns[q] = INFINITY, mxs[q] = 0;
    const size_t n8 = nx & ~size_t(7);
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
inline double otsu_threshold(const std::vector<double>& X, double atol) {
    double mn, mx;
    abs_extrema(X.data(), X.size(), mn, mx);
    double edges[OTSU_NB + 1];
    otsu_edges(mn, mx, atol, edges);
    // counted without branches (the loop vectorises; neig^2 values go through it)
    int64_t cnt[OTSU_NB + 2];
    host_count_edges17(X.data(), X.size(), edges, cnt);  // cnt[c]: c edges <= x
    return otsu_pick(edges, cnt);
}

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
// the two feeds of the union-find, both in the reference's order (i, then j > i; :208-217): a threshold over a symmetric
// neig x neig matrix, or one bit per pair in rows of W 64-bit words (a pair whose ends already share a root is a no-op)
inline void unite_coupled(DisjointSets& K, const std::vector<double>& norms, int neig, double thr) {
    for (int i = 0; i < neig; ++i)
        for (int j = i + 1; j < neig; ++j)
            if (norms[(size_t)i * neig + j] >= thr) K.unite(i, j);
}
inline void unite_pair_bits(DisjointSets& K, const unsigned long long* bits, int neig, int W) {
    for (int i = 0; i < neig; ++i) {
        const unsigned long long* row = bits + (size_t)i * W;
        for (int w = i / 64; w < W; ++w) {
            unsigned long long m = row[w];
            while (m) {
                const int j = 64 * w + __builtin_ctzll(m);
                m &= m - 1;
                K.unite(i, j);
            }
        }
    }
}
// kpart = the root of every eigenspace; the verdict is __isconsistent (:163-167): every root is the first member of its class
inline bool kpartition(DisjointSets& K, std::vector<int>& kpart) {
    const int neig = (int)K.parent.size();
    kpart.resize(neig);
    for (int i = 0; i < neig; ++i) kpart[i] = K.find(i);
    std::vector<int> first(neig, -1);
    for (int i = 0; i < neig; ++i)
        if (first[kpart[i]] < 0) first[kpart[i]] = i;
    for (int i = 0; i < neig; ++i)
        if (first[kpart[i]] != kpart[i]) return false;
    return true;
}
constexpr const char* KPARTITION_INCONSISTENT =
    "eigen_decomposition: the K-partition seems inconsistent with eigenspaces. Decrease atol, or simply try again.";

// dim of the algebra the classes stand for: sum over the classes of cnt (cnt + 1) / 2 (check_block_sizes, src/diagonalize.jl:1-11)
inline int64_t classes_dim(const std::vector<int>& kpart) {
    std::vector<int> cnt(kpart.size(), 0);
    for (int r : kpart) ++cnt[r];
    int64_t fd = 0;
    for (int k : cnt) fd += (int64_t)k * (k + 1) / 2;
    return fd;
}
// no further coupling element is drawn: two extra ones were, or the caller does not know dim(P) (expect_dim < 0), or it keeps
// the reference's single element, or the (consistent) classes add up to dim(P)
inline bool coupling_settled(int extra, int64_t expect_dim, bool single_element, bool consistent, const std::vector<int>& kpart) {
    return extra >= 2 || expect_dim < 0 || single_element || (consistent && classes_dim(kpart) == expect_dim);
}
inline int count_classes(const std::vector<int>& kpart) {
    std::vector<int> roots(kpart);
    std::sort(roots.begin(), roots.end());
    return (int)(std::unique(roots.begin(), roots.end()) - roots.begin());
}

// roots (first-occurrence order, src/eigen_decomposition.jl:303) and members of every class
inline void class_structure(const std::vector<int>& kpart, std::vector<int>& roots, std::vector<std::vector<int>>& members) {
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
// one block per class, its size the number of members: S1 = sum s_k (columns of Q_hat), S = sum s_k^2 (entries of one image)
inline void block_sizes(const std::vector<std::vector<int>>& members, std::vector<int32_t>& sizes, int64_t& S1, int64_t& S) {
    sizes.assign(members.size(), 0);
    S1 = 0;
    S = 0;
    for (size_t p = 0; p < members.size(); ++p) {
        sizes[p] = (int32_t)members[p].size();
        S1 += sizes[p];
        S += (int64_t)sizes[p] * sizes[p];
    }
}

// blocks side by side: first column of Q_hat and size of every block (colsz = nb first columns, then nb sizes) and the
// offset of its s_k x s_k image
struct BlockLayout {
    int nb = 0, max_size = 0;
    std::vector<int32_t> colsz;
    std::vector<int64_t> off;
    const int32_t* col() const { return colsz.data(); }
    const int32_t* size() const { return colsz.data() + nb; }
};
inline BlockLayout block_layout(const std::vector<int32_t>& sizes) {
    BlockLayout lay;
    lay.nb = (int)sizes.size();
    lay.colsz.resize(2 * sizes.size());
    lay.off.resize(sizes.size());
    int64_t colbase = 0, off = 0;
    for (int k = 0; k < lay.nb; ++k) {
        lay.colsz[k] = (int32_t)colbase;
        lay.colsz[lay.nb + k] = sizes[k];
        lay.off[k] = off;
        colbase += sizes[k];
        off += (int64_t)sizes[k] * sizes[k];
        lay.max_size = std::max(lay.max_size, (int)sizes[k]);
    }
    return lay;
}
// the two columns of Q_hat every output multiplies, blocks side by side, column-major inside: S columns a, then S columns b
inline std::vector<int32_t> pair_descriptor(const std::vector<int32_t>& sizes, int64_t S) {
    std::vector<int32_t> desc(2 * (size_t)S);
    int64_t o = 0, colbase = 0;
    for (int32_t sz : sizes) {
        for (int b = 0; b < sz; ++b)
            for (int a = 0; a < sz; ++a) {
                desc[o] = (int32_t)(colbase + a);
                desc[S + o] = (int32_t)(colbase + b);
                ++o;
            }
        colbase += sz;
    }
    return desc;
}
// every class of class_ptr (size d + 2, class i = class_ptr[i] .. class_ptr[i + 1], i = 1 .. d) cut into chunks of at most
// `chunk` entries, each starting at the class's own first entry: chunk_ptr[i - 1] .. chunk_ptr[i] = the chunks of class i,
// chunk q = entries cb[q] .. ce[q].  A class's chunks depend on nothing but the class.
inline void cut_chunks(const std::vector<int64_t>& class_ptr, int64_t d, int64_t chunk, std::vector<int64_t>& chunk_ptr,
                       std::vector<int64_t>& cb, std::vector<int64_t>& ce) {
    chunk_ptr.assign(d + 1, 0);
    for (int64_t i = 1; i <= d; ++i) {
        chunk_ptr[i - 1] = (int64_t)cb.size();
        for (int64_t p = class_ptr[i]; p < class_ptr[i + 1]; p += chunk) {
            cb.push_back(p);
            ce.push_back(std::min(p + chunk, class_ptr[i + 1]));
        }
    }
    chunk_ptr[d] = (int64_t)cb.size();
}

}  // namespace sdpsr
