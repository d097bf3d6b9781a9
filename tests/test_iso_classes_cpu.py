"""The host arithmetic between the eigensolver and the block images (csrc/iso_classes.h) alone, against the CPU oracle: compiled
with g++ under AddressSanitizer + UBSan into a program of its own (with host_syev.cpp for the edge counts) and run as a program
(nothing is loaded into Python).  The program reads the cases from a file this test writes and prints its results."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import sdpsr_oracle as O  # noqa: E402

# the matrices and the restatement of the oracle's chain live with the references of the GPU test of the same steps
from dense_steps_ref import ATOL, _expected_classes, _matrix_cases, _oracle_chain  # noqa: E402

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include "iso_classes.h"
using namespace sdpsr;
template <class V> static void line(const char* tag, const V& v) {
    printf("%s", tag);
    for (auto x : v) printf(" %lld", (long long)x);
    printf("\n");
}
static void classes(DisjointSets& K, int64_t expect) {
    std::vector<int> kpart, roots;
    std::vector<std::vector<int>> members;
    printf("verdict %d\n", (int)kpartition(K, kpart));
    line("kpart", kpart);
    class_structure(kpart, roots, members);
    line("roots", roots);
    for (const auto& m : members) line("members", m);
    std::vector<int32_t> sizes;
    int64_t S1, S;
    block_sizes(members, sizes, S1, S);
    line("sizes", sizes);
    printf("sums %lld %lld %lld %d\n", (long long)S1, (long long)S, (long long)classes_dim(kpart), count_classes(kpart));
    printf("settled %d %d %d %d %d\n", (int)coupling_settled(0, expect, false, true, kpart), (int)coupling_settled(0, expect, false, false, kpart),
           (int)coupling_settled(2, expect, false, false, kpart), (int)coupling_settled(0, -1, false, false, kpart), (int)coupling_settled(0, expect, true, false, kpart));
    const BlockLayout lay = block_layout(sizes);
    line("colsz", lay.colsz);
    line("off", lay.off);
    printf("laymax %d %d\n", lay.nb, lay.max_size);
    line("desc", pair_descriptor(sizes, S));
}
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "r");
    if (argc < 2 || !f) return 2;
    char kind[16];
    while (fscanf(f, "%15s", kind) == 1) {
        int n;
        double atol;
        long long expect;
        if (fscanf(f, "%d %lf %lld", &n, &atol, &expect) != 3) return 3;
        printf("case %s %d\n", kind, n);
        if (kind[0] == 'v') {  // values: eigenspace boundaries
            std::vector<double> v(n);
            for (double& x : v) if (fscanf(f, "%la", &x) != 1) return 3;
            const std::vector<int> ptrs = eigenspace_ptrs(v.data(), n, atol);
            line("ptrs", ptrs);
            line("space", space_of_ptrs(ptrs));
        } else if (kind[0] == 'm') {  // eigenspace boundaries + raw coupling matrix: the whole chain
            std::vector<int> ptrs(n + 1);
            for (int& p : ptrs) if (fscanf(f, "%d", &p) != 1) return 3;
            std::vector<double> raw((size_t)n * n), sym((size_t)n * n);
            for (double& x : raw) if (fscanf(f, "%la", &x) != 1) return 3;
            symmetrize_coupling(ptrs, raw.data(), sym.data());
            printf("sym");
            for (double x : sym) printf(" %a", x);
            printf("\n");
            double mn, mx, edges[OTSU_NB + 1], counts[OTSU_NB];
            abs_extrema(sym.data(), sym.size(), mn, mx);
            otsu_edges(mn, mx, atol, edges);
            int64_t cnt[OTSU_NB + 2];
            host_count_edges17(sym.data(), sym.size(), edges, cnt);
            otsu_bins(cnt, counts);
            printf("counts");
            for (double x : counts) printf(" %lld", (long long)x);
            printf("\nbest %d\n", otsu_best_bin(edges, counts));
            const double thr = otsu_threshold(sym, atol);
            printf("thr %.17g %d\n", thr, (int)(thr == otsu_pick(edges, cnt)));
            DisjointSets K(n);
            unite_coupled(K, sym, n, thr);
            classes(K, expect);
        } else {  // bits: one bit per pair, rows of W words
            const int W = (n + 63) / 64;
            std::vector<unsigned long long> bits((size_t)n * W);
            for (auto& b : bits) if (fscanf(f, "%llx", &b) != 1) return 3;
            DisjointSets K(n);
            unite_pair_bits(K, bits.data(), n, W);
            classes(K, expect);
        }
    }
    return 0;
}
'''


def _parse(lines):
    cases, cur = [], None
    for ln in lines:
        tag, *rest = ln.split()
        if tag == "case":
            cur = {"name": rest[0], "members": []}
            cases.append(cur)
        elif tag == "members":
            cur["members"].append([int(x) for x in rest])
        elif tag == "sym":
            cur[tag] = [float.fromhex(x) for x in rest]
        elif tag == "thr":
            cur[tag] = (float(rest[0]), int(rest[1]))
        else:
            cur[tag] = [int(x) for x in rest]
    return cases


def _check_classes(got, K, expect, name):
    for key, want in _expected_classes(K, expect).items():
        assert got[key] == [int(x) for x in want] if key != "members" else got[key] == want, (name, key, got[key], want)


def test_iso_classes_match_the_oracle():
    """Exactly equal to the oracle: the eigenspace boundaries and the eigenspace of every eigenvector (eigenspace_ptrs; n = 1, a
    gap of exactly atol -- no boundary --, a NaN -- a boundary on both sides); the symmetrised matrix, the counts per bin
    (log_histogram), the chosen bin, kpart in the merge order of isomorphism_partition on IntDisjointSets, the verdict of
    __isconsistent (false for the chain, from the matrix and from the pair bits), roots, members, sizes, S1, S, classes_dim,
    the settle rule, the layout and the (a, b) descriptors.  The threshold to a relative 1e-12: the two sides differ only in how
    exp(linspace(log .)) is rounded, a few ulps of a logarithm of magnitude <= 40, hence <~ 1e-14 relative.  The exact
    comparisons are well defined because no value lies within a relative 1e-9 of an interior oracle edge (asserted; the first and
    the last edge put a value into the same bin from either side, and `equal` has exact edges)."""
    value_cases = [("v1", [0.25]), ("v2", [1.0, 1.0 + 3 * ATOL]), ("v17", list(np.repeat(np.arange(6.0), [1, 3, 2, 5, 4, 2]))),
                   ("vgap", [0.0, ATOL, 2 * ATOL, 1.0, 1.0 + ATOL / 2, float("nan"), 2.0]),
                   ("v300", list(np.sort(np.random.default_rng(2).integers(0, 40, size=300)).astype(float)))]
    matrix_cases = _matrix_cases()
    chain_bits = [1 << 3, 1 << 2, 1 << 3, 0, 0]  # the chain's pairs (0,3), (1,2), (2,3), row by row
    expects, oracle = {}, {}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "cases.txt"), "w") as f:
            for name, v in value_cases:
                f.write(f"v_{name} {len(v)} {ATOL!r} 0\n" + " ".join(float(x).hex() for x in v) + "\n")
            for name, dims, raw in matrix_cases:
                oracle[name] = _oracle_chain(dims, raw)
                K = oracle[name][5]
                expects[name] = sum(s * (s + 1) // 2 for s in np.bincount([K.find_root(i) for i in range(len(K))]))
                ptrs = np.concatenate([[0], np.cumsum(dims)])
                f.write(f"m_{name} {len(dims)} {ATOL!r} {expects[name]}\n" + " ".join(map(str, ptrs)) + "\n" +
                        " ".join(float(x).hex() for x in raw.ravel()) + "\n")
            f.write(f"b_chain 5 {ATOL!r} 10\n" + " ".join(f"{b:x}" for b in chain_bits) + "\n")
            big = [0] * (130 * 3)  # 130 eigenspaces, three words per row: pairs (0, 129), (64, 65), (1, 128) across the words
            for i, j in ((0, 129), (64, 65), (1, 128)):
                big[3 * i + j // 64] |= 1 << (j % 64)
            f.write(f"b_words 130 {ATOL!r} 0\n" + " ".join(f"{b:x}" for b in big) + "\n")
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                               os.path.join(CSRC, "host_syev.cpp"), os.path.join(d, "t.cpp"), "-o", os.path.join(d, "t")])
        out = subprocess.run([os.path.join(d, "t"), os.path.join(d, "cases.txt")], check=True, capture_output=True, text=True).stdout
    got = _parse(out.splitlines())
    assert [g["name"] for g in got] == ["v_" + c[0] for c in value_cases] + ["m_" + c[0] for c in matrix_cases] + ["b_chain", "b_words"]
    for (name, v), g in zip(value_cases, got):
        ptrs, _ = O.eigenspace_ptrs(v, ATOL)
        assert g["ptrs"] == ptrs, (name, g["ptrs"], ptrs)
        assert g["space"] == [b for b in range(len(ptrs) - 1) for _ in range(ptrs[b], ptrs[b + 1])], name
    assert got[3]["ptrs"] == [0, 3, 5, 6, 7]  # vgap: |dv| == atol merges, atol / 2 merges, a NaN separates on both sides
    verdicts = {}
    for (name, dims, raw), g in zip(matrix_cases, got[len(value_cases):]):
        sym, counts, edges, best, thr, K = oracle[name]
        if name not in ("one", "equal"):  # no value near an interior edge: the bins of both sides are the same sets
            rel = np.abs(sym[sym > 0][:, None] - edges[None, 1:-1]) / edges[None, 1:-1]
            assert rel.min() > 1e-9, (name, rel.min())
        assert g["sym"] == list(sym.ravel()), name
        assert g["counts"] == [int(x) for x in counts], (name, g["counts"], counts)
        assert g["best"] == [best], (name, g["best"], best)
        assert abs(g["thr"][0] - thr) <= 1e-12 * thr and g["thr"][1] == 1, (name, g["thr"], thr)
        _check_classes(g, K, expects[name], name)
        verdicts[name] = g["verdict"][0]
        print(f"{name}: neig={len(dims)} counts={g['counts']} best={best} thr={g['thr'][0]:.17g} oracle={thr:.17g} "
              f"classes={len(g['roots'])} verdict={g['verdict'][0]}")
    assert verdicts.pop("chain") == 0 and all(v == 1 for v in verdicts.values())
    assert got[len(value_cases) + 5]["counts"] == [0] * 15 + [25] and got[len(value_cases) + 5]["best"] == [0]  # equal: the first NaN
    mixed = got[len(value_cases) + 3]
    assert mixed["sym"].count(0.0) > 0 and len(mixed["roots"]) > 4  # the dimension rule zeroed entries and split the classes
    # the pair bits: the chain again (the same kpart as from the matrix, verdict false), and pairs beyond the first word
    K = O.IntDisjointSets(5)
    for i, j in ((0, 3), (1, 2), (2, 3)):
        K.union(i, j)
    _check_classes(got[-2], K, 10, "b_chain")
    assert got[-2]["verdict"] == [0] and got[-2]["kpart"] == [1, 1, 1, 1, 4]
    assert got[-2]["kpart"] == got[len(value_cases) + len(matrix_cases) - 1]["kpart"]
    K = O.IntDisjointSets(130)
    for i, j in ((0, 129), (1, 128), (64, 65)):  # row order
        K.union(i, j)
    _check_classes(got[-1], K, 0, "b_words")
    assert got[-1]["verdict"] == [1] and len(got[-1]["roots"]) == 127
