"""sdpsr_compress_constraints without a GPU: the NumPy reference pinned on the esc16j fixture, and the host Jacobi
(csrc/host_gram_jacobi.cpp) compiled with g++ into stand-alone programs -- under AddressSanitizer + UBSan at -O1 and at the
Makefile's -O3 -- run as programs on record files (nothing is loaded into Python).  The two device steps of the iteration
(Gram matrix, row rotation) are played by NumPy (compress_ref.pass_scheme), so the whole scheme runs here."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import compress_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpsymmetryreduction.jl_amd", "csrc")

# record in:  int32 m, int32 max_sweeps, double tau, double floor2, G (m x m doubles)
# record out: doubles: rotations, sweeps, largest rotated |g_pq| / sqrt(g_pp g_qq), J (m x m, column-major, NaN before the call),
#             G afterwards (m x m)
SRC = r'''
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
namespace sdpsr {
int64_t host_gram_jacobi(int m, double* G, double* J, double tau, double floor2, int max_sweeps, int* sweeps_out, double* max_rel_out);
}
int main(int argc, char** argv) {
    FILE *in, *out;
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    int32_t h[2];
    while (fread(h, 1, sizeof h, in) == sizeof h) {
        double p[2];
        if (fread(p, 1, sizeof p, in) != sizeof p) return 3;
        const size_t mm = (size_t)h[0] * h[0];
        std::vector<double> G(mm), J(mm, std::numeric_limits<double>::quiet_NaN());
        if (mm && fread(G.data(), 8, mm, in) != mm) return 3;
        int sweeps = -1;
        double max_rel = -1.0;
        const int64_t rot = sdpsr::host_gram_jacobi(h[0], G.data(), J.data(), p[0], p[1], h[1], &sweeps, &max_rel);
        const double head[3] = {(double)rot, (double)sweeps, max_rel};
        fwrite(head, 8, 3, out);
        if (mm) fwrite(J.data(), 8, mm, out);
        if (mm) fwrite(G.data(), 8, mm, out);
    }
    return fclose(out) == 0 ? 0 : 5;
}
'''

BUILDS = {"asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "O3": ["-O3"]}
NAMES = ["graded_6x37", "graded_7x4097", "integer_9x5", "duplicates_6x70", "esc16j"]


@pytest.fixture(scope="module")
def cases(problems, golden):
    return R.inputs(problems, golden)


@pytest.fixture(scope="module")
def programs():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(SRC)
        for name, flags in BUILDS.items():
            subprocess.check_call(["g++", "-std=c++17", *flags, os.path.join(CSRC, "host_gram_jacobi.cpp"), os.path.join(d, "driver.cpp"),
                                   "-o", os.path.join(d, name)])

        def jacobi(build):
            def run(G, tau, floor2, max_sweeps):
                m = G.shape[0]
                fi, fo = os.path.join(d, build + ".in"), os.path.join(d, build + ".out")
                with open(fi, "wb") as f:
                    f.write(struct.pack("<2i2d", m, max_sweeps, tau, floor2) + np.ascontiguousarray(G).tobytes())
                subprocess.run([os.path.join(d, build), fi, fo], check=True)
                got = np.fromfile(fo, dtype=np.float64)
                assert got.size == 3 + 2 * m * m
                run.sweeps.append(int(got[1]))
                run.last_G = got[3 + m * m:].reshape(m, m)
                return int(got[0]), got[3:3 + m * m].reshape((m, m), order="F"), float(got[2])
            run.sweeps = []
            return run
        yield jacobi


def test_reference_helper_on_esc16j(cases):
    newA, b, _ = cases["esc16j"]
    M = R.stack(newA, b)
    assert M.shape == (33, 151)
    s, r, rows = R.reference(M)
    assert r == 9 and rows.shape == (9, 151) and np.linalg.matrix_rank(M) == 9
    assert R.rank_is_unambiguous(s)
    assert R.orth(rows) <= 151 * R.EPS and R.resid(M, rows) <= 151 * R.EPS
    assert R.sverr(np.concatenate([s, np.zeros(0)]), s, 33) == 0.0


def test_single_eigen_decomposition_of_the_gram_matrix_gets_the_rank_wrong(cases):
    """Why the routine exists: the eigenvalue shortcut on M M' loses every singular value below sqrt(eps) sigma_1 and
    counts noise instead (ranks 5, 6, 7, 4, 20 here for 4, 4, 5, 3, 9)."""
    wrong = 0
    for name in NAMES:
        newA, b, r = cases[name]
        M = R.stack(newA, b)
        w = np.linalg.eigvalsh(M @ M.T)[::-1]
        sv = np.sqrt(np.maximum(w, 0))
        wrong += int(np.count_nonzero(sv > min(M.shape) * R.EPS * sv[0]) != r)
    assert wrong >= 4


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", NAMES)
def test_pass_scheme_with_the_host_jacobi(cases, programs, build, name):
    """Reference rank, orth and resid within max(8 x LAPACK's own figure, ncols eps), sverr <= ncols eps, inside the pass
    limit; every sweep loop ended by itself (no sweep limit reached); J orthogonal; J G J' diagonal where rows took part."""
    newA, b, r_ref = cases[name]
    M = R.stack(newA, b)
    m, ncols = M.shape
    s, r, rows = R.reference(M)
    assert r == r_ref and R.rank_is_unambiguous(s)
    jac = programs(build)
    Rg, rg, sv, passes, converged = R.pass_scheme(M, jac)
    print(name, build, "passes", passes, "sweeps", jac.sweeps, "orth", R.orth(Rg), "resid", R.resid(M, Rg), "sverr", R.sverr(sv, s, m))
    assert converged and passes <= R.MAX_PASSES
    assert max(jac.sweeps) < R.MAX_SWEEPS
    assert rg == r
    bound = ncols * R.EPS
    assert R.orth(Rg) <= max(8 * R.orth(rows), bound)
    assert R.resid(M, Rg) <= max(8 * R.resid(M, rows), bound)
    assert R.sverr(sv, s, m) <= bound
    assert np.all(np.diff(sv) <= 0)
    assert np.all(Rg[np.arange(rg), np.abs(Rg).argmax(axis=1)] > 0)


@pytest.mark.parametrize("build", list(BUILDS))
def test_host_jacobi_alone(programs, build):
    """One call on a Gram matrix: J is orthogonal, J G J' is what the routine left in G, and its off-diagonal entries obey
    the relative rule; m = 0 and m = 1 make no rotation; rows under the floor are left alone."""
    rng = np.random.default_rng(2)
    W = rng.standard_normal((12, 40)) * 10.0 ** -np.arange(12)[:, None]
    G = W @ W.T
    jac = programs(build)
    rot, J, max_rel = jac(G, 4 * R.EPS, 0.0, 60)
    assert rot > 0 and jac.sweeps[-1] < 60 and 4 * R.EPS < max_rel <= 1.0
    assert np.abs(J @ J.T - np.eye(12)).max() <= 50 * R.EPS
    D = jac.last_G
    dd = np.sqrt(np.abs(np.diag(D)))
    off = np.abs(D - np.diag(np.diag(D))) / (dd[:, None] * dd[None, :])
    assert off.max() <= 4 * R.EPS
    assert np.abs(J @ G @ J.T - D).max() <= 100 * R.EPS * np.abs(G).max()
    for m in (0, 1):
        rot, J, max_rel = jac(np.ones((m, m)), R.EPS, 0.0, 60)
        assert rot == 0 and max_rel == 0.0 and np.array_equal(J, np.eye(m))
    # the floor: rows 2.. of this G are 1e-20 of the first and stay out, though fully coupled
    G = np.ones((4, 4)) * 1e-20
    G[0, 0], G[1, 1], G[0, 1], G[1, 0] = 1.0, 1.0, 0.5, 0.5
    rot, J, _ = jac(G, R.EPS, 1e-19, 60)
    assert rot >= 1 and np.array_equal(J[2:], np.eye(4)[2:]) and np.array_equal(J[:, 2:], np.eye(4)[:, 2:])
