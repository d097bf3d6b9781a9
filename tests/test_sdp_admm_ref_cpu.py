"""The NumPy restatement of the first-order SDP solver (tests/sdp_admm_ref.py) held to the reference's pinned optima on
reduced SDPs built by the oracle (admissible_subspace -> block_diagonalize -> A PMat), and the new surface of the library.
No GPU.

Pins: test/lovasz.jl:16,32,48 and test/qap.jl:31 of the reference.  The theta' rows: 1e-6 relative at rho = 1, eps = 1e-9
within 20 000 iterations (measured: at most 5.1e-8, which is the pins' own 8-digit rounding).  esc16j: 5e-4 at rho = 10 after
exactly 20 000 iterations (measured 6.3e-5: the instance is degenerate and ADMM does not converge on it)."""
import ctypes as C
import pathlib

import numpy as np
import pytest

from blockop_ref import adjoint_ref, apply_ref, block_offsets, full_entries
from sdp_admm_ref import admm_ref, dense_B, psd_project_ref, reduced_sdp_ref, setup

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _solve(oracle, Cv, A, b, sense, labels=None, **kw):
    sizes, sp, newA, newB, newC = reduced_sdp_ref(oracle, Cv, A, b, labels=labels)
    full = full_entries(sp["classptr"], sp["blk"], sp["row"], sp["col"], sp["val"], sizes, upper=True)
    B = dense_B(full, block_offsets(sizes)[-1], newC.size)
    return admm_ref(B, sizes, newA, newB, newC, sense=sense, **kw), sizes, B, newA, newB


@pytest.mark.parametrize("name,pin", [("petersen", 4.0), ("er3", 5.0), ("er5", 10.066926), ("er7", 15.743402)])
def test_theta_prime_pins(oracle, problems, name, pin):
    adj = problems.petersen_adjacency() if name == "petersen" else problems.er_graph_adjacency(int(name[2:]))
    res, sizes, B, newA, newB = _solve(oracle, *problems.theta_prime_problem(adj), "max")
    rel = abs(res.objective - pin) / pin
    print(f"{name}: {res.objective:.10f} relative {rel:.2e} iterations {res.iters}")
    assert res.status == "converged" and res.iters <= 20000 and rel <= 1e-6
    assert np.abs(newA @ res.x - newB).max() <= 1e-9 and res.x.min() >= -1e-8
    assert min(np.linalg.eigvalsh(Z).min() for Z in _blocks(B @ res.x, sizes)) >= -1e-8


def test_esc16j_pin(oracle, problems, golden):
    fa, fb = problems.read_qapdata(ROOT / "tests" / "golden" / "esc16j.dat")
    res, sizes, _, _, _ = _solve(oracle, *problems.qap_problem(fa, fb), "min", labels=golden["esc16j_P"], rho=10.0)
    rel = abs(res.objective - 7.7942186) / 7.7942186
    print(f"esc16j: {res.objective:.8f} relative {rel:.2e} iterations {res.iters} {res.status}")
    assert sorted(sizes) == [1] * 10 + [7] * 5 and res.iters == 20000 and rel <= 5e-4


def _blocks(flat, sizes):
    off = block_offsets(sizes)
    return [flat[off[k]:off[k + 1]].reshape(s, s, order="F") for k, s in enumerate(sizes)]


def test_projection_reference():
    rng = np.random.default_rng(3)
    sizes = [1, 4, 2]
    blocks = [A + A.T for A in (rng.standard_normal((s, s)) for s in sizes)]
    flat = np.concatenate([b.ravel(order="F") for b in blocks])
    poisoned = np.concatenate([np.where(np.triu(np.ones_like(b), 1) > 0, np.nan, b).ravel(order="F") for b in blocks])
    P, lm = psd_project_ref(poisoned, sizes, return_lambda_min=True)  # only the lower triangles are read
    for Z, Pk, l in zip(blocks, _blocks(P, sizes), lm):
        w = np.linalg.eigvalsh(Z)
        assert np.array_equal(Pk, Pk.T) and abs(l - w[0]) <= 1e-14 * np.abs(Z).max()
        assert np.linalg.eigvalsh(Pk).min() >= -1e-14 * np.abs(Z).max()
        # the projection: Z - P is negative semidefinite and orthogonal to P
        assert np.linalg.eigvalsh(Z - Pk).max() <= 1e-14 * np.abs(Z).max() and abs(np.vdot(Z - Pk, Pk)) <= 1e-13 * np.abs(Z).max() ** 2
        assert abs(np.linalg.norm(Z - Pk) ** 2 - np.sum(np.minimum(w, 0) ** 2)) <= 1e-13 * np.abs(Z).max() ** 2


def test_affine_step_keeps_the_constraints_and_the_summation_order_does_not_matter():
    from blockop_ref import random_triplets
    sizes, d = [2, 3, 1], 7
    rng = np.random.default_rng(5)
    trip = random_triplets(sizes, d, 0.6, 6)
    full = full_entries(*trip, sizes)
    n = int(block_offsets(sizes)[-1])
    B = dense_B(full, n, d)
    A = rng.standard_normal((2, d))
    xs = rng.uniform(0.5, 1.5, d)
    b = A @ xs
    Kt, x0 = setup(B, A, b)
    assert np.abs(A @ Kt).max() <= 1e-13 and np.abs(A @ x0 - b).max() <= 1e-13 and np.abs(Kt - Kt.T).max() <= 1e-14
    c = rng.standard_normal(d)
    kw = dict(max_iters=60, check_every=60)
    r1 = admm_ref(B, sizes, A, b, c, **kw)
    r2 = admm_ref(B, sizes, A, b, c, apply=lambda x: apply_ref(x, full, n)[0], adjoint=lambda S: adjoint_ref(S, full, d)[0], **kw)
    assert r1.iters == r2.iters == 60 and np.abs(r1.x - r2.x).max() <= 1e-12 and np.abs(A @ r1.x - b).max() <= 1e-12
    r3 = admm_ref(B, sizes, np.zeros((0, d)), np.zeros(0), -np.abs(c) - 0.1, max_iters=3000)  # r = 0: the optimum is x = 0
    assert r3.status == "converged" and np.abs(r3.x).max() <= 1e-8


def test_new_surface_is_declared_exported_and_mirrored(pkg):
    header = (ROOT / "include" / "sdpsr.h").read_text()
    names = pkg._lib.declared_symbols()
    lib = C.CDLL(str(ROOT / "sdpsymmetryreduction.jl_amd" / "libsdpsr_hip.so"))  # (loading initialises no device)
    for name in ("sdpsr_psd_project", "sdpsr_sdp_solve"):
        assert name in names and hasattr(lib, name), name
    assert "sdpsr_sdp_opts" in header and "sdpsr_sdp_info" in header
    assert C.sizeof(pkg._lib.SdpOpts) == 56 and C.sizeof(pkg._lib.SdpInfo) == 64
    assert callable(pkg.psd_project) and callable(pkg.BlockOperator.solve) and callable(pkg.reduce_and_solve)
    assert lib.sdpsr_version() == 5
    julia = (ROOT / "sdpsymmetryreduction.jl_amd" / "julia" / "SDPSymmetryReductionHIP.jl").read_text()
    assert ":sdpsr_psd_project" in julia and ":sdpsr_sdp_solve" in julia
