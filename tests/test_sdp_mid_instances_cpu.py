"""The instances of tests/sdp_mid_instances.py (one PSD block of order 65 / 66) under the NumPy restatement alone: they
converge at the solver's default settings and their dual certificates close, so the device solver can be held to them
(tests/test_gpu_sdp_solve_mid.py).  And the ABI of the opt-in: sdpsr_set_psd_max_order / sdpsr_psd_max_order.

Recorded with the restatement at rho = 1, eps = 1e-9, check_every = 50: (a) s = 65 / 97 / 128 converge after 2500 / 3600 / 4800
iterations at -1.89800008 / -1.91305692 / -1.93010700, |objective - bound| <= 8.3e-10; (b) n = 66 after 5450 iterations at
8.286706770 under the bound 8.286706781."""
import ctypes as C

import numpy as np

from sdp_mid_instances import instance, restatement


def test_lmin_instance_converges_to_its_certificate():
    t, ref = instance("lmin65"), restatement("lmin65")
    bound = t.bound(ref.Y)
    F = t.F
    Zx = F[0] + sum(ref.x[i] * F[i] for i in range(2, t.d))
    lmin = float(np.linalg.eigvalsh(Zx)[0])
    print(f"(a) s = 65: {ref.status} after {ref.iters} iterations, objective {ref.objective:.10f}, bound {bound:.10f}, "
          f"gap {abs(ref.objective - bound):.2e}, lambda_min(F_0 + sum x_i F_i) {lmin:.10f}")
    assert t.B.shape == (65 * 65, 6) and np.array_equal(F[1], -np.eye(65)) and all(abs(np.trace(Fi)) <= 1e-13 for Fi in F[2:])
    assert ref.status == "converged"
    assert abs(ref.objective - bound) <= 1e-8
    assert abs(ref.x[0] - 1.0) <= 1e-9 and abs(ref.objective - lmin) <= 1e-8  # the objective is the eigenvalue it stands for
    Yh = -ref.Y.reshape(65, 65, order="F")
    assert np.linalg.eigvalsh(Yh)[0] >= -1e-12 * np.abs(Yh).max()  # the multiplier is a projection's complement: NSD


def test_lmin_triplets_are_the_dense_pencil():
    from blockop_ref import full_entries
    from sdp_admm_ref import dense_B
    for name in ("lmin65", "theta66"):
        t = instance(name)
        ptr, blk, row, col, val = t.trip
        assert np.all(row <= col) and ptr[-1] == val.size and ptr.size == t.d + 1
        assert np.array_equal(dense_B(full_entries(*t.trip, t.sizes), t.sizes[0] ** 2, t.d), t.B)
        if t.apply is not None:
            rng = np.random.default_rng(3)
            x, S = rng.standard_normal(t.d), rng.standard_normal(t.sizes[0] ** 2)
            assert np.array_equal(t.apply(x), t.B @ x) and np.array_equal(t.adjoint(S), t.B.T @ S)


def test_theta_instance_converges_under_its_bound():
    t, ref = instance("theta66"), restatement("theta66")
    bound = t.bound(ref.Y)
    print(f"(b) n = 66: {ref.status} after {ref.iters} iterations, objective {ref.objective:.9f}, bound {bound:.9f}, "
          f"gap {bound - ref.objective:.2e}")
    assert t.d == 1123 and t.sizes == [66]
    assert ref.status == "converged"
    assert abs(ref.objective - bound) <= 1e-6 * abs(ref.objective)  # (the solver's own criterion; recorded: 1.3e-9 relative)
    assert abs(ref.objective - 8.286706770) <= 1e-8
    assert ref.x.min() >= -1e-8 and abs(ref.x[:66].sum() - 1.0) <= 1e-9


def test_abi_of_the_opt_in(pkg):
    """Fails on a tree without the feature: the two entry points are declared, exported and bound; nothing else of the ABI moved."""
    L = pkg._lib
    lib = pkg.load_library()
    names = L.declared_symbols()
    for s in ("sdpsr_set_psd_max_order", "sdpsr_psd_max_order"):
        assert s in names and hasattr(lib, s), s
    assert C.sizeof(L.SdpOpts) == 56 and C.sizeof(L.SdpInfo) == 64
    assert lib.sdpsr_version() == 5
    assert lib.sdpsr_set_psd_max_order(None, 128) == 5 and lib.sdpsr_psd_max_order(None) == 5  # no ctx: SDPSR_BAD_ARGUMENT
