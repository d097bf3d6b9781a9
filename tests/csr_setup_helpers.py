"""What the tests of the device setup stage share (tests/test_gpu_csr_setup.py, tests/test_gpu_primitives.py): the comparison of a device
setup (n, CL, X0L, U) with the NumPy setup of api.admissible_setup.  The bounds belong to this helper, not to its callers."""
import numpy as np


def _host_partition(v):
    """Canonical labels of equal values, first occurrence in column-major order, 0.0 -> 0 (src/partitions.jl:24-35)."""
    v = np.asarray(v).reshape(-1)
    _, first, inv = np.unique(v, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    nz = v[first] != 0
    order = np.argsort(first[nz], kind="stable")
    ids = np.flatnonzero(nz)[order]
    rank[:] = 0
    rank[ids] = np.arange(1, ids.size + 1)
    return rank[inv]


def _rounding_units(a, b):
    """max |a - b| in units of the rounding step 1e-7 2^e of the larger operand."""
    big = np.maximum(np.abs(a), np.abs(b))
    _, e = np.frexp(big)
    return float(np.max(np.abs(a - b) / np.ldexp(1.0000001e-7, e), initial=0.0))


def _within_one_rounding_unit(a, b):
    big = np.maximum(np.abs(a), np.abs(b))
    _, e = np.frexp(big)
    return np.all(np.abs(a - b) <= np.ldexp(1.0000001e-7, e))


def _compare_with_host_setup(pkg, Sd, Sh, seed=0):
    """Asserts; returns the figures it bounded, each as a fraction of its bound."""
    n, CLd, X0d, Ud = Sd
    _, CLh, X0h, Uh = Sh
    Ud = Ud.cpu().numpy() if hasattr(Ud, "cpu") else Ud
    CLd = CLd.cpu().numpy() if hasattr(CLd, "cpu") else CLd
    X0d = X0d.cpu().numpy() if hasattr(X0d, "cpu") else X0d
    assert Ud.shape[1] == Uh.shape[1]
    r = Ud.shape[1]
    seen = {"orthonormality": 0.0, "projector": 0.0}
    if r:
        orth = np.abs(Ud.T @ Ud - np.eye(r)).max()
        assert orth <= 1e-13
        seen["orthonormality"] = float(orth / 1e-13)
        rng = np.random.default_rng(seed)
        for _ in range(3):
            x = rng.standard_normal(n * n)
            pd, ph = Ud @ (Ud.T @ x), Uh @ (Uh.T @ x)
            assert np.linalg.norm(pd - ph) <= 1e-12 * np.linalg.norm(x)
            seen["projector"] = max(seen["projector"], float(np.linalg.norm(pd - ph) / (1e-12 * np.linalg.norm(x))))
    assert np.array_equal(_host_partition(CLd), _host_partition(CLh))
    assert np.array_equal(_host_partition(X0d), _host_partition(X0h))
    assert _within_one_rounding_unit(CLd, CLh) and _within_one_rounding_unit(X0d, X0h)
    seen["rounding_unit"] = max(_rounding_units(CLd, CLh), _rounding_units(X0d, X0h))
    return seen
