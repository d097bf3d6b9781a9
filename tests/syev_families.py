"""The symmetric test matrices of the small-eigensolver tests (test_host_syev_cpu.py, test_gpu_small_syev.py), seeded per
family and order, with LAPACK's eigenvalues as the reference."""
import functools

import numpy as np

C4 = np.array([[2, 1, 0, 1], [1, 2, 1, 0], [0, 1, 2, 1], [1, 0, 1, 2]], dtype=float)


def _sym(n, rng):
    G = rng.standard_normal((n, n))
    return (G + G.T) / 2


def _spectrum(vals):
    def make(n, rng):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (Q * np.resize(vals(rng), n)) @ Q.T
        return (A + A.T) / 2
    return make


def _graded(n, rng):
    s = 10.0 ** (-12.0 * np.arange(n) / n)
    return s[:, None] * _sym(n, rng) * s[None, :]


def _decoupled(n, rng):  # column n // 2 - 1 is zero below the diagonal: the tau = 0 branch of a tridiagonalisation
    B, n1 = np.zeros((n, n)), n // 2
    B[:n1, :n1], B[n1:, n1:] = _sym(n1, rng), _sym(n - n1, rng)
    return B


def _arrow(n, rng):
    A = np.diag(np.arange(1.0, n + 1))
    A[0, :] += 1.0
    A[:, 0] += 1.0
    return A


def _zero_one(n, rng):
    R = np.triu((rng.random((n, n)) < 0.5).astype(float))
    return R + np.triu(R, 1).T


FAMILIES = {
    "random symmetric": _sym,
    "two eigenvalues": _spectrum(lambda rng: np.array([1.0, -2.0])),
    "five eigenvalues": _spectrum(lambda rng: rng.standard_normal(5)),
    "identity": lambda n, rng: np.eye(n),
    "zero": lambda n, rng: np.zeros((n, n)),
    "descending diagonal": lambda n, rng: np.diag(np.arange(n, 0, -1.0)),
    "rank one, ones": lambda n, rng: np.ones((n, n)),
    "rank one, scaled": lambda n, rng: 0.3 * np.ones((n, n)),
    "rank one, outer": lambda n, rng: np.outer(np.arange(1.0, n + 1), np.arange(1.0, n + 1)),
    "kron, rank 3": lambda n, rng: np.kron(np.ones((n // 4, n // 4)), C4),  # 4 | n
    "kron, rank 4": lambda n, rng: np.kron(np.eye(4), np.ones((n // 4, n // 4))),  # 4 | n
    "wilkinson": lambda n, rng: np.diag(np.abs(np.arange(n) - n // 2).astype(float)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1),
    "graded": _graded,
    "decoupled blocks": _decoupled,
    "arrow": _arrow,
    "random 0/1": _zero_one,
    # both slow branches of the host solver's pythag and the IEEE branch of the device's jacobi_angle; squares stay finite
    "scale 1e145": lambda n, rng: _sym(n, rng) * 1e145,
    "scale 1e-145": lambda n, rng: _sym(n, rng) * 1e-145,
}
EXTREME = ("scale 1e145", "scale 1e-145")
LOW_RANK = ("rank one, ones", "rank one, scaled", "rank one, outer", "kron, rank 3", "kron, rank 4")


def names(n, extreme=True):
    return [f for f in FAMILIES if (n % 4 == 0 or not f.startswith("kron")) and (extreme or f not in EXTREME)]


def matrix(name, n):
    A = FAMILIES[name](n, np.random.default_rng([n, list(FAMILIES).index(name)]))
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """(A, numpy.linalg.eigvalsh(A), |A| = max |eigenvalue|, or 1 for the zero matrix): made once, read-only."""
    A = matrix(name, n)
    wl = np.linalg.eigvalsh(A)
    wl.setflags(write=False)
    return A, wl, float(np.abs(wl).max()) or 1.0
