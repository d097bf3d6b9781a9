"""NumPy reference for sdpsr_compress_constraints (the row space of M = [A * PMat, b] and its rank,
docs/src/examples/ReduceAndSolveJuMP.jl:44-50 of the reference): LAPACK's SVD, Julia's dense ``rank`` default, the three figures
the tests compare on, the five test inputs, and the pass scheme of csrc/rowspace.cpp with its two device steps (Gram matrix,
row rotation) played by NumPy.  Comparisons are on invariants, never entry by entry: repeated singular values leave a
rotation free (esc16j has sigma = 16 four times)."""
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
EPS = float(np.finfo(np.float64).eps)
MAX_PASSES = 16   # csrc/rowspace.cpp: COMPRESS_MAX_PASSES
MAX_SWEEPS = 60   # ... COMPRESS_MAX_SWEEPS


def reference(M):
    """(s, rank, rows): LAPACK's singular values, the count of s > min(m, ncols) eps s[0], and the first `rank` right
    singular vectors as rows."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape[0] == 0 or M.shape[1] == 0:
        return np.zeros(0), 0, np.zeros((0, M.shape[1]))
    _, s, Vt = np.linalg.svd(M, full_matrices=False)
    r = int(np.count_nonzero(s > min(M.shape) * EPS * s[0])) if s[0] > 0 else 0
    return s, r, Vt[:r]


def orth(R):
    return float(np.abs(R @ R.T - np.eye(R.shape[0])).max()) if R.shape[0] else 0.0


def resid(M, R):
    s1 = np.linalg.norm(M, 2)
    return float(np.abs(M - (M @ R.T) @ R).max() / s1)


def sverr(sv, s, m):
    """max |sv - s| / sigma_1 with LAPACK's min(m, ncols) values padded with zeros to m."""
    full = np.zeros(m)
    full[:s.size] = s
    return float(np.abs(np.asarray(sv) - full).max() / s[0])


def rank_is_unambiguous(s):
    """The tests' precondition: no reference singular value in [1e-13, 1e-10] sigma_1."""
    return not np.any((s >= 1e-13 * s[0]) & (s <= 1e-10 * s[0]))


def _graded(m, ncols, sigma, seed):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((m, m)))
    V, _ = np.linalg.qr(rng.standard_normal((ncols, m)))
    return (U * np.asarray(sigma)) @ V.T


def esc16j_constraints(problems, golden):
    """(newA 33 x 150, b 33): A * PMat of the esc16j QAP relaxation on its golden partition, with SciPy."""
    import scipy.sparse as sp
    fa, fb = problems.read_qapdata(ROOT / "tests" / "golden" / "esc16j.dat")
    _, A, b = problems.qap_problem(fa, fb)
    L = np.asarray(golden["esc16j_P"]).reshape(-1, order="F").astype(np.int64)
    d = int(L.max())
    keep = np.nonzero(L)[0]
    PMat = sp.csr_matrix((np.ones(keep.size), (keep, L[keep] - 1)), shape=(L.size, d))
    newA = np.asarray((sp.csr_matrix(A) @ PMat).todense(), dtype=np.float64)
    return np.asfortranarray(newA), np.ascontiguousarray(b, dtype=np.float64)


def inputs(problems, golden):
    """{name: (newA, b, reference rank)}: M = [newA | b] is the matrix of the issue's table."""
    out = {}
    M = _graded(6, 37, [1, 1e-3, 1e-6, 1e-9, 0, 0], 11)
    out["graded_6x37"] = (M[:, :-1], M[:, -1], 4)
    M = _graded(7, 4097, [1, 1e-3, 1e-6, 1e-9, 0, 0, 0], 12)
    out["graded_7x4097"] = (M[:, :-1], M[:, -1], 4)
    M = np.random.default_rng(13).integers(-3, 4, size=(9, 5)).astype(np.float64)
    out["integer_9x5"] = (M[:, :-1], M[:, -1], 5)
    d0, d1, d2 = np.random.default_rng(14).integers(-4, 5, size=(3, 70)).astype(np.float64)
    M = np.stack([d0, d1, d0, d2, 2 * d1, d0 + d2])
    out["duplicates_6x70"] = (M[:, :-1], M[:, -1], 3)
    newA, b = esc16j_constraints(problems, golden)
    out["esc16j"] = (newA, b, 9)
    return {k: (np.asfortranarray(a), np.ascontiguousarray(b), r) for k, (a, b, r) in out.items()}


def stack(newA, b):
    return np.asarray(newA) if b is None else np.hstack([np.asarray(newA), np.asarray(b).reshape(-1, 1)])


def stop_threshold(ncols):
    """csrc/rowspace.cpp: a pass whose rotated |g_pq| / sqrt(g_pp g_qq) all lie under twice the probable rounding error of a
    length-ncols dot product is the last."""
    return 2.0 * np.sqrt(float(ncols)) * EPS


def pass_scheme(M, jacobi, rtol=0.0):
    """The iteration of csrc/rowspace.cpp on the CPU.  jacobi(G, tau, floor2, max_sweeps) -> (rotations, J, largest rotated
    |g_pq| / sqrt(g_pp g_qq)) is csrc/host_gram_jacobi.cpp.  Returns (rows r x ncols, rank, sv (m), passes, converged)."""
    M = np.asarray(M, dtype=np.float64)
    m, ncols = M.shape
    rt = rtol if rtol > 0 else min(m, ncols) * EPS
    mx = np.abs(M).max() if M.size else 0.0
    if mx == 0:
        return np.zeros((0, ncols)), 0, np.zeros(m), 0, True
    scale = 2.0 ** -np.frexp(mx)[1]
    W = M * scale
    passes, converged = 0, False
    while passes < MAX_PASSES:
        passes += 1
        rot, J, max_rel = jacobi(W @ W.T, EPS, rt * rt, MAX_SWEEPS)
        if rot:
            W = J @ W
        if max_rel <= stop_threshold(ncols):
            converged = True
            break
    sigma = np.sqrt((W * W).sum(axis=1))
    order = np.argsort(-sigma, kind="stable")
    r = int(np.count_nonzero(sigma > rt * sigma.max()))
    R = W[order[:r]] / sigma[order[:r], None]
    lead = np.abs(R).argmax(axis=1)
    R = R * np.where(R[np.arange(r), lead] < 0, -1.0, 1.0)[:, None]
    return R, r, sigma[order] / scale, passes, converged
