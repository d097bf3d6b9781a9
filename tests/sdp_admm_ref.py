"""NumPy restatement of sdpsr_psd_project and sdpsr_sdp_solve (the first-order solver of the reduced SDP, include/sdpsr.h
"Solving the reduced SDP").  tests/test_sdp_admm_ref_cpu.py holds it to the reference's pinned optima on its own,
tests/test_gpu_psd_project.py and tests/test_gpu_sdp_solve.py compare the library with it.  No dependence on the library.

Problem (test/sd_problems.jl:39-52,120-134 of the reference):  max / min c'x  s.t.  A x = b,  x >= 0,  Z_k(x) >= 0 for all k,
with B: x -> (Z_k(x))_k the pencil of tests/blockop_ref.py acting on FULL entries, B' its adjoint.  Split x = u (u >= 0) and
B x = S (S PSD) with scaled duals lam, Lam; chat = -+c / |c|_2 (minus for max); M = I + B'B, G = A M^-1 A',
Kt = M^-1 - M^-1 A' G^-1 A M^-1, x0 = M^-1 A' G^-1 b.  One iteration:
    g  = (u - lam) + B'(S - Lam) - chat / rho
    x  = Kt g + x0
    u+ = max(0, x + lam)            S+ = proj_PSD(B x + Lam)      (block by block, from the LOWER triangles)
    lam+ = (x + lam) - u+           Lam+ = (B x + Lam) - S+
    r_p^2 = |x - u+|^2 + |B x - S+|^2,   r_d^2 = rho^2 (|u+ - u|^2 + |S+ - S|^2)
checked every `check_every` iterations (and at the last one): stop when r_p <= eps and r_d <= eps."""
import numpy as np

from blockop_ref import block_offsets


def dense_B(full, sum_sq, d):
    """The sum_sq x d matrix of the pencil from the full entry list (duplicates add)."""
    cls, pos, v = full
    B = np.zeros((int(sum_sq), int(d)))
    np.add.at(B, (pos, cls), v)
    return B


def psd_project_ref(flat, sizes, return_lambda_min=False):
    """P_k = V max(w, 0) V' of every block of the flat one-class array, from its lower triangle (numpy's eigh and a clamp)."""
    flat = np.asarray(flat, dtype=np.float64)
    off = block_offsets(sizes)
    out, lmin = np.empty_like(flat), np.empty(len(sizes))
    for k, s in enumerate(sizes):
        W = flat[off[k]:off[k + 1]].reshape(int(s), int(s), order="F")
        w, V = np.linalg.eigh(W, UPLO="L")
        P = (V * np.maximum(w, 0.0)) @ V.T
        out[off[k]:off[k + 1]] = ((P + P.T) / 2).ravel(order="F")
        lmin[k] = w[0]
    return (out, lmin) if return_lambda_min else out


def setup(B, A, b):
    """(Kt, x0) of the header; A is r x d with independent rows (r = 0 is legal)."""
    d = B.shape[1]
    Minv = np.linalg.inv(np.eye(d) + B.T @ B)
    Minv = (Minv + Minv.T) / 2
    A = np.asarray(A, dtype=np.float64).reshape(-1, d)
    if A.shape[0] == 0:
        return Minv, np.zeros(d)
    T = Minv @ A.T
    G = A @ T
    Ginv = np.linalg.inv((G + G.T) / 2)
    U = T @ Ginv
    return Minv - U @ T.T, U @ np.asarray(b, dtype=np.float64)


class Result:
    pass


def admm_ref(B, sizes, A, b, c, sense="max", rho=1.0, eps=1e-9, max_iters=20000, check_every=50, adapt_rho=False, nonneg=True,
             apply=None, adjoint=None):
    """The iteration above.  B: the dense pencil (the setup always uses it); apply / adjoint: optional callables that replace
    B @ x and B.T @ S inside the loop (another summation order).  Returns a Result with x, S, Y = rho Lam, objective, status,
    iters, rho, rho_changes, r_primal, r_dual."""
    B = np.asarray(B, dtype=np.float64)
    n, d = B.shape
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    apply = (lambda x: B @ x) if apply is None else apply
    adjoint = (lambda S: B.T @ S) if adjoint is None else adjoint
    Kt, x0 = setup(B, A, b)
    nc = np.linalg.norm(c)
    chat = (-c if sense == "max" else c) / (nc if nc > 0 else 1.0)
    u, lam, S, Lam, x = np.zeros(d), np.zeros(d), np.zeros(n), np.zeros(n), np.zeros(d)
    it, changes, rp, rd, status = 0, 0, np.inf, np.inf, "iteration_limit"
    while it < max_iters:
        g = (u - lam) + adjoint(S - Lam) - chat / rho
        x = Kt @ g + x0
        t = x + lam
        un = np.maximum(t, 0.0) if nonneg else t
        Bx = apply(x)
        W = Bx + Lam
        Sn = psd_project_ref(W, sizes)
        rp2 = np.sum((x - un) ** 2) + np.sum((Bx - Sn) ** 2)
        rd2 = np.sum((un - u) ** 2) + np.sum((Sn - S) ** 2)
        lam, Lam, u, S = t - un, W - Sn, un, Sn
        it += 1
        if it % check_every == 0 or it == max_iters:
            rp, rd = np.sqrt(rp2), rho * np.sqrt(rd2)
            if rp <= eps and rd <= eps:
                status = "converged"
                break
            if adapt_rho and it < max_iters:
                new = rho * 2 if rp > 10 * rd else (rho / 2 if rd > 10 * rp else rho)
                if new != rho:
                    lam, Lam = lam * (rho / new), Lam * (rho / new)
                    rho, changes = new, changes + 1
    r = Result()
    r.x, r.S, r.Y, r.objective, r.status, r.iters = x, S, rho * Lam, float(c @ x), status, it
    r.rho, r.rho_changes, r.r_primal, r.r_dual = rho, changes, float(rp), float(rd)
    return r


def reduced_sdp_ref(O, C, A, b, seed=0, labels=None):
    """The oracle's reduction of (C, A, b): (sizes, triplets dict, newA r x d, newB, newC) with the dependent rows of
    [A PMat, b] dropped by LAPACK's SVD (docs/src/examples/ReduceAndSolveJuMP.jl:42-51).  labels: a recorded admissible
    partition (tests/golden) instead of the oracle's own loop."""
    import scipy.sparse as sp
    from compress_ref import reference
    from sparse_images_ref import sparse_ref
    rng = np.random.default_rng(seed)
    P = O.admissible_subspace(C, A, b, rng=rng) if labels is None else O.partition_from_labels(np.asarray(labels))
    sizes, blks, _ = O.block_diagonalize(P, rng=rng)
    d = P.nparts
    L = np.asarray(P.matrix).reshape(-1, order="F").astype(np.int64)
    keep = np.nonzero(L)[0]
    PMat = sp.csr_matrix((np.ones(keep.size), (keep, L[keep] - 1)), shape=(L.size, d))
    newA = np.asarray((sp.csr_matrix(A) @ PMat).todense(), dtype=np.float64)
    newC = np.asarray((sp.csr_matrix(np.asarray(C, dtype=np.float64).reshape(1, -1)) @ PMat).todense()).reshape(-1)
    _, r, rows = reference(np.hstack([newA, np.asarray(b, dtype=np.float64).reshape(-1, 1)]))
    rows = np.where(np.abs(rows) <= 1e-8, 0.0, rows)
    flat = np.concatenate([np.asarray(blks[i][k], dtype=np.float64).ravel(order="F") for i in range(d) for k in range(len(sizes))])
    return [int(s) for s in sizes], sparse_ref(flat, sizes, upper=True), rows[:, :d], rows[:, d], newC
