"""Two SDPs with one PSD block of order 65 .. 128 and a dual certificate each, for the PSD projection and the solver above
order 64 (a context with psd_max_order = 128).  Builders only: no dependence on the library.

(a) lmin_instance(s): maximise lambda_min(F_0 + sum_{i >= 2} x_i F_i) over x_2 .. x_{d-1}, as the SDP
        max x_1   s.t.   x_0 = 1,   x_0 F_0 - x_1 I + sum_{i >= 2} x_i F_i  PSD          (x free)
    with F_i = (G + G') / sqrt(2 s), G standard normal, traceless for i >= 2.  Certificate: Yh = -Y / tr(-Y) is PSD with trace 1,
    <Yh, F_i> = 0 for i >= 2 at the optimum, and then lambda_min(F_0 + sum x_i F_i) <= <Yh, F_0 + sum x_i F_i> = <Yh, F_0>.
(b) theta_instance(n, p): theta' of G(n, p) with no reduction at all -- X_ij = 0 on the edges, tr X = 1, X >= 0 entrywise, maximise
    <J, X>.  Variables: the n diagonal entries, then the non-edge pairs i < j (row-major).  Certificate: with W = -Y |c|_2 PSD and
    g = c + B'W, every feasible x has c'x = g'x - <W, Bx> <= g'x <= max(g[:n]) sum x[:n] + sum_k max(g_k, 0) x_k, and tr X = 1 with
    X PSD bounds an off-diagonal entry by 1/2: the bound is max(g[:n]) + 1/2 sum max(g[n:], 0)."""
import functools

import numpy as np

from sdp_admm_ref import admm_ref


class Instance:
    pass


def _upper_triplets(mats, s):
    """Triplets (classptr, blk, row, col, val) of one block of order s: the non-zero upper-triangle entries of every matrix,
    column-major inside the block."""
    col, row = np.nonzero(np.triu(np.ones((s, s))).T)  # (row <= col), columns ascending, rows ascending inside a column
    ptr, rows, cols, vals = [0], [], [], []
    for F in mats:
        v = F[row, col]
        keep = v != 0.0
        rows.append(row[keep])
        cols.append(col[keep])
        vals.append(v[keep])
        ptr.append(ptr[-1] + int(keep.sum()))
    rows, cols = np.concatenate(rows).astype(np.int32), np.concatenate(cols).astype(np.int32)
    return np.asarray(ptr, dtype=np.int64), np.zeros(rows.size, dtype=np.int32), rows, cols, np.concatenate(vals)


def lmin_instance(s, d=6, seed=None):
    rng = np.random.default_rng(500 + s if seed is None else seed)
    F = []
    for i in range(d):
        G = rng.standard_normal((s, s))
        Fi = (G + G.T) / np.sqrt(2.0 * s)
        if i >= 2:
            Fi = Fi - (np.trace(Fi) / s) * np.eye(s)
        F.append(Fi)
    F[1] = -np.eye(s)
    t = Instance()
    t.name, t.sizes, t.d, t.F = f"lmin{s}", [s], d, F
    t.B = np.stack([Fi.ravel(order="F") for Fi in F], axis=1)
    t.trip = _upper_triplets(F, s)
    t.A, t.b, t.c = np.eye(d)[:1], np.ones(1), np.eye(d)[1]
    t.sense, t.nonneg = "max", False
    t.apply = t.adjoint = None
    t.bound = lambda Y: _lmin_bound(np.asarray(Y, dtype=np.float64).reshape(s, s, order="F"), F[0])
    return t


def _lmin_bound(Y, F0):
    Yh = -Y / np.trace(-Y)
    return float(np.sum(Yh * F0))


def theta_instance(n=66, p=0.5, seed=1):
    adj = np.triu(np.random.default_rng(seed).random((n, n)) < p, 1)
    adj = adj | adj.T
    pi, pj = np.nonzero(np.triu(~adj, 1))  # the non-edge pairs i < j, row-major
    d = n + pi.size
    dg = np.arange(n) * (n + 1)
    lo, up = np.concatenate([dg, pj + pi * n]), np.concatenate([dg, pi + pj * n])  # flat positions (column-major): (j, i) and (i, j)
    t = Instance()
    t.name, t.sizes, t.d, t.n = f"theta{n}", [n], d, n
    t.B = np.zeros((n * n, d))
    t.B[lo, np.arange(d)] = 1.0
    t.B[up, np.arange(d)] = 1.0
    # upper triplets, one per variable: (i, i) for the diagonal, (i, j) with i < j for a pair
    t.trip = (np.arange(d + 1, dtype=np.int64), np.zeros(d, dtype=np.int32), np.concatenate([np.arange(n), pi]).astype(np.int32),
              np.concatenate([np.arange(n), pj]).astype(np.int32), np.ones(d))
    t.c = np.concatenate([np.ones(n), np.full(pi.size, 2.0)])
    t.A, t.b = np.concatenate([np.ones(n), np.zeros(pi.size)])[None, :], np.ones(1)
    t.sense, t.nonneg = "max", True

    def apply(x):  # B @ x: one variable per position, so no sum at all
        Z = np.zeros(n * n)
        Z[lo] = x
        Z[up] = x
        return Z

    def adjoint(S):  # B' @ S: the diagonal once (lo == up there), a pair as the sum of its two positions
        g = S[lo] + S[up]
        g[:n] = S[lo[:n]]
        return g

    t.apply, t.adjoint = apply, adjoint
    cn = float(np.linalg.norm(t.c))

    def bound(Y):
        g = t.c + adjoint(-np.asarray(Y, dtype=np.float64).reshape(-1) * cn)
        return float(g[:n].max() + 0.5 * np.maximum(g[n:], 0.0).sum())

    t.bound = bound
    return t


SOLVER = dict(rho=1.0, eps=1e-9, check_every=50)


@functools.lru_cache(maxsize=None)
def instance(name):
    """'lmin65', 'lmin97', 'lmin128' or 'theta66', built once."""
    return theta_instance(int(name[5:])) if name.startswith("theta") else lmin_instance(int(name[4:]))


@functools.lru_cache(maxsize=None)
def restatement(name):
    """The NumPy restatement (tests/sdp_admm_ref.py) on an instance at SOLVER's settings, once per process.  (b) applies its 0/1
    pencil by indexing: every position holds one variable and every variable at most two positions, so B x and B'S are the
    same numbers as the dense products, without 4356 x 1123 multiplications by zero per iteration."""
    t = instance(name)
    return admm_ref(t.B, t.sizes, t.A, t.b, t.c, sense=t.sense, nonneg=t.nonneg, apply=t.apply, adjoint=t.adjoint, **SOLVER)
