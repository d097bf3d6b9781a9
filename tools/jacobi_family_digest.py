"""One SHA-256 per case over the raw output bytes of every entry point that runs a workgroup Jacobi kernel behind the shared
block frame (csrc/jacobi_frame.h), on fixed seeds: sdpsr_syev_f64 up to order 128, sdpsr_blocks_syev, sdpsr_psd_project on a
default context and on one with psd_max_order = 128, and sdpsr_sdp_solve for a fixed 50 iterations.  A change that must not
move a bit -- a refactor of the frame, of a core's wrapper, of the projection body -- is checked by running this at both
commits, each in a tree of its own, and comparing the listings line by line.  Bit patterns depend on the compiler release:
this is a tool and a record (profiles/), not a test.

  python tools/jacobi_family_digest.py [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402

HOST = 0
LINES = []


def emit(case, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    LINES.append(f"{case:<58s} {h.hexdigest()}")
    print(LINES[-1], flush=True)


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def sym(rng, s):
    A = rng.standard_normal((s, s))
    return A + A.T


def spectrum(rng, s, w):
    Q, _ = np.linalg.qr(rng.standard_normal((s, s)))
    B = (Q * np.asarray(w, dtype=np.float64)) @ Q.T
    return (B + B.T) / 2


def flat(blocks):
    return np.concatenate([np.asarray(B, dtype=np.float64).ravel(order="F") for B in blocks])


def syev(lib, ctx):
    def one(case, A):
        n = A.shape[0]
        B = np.array(A, order="F")
        w, V = np.full(n, 7.0), np.full((n, n), 7.0, order="F")
        st = lib.sdpsr_syev_f64(ctx._h, n, vp(B), vp(w), vp(V), HOST)
        emit(case, np.int32(st), w, V.ravel(order="F"))

    for n in (1, 2, 3, 16, 17, 63, 64, 65, 96, 97, 98, 127, 128):
        one(f"syev_f64 n={n}", sym(np.random.default_rng(1000 + n), n))
    for n in (48, 100):
        A = sym(np.random.default_rng(2000 + n), n)
        one(f"syev_f64 n={n} times 2^500", np.ldexp(A, 500))
        one(f"syev_f64 n={n} times 2^-600", np.ldexp(A, -600))


def blocks_syev(lib, ctx):
    rng = np.random.default_rng(3)
    sizes = [int(s) for s in rng.permutation(np.arange(1, 65))] + [1, 1, 5, 64]
    blocks = [sym(rng, s) for s in sizes]
    blocks[-2] = np.ldexp(blocks[-2], 600)  # scaled inside the kernel
    blocks[-1] = np.ldexp(blocks[-1], -600)
    Z, sz = flat(blocks), np.asarray(sizes, dtype=np.int32)
    for vectors in (True, False):
        w, V = np.full(int(sz.sum()), 7.0), (np.full(Z.size, 7.0) if vectors else None)
        st = lib.sdpsr_blocks_syev(ctx._h, len(sizes), vp(sz), vp(Z), vp(w), vp(V), HOST)
        emit(f"blocks_syev orders 1..64 mixed, V={'yes' if vectors else 'NULL'}", np.int32(st), w, *([V] if vectors else []))


def psd_batch(orders, special_orders, seed):
    """The plain orders, several blocks of order 1, and at every special order: all-negative, exactly n/2 and n/2 + 1 positive
    eigenvalues, times 2^500, times 2^-500, and one block holding a NaN."""
    rng = np.random.default_rng(seed)
    sizes = list(orders) + [1, 1, 1]
    blocks = [sym(rng, s) for s in sizes]
    for s in special_orders:
        w = rng.uniform(0.5, 2.0, s)
        bad = sym(rng, s)
        bad[s - 1, s // 2] = np.nan
        blocks += [spectrum(rng, s, -w), spectrum(rng, s, np.where(np.arange(s) < s // 2, w, -w)),
                   spectrum(rng, s, np.where(np.arange(s) < s // 2 + 1, w, -w)), np.ldexp(sym(rng, s), 500), np.ldexp(sym(rng, s), -500), bad]
        sizes += [s] * 6
    return sizes, flat(blocks)


def psd_project(lib, ctx, label, sizes, Z):
    sz = np.asarray(sizes, dtype=np.int32)
    for alias in (False, True):
        Zc = Z.copy()
        P, lm = (Zc if alias else np.full(Z.size, 7.0)), np.full(len(sizes), 7.0)
        st = lib.sdpsr_psd_project(ctx._h, len(sizes), vp(sz), vp(Zc), vp(P), vp(lm), HOST)  # the NaN block: a status, outputs written
        emit(f"psd_project {label}{', P aliases Z' if alias else ''}", np.int32(st), P, lm)


def solve(pkg, ctx, label, op, A, b, c, **kw):
    sol = op.solve(A, b, c, eps=1e-30, max_iters=50, return_S=True, return_Y=True, **kw)  # eps out of reach: 50 iterations exactly
    assert sol.iters == 50 and sol.status == "iteration_limit", (sol.iters, sol.status)
    info = np.asarray([sol.objective, sol.iters, sol.r_primal, sol.r_dual, sol.rho, sol.rho_changes, sol.eq_residual, sol.min_x, sol.lambda_min])
    emit(f"sdp_solve {label}, 50 iterations", sol.x, flat(sol.S), flat(sol.Y), info)


def sdp_solve(pkg, ctx, mid):
    pr = pkg.problems
    # theta' of Petersen (the reduction leaves three blocks of order 1: the clamps) and of ER(7) (blocks of order 2 and 3)
    for name, adj in (("petersen", pr.petersen_adjacency()), ("er7", pr.er_graph_adjacency(7))):
        Cv, A, b = pr.theta_prime_problem(adj)
        P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
        bd = pkg.blockDiagonalize(P, retries=2, ctx=ctx)
        newA, newB, newC = pkg.reduced_sdp(P, A, b, Cv, ctx=ctx)
        with pkg.BlockOperator(pkg.basis_image_sparse(bd.Q_hat, P, ctx=ctx), ctx=ctx) as op:
            solve(pkg, ctx, f"{name} (blocks {sorted(bd.blkSizes)})", op, np.asarray(newA), np.asarray(newB), np.asarray(newC), sense="max")
    from sdp_mid_instances import instance
    for name in ("lmin65", "lmin98"):
        t = instance(name)
        with pkg.BlockOperator(pkg.SparseBlocks(*t.trip, t.sizes, len(t.trip[4])), ctx=mid) as op:
            solve(pkg, mid, name, op, t.A, t.b, t.c, sense=t.sense, nonneg=t.nonneg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("jacobi_family_digest.py runs the kernels on the GPU: none is visible")
    pkg = load_package()
    lib = pkg.load_library()
    with pkg.Context(device=0, seed=11) as ctx, pkg.Context(device=0, seed=11, psd_max_order=128) as mid:
        syev(lib, ctx)
        blocks_syev(lib, ctx)
        psd_project(lib, ctx, "default ctx, orders <= 64", *psd_batch([1, 2, 3, 17, 64], [16, 17, 64], 5))
        psd_project(lib, mid, "psd_max_order=128, orders <= 128", *psd_batch([1, 2, 3, 17, 64, 65, 97, 98, 128], [17, 64, 65, 98, 128], 6))
        sdp_solve(pkg, ctx, mid)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
