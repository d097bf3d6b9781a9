"""sdpsr_compress_constraints (the independent rows of [A * PMat, b], docs/src/examples/ReduceAndSolveJuMP.jl:44-50) on a
device-resident newA, as sdpsr_reduce_constraints_sparse leaves it, against the route without it: D2H of newA, then
numpy.linalg.svd on the host, rank, rows and the drop -- timed end to end in the same process.  Instances: esc16j,
configs[2] (grid QAP n = 30) and the grid QAP with N = 4096, each on its own admissible subspace.

The library's call is timed with device events on its stream (they span the host's Jacobi work between the passes too) and
by the wall clock; best of 5 after a warm-up; passes and host waits of one call beside them.

  python tools/compress_constraints_time.py [--out profiles/r17_compress_constraints.txt] [--instances a,b]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

INSTANCES = ("esc16j", "configs[2] grid QAP n=30", "grid QAP N=4096")
EPS = float(np.finfo(np.float64).eps)


def instance(pr, name):
    if name == "esc16j":
        fa, fb = pr.read_qapdata(os.path.join(ROOT, "tests", "golden", "esc16j.dat"))
        return pr.qap_problem(fa, fb)
    if name.startswith("configs[2]"):
        return pr.qap_problem(*pr.grid_qap_instance(5, 6, seed=4))
    return pr.qap_problem(*pr.grid_qap_instance(8, 8, seed=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_compress_constraints.txt"))
    ap.add_argument("--instances", default=",".join(INSTANCES))
    args = ap.parse_args()
    import torch
    pkg = load_package()
    prof = pkg._lib.load_prof_library()
    stream = torch.cuda.Stream()
    ctx = pkg.Context(device=0, seed=1)
    ctx.set_stream(stream.cuda_stream)

    def waits():
        w = C.c_uint64(0)
        prof.sdpsr_profile_host_waits(ctx._h, C.byref(w))
        return int(w.value)

    lines = ["compress_constraints on a device-resident newA against D2H + numpy.linalg.svd on the host; best of 5 after a warm-up", ""]
    for name in [s for s in args.instances.split(",") if s]:
        Cv, A, b = instance(pkg.problems, name)
        b = np.ascontiguousarray(b, dtype=np.float64)
        ln = A.shape[1]
        with pkg.SparseConstraints(A, ln, ctx=ctx) as S:
            P = pkg.admissible_subspace(Cv, S, b, ctx=ctx)
            newA = pkg.api._reduce_constraints_sparse(P, S, ln, ctx, keep_on_device=True) if pkg.api._is_torch(P.matrix) else \
                torch.from_numpy(np.ascontiguousarray(pkg.reduce_constraints_csr(P, S, ctx=ctx).reshape(-1, order="F"))).cuda()
        m, d = S.m, int(P.nparts)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev, wall, info, w_call = [], [], None, 0
        for rep in range(6):
            w0, t0 = waits(), time.perf_counter()
            e0.record(stream)
            A2, B2, info = pkg.compress_constraints(newA, b, ctx=ctx, return_info=True, m=m)
            e1.record(stream)
            e1.synchronize()
            if rep:  # (the first call allocates the ctx's buffers)
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
            w_call = waits() - w0
        host, r_host = [], None
        for rep in range(6):
            t0 = time.perf_counter()
            M = np.hstack([newA.cpu().numpy().reshape(m, d, order="F"), b.reshape(-1, 1)])
            _, s, Vt = np.linalg.svd(M, full_matrices=False)
            r_host = int(np.count_nonzero(s > min(M.shape) * EPS * s[0]))
            rows = Vt[:r_host]
            rows[np.abs(rows) <= 1e-8] = 0.0
            if rep:
                host.append((time.perf_counter() - t0) * 1e3)
        R2 = np.hstack([A2.cpu().numpy(), B2.cpu().numpy().reshape(-1, 1)])
        resid = float(np.abs(M - (M @ R2.T) @ R2).max() / s[0])
        verdict = "gain" if min(wall) < min(host) else "LOSS"
        lines += [
            f"{name}: newA {m} x {d} (+ b), rank {info['rank']} (host SVD: {r_host}), {info['nnz']} non-zeros kept, resid {resid:.2e}",
            f"  compress_constraints   {min(wall):10.3f} ms wall   {min(ev):10.3f} ms between device events   {info['passes']} passes, {w_call} host waits",
            f"  D2H + numpy svd        {min(host):10.3f} ms wall   {verdict}",
            "",
        ]
        print("\n".join(lines[-4:]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
