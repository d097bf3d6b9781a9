"""sdpsr_sdp_solve and sdpsr_psd_project on one GPU.

Solver: the five instances with a pinned optimum in the reference (theta' of Petersen, ER(3), ER(5), ER(7) at rho = 1; esc16j at
rho = 10, 20 000 iterations), reduced by the device pipeline (admissible_subspace -> blockDiagonalize -> reduced_sdp ->
basis_image_sparse).  Device events on the library's stream around the whole call, best of --reps after a warm-up: total ms,
the setup (M, Kt: the same call with max_iters = 1, which also makes one iteration and the report), us per iteration from
the difference, host waits per solve (sdpsr_profile_host_waits), and beside it the wall time of the NumPy restatement
(tests/sdp_admm_ref.py) on the same inputs -- the only other solver in the tree.  A loss is reported as a loss.

Projection: 10^4 blocks each of order 2, 3, 7 and 64, device-resident: us per launch and blocks per second.

  python tools/sdp_solve_time.py [--reps 5] [--instances petersen,er3,er5,er7,esc16j] [--no-numpy]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402

PINS = {"petersen": 4.0, "er3": 5.0, "er5": 10.066926, "er7": 15.743402, "esc16j": 7.7942186}


def timed(stream, reps, fn):
    """Best device time (s) of fn over reps calls after a warm-up: events on `stream` around the call."""
    import torch
    best = None
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        s = e0.elapsed_time(e1) * 1e-3
        if i:
            best = s if best is None else min(best, s)
    return best


def problem(pr, name):
    if name == "petersen":
        return pr.theta_prime_problem(pr.petersen_adjacency()) + ("max",)
    if name.startswith("er"):
        return pr.theta_prime_problem(pr.er_graph_adjacency(int(name[2:]))) + ("max",)
    fa, fb = pr.read_qapdata(os.path.join(ROOT, "tests", "golden", "esc16j.dat"))
    return pr.qap_problem(fa, fb) + ("min",)


def solver(pkg, ctx, stream, prof, name, reps, with_numpy):
    from blockop_ref import block_offsets, full_entries
    from sdp_admm_ref import admm_ref, dense_B
    Cv, A, b, sense = problem(pkg.problems, name)
    P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
    bd = pkg.blockDiagonalize(P, retries=2, ctx=ctx)
    newA, newB, newC = pkg.reduced_sdp(P, A, b, Cv, ctx=ctx)
    sp = pkg.basis_image_sparse(bd.Q_hat, P, ctx=ctx)
    kw = dict(rho=10.0) if name == "esc16j" else {}
    out = {}
    with pkg.BlockOperator(sp, ctx=ctx) as op:
        def run(**o):
            out["sol"] = op.solve(newA, newB, newC, sense=sense, **kw, **o)
        t_total = timed(stream, reps, run)
        sol = out["sol"]
        w0, w1 = C.c_uint64(0), C.c_uint64(0)
        prof.sdpsr_profile_host_waits(ctx._h, C.byref(w0))
        run()
        prof.sdpsr_profile_host_waits(ctx._h, C.byref(w1))
        t_setup = timed(stream, reps, lambda: run(max_iters=1))
    res = {"instance": name, "d": int(P.nparts), "blocks": sorted(int(s) for s in bd.blkSizes), "r": int(np.asarray(newA).shape[0]),
           "objective": sol.objective, "relative_error_to_pin": abs(sol.objective - PINS[name]) / PINS[name], "status": sol.status,
           "iters": sol.iters, "total_ms": round(t_total * 1e3, 3), "setup_and_one_iteration_ms": round(t_setup * 1e3, 3),
           "us_per_iteration": round((t_total - t_setup) / max(1, sol.iters - 1) * 1e6, 2), "host_waits": int(w1.value - w0.value)}
    if with_numpy:
        full = full_entries(*(np.asarray(a) for a in (sp.classptr, sp.blk, sp.row, sp.col, sp.val)), sp.sizes, upper=sp.upper)
        B = dense_B(full, block_offsets(sp.sizes)[-1], int(P.nparts))
        t = time.perf_counter()
        ref = admm_ref(B, list(sp.sizes), np.asarray(newA), np.asarray(newB), np.asarray(newC), sense=sense, **kw)
        res.update(numpy_ms=round((time.perf_counter() - t) * 1e3, 1), numpy_iters=ref.iters, numpy_objective=ref.objective)
        res["speedup_over_numpy"] = round(res["numpy_ms"] / res["total_ms"], 2)
    return res


def projection(pkg, ctx, stream, order, count, reps):
    import torch
    g = torch.Generator(device="cuda").manual_seed(order)
    Z = torch.randn(count, order, order, dtype=torch.float64, device="cuda", generator=g)
    Z = (Z + Z.transpose(1, 2)).reshape(-1).contiguous()
    P, lm = torch.empty_like(Z), torch.empty(count, dtype=torch.float64, device="cuda")
    sz = np.full(count, order, dtype=np.int32)
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    t = timed(stream, reps, lambda: ctx.check(ctx._lib.sdpsr_psd_project(ctx._h, count, C.c_void_p(sz.ctypes.data), vp(Z), vp(P), vp(lm),
                                                                          pkg._lib.MEM_DEVICE)))
    return {"psd_project_order": order, "blocks": count, "us_per_call": round(t * 1e6, 1), "blocks_per_s": round(count / t),
            "note": "the call uploads its job table (16 bytes per block) and makes one host wait"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", default="petersen,er3,er5,er7,esc16j")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sdp_solve_time.py measures on the GPU: none is visible")
    torch.cuda.init()
    pkg = load_package()
    prof = pkg._lib.load_prof_library()
    with pkg.Context(seed=1) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)  # the events are recorded on the stream the library works on
        for name in [s for s in args.instances.split(",") if s]:
            print(json.dumps(solver(pkg, ctx, stream, prof, name, args.reps, not args.no_numpy)), flush=True)
        for order in (2, 3, 7, 64):
            print(json.dumps(projection(pkg, ctx, stream, order, 10000, args.reps)), flush=True)


if __name__ == "__main__":
    main()
