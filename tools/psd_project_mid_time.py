"""sdpsr_psd_project and sdpsr_sdp_solve on blocks of order 65 .. 128 (a context with psd_max_order = 128) on one GPU.

Projection: 1 and 256 device-resident blocks of order 65, 96, 97, 98 and 128 -- V sits in LDS up to order 97 and in global memory
from 98 on, so 97 | 98 shows what that costs -- with device events on the library's stream, best of --reps after a warm-up, beside
the route a caller had before on the same device arrays: torch.linalg.eigh batched, a clamp and a matmul.

Solver: the instances of tests/sdp_mid_instances.py -- (a) at s = 65, 97, 128 and (b) theta' of G(66, 0.5) unreduced -- to
convergence: total ms, the setup (the same call with max_iters = 1), us per iteration from the difference, beside the wall time
of the NumPy restatement (tests/sdp_admm_ref.py) on one CPU process.  A loss is reported as a loss.

  python tools/psd_project_mid_time.py [--reps 5] [--instances lmin65,lmin97,lmin128,theta66] [--no-numpy] [--no-projection]
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
from sdp_solve_time import timed  # noqa: E402


def projection(pkg, ctx, stream, order, count, reps):
    import torch
    g = torch.Generator(device="cuda").manual_seed(order)
    Z3 = torch.randn(count, order, order, dtype=torch.float64, device="cuda", generator=g)
    Z3 = Z3 + Z3.transpose(1, 2)
    Z = Z3.reshape(-1).contiguous()
    P, lm = torch.empty_like(Z), torch.empty(count, dtype=torch.float64, device="cuda")
    sz = np.full(count, order, dtype=np.int32)
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    t = timed(stream, reps, lambda: ctx.check(ctx._lib.sdpsr_psd_project(ctx._h, count, C.c_void_p(sz.ctypes.data), vp(Z), vp(P), vp(lm),
                                                                          pkg._lib.MEM_DEVICE)))
    out = {}

    def eigh_route():
        w, V = torch.linalg.eigh(Z3)
        out["P"] = (V * w.clamp(min=0).unsqueeze(1)) @ V.transpose(1, 2)

    with torch.cuda.stream(stream):
        t_eigh = timed(stream, reps, eigh_route)
    diff = float((out["P"] - P.reshape(count, order, order)).abs().max())
    return {"psd_project_order": order, "blocks": count, "us_per_call": round(t * 1e6, 1), "us_per_block": round(t * 1e6 / count, 2),
            "torch_eigh_clamp_matmul_us": round(t_eigh * 1e6, 1), "speedup_over_torch": round(t_eigh / t, 2), "max_abs_difference": diff}


def solver(pkg, ctx, stream, name, reps, with_numpy):
    from sdp_mid_instances import SOLVER, instance, restatement
    t = instance(name)
    sp = pkg.SparseBlocks(*t.trip, t.sizes, len(t.trip[4]))
    out = {}
    with pkg.BlockOperator(sp, ctx=ctx) as op:
        def run(**o):
            out["sol"] = op.solve(t.A, t.b, t.c, sense=t.sense, nonneg=t.nonneg, **{**SOLVER, **o})
        t_total = timed(stream, reps, run)
        sol = out["sol"]
        t_setup = timed(stream, reps, lambda: run(max_iters=1))
    res = {"instance": name, "d": t.d, "blocks": t.sizes, "objective": sol.objective, "status": sol.status, "iters": sol.iters,
           "total_ms": round(t_total * 1e3, 3), "setup_and_one_iteration_ms": round(t_setup * 1e3, 3),
           "us_per_iteration": round((t_total - t_setup) / max(1, sol.iters - 1) * 1e6, 2)}
    if with_numpy:
        t0 = time.perf_counter()
        ref = restatement(name)
        res.update(numpy_ms=round((time.perf_counter() - t0) * 1e3, 1), numpy_iters=ref.iters, numpy_objective=ref.objective)
        res["numpy_us_per_iteration"] = round(res["numpy_ms"] * 1e3 / ref.iters, 1)
        res["speedup_over_numpy"] = round(res["numpy_ms"] / res["total_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", default="lmin65,lmin97,lmin128,theta66")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-projection", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("psd_project_mid_time.py measures on the GPU: none is visible")
    torch.cuda.init()
    pkg = load_package()
    with pkg.Context(seed=1, psd_max_order=128) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)  # the events are recorded on the stream the library works on
        if not args.no_projection:
            for order in (65, 96, 97, 98, 128):
                for count in (1, 256):
                    print(json.dumps(projection(pkg, ctx, stream, order, count, args.reps)), flush=True)
        for name in [s for s in args.instances.split(",") if s]:
            print(json.dumps(solver(pkg, ctx, stream, name, args.reps, not args.no_numpy)), flush=True)


if __name__ == "__main__":
    main()
