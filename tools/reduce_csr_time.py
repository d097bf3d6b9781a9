"""Reduced-SDP assembly newA = A * PMat (README.md:57-60) for a sparse A on esc16j, configs[2] (grid QAP n = 30, N = 900)
and a grid QAP with n = 64 (N = 4096); P comes from admissible_subspace(csr_setup=True).  Per problem, best of the
repetitions after a warm-up call:

  csr host    sdpsr_reduce_constraints_csr from canonical host CSR arrays, host labels and host out: wall ms, H2D bytes
              (sdpsr_transfer_bytes)
  csr device  the same with labels and out resident on the device (only the CSR arrays travel)
  convert     csr_arrays(A) of the Python mirror (SciPy's canonicalisation), not part of the two above
  dense       route (a) of the parent: reduce_constraints on the densified A, where it accepts the shape
  scipy       route (b) of the parent: A @ PMat on the host from the downloaded partition (PMat built once, not timed)

The entry's host pass (canonicalize_csr), its uploads and its kernels are one call and are not separated here.

  python tools/reduce_csr_time.py [--reps K] [--json] [--skip-large]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def problems(pr, skip_large):
    fa, fb = pr.read_qapdata(os.path.join(ROOT, "tests", "golden", "esc16j.dat"))
    yield "esc16j", pr.qap_problem(fa, fb)
    flow, dist = pr.grid_qap_instance(5, 6, seed=4)
    yield "configs[2] grid QAP n=30", pr.qap_problem(flow, dist)
    if not skip_large:
        flow, dist = pr.grid_qap_instance(8, 8, seed=1)
        yield "grid QAP n=64", pr.qap_problem(flow, dist)


def best_of(reps, fn):
    fn()  # warm-up: the first call allocates the ctx's buffers
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    L = pkg._lib
    import torch
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rows = []
    for name, (Cv, A, b) in problems(pkg.problems, args.skip_large):
        A = sp.csr_matrix(A)
        m, ln = A.shape
        with pkg.Context(seed=1) as ctx:
            P = pkg.admissible_subspace(Cv, A, b, ctx=ctx, csr_setup=True)
            d = P.nparts
            lab = np.ascontiguousarray(np.asarray(P.matrix).ravel(order="F"), dtype=np.uint32)
            t = time.perf_counter()
            rp, ci, va = pkg.csr_arrays(A, ln)
            convert_ms = (time.perf_counter() - t) * 1e3
            row = {"problem": name, "N": int(round(ln ** 0.5)), "m": m, "nnz": int(A.nnz), "dim": d, "convert_ms": round(convert_ms, 3)}
            out = np.empty((m, d), order="F")

            def host_call():
                ctx.check(ctx._lib.sdpsr_reduce_constraints_csr(ctx._h, ln, p(lab), d, m, p(rp), p(ci), p(va), 0, p(out), L.MEM_HOST))

            h0 = ctx.transfer_bytes()[0]
            host_call()
            row["csr_host_h2d_bytes"] = ctx.transfer_bytes()[0] - h0
            row["csr_host_ms"] = round(best_of(args.reps, host_call), 3)
            t_lab = torch.from_numpy(lab.view(np.int32)).cuda()
            t_out = torch.empty(m * d, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()

            def dev_call():
                ctx.check(ctx._lib.sdpsr_reduce_constraints_csr(ctx._h, ln, C.c_void_p(t_lab.data_ptr()), d, m, p(rp), p(ci), p(va), 0,
                                                                C.c_void_p(t_out.data_ptr()), L.MEM_DEVICE))

            h0 = ctx.transfer_bytes()[0]
            dev_call()
            row["csr_device_h2d_bytes"] = ctx.transfer_bytes()[0] - h0
            row["csr_device_ms"] = round(best_of(args.reps, dev_call), 3)
            same = np.array_equal(t_out.cpu().numpy().reshape(m, d, order="F"), out)
            del t_out
            # route (b): SciPy on the host
            idx = np.flatnonzero(lab > 0)
            PMat = sp.csr_matrix((np.ones(idx.size), (idx, lab[idx].astype(np.int64) - 1)), shape=(ln, d))
            ref = [None]

            def scipy_call():
                ref[0] = A @ PMat

            row["scipy_ms"] = round(best_of(args.reps, scipy_call), 3)
            row["equals_scipy"] = bool(same and np.array_equal(out, ref[0].toarray())) if m * d <= (1 << 26) else \
                bool(same and abs(sp.csr_matrix(out) - ref[0]).max() == 0)
            # route (a): the dense entry, where it takes the shape and a dense A is affordable
            if m * ln * 8 <= (1 << 30):
                Ad = A.toarray()
                try:
                    row["dense_ms"] = round(best_of(args.reps, lambda: pkg.reduce_constraints(P, Ad, ctx=ctx)), 3)
                    row["dense_h2d_bytes"] = m * ln * 8 + ln * 4
                except pkg.SdpsrError as e:
                    row["dense"] = "refused: " + str(e)
            else:
                row["dense"] = f"not tried: dense A is {m * ln * 8 / 2**30:.1f} GiB"
        rows.append(row)
        print(json.dumps(row) if args.json else
              f"{name:26s} m {m:4d} nnz {row['nnz']:9d} dim {d:7d} | csr host {row['csr_host_ms']:9.2f} ms H2D {row['csr_host_h2d_bytes'] / 1e6:7.1f} MB"
              f" | csr device {row['csr_device_ms']:9.2f} ms H2D {row['csr_device_h2d_bytes'] / 1e6:7.1f} MB | convert {row['convert_ms']:8.2f} ms"
              f" | scipy {row['scipy_ms']:9.2f} ms | dense "
              + (f"{row['dense_ms']:9.2f} ms" if "dense_ms" in row else row["dense"]) + f" | equals scipy: {row['equals_scipy']}", flush=True)
    if args.json:
        print(json.dumps(rows))


if __name__ == "__main__":
    main()
