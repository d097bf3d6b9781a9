"""admissible_subspace from host (C, A, b) through the three setup paths -- the CSR entry (sdpsr_admissible_subspace_csr),
the dense device entry (sdpsr_admissible_subspace_dense) and the NumPy setup (admissible_setup + sdpsr_admissible_subspace)
-- on esc16j, configs[2] (grid QAP n = 30, N = 900) and a grid QAP with n = 64 (N = 4096).  Per problem and path: wall ms
of the whole call (best of the repetitions), the loop's own ms (phase_ms[T_TOTAL]) and the rest (setup), host waits
(sdpsr_profile_host_waits), H2D bytes (sdpsr_transfer_bytes) and which orthogonalisation ran.  Paths that cannot run
(the dense entry above 4 GiB of dense A, the host QR of a 17 GB matrix) are reported as skipped.

  python tools/csr_setup_time.py [--reps K] [--json]
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
from __graft_entry__ import load_package  # noqa: E402

PATH_NAMES = {0: "none (m = 0)", 1: "CholeskyQR2", 2: "MGS"}


def problems(pr):
    fa, fb = pr.read_qapdata(os.path.join(ROOT, "tests", "golden", "esc16j.dat"))
    yield "esc16j", pr.qap_problem(fa, fb)
    flow, dist = pr.grid_qap_instance(5, 6, seed=4)
    yield "configs[2] grid QAP n=30", pr.qap_problem(flow, dist)
    flow, dist = pr.grid_qap_instance(8, 8, seed=1)
    yield "grid QAP n=64", pr.qap_problem(flow, dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    prof = pkg._lib.load_prof_library()
    L = pkg._lib
    import torch  # noqa: F401  (the library shares torch's HIP runtime)

    def waits(ctx):
        w = C.c_uint64(0)
        prof.sdpsr_profile_host_waits(ctx._h, C.byref(w))
        return int(w.value)

    rows = []
    for name, (Cv, A, b) in problems(load_package().problems):
        m, ln = A.shape
        nnz = A.nnz
        dense_bytes = m * ln * 8
        paths = [("csr", lambda ctx: pkg.admissible_subspace(Cv, A, b, ctx=ctx, csr_setup=True))]
        if dense_bytes <= (4 << 30):
            paths.append(("dense", lambda ctx: pkg.admissible_subspace(Cv, A, b, ctx=ctx)))
        else:
            rows.append({"problem": name, "path": "dense", "skipped": f"dense A is {dense_bytes / 2**30:.1f} GiB (> 4 GiB)"})
        if dense_bytes <= (1 << 30):
            paths.append(("numpy", lambda ctx: pkg.admissible_subspace(Cv, A, b, ctx=ctx, host_setup=True)))
        else:
            rows.append({"problem": name, "path": "numpy", "skipped": f"host QR of a {dense_bytes / 2**30:.1f} GiB dense A"})
        for path, call in paths:
            with pkg.Context(seed=1) as ctx:
                reps = args.reps if ln < (1 << 22) else 1
                best = None
                for rep in range(reps + 1):  # the first call allocates the ctx's buffers: not counted
                    w0, (h0, _) = waits(ctx), ctx.transfer_bytes()
                    t = time.perf_counter()
                    P = call(ctx)
                    wall = (time.perf_counter() - t) * 1e3
                    w1, (h1, _) = waits(ctx), ctx.transfer_bytes()
                    if rep == 0 and reps > 1:
                        continue
                    if best is None or wall < best["wall_ms"]:
                        loop = float(P.phase_ms[L.T_TOTAL])
                        best = {"problem": name, "path": path, "N": int(round(ln ** 0.5)), "m": m, "nnz": nnz, "wall_ms": round(wall, 3),
                                "loop_ms": round(loop, 3), "setup_ms": round(wall - loop, 3), "host_waits": w1 - w0, "h2d_bytes": h1 - h0,
                                "dim": P.nparts, "iterations": P.iterations}
                if path == "csr":
                    # the C entry alone, from canonical CSR arrays (no Python conversion): its host pass + upload + device work
                    c = np.ascontiguousarray(np.asarray(Cv, dtype=np.float64).reshape(-1))
                    rp, ci, va = pkg.csr_arrays(A, ln)
                    bb = np.ascontiguousarray(b, dtype=np.float64)
                    CLd, X0d = torch.empty(ln, dtype=torch.float64, device="cuda"), torch.empty(ln, dtype=torch.float64, device="cuda")
                    Ud = torch.empty((m, ln), dtype=torch.float64, device="cuda")
                    r_, h_, i_ = C.c_int64(0), C.c_int(0), C.c_int32(0)
                    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
                    entry = []
                    for _ in range(2 if ln >= (1 << 22) else reps + 1):
                        w0 = waits(ctx)
                        t = time.perf_counter()
                        ctx.check(ctx._lib.sdpsr_admissible_setup_csr(ctx._h, best["N"], m, p(rp), p(ci), p(va), 0, p(bb), p(c), pkg.api.RTOL_DEFAULT,
                                                                      C.c_void_p(CLd.data_ptr()), C.c_void_p(X0d.data_ptr()), C.c_void_p(Ud.data_ptr()),
                                                                      C.byref(r_), C.byref(h_), C.byref(i_), L.MEM_DEVICE))
                        entry.append(((time.perf_counter() - t) * 1e3, waits(ctx) - w0))
                    best["setup_entry_ms"] = round(min(e[0] for e in entry[1:]), 3)
                    best["setup_entry_host_waits"] = entry[-1][1]
                    del CLd, X0d, Ud
                    t = time.perf_counter()
                    S = pkg.admissible_setup_csr(Cv, A, b, ctx=ctx)
                    best["setup_only_wall_ms"] = round((time.perf_counter() - t) * 1e3, 3)
                    best["orthogonalisation"] = PATH_NAMES[S.info]
                    best["r"] = int(S[3].shape[1])
                    del S
                elif path == "dense":
                    # the dense entry's uploads of A and C are plain copies the counter does not see
                    best["h2d_bytes"] = dense_bytes + ln * 8
                    best["h2d_note"] = "array bytes of A and C"
                    best["orthogonalisation"] = "MGS (dense entry)"
                else:
                    best["orthogonalisation"] = "host pivoted QR"
                rows.append(best)
            print(json.dumps(rows[-1]) if args.json else
                  f"{name:26s} {path:6s} wall {best['wall_ms']:9.2f} ms  setup {best['setup_ms']:9.2f}  loop {best['loop_ms']:8.2f}  "
                  f"waits {best['host_waits']:4d}  H2D {best['h2d_bytes'] / 1e6:9.1f} MB  {best['orthogonalisation']}  dim {best['dim']}"
                  + (f"  | C setup entry {best['setup_entry_ms']:.2f} ms, {best['setup_entry_host_waits']} waits" if path == "csr" else ""),
                  flush=True)
    for r in rows:
        if "skipped" in r:
            print(f"{r['problem']:26s} {r['path']:6s} skipped: {r['skipped']}")
    if args.json:
        print(json.dumps(rows))


if __name__ == "__main__":
    main()
