"""One full flow from a sparse A -- the setup stage and the assembly A * PMat -- through a sparse-constraints handle
(sdpsr_sparse_create once, then sdpsr_admissible_setup_sparse and sdpsr_reduce_constraints_sparse) against the route
without one (sdpsr_admissible_setup_csr + sdpsr_reduce_constraints_csr from the same raw arrays, each with its host pass
and its upload), on esc16j, configs[2] (grid QAP n = 30, 864 k non-zeros) and the grid QAP with n = 64 (N = 4096, 17.2 M).

Per instance, best of 3 after a warm-up, wall ms of the C entry alone: create from raw host arrays, from device arrays
and from shuffled arrays with duplicates (which forces the sort); setup and assembly from the handle; their sum for one
flow; the _csr route; H2D bytes from sdpsr_transfer_bytes and the host waits of create (sdpsr_profile_host_waits).

  python tools/sparse_handle_time.py [--out profiles/r14_sparse_handle.txt] [--parent-lib PATH/libsdpsr_hip.so] [--rounds 2]

--parent-lib: a libsdpsr_hip.so built from the parent commit; its _csr route is measured too, each side in processes of
its own that alternate (parent, this, parent, this, ...), and every figure is the best over the rounds.  Without it the
_csr column is this build's own _csr entries (the same code behind the refactor).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ATOL = float(np.sqrt(np.finfo(np.float64).eps))
INSTANCES = ("esc16j", "configs[2] grid QAP n=30", "grid QAP n=64")


def instance(pr, name):
    if name == "esc16j":
        fa, fb = pr.read_qapdata(os.path.join(ROOT, "tests", "golden", "esc16j.dat"))
        return pr.qap_problem(fa, fb)
    if name.startswith("configs[2]"):
        return pr.qap_problem(*pr.grid_qap_instance(5, 6, seed=4))
    return pr.qap_problem(*pr.grid_qap_instance(8, 8, seed=1))


def shuffled_with_duplicates(rp, ci, va):
    """Every row reversed and every 16th entry split into two halves: unsorted rows with duplicates, the same matrix."""
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    src = rp[rows] + rp[rows + 1] - 1 - np.arange(ci.size)  # position p of row i reads position rp[i] + rp[i + 1] - 1 - p
    reps = 1 + (np.arange(ci.size) % 16 == 0)
    ci2, va2 = np.repeat(ci[src], reps), np.repeat(va[src] / reps, reps)
    rp2 = np.concatenate([[0], np.cumsum(reps)])[rp]
    return rp2.astype(np.int64), np.ascontiguousarray(ci2, dtype=np.int64), np.ascontiguousarray(va2, dtype=np.float64)


def best_of(f, reps=3):
    f()  # warm-up: the ctx's buffers are allocated here
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return round(min(out), 3)


def bind(lib):
    vp, i64, dbl = C.c_void_p, C.c_int64, C.c_double
    pi64, pi32, pint = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int)
    sigs = {
        "sdpsr_create": [C.c_int, C.c_uint64, vp, C.POINTER(vp)],
        "sdpsr_destroy": [vp],
        "sdpsr_transfer_bytes": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
        "sdpsr_admissible_setup_csr": [vp, i64, i64, vp, vp, vp, C.c_int, vp, vp, dbl, vp, vp, vp, pi64, pint, pi32, C.c_int],
        "sdpsr_admissible_subspace_csr": [vp, i64, i64, vp, vp, vp, C.c_int, vp, vp, dbl, vp, pi64, pi32, vp, C.c_int],
        "sdpsr_reduce_constraints_csr": [vp, i64, vp, i64, i64, vp, vp, vp, C.c_int, vp, C.c_int],
        "sdpsr_sparse_create": [vp, i64, i64, i64, vp, vp, vp, C.c_int, C.c_int, C.POINTER(vp)],
        "sdpsr_sparse_destroy": [vp],
        "sdpsr_admissible_setup_sparse": [vp, i64, vp, vp, vp, dbl, vp, vp, vp, pi64, pint, pi32, C.c_int],
        "sdpsr_reduce_constraints_sparse": [vp, vp, vp, i64, vp, C.c_int],
    }
    for name, args in sigs.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = None if name == "sdpsr_destroy" else C.c_int
    return lib


def measure(side, lib_path, names):
    """One side in this process: 'csr' (the route without a handle, from lib_path when given) or 'handle'."""
    import torch
    pkg = load_package()
    L = pkg._lib
    lib = bind(C.CDLL(lib_path)) if lib_path else bind(L.load_library())
    prof = None if lib_path else L.load_prof_library()
    o = L.Opts()
    o.struct_size = C.sizeof(L.Opts)
    ctx = C.c_void_p()
    assert lib.sdpsr_create(0, 1, C.byref(o), C.byref(ctx)) == 0
    p = lambda a: C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else C.c_void_p(a.ctypes.data)  # noqa: E731

    def ok(st):
        assert st == 0, st

    def h2d():
        a, b = C.c_uint64(0), C.c_uint64(0)
        lib.sdpsr_transfer_bytes(ctx, C.byref(a), C.byref(b))
        return int(a.value)

    def waits():
        w = C.c_uint64(0)
        prof.sdpsr_profile_host_waits(ctx, C.byref(w))
        return int(w.value)

    rows = []
    for name in names:
        Cv, A, b = instance(pkg.problems, name)
        A = A.tocsr()
        rp, ci, va = A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(A.data, dtype=np.float64)
        m, ln = A.shape
        n, nnz = int(round(ln ** 0.5)), ci.size
        c = np.ascontiguousarray(np.asarray(Cv.todense() if hasattr(Cv, "todense") else Cv, dtype=np.float64).reshape(-1))
        bb = np.ascontiguousarray(b, dtype=np.float64)
        CLd, X0d = (torch.empty(ln, dtype=torch.float64, device="cuda") for _ in range(2))
        Ud = torch.empty((m, ln), dtype=torch.float64, device="cuda")
        r_, h_, i_ = C.c_int64(0), C.c_int(0), C.c_int32(0)
        # the partition the assembly is measured on: the instance's own admissible subspace
        lab = np.zeros(ln, dtype=np.uint32)
        d_, it_ = C.c_int64(0), C.c_int32(0)
        ok(lib.sdpsr_admissible_subspace_csr(ctx, n, m, p(rp), p(ci), p(va), 0, p(bb), p(c), ATOL, p(lab), C.byref(d_), C.byref(it_), None, 0))
        d = int(d_.value)
        out = np.zeros((m, d), order="F")
        row = {"instance": name, "N": n, "m": m, "nnz": int(nnz), "dim": d, "side": side}
        if side == "csr":
            setup = lambda: ok(lib.sdpsr_admissible_setup_csr(ctx, n, m, p(rp), p(ci), p(va), 0, p(bb), p(c), ATOL, p(CLd), p(X0d), p(Ud),  # noqa: E731
                                                              C.byref(r_), C.byref(h_), C.byref(i_), 1))
            asm = lambda: ok(lib.sdpsr_reduce_constraints_csr(ctx, ln, p(lab), d, m, p(rp), p(ci), p(va), 0, p(out), 0))  # noqa: E731
            row["csr_setup_ms"], row["csr_assembly_ms"] = best_of(setup), best_of(asm)
            u0 = h2d()
            setup()
            asm()
            row["csr_h2d_bytes"] = h2d() - u0
            row["csr_flow_ms"] = round(row["csr_setup_ms"] + row["csr_assembly_ms"], 3)
        else:
            hs = []

            def create(arrs, mem):
                h = C.c_void_p()
                ok(lib.sdpsr_sparse_create(ctx, ln, m, arrs[1].shape[0], p(arrs[0]), p(arrs[1]), p(arrs[2]), 0, mem, C.byref(h)))
                hs.append(h)

            def timed_create(arrs, mem):
                t = best_of(lambda: create(arrs, mem))
                while len(hs) > 1:  # keep the last handle only
                    lib.sdpsr_sparse_destroy(hs.pop(0))
                return t

            row["create_host_ms"] = timed_create((rp, ci, va), 0)
            u0, w0 = h2d(), waits()
            create((rp, ci, va), 0)
            row["create_h2d_bytes"], row["create_host_waits"] = h2d() - u0, waits() - w0
            lib.sdpsr_sparse_destroy(hs.pop(0))
            dev = tuple(torch.from_numpy(a).cuda() for a in (rp, ci, va))
            torch.cuda.synchronize()
            row["create_device_ms"] = timed_create(dev, 1)
            lib.sdpsr_sparse_destroy(hs.pop(0))
            del dev
            sh = shuffled_with_duplicates(rp, ci, va)
            row["create_shuffled_ms"] = timed_create(sh, 0)
            row["shuffled_nnz"] = int(sh[1].size)
            h = hs[0]  # (the shuffled arrays are the same matrix: the same canonical arrays)
            setup = lambda: ok(lib.sdpsr_admissible_setup_sparse(ctx, n, h, p(bb), p(c), ATOL, p(CLd), p(X0d), p(Ud), C.byref(r_), C.byref(h_),  # noqa: E731
                                                                 C.byref(i_), 1))
            asm = lambda: ok(lib.sdpsr_reduce_constraints_sparse(ctx, h, p(lab), d, p(out), 0))  # noqa: E731
            row["setup_ms"], row["assembly_ms"] = best_of(setup), best_of(asm)
            u0 = h2d()
            setup()
            asm()
            row["consumers_h2d_bytes"] = h2d() - u0
            row["flow_ms"] = round(row["create_host_ms"] + row["setup_ms"] + row["assembly_ms"], 3)
            lib.sdpsr_sparse_destroy(hs.pop(0))
        row["setup_path"], row["hint"] = int(i_.value), int(h_.value)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del CLd, X0d, Ud
    lib.sdpsr_destroy(ctx)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_sparse_handle.txt"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--side", choices=("csr", "handle"), default=None, help="(internal) measure one side in this process")
    ap.add_argument("--lib", default=None, help="(internal) the library of the csr side")
    ap.add_argument("--instances", default=",".join(INSTANCES))
    args = ap.parse_args()
    names = [s for s in args.instances.split(",") if s]
    if args.side:
        measure(args.side, args.lib, names)
        return
    best = {}
    sides = [("csr", args.parent_lib), ("handle", None)]
    for _ in range(max(1, args.rounds)):
        for side, lib in sides:  # alternating processes: parent, this, parent, this, ...
            cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--instances", ",".join(names)] + (["--lib", lib] if lib else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                sys.exit(f"{side} side failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
            for line in res.stdout.splitlines():
                if line.startswith("{"):
                    row = json.loads(line)
                    acc = best.setdefault(row["instance"], {})
                    for k, v in row.items():
                        acc[k] = min(acc[k], v) if k.endswith("_ms") and k in acc else v
    csr_name = "parent commit's _csr route" if args.parent_lib else "this build's _csr route"
    lines = [f"sparse-constraints handle against the {csr_name}; wall ms of the C entries, best of 3 after a warm-up, best of "
             f"{max(1, args.rounds)} alternating processes per side", ""]
    for name in names:
        r = best[name]
        r["flow_ms"] = round(r["create_host_ms"] + r["setup_ms"] + r["assembly_ms"], 3)
        r["csr_flow_ms"] = round(r["csr_setup_ms"] + r["csr_assembly_ms"], 3)
        verdict = "gain" if r["flow_ms"] < r["csr_flow_ms"] else "LOSS"
        lines += [
            f"{name}: N = {r['N']}, m = {r['m']}, nnz = {r['nnz']}, dim(P) = {r['dim']}",
            f"  create from raw host arrays      {r['create_host_ms']:10.3f} ms   H2D {r['create_h2d_bytes']} B, {r['create_host_waits']} host waits",
            f"  create from device arrays        {r['create_device_ms']:10.3f} ms",
            f"  create, shuffled + duplicates    {r['create_shuffled_ms']:10.3f} ms   ({r['shuffled_nnz']} raw entries, the sort runs)",
            f"  setup from the handle            {r['setup_ms']:10.3f} ms   against {r['csr_setup_ms']:10.3f} ms (setup_csr)"
            f"      {'gain' if r['setup_ms'] < r['csr_setup_ms'] else 'LOSS'}",
            f"  assembly from the handle         {r['assembly_ms']:10.3f} ms   against {r['csr_assembly_ms']:10.3f} ms (reduce_constraints_csr)"
            f"   {'gain' if r['assembly_ms'] < r['csr_assembly_ms'] else 'LOSS'}",
            f"  one flow: create + setup + assembly {r['flow_ms']:10.3f} ms   against {r['csr_flow_ms']:10.3f} ms   {verdict}"
            f"   (H2D {r['create_h2d_bytes'] + r['consumers_h2d_bytes']} B against {r['csr_h2d_bytes']} B)",
            "",
        ]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
