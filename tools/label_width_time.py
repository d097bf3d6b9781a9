"""Label arrays in the reference's own widths (Partition{T}, T = UInt8 / UInt16; sdpsr_set_label_width): two measurements.

  convert   sdpsr_labels_convert at len = 4096^2 on device-resident arrays, the four directions 32 -> 16, 32 -> 8, 16 -> 32,
            8 -> 32: best of 5 calls after a warm-up, device events around the call on the ctx's stream (and the host wall time of the
            call: launch + the wait for the stream that every entry point ends with), in us and in TB/s of bytes moved (bytes
            read + bytes written over the device time).
  batch     sdpsr_problem_reduce_batch with 4 restarts and HOST outputs (labels and block images of every restart copied into
            pageable host arrays) on the closed_scheme instance of bench.py at N = 4096, at label widths 32, 16 and 8: best of
            5 calls after a warm-up, reductions/s, and the sdpsr_transfer_bytes deltas per call.

  python tools/label_width_time.py [--widths 32,16,8] [--skip-convert] [--n 4096] [--reps 5] [--runs 1]

--widths 32 --skip-convert runs on a library without the label-width entry points too (the parent of the change that added
them): the width-32 leg is the same code path, and `--runs 5` repeats it to give that path's own spread.
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

ATOL = float(np.sqrt(np.finfo(np.float64).eps))
DTYPES = {8: np.uint8, 16: np.uint16, 32: np.uint32}


def best_of(reps, fn):
    fn()  # warm-up: the first call allocates the ctx's buffers
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        s = time.perf_counter() - t
        best = s if best is None else min(best, s)
    return best


def convert_rows(pkg, n, reps):
    import torch
    len_ = n * n
    rows = []
    with pkg.Context(seed=1) as ctx:
        lib = ctx._lib
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)  # (the events below are recorded on the stream the library works on)
        rng = np.random.default_rng(0)
        for in_bits, out_bits in ((32, 16), (32, 8), (16, 32), (8, 32)):
            src = rng.integers(0, 1 << min(in_bits, out_bits), size=len_, dtype=np.uint64).astype(DTYPES[in_bits])
            tin = torch.from_numpy(src.view(np.uint8)).cuda()
            tout = torch.empty(len_ * (out_bits // 8), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            ev = [0.0]

            def call():  # device events around the call on the ctx's stream: the pass itself, without the host's launch and wait
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.check(lib.sdpsr_labels_convert(ctx._h, len_, C.c_void_p(tin.data_ptr()), in_bits, C.c_void_p(tout.data_ptr()), out_bits, 1))
                e1.record(stream)
                e1.synchronize()
                ev[0] = e0.elapsed_time(e1) * 1e-3

            call()  # warm-up
            s_dev, s_wall = None, None
            for _ in range(reps):
                t = time.perf_counter()
                call()
                w = time.perf_counter() - t
                s_dev = ev[0] if s_dev is None else min(s_dev, ev[0])
                s_wall = w if s_wall is None else min(s_wall, w)
            ok = bool(np.array_equal(tout.cpu().numpy().view(DTYPES[out_bits]), src.astype(DTYPES[out_bits])))
            moved = len_ * (in_bits + out_bits) // 8
            rows.append({"convert": f"{in_bits}->{out_bits}", "len": len_, "device_us": round(s_dev * 1e6, 1), "call_wall_us": round(s_wall * 1e6, 1),
                         "bytes_moved": moved, "TB_per_s": round(moved / s_dev / 1e12, 3), "equals_astype": ok})
            del tin, tout
    return rows


def batch_rows(pkg, n, widths, reps, runs):
    pr = pkg.problems
    Ls, d = pr.synthetic_jordan_partition(n, seed=1)
    Cv, A, b = pr.partition_as_sdp(Ls, seed=1)
    setup = pkg.admissible_setup(Cv, A, b)
    _, CL, X0L, U = setup
    r = U.shape[1]
    Uf = np.asfortranarray(U) if r else None
    golden = np.ascontiguousarray(Ls.ravel(order="F"))
    R = 4
    hp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    rows = []
    for width in widths:
        for run in range(runs):
            with pkg.Context(seed=1000) as ctx:
                lib = ctx._lib
                if width != 32:
                    ctx.label_width = width
                hprob = C.c_void_p()
                ctx.check(lib.sdpsr_problem_create(ctx._h, n, hp(CL), hp(X0L), hp(Uf), r, int(getattr(setup, "hint", 0)), 0, C.byref(hprob)))
                try:
                    Ps = [np.zeros(n * n, dtype=DTYPES[width]) for _ in range(R)]
                    bl = [np.zeros(max(1, d * d)) for _ in range(R)]  # every block is 1 x 1: dim * sum_sq = d * d doubles
                    pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
                    pb = (C.c_void_p * R)(*[a.ctypes.data for a in bl])
                    cap = (C.c_int64 * R)(*[a.size for a in bl])
                    dd, st = (C.c_int64 * R)(), (C.c_int32 * R)()
                    oks = []

                    def call():
                        lib.sdpsr_problem_reduce_batch(ctx._h, hprob, R, None, ATOL, ATOL, C.cast(pP, C.c_void_p), dd, None, None, None, None,
                                                       C.cast(pb, C.c_void_p), cap, st, 0)
                        oks.append(sum(1 for x in st if x == 0))

                    call()
                    b0 = ctx.transfer_bytes()
                    call()
                    b1 = ctx.transfer_bytes()
                    s = best_of(reps, call)
                    same = all(dd[i] == d and np.array_equal(Ps[i], golden.astype(DTYPES[width])) for i in range(R))
                    rows.append({"batch_of_4_host_outputs": width, "run": run, "N": n, "dim": int(d), "ms_per_call": round(s * 1e3, 3),
                                 "reductions_per_s": round(R / s, 1), "restarts_ok_min": min(oks), "h2d_bytes_per_call": b1[0] - b0[0],
                                 "d2h_bytes_per_call": b1[1] - b0[1], "label_MB_per_restart": round(n * n * width / 8 / 1e6, 1),
                                 "equals_generator_partition": bool(same)})
                finally:
                    lib.sdpsr_problem_destroy(hprob)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="32,16,8")
    ap.add_argument("--skip-convert", action="store_true")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=1)
    args = ap.parse_args()
    pkg = load_package()
    widths = [int(x) for x in args.widths.split(",") if x]
    if not args.skip_convert:
        for row in convert_rows(pkg, args.n, args.reps):
            print(json.dumps(row), flush=True)
    for row in batch_rows(pkg, args.n, widths, args.reps, args.runs):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
