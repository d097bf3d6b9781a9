"""The agreement of R restarts on one GPU (sdpsr_meet_keys, sdpsr_agree_partitions) against the route that existed before
(parallel.agree_partitions over torch.distributed): N = 4096, R = 4, device-resident labels, label widths 32 and 16.

  keys     sdpsr_meet_keys alone: us and TB/s of its (R * B / 8 + 8) * n^2 bytes;
  agree    sdpsr_agree_partitions (comm = NULL) on four equal partitions (checksums only) and with one restart coarsened
           (checksums, key pass, relabel, delivery into the four arrays);
  old      parallel.agree_partitions for the same two cases in a one-rank `nccl` process group, with the device checksum
           (partition_checksum) and relabel_keys as its callbacks -- in a process of its own (this script with --old-route).

Best of --reps calls after a warm-up; device events on the stream the library works on around each call, and the host wall
time of the call.  One JSON line per row.

  python tools/agree_time.py [--n 4096] [--restarts 4] [--widths 32,16] [--reps 5]
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

DTYPES = {8: np.uint8, 16: np.uint16, 32: np.uint32}


def instance(pkg, n):
    """(fine, coarse) flat column-major labels: the synthetic Jordan partition of bench.py and the same with its last class merged
    into the first (still canonical: the labels 1 .. d - 1 keep their first occurrences)."""
    L, d = pkg.problems.synthetic_jordan_partition(n, seed=1)
    fine = np.ascontiguousarray(L.ravel(order="F")).astype(np.int64)
    coarse = fine.copy()
    coarse[coarse == d] = 1
    return fine, coarse, int(d)


def timed(stream, reps, call, before=None):
    import torch
    best_dev = best_wall = None
    for rep in range(reps + 1):  # the first call is the warm-up: it allocates the ctx's buffers
        if before:
            before()
            stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        wall = time.perf_counter() - t
        dev = e0.elapsed_time(e1) * 1e-3
        if rep:
            best_dev = dev if best_dev is None else min(best_dev, dev)
            best_wall = wall if best_wall is None else min(best_wall, wall)
    return best_dev, best_wall


def to_device(a, bits):
    import torch
    return torch.from_numpy(a.astype(DTYPES[bits]).view(np.uint8)).cuda()


def new_route(pkg, n, R, widths, reps):
    import torch
    fine, coarse, d = instance(pkg, n)
    len_ = n * n
    for bits in widths:
        with pkg.Context(seed=1, label_width=bits) as ctx:
            lib = ctx._lib
            stream = torch.cuda.Stream()
            ctx.set_stream(stream.cuda_stream)
            tf, tc = to_device(fine, bits), to_device(coarse, bits)
            arrs = [tf.clone() for _ in range(R)]
            keys = torch.empty(len_, dtype=torch.int64, device="cuda")
            ptrs = (C.c_void_p * R)(*[t.data_ptr() for t in arrs])
            torch.cuda.synchronize()
            dev, wall = timed(stream, reps, lambda: ctx.check(lib.sdpsr_meet_keys(ctx._h, R, C.cast(ptrs, C.c_void_p), None, len_, 0,
                                                                                   C.c_void_p(keys.data_ptr()), 1)))
            moved = (R * bits // 8 + 8) * len_
            yield {"keys": "sdpsr_meet_keys", "bits": bits, "R": R, "N": n, "device_us": round(dev * 1e6, 1), "call_wall_us": round(wall * 1e6, 1),
                   "bytes_moved": moved, "TB_per_s": round(moved / dev / 1e12, 3)}
            dim, met = C.c_int64(0), C.c_int32(-1)

            def agree():
                ctx.check(lib.sdpsr_agree_partitions(ctx._h, None, R, C.cast(ptrs, C.c_void_p), None, len_, C.byref(dim), C.byref(met), 1))

            dev, wall = timed(stream, reps, agree)
            yield {"agree": "sdpsr_agree_partitions", "case": "agreeing", "bits": bits, "R": R, "N": n, "met": met.value,
                   "device_us": round(dev * 1e6, 1), "call_wall_us": round(wall * 1e6, 1)}

            def coarsen():
                with torch.cuda.stream(stream):
                    arrs[R - 1].copy_(tc)

            dev, wall = timed(stream, reps, agree, before=coarsen)
            ok = all(bool((t == tf).all()) for t in arrs)
            yield {"agree": "sdpsr_agree_partitions", "case": "one_coarsened", "bits": bits, "R": R, "N": n, "met": met.value, "dim": dim.value,
                   "dim_expected": d, "all_arrays_fine": ok, "device_us": round(dev * 1e6, 1), "call_wall_us": round(wall * 1e6, 1)}


def old_route(pkg, n, R, bits, reps):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29573", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", device_id=dev)
    fine, coarse, d = instance(pkg, n)
    tdt = {32: torch.int32, 16: getattr(torch, "uint16", torch.int16)}[bits]
    with pkg.Context(seed=1, label_width=bits) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        tf, tc = to_device(fine, bits).view(tdt), to_device(coarse, bits).view(tdt)
        torch.cuda.synchronize()
        for case, last in (("agreeing", tf), ("one_coarsened", tc)):
            arrs = [tf] * (R - 1) + [last]
            res = [None]

            def call():
                with torch.cuda.stream(stream):
                    res[0] = pkg.parallel.agree_partitions(arrs, lambda sig: pkg.relabel_keys(sig, ctx=ctx),
                                                           checksum=lambda t: pkg.partition_checksum(t, ctx=ctx))

            dev_s, wall = timed(stream, reps, call)
            agreed, lab = res[0]
            ok = bool((lab.view(torch.uint8) == tf.view(torch.uint8)).all())
            print(json.dumps({"old": "parallel.agree_partitions (nccl, one rank)", "case": case, "bits": bits, "R": R, "N": n,
                              "met": int(not agreed), "result_fine": ok, "device_us": round(dev_s * 1e6, 1),
                              "call_wall_us": round(wall * 1e6, 1)}), flush=True)
    torch.cuda.synchronize()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--restarts", type=int, default=4)
    ap.add_argument("--widths", default="32,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-route", type=int, default=0, help="(internal) run the old route at this width in this process")
    args = ap.parse_args()
    pkg = load_package()
    if args.old_route:
        old_route(pkg, args.n, args.restarts, args.old_route, args.reps)
        return 0
    widths = [int(x) for x in args.widths.split(",") if x]
    for row in new_route(pkg, args.n, args.restarts, widths, args.reps):
        print(json.dumps(row), flush=True)
    env = dict(os.environ, NCCL_SOCKET_IFNAME="lo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    rc = 0
    for bits in widths:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--old-route", str(bits), "--n", str(args.n), "--restarts",
                              str(args.restarts), "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=600)
        sys.stdout.write(out.stdout)
        if out.returncode != 0:
            print(json.dumps({"old": "parallel.agree_partitions", "bits": bits, "failed": out.stderr[-800:]}), flush=True)
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
