"""sdpsr_block_images_sparse on one GPU, everything device-resident: the compaction of dense block images into solver
triplets beside the route a caller had before it (torch.nonzero on the device plus index arithmetic).

  synthetic      a 1 GiB real window (blocks 128, 64, 32, 1; 6241 classes) at densities 1 %, 25 % and 100 %, upper and full
  closed_scheme  the block images of bench.py's closed_scheme instance (N = 4096, d = 34)
  config2        configs[2] (QAP, N = 900, dim 27 828, blocks up to 81) in the 8 slabs of class_window(27828, 8, .): every slab
                 made by sdpsr_basis_image on the device, compacted there; the measured density of its images

Per row: the filling call (capacity = nnz: both sweeps, the scan, the read-back of nnz and the stores) and the sizing call
(capacity 0), each the best of --reps calls after a warm-up, device events on the ctx's stream around the call; the bytes the
filling call reads and writes (the window twice, 20 bytes per entry, classptr) over its time; the torch route's time and peak
temporary memory on the same input, and whether both give the same entries; the D2H bytes of the dense slab beside those of
the triplets.  The yardstick for a pass of this kind is sdpsr_labels_convert's 3.0-3.3 TB/s (profiles/r08_label_width.txt).
One JSON line per row.

  python tools/block_images_sparse_time.py [--instances synthetic,closed_scheme,config2] [--reps 5] [--gib 1.0]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


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


def torch_route(flat, sizes, upper, tol):
    """What a caller wrote before the entry existed: nonzero on the device, then index arithmetic on the int64 positions."""
    import torch
    dev = flat.device
    sz = torch.tensor(sizes, dtype=torch.int64, device=dev)
    pre = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sz * sz, 0)])
    S = int(pre[-1])
    idx = torch.nonzero(~(flat.abs() <= tol)).squeeze(1)
    cls = idx // S
    r = idx - cls * S
    k = torch.searchsorted(pre, r, right=True) - 1
    o = r - pre[k]
    s = sz[k]
    col = o // s
    row = o - col * s
    if upper:
        keep = row <= col
        idx, cls, k, row, col = idx[keep], cls[keep], k[keep], row[keep], col[keep]
    classptr = torch.searchsorted(cls, torch.arange(flat.numel() // S + 1, dtype=torch.int64, device=dev))
    return classptr, k.to(torch.int32), row.to(torch.int32), col.to(torch.int32), flat[idx]


def measure(pkg, ctx, stream, name, flat, sizes, upper, reps, torch_reps):
    """One row: the window `flat` (a device tensor of float64) through the entry and through the torch route."""
    import torch
    lib, Lm = ctx._lib, pkg._lib
    sz = np.asarray(sizes, dtype=np.int32)
    S = int(sum(int(s) ** 2 for s in sizes))
    count = flat.numel() // S
    classptr = torch.empty(count + 1, dtype=torch.int64, device=flat.device)
    nnz = C.c_int64(0)
    tri = Lm.TRI_UPPER if upper else Lm.TRI_FULL
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(cap, arrs):
        ctx.check(lib.sdpsr_block_images_sparse(ctx._h, len(sz), C.c_void_p(sz.ctypes.data), count, vp(flat), 0, tri, 0.0, 0, cap, vp(classptr),
                                                vp(arrs[0]), vp(arrs[1]), vp(arrs[2]), vp(arrs[3]), C.byref(nnz), None, Lm.MEM_DEVICE))

    torch.cuda.synchronize()
    t_size = timed(stream, reps, lambda: call(0, [None] * 4))
    m = nnz.value
    arrs = [torch.empty(m, dtype=torch.int32, device=flat.device) for _ in range(3)] + [torch.empty(m, dtype=torch.float64, device=flat.device)]
    t_fill = timed(stream, reps, lambda: call(m, arrs))
    window = flat.numel() * 8
    moved = 2 * window + m * 20 + (count + 1) * 8
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    cur = torch.cuda.current_stream()
    ref = [None]

    def route():
        ref[0] = None
        ref[0] = torch_route(flat, sizes, upper, 0.0)

    t_torch = timed(cur, torch_reps, route)
    peak = torch.cuda.max_memory_allocated() - base
    same = bool(torch.equal(ref[0][0], classptr) and all(torch.equal(a, b) for a, b in zip(ref[0][1:4], arrs[:3])) and
                torch.equal(ref[0][4].view(torch.int64), arrs[3].view(torch.int64)))
    ref[0] = None
    virtual = count * S
    scanned = virtual if not upper else count * sum(int(s) * (int(s) + 1) // 2 for s in sizes)
    return {"instance": name, "triangle": "upper" if upper else "full", "classes": count, "sum_sq": S, "window_MB": round(window / 1e6, 2), "nnz": m,
            "density_of_scanned_positions": round(m / scanned, 6) if scanned else 0.0, "sizing_call_us": round(t_size * 1e6, 1),
            "filling_call_us": round(t_fill * 1e6, 1), "bytes_moved": moved, "TB_per_s": round(moved / t_fill / 1e12, 3),
            "window_read_once_TB_per_s_sizing": round(window / t_size / 1e12, 3), "torch_route_us": round(t_torch * 1e6, 1),
            "torch_route_peak_temporary_MB": round(peak / 1e6, 1), "entry_workspace_MB": round((virtual + 2047) // 2048 * 12 / 1e6, 3),
            "equal_to_torch_route": same, "d2h_dense_MB": round(window / 1e6, 2), "d2h_triplets_MB": round((m * 20 + (count + 1) * 8) / 1e6, 2)}


def config2_inputs(pkg, ctx):
    """(labels tensor, n, d, sizes, Q_hat tensor) of configs[2], block-diagonalized on ctx."""
    import torch
    pr, Lm, lib = pkg.problems, pkg._lib, ctx._lib
    flow, dist = pr.grid_qap_instance(5, 6, seed=4)
    Cv, A, b = pr.qap_problem(flow, dist)
    P = pkg.admissible_subspace(Cv, A, b, ctx=ctx)
    n, d = P.shape[0], P.nparts
    tP = torch.from_numpy(np.ascontiguousarray(np.asarray(P.matrix).ravel(order="F").astype(np.uint32)).view(np.int32)).cuda()
    torch.cuda.synchronize()
    nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    for seed in range(1, 6):  # the reference's randomized failures: the next seed
        ctx.set_seed(seed)
        st = lib.sdpsr_block_diagonalize(ctx._h, n, C.c_void_p(tP.data_ptr()), d, 1e-8, C.byref(nb), C.byref(ssq), C.byref(ss), None, Lm.MEM_DEVICE)
        if st not in (2, 3):
            break
    ctx.check(st)
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(lib.sdpsr_block_sizes(ctx._h, C.c_void_p(sizes.ctypes.data)))
    q = torch.empty(n * ss.value, dtype=torch.float64, device="cuda")
    ctx.check(lib.sdpsr_q_hat(ctx._h, C.c_void_p(q.data_ptr()), Lm.MEM_DEVICE))
    return tP, n, d, sizes, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", default="synthetic,closed_scheme,config2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gib", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("block_images_sparse_time.py measures on the GPU: none is visible")
    torch.cuda.init()
    pkg = load_package()
    Lm = pkg._lib
    names = args.instances.split(",")
    with pkg.Context(seed=1) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)  # the events are recorded on the stream the library works on
        if "synthetic" in names:
            sizes = [128, 64, 32, 1]
            S = sum(s * s for s in sizes)
            count = int(args.gib * 2 ** 30 / 8) // S
            g = torch.Generator(device="cuda").manual_seed(1)
            for density in (0.01, 0.25, 1.0):
                flat = torch.randn(count * S, dtype=torch.float64, device="cuda", generator=g)
                if density < 1.0:
                    flat *= torch.rand(count * S, device="cuda", generator=g) < density
                for upper in (True, False):
                    row = measure(pkg, ctx, stream, f"synthetic {args.gib:g} GiB, density {density:g}", flat, sizes, upper, args.reps, 2)
                    print(json.dumps(row), flush=True)
                del flat
                torch.cuda.empty_cache()
        if "closed_scheme" in names:
            L, d = pkg.problems.synthetic_jordan_partition(4096, seed=1)
            bd = pkg.blockDiagonalize(pkg.Partition(d, np.asarray(L).astype(np.uint32)), ctx=ctx, retries=4)
            flat = torch.from_numpy(np.concatenate([b.ravel(order="F") for r in bd.blks for b in r])).cuda()
            for upper in (True, False):
                print(json.dumps(measure(pkg, ctx, stream, "closed_scheme N = 4096", flat, bd.blkSizes, upper, args.reps, 2)), flush=True)
        if "config2" in names:
            tP, n, d, sizes, q = config2_inputs(pkg, ctx)
            S = int(sum(int(s) ** 2 for s in sizes))
            wins = [pkg.class_window(d, 8, j) for j in range(8)]
            slab = torch.empty(max(c for _, c in wins) * S, dtype=torch.float64, device="cuda")
            route = C.c_int32(0)
            for j, (first, cnt) in enumerate(wins):
                ctx.check(ctx._lib.sdpsr_basis_image(ctx._h, n, C.c_void_p(tP.data_ptr()), d, len(sizes), C.c_void_p(sizes.ctypes.data), C.c_void_p(q.data_ptr()),
                                                     first, cnt, -1.0, C.c_void_p(slab.data_ptr()), C.byref(route), None, Lm.MEM_DEVICE))
                for upper in (True, False):
                    row = measure(pkg, ctx, stream, f"configs[2] slab {j} of 8 (classes {first}..{first + cnt - 1})", slab[:cnt * S], [int(s) for s in sizes],
                                  upper, args.reps, 1)
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
