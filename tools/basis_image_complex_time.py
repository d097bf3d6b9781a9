"""sdpsr_basis_image_complex beside sdpsr_block_images_complex on one GPU, on the instances of
test_complex_path_beyond_one_workgroup and test_complex_path_largest_orders (tests/test_gpu_parity.py): Z_100, C[S3] (x)
{I, J - I} on 12, 64 and 560 points (n = 72, 384, 3360).  Everything device-resident.

Per instance, after blockDiagonalize(P; complex=true) on the ctx:
  (a) sdpsr_block_images_complex (the existing kernel, unchanged);
  (b) sdpsr_basis_image_complex on the same Q_hat and desymmetrized partition at full range under auto, outer and chunk;
  (c) the sweep over the 8 windows of class_window(d, 8, .) under auto: the sum of the windows' times;
  and max |(a) - (b)| over the output against 2e-12 n.  As a witness for where a difference comes from, both are also compared
  with Q_k^H (1[P == i] Q_k) formed by torch's complex128 matrix products on the device (blocked sums, another order again).

Every time is the best of --reps calls after a warm-up, between two device events on the library's stream (the ctx is put on
a stream of the tool's own with sdpsr_set_stream).  One JSON line per instance, then a table.

  python tools/basis_image_complex_time.py [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def instances(pr):
    from basis_image_complex_helpers import directed, s3_cayley_labels
    out = [("Z_100", directed(100))]
    for k, seed in [(12, 3), (64, 4), (560, 6)]:
        out.append((f"S3xK{k}", pr.kron_with_complete(s3_cayley_labels(), k, seed=seed)[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from __graft_entry__ import load_package
    pkg = load_package()
    Lm = pkg._lib
    stream = torch.cuda.Stream()
    rows = []
    for name, L in instances(pkg.problems):
        n = L.shape[0]
        res = {}
        with pkg.Context(seed=11) as ctx, pkg.Context(seed=12, basis_image_kernel="outer") as ctx_outer, \
                pkg.Context(seed=13, basis_image_kernel="chunk") as ctx_chunk:
            lib = ctx._lib
            for c in (ctx, ctx_outer, ctx_chunk):
                c.set_stream(stream.cuda_stream)
            P = pkg.Partition.from_matrix(L, ctx=ctx)
            lab = np.ascontiguousarray(np.asarray(P.matrix).ravel(order="F").astype(np.uint32))
            tL = torch.from_numpy(lab.view(np.int32).copy()).cuda()  # labels in, desymmetrized labels out, both on the device
            tP = torch.empty(n * n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dd, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
            for _ in range(4):  # the reference's randomized failures: try again
                st = lib.sdpsr_block_diagonalize_complex(ctx._h, n, C.c_void_p(tL.data_ptr()), P.nparts, 1e-8, C.c_void_p(tP.data_ptr()), C.byref(dd),
                                                         C.byref(nb), C.byref(ssq), C.byref(ss), Lm.MEM_DEVICE)
                if st not in (2, 3):
                    break
            ctx.check(st)
            d, S, S1 = dd.value, ssq.value, ss.value
            sizes = np.zeros(nb.value, dtype=np.int32)
            ctx.check(lib.sdpsr_block_sizes_complex(ctx._h, C.c_void_p(sizes.ctypes.data)))
            own = torch.empty(d * S, dtype=torch.complex128, device="cuda")
            q = torch.empty(n * S1, dtype=torch.complex128, device="cuda")
            new = torch.empty(d * S, dtype=torch.complex128, device="cuda")
            route = C.c_int32(0)

            def best(cx, call):
                t = []
                for _ in range(args.reps + 1):  # the first call is the warm-up: it allocates the ctx's buffers
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    cx.check(call())
                    e1.record(stream)
                    e1.synchronize()
                    t.append(e0.elapsed_time(e1))
                return min(t[1:])

            def entry(cx, out, first, count):
                return lambda: lib.sdpsr_basis_image_complex(cx._h, n, C.c_void_p(tP.data_ptr()), d, len(sizes), C.c_void_p(sizes.ctypes.data),
                                                             C.c_void_p(q.data_ptr()), first, count, -1.0, C.c_void_p(out.data_ptr()), C.byref(route),
                                                             None, Lm.MEM_DEVICE)
            ctx.check(lib.sdpsr_block_images_complex(ctx._h, C.c_void_p(own.data_ptr()), C.c_void_p(q.data_ptr()), Lm.MEM_DEVICE))
            res.update(instance=name, n=n, d=d, blocks=sorted(int(s) for s in sizes), bound=2e-12 * n, within_bound=True,
                       block_images_complex_ms=best(ctx, lambda: lib.sdpsr_block_images_complex(ctx._h, C.c_void_p(own.data_ptr()), None, Lm.MEM_DEVICE)))
            # the witness: torch's own complex128 products, class by class
            Qm = q.view(S1, n).t()  # n x S1 (q is column-major)
            Pm = tP.view(n, n).t()
            wit = torch.empty(d, S, dtype=torch.complex128, device="cuda")
            for i in range(d):
                MQ = (Pm == i + 1).to(torch.complex128) @ Qm
                c0 = off = 0
                for s_k in (int(v) for v in sizes):
                    blk = Qm[:, c0:c0 + s_k].conj().t() @ MQ[:, c0:c0 + s_k]
                    wit[i, off:off + s_k * s_k] = blk.t().reshape(-1)  # column-major
                    c0, off = c0 + s_k, off + s_k * s_k
            wit = wit.view(-1)
            res["old_vs_witness"] = float((own - wit).abs().max().item())
            for kernel, cx in (("auto", ctx), ("outer", ctx_outer), ("chunk", ctx_chunk)):
                res[f"basis_image_complex_{kernel}_ms"] = best(cx, entry(cx, new, 1, d))
                res[f"route_{kernel}"] = route.value
                diff = float((own - new).abs().max().item())
                res[f"max_diff_{kernel}"] = diff
                res[f"new_{kernel}_vs_witness"] = float((new - wit).abs().max().item())
                res["within_bound"] = res["within_bound"] and diff <= 2e-12 * n
            wins = [pkg.class_window(d, 8, j) for j in range(8)]
            slab = torch.empty(max(c for _, c in wins) * S, dtype=torch.complex128, device="cuda")
            per = [best(ctx, entry(ctx, slab, f, c)) if c else 0.0 for f, c in wins]
            res.update(window_ms=[round(x, 4) for x in per], windows_total_ms=sum(per))
        rows.append(res)
        print(json.dumps(res), flush=True)
    print("# times in ms, best of %d after a warm-up; device-resident arrays; routes: 4 = outer, 5 = chunk" % args.reps)
    print("# instance      n     d | block_images_complex | new auto (route) | new outer | new chunk | 8 windows, sum | old / new auto | max |diff| (bound)")
    for r in rows:
        print(f"# {r['instance']}: against torch's complex128 products: block_images_complex {r['old_vs_witness']:.2e}, new auto {r['new_auto_vs_witness']:.2e}, "
              f"outer {r['new_outer_vs_witness']:.2e}, chunk {r['new_chunk_vs_witness']:.2e}")
    for r in rows:
        a, b = r["block_images_complex_ms"], r["basis_image_complex_auto_ms"]
        note = "" if b <= a else "   <- the new entry is SLOWER here"
        md = max(r["max_diff_auto"], r["max_diff_outer"], r["max_diff_chunk"])
        print(f"{r['instance']:>10} {r['n']:5d} {r['d']:5d} | {a:20.4f} | {b:12.4f} ({r['route_auto']}) | {r['basis_image_complex_outer_ms']:9.4f} | "
              f"{r['basis_image_complex_chunk_ms']:9.4f} | {r['windows_total_ms']:14.4f} | {a / b:14.2f} | {md:.2e} ({r['bound']:.2e}){' OK' if r['within_bound'] else ' EXCEEDED'}{note}")


if __name__ == "__main__":
    main()
