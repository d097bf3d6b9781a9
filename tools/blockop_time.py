"""sdpsr_blockop_* and sdpsr_blocks_syev on one GPU, everything device-resident: the reduced PSD pencil Z(x), its adjoint and
the block spectra beside the route a caller had before them (torch on the same device arrays).

  closed_scheme  bench.py's closed_scheme instance (N = 4096, d = 34, every block 1 x 1)
  theta_er7xk72  bench.py's theta instance (N = 4104, d = 36, blocks 2 and 3)
  config2        configs[2] (QAP, N = 900, dim 27 828, blocks up to 81), triplets from basis_image_sparse(parts=8)

Per instance: create (the whole call, its two host waits included), apply, adjoint and blocks_syev, each the best of --reps
calls after a warm-up with device events on the ctx's stream around the call; the bytes apply / adjoint move (16 per full
entry, the gathered vector once, the output twice: memset and stores) over their time, against the 3.0-3.3 TB/s of
sdpsr_labels_convert (profiles/r08_label_width.txt); the torch route -- index_add_ into a zero tensor for apply,
gather-multiply-index_add_ for the adjoint (atomics: not reproducible bit for bit), torch.linalg.eigvalsh per block for the
spectra -- and the largest difference between the two.  One JSON line per instance; a loss is reported as a loss.

  python tools/blockop_time.py [--instances closed_scheme,theta_er7xk72,config2] [--reps 5]
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


def full_list(sp):
    """(class, position, value) of the full entry list as device tensors: what the torch route indexes with."""
    import torch
    dev = sp.val.device
    sz = torch.tensor(sp.sizes, dtype=torch.int64, device=dev)
    pre = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sz * sz, 0)])
    b, r, c = (a.to(torch.int64) - sp.index_base for a in (sp.blk, sp.row, sp.col))
    cls = sp.cls.to(torch.int64) - sp.index_base
    pos, mpos = pre[b] + r + c * sz[b], pre[b] + c + r * sz[b]
    if not sp.upper:
        return cls, pos, sp.val
    off = r != c
    return torch.cat([cls, cls[off]]), torch.cat([pos, mpos[off]]), torch.cat([sp.val, sp.val[off]])


def measure(pkg, ctx, stream, name, sp, reps):
    import torch
    lib = ctx._lib
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    made = []

    def create():
        made.append(pkg.BlockOperator(sp, ctx=ctx))
        if len(made) > 1:
            made.pop(0).close()

    t_create = timed(stream, reps, create)
    op = made[-1]
    d, S, nf = op.d, op.sum_sq, op.nnz_full
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(d, dtype=torch.float64, device="cuda", generator=g)
    Sm = torch.randn(S, dtype=torch.float64, device="cuda", generator=g)
    Z, gr = torch.empty(S, dtype=torch.float64, device="cuda"), torch.empty(d, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t_apply = timed(stream, reps, lambda: ctx.check(lib.sdpsr_blockop_apply(ctx._h, op._h, vp(x), vp(Z), pkg._lib.MEM_DEVICE)))
    t_adj = timed(stream, reps, lambda: ctx.check(lib.sdpsr_blockop_adjoint(ctx._h, op._h, vp(Sm), vp(gr), pkg._lib.MEM_DEVICE)))
    sz = np.asarray(op.sizes, dtype=np.int32)
    w = torch.empty(int(sz.sum()), dtype=torch.float64, device="cuda")
    t_syev = timed(stream, reps, lambda: ctx.check(lib.sdpsr_blocks_syev(ctx._h, len(sz), C.c_void_p(sz.ctypes.data), vp(Z), vp(w), None,
                                                                         pkg._lib.MEM_DEVICE)))
    # the torch route on the same device arrays
    cls, pos, val = full_list(sp)
    cur = torch.cuda.current_stream()
    out = {}

    def t_apply_route():
        out["Z"] = torch.zeros(S, dtype=torch.float64, device="cuda").index_add_(0, pos, x[cls] * val)

    def t_adjoint_route():
        out["g"] = torch.zeros(d, dtype=torch.float64, device="cuda").index_add_(0, cls, val * Sm[pos])

    def t_eig_route():
        ws, off = [], 0
        for s in op.sizes:
            ws.append(torch.linalg.eigvalsh(Z[off:off + s * s].view(s, s), UPLO="U"))  # (column-major lower = row-major upper)
            off += s * s
        out["w"] = torch.cat(ws)

    tt_apply, tt_adj, tt_eig = timed(cur, reps, t_apply_route), timed(cur, reps, t_adjoint_route), timed(cur, max(1, reps // 2), t_eig_route)
    moved_apply, moved_adj = nf * 16 + d * 8 + 2 * S * 8, nf * 16 + S * 8 + 2 * d * 8
    op.close()
    return {"instance": name, "d": d, "blocks": len(op.sizes), "largest_block": int(max(op.sizes)), "sum_sq": S, "nnz": int(sp.nnz), "nnz_full": nf,
            "handle_MB": round(nf * 32 / 1e6, 2), "create_ms": round(t_create * 1e3, 3), "apply_us": round(t_apply * 1e6, 1),
            "adjoint_us": round(t_adj * 1e6, 1), "blocks_syev_us": round(t_syev * 1e6, 1),
            "apply_TB_per_s": round(moved_apply / t_apply / 1e12, 3), "adjoint_TB_per_s": round(moved_adj / t_adj / 1e12, 3),
            "torch_apply_us": round(tt_apply * 1e6, 1), "torch_adjoint_us": round(tt_adj * 1e6, 1), "torch_eigvalsh_us": round(tt_eig * 1e6, 1),
            "apply_speedup": round(tt_apply / t_apply, 2), "adjoint_speedup": round(tt_adj / t_adj, 2), "syev_speedup": round(tt_eig / t_syev, 2),
            "max_abs_diff_apply": float((out["Z"] - Z).abs().max()) if S else 0.0, "max_abs_diff_adjoint": float((out["g"] - gr).abs().max()) if d else 0.0,
            "max_abs_diff_eigenvalues": float((out["w"] - w).abs().max())}


def triplets(pkg, ctx, name):
    """SparseBlocks on the device for one instance."""
    import torch
    pr, Lm, lib = pkg.problems, pkg._lib, ctx._lib
    if name != "config2":
        golden = np.load(os.path.join(ROOT, "tests", "golden", "golden_partitions.npz"))
        _, _, _, L, d, _, _ = pr.bench_instance(name, golden["er7_P"])
        P = pkg.Partition(d, np.asarray(L).astype(np.uint32))
        bd = pkg.blockDiagonalize(P, ctx=ctx, retries=4)
        Pt = pkg.Partition(P.nparts, torch.from_numpy(np.ascontiguousarray(np.asarray(P.matrix)).astype(np.int32)).cuda())
        return pkg.basis_image_sparse(bd.Q_hat, Pt, ctx=ctx)
    # configs[2]: Q-hat alone, on the device -- its dense images (12 GB) are never formed at once, let alone brought to the host
    flow, dist = pr.grid_qap_instance(5, 6, seed=4)
    P = pkg.admissible_subspace(*pr.qap_problem(flow, dist), ctx=ctx)
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
    Pt = pkg.Partition(d, tP.view(n, n).t())
    return pkg.basis_image_sparse((q.view(ss.value, n).t(), sizes), Pt, parts=8, ctx=ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", default="closed_scheme,theta_er7xk72,config2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("blockop_time.py measures on the GPU: none is visible")
    torch.cuda.init()
    pkg = load_package()
    with pkg.Context(seed=1) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)  # the events are recorded on the stream the library works on
        for name in args.instances.split(","):
            sp = triplets(pkg, ctx, name)
            print(json.dumps(measure(pkg, ctx, stream, name, sp, args.reps)), flush=True)


if __name__ == "__main__":
    main()
