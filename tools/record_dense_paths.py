"""The dense-path table of tests/test_gpu_dense_paths.py: its rows, how one row is run, and the recorder that writes what a
given csrc computes for every row to tests/golden/dense_paths.json.

Each row is one call on a fresh Context(seed, eig_driver=4, flags): the dense diagonalize driver (csrc/eigdec.cpp) and the
basis_image routes (csrc/blockdiag.cpp).  Four kinds of row:
  bd     blockDiagonalize (retries=0), instance x seed x one flag;
  route  blockDiagonalize on one basis_image route of tests/test_gpu_outputs.py ROUTES, on the first of its SEEDS that does not
         end in the randomized failure (the seed is a field of the row);
  retry  the raw sdpsr_block_diagonalize with d + 1 in place of d: the classes can never add up, both extra coupling elements are
         drawn, the irreducible step draws a fresh element, the call ends in DIMENSION_MISMATCH with the sizes and Q_hat stored;
  ed     six consecutive sdpsr_eigen_decomposition calls on one ctx (320 eigenspaces: the classes are formed on the device
         unless COUPLING_ON_HOST), and one sdpsr_eigen_decomposition_batched of three runs at n = 200 (the serial branch).
A row records the status (or the error code and its message), the block sizes in the order returned, the ctx's draw position
after the call, the host waits of the call and a CRC32 of the Q_hat bytes and of all blks bytes; an `ed` row records
(neig, nclasses) or the error of every call.

    python tools/record_dense_paths.py --csrc-commit <commit whose csrc is built> [--out tests/golden/dense_paths.json]

The file is recorded ONCE, from the csrc before a change to the drivers, and then compared against (never regenerated from
the code under test).  A row whose CRCs did not reproduce between two recordings of that csrc carries its integer fields only."""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_paths.json")
EIG_DRIVER = 4  # the dense driver, forced
SEEDS = (3, 4, 5)
FLAGS = ("0", "FRESH_IRREDUCIBLE_ELEMENT", "SINGLE_COUPLING_ELEMENT", "COUPLING_ON_HOST")
BD_INSTANCES = ("circ256", "er7k8", "K17", "K2", "DS", "nonsym24")
ROUTES = (("two_stage", {"basis_image_kernel": "two_stage"}), ("outer", {"basis_image_kernel": "outer"}),
          ("chunk", {"basis_image_kernel": "chunk"}), ("auto", {}), ("auto_full", {"flags": 1 << 10}))  # test_gpu_outputs.ROUTES
ROUTE_SEEDS = (101, 102, 103)  # test_gpu_outputs.SEEDS
ROUTE_INSTANCES = ("K17", "K2", "K40", "DS")
RETRY_INSTANCES = ("er7k8", "K17")
ED_FLAGS = ("0", "COUPLING_ON_HOST")
ED_SEED, ED_CALLS, BATCH_COUNT = 77, 6, 3
INT_FIELDS = ("status", "sizes", "draws", "host_waits")
RETRYABLE = (2, 3)  # NUMERICAL_INCONSISTENCY, DIMENSION_MISMATCH: the reference's "try again"


def instances(pr, golden):
    """name -> (labels uint32 n x n, dim): circ256 (commutative), er7k8 (n = 456), K17 (n = 68: blocks of 17, eigenspaces of
    dimension > 1, merged classes), K2 (n = 200), K40 (n = 120), DS (n = 76, blocks of different sizes), nonsym24 (the
    not-symmetric verdict), generic320 (no symmetry: 320 eigenspaces)."""
    nonsym = np.random.default_rng(11).integers(1, 4, size=(24, 24))  # test_nonsymmetric_partition_rejected_by_both_drivers
    n = 320  # test_generic_partition_failure_rate_matches_the_oracle
    iu = np.triu_indices(n)
    G = np.zeros((n, n), dtype=np.int64)
    G[iu] = np.arange(1, len(iu[0]) + 1)
    G = np.maximum(G, G.T)
    inst = {"circ256": (golden["circ256_P"], int(golden["circ256_P"].max())),
            "er7k8": pr.kron_with_complete(golden["er7_P"], 8, seed=5),
            "K17": pr.known_blocks_instance("K17")[:2],
            "K2": pr.known_blocks_instance("K2")[:2],
            "K40": pr.known_blocks_instance("K40")[:2],
            "DS": pr.known_blocks_instance("DS")[:2],
            "nonsym24": (nonsym, 3),
            "generic320": pr.canonical_labels(G)}
    return {k: (np.asarray(L).astype(np.uint32), int(d)) for k, (L, d) in inst.items()}


def rows():
    """(id, kind, instance, seeds, flag, ctx keywords) of every row."""
    out = [(f"bd-{name}-s{seed}-{flag}", "bd", name, (seed,), flag, {}) for name in BD_INSTANCES for seed in SEEDS for flag in FLAGS]
    out += [(f"route-{name}-{route}", "route", name, ROUTE_SEEDS, "0", kw) for name in ROUTE_INSTANCES for route, kw in ROUTES]
    out += [(f"retry-{name}-s{seed}", "retry", name, (seed,), "0", {}) for name in RETRY_INSTANCES for seed in SEEDS]
    out += [(f"ed-generic320-{flag}", "ed", "generic320", (ED_SEED,), flag, {}) for flag in ED_FLAGS]
    out += [("ed-K2-batched", "edb", "K2", (ED_SEED,), "0", {})]
    return out


def _crc(mats):
    crc = 0
    for m in mats:
        crc = zlib.crc32(np.asarray(m).tobytes(order="F"), crc)
    return crc


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _block_diagonalize(pkg, ctx, L, d):
    bd = pkg.blockDiagonalize(pkg.Partition(d, L), ctx=ctx, retries=0)
    return {"status": 0, "sizes": [int(s) for s in bd.blkSizes], "crc32_qhat": _crc(bd.Q_hat),
            "crc32_blks": _crc(b for row in bd.blks for b in row)}


def _retry(pkg, ctx, L, d):
    """sdpsr_block_diagonalize with d + 1: the library uses d for the eligibility of the compression driver (off under
    eig_driver = 4), as the dimension the classes should add up to, and in the final check -- never to index a class."""
    n = L.shape[0]
    lab = np.ascontiguousarray(L.ravel(order="F"))
    nb, ssq, ss = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    st = ctx._lib.sdpsr_block_diagonalize(ctx._h, n, _vp(lab), d + 1, pkg.api.RTOL_DEFAULT, C.byref(nb), C.byref(ssq), C.byref(ss),
                                          None, pkg._lib.MEM_HOST)
    msg = ctx._lib.sdpsr_last_error(ctx._h).decode()
    if st != 3:  # anything but DIMENSION_MISMATCH leaves nothing stored
        return {"status": st, "message": msg, "sizes": None}
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, _vp(sizes)))
    qh = np.zeros(n * ss.value)
    ctx.check(ctx._lib.sdpsr_q_hat(ctx._h, _vp(qh), pkg._lib.MEM_HOST))
    return {"status": st, "message": msg, "sizes": [int(s) for s in sizes], "crc32_qhat": _crc([qh])}


def _eigen_decompositions(pkg, ctx, L, d):
    calls = []
    for _ in range(ED_CALLS):
        try:
            calls.append(list(pkg.eigen_decomposition(pkg.Partition(d, L), ctx=ctx)))
        except pkg.api.SdpsrError as e:
            calls.append({"status": e.status, "message": str(e)})
    return {"status": 0, "sizes": None, "calls": calls}


def _eigen_decomposition_batched(pkg, ctx, L, d):
    n = L.shape[0]
    lab = np.ascontiguousarray(L.ravel(order="F"))
    st, ne, nc = (np.zeros(BATCH_COUNT, dtype=np.int32) for _ in range(3))
    rc = ctx._lib.sdpsr_eigen_decomposition_batched(ctx._h, n, _vp(lab), d, 1e-12 * n, BATCH_COUNT, None, _vp(st), _vp(ne), _vp(nc),
                                                    pkg._lib.MEM_HOST)
    return {"status": rc, "message": ctx._lib.sdpsr_last_error(ctx._h).decode(), "sizes": None,
            "calls": [[int(a), int(b), int(c)] for a, b, c in zip(st, ne, nc)]}


_ENTRY = {"bd": _block_diagonalize, "route": _block_diagonalize, "retry": _retry, "ed": _eigen_decompositions,
          "edb": _eigen_decomposition_batched}


def run_row(pkg, inst, row):
    """What the library computes for one row: a call that fails is a row too (its code and message).  A `route` row moves on
    to its next seed after a retryable failure, as test_gpu_outputs does, and records the seed it ended on."""
    _, kind, name, seeds, flag, kw = row
    lib, prof = pkg._lib, pkg._lib.load_prof_library()
    L, d = inst[name]
    kw = dict(kw)
    flags = kw.pop("flags", 0) | (0 if flag == "0" else getattr(lib, "FLAG_" + flag))
    for seed in seeds:
        with pkg.Context(seed=seed, eig_driver=EIG_DRIVER, flags=flags, **kw) as ctx:
            w0, w1, cnt = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 4)()
            ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w0)))
            try:
                rec = _ENTRY[kind](pkg, ctx, L, d)
            except pkg.api.SdpsrError as e:
                rec = {"status": e.status, "message": str(e), "sizes": None}
            ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w1)))
            ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, cnt))
            rec.update(draws=int(cnt[0]), host_waits=int(w1.value - w0.value))
        if kind == "route":
            rec["seed"] = seed
        if not (kind == "route" and rec["status"] in RETRYABLE):
            break
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--csrc-commit", required=True, help="the commit whose csrc the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--only", default="", help="record only the rows whose id starts with this")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    inst = instances(pkg.problems, np.load(os.path.join(ROOT, "tests", "golden", "golden_partitions.npz")))
    table = {row[0]: run_row(pkg, inst, row) for row in rows() if row[0].startswith(args.only)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"csrc_commit": args.csrc_commit, "rows": table}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} rows recorded to {args.out}")


if __name__ == "__main__":
    main()
