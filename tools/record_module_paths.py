"""The module-path table of tests/test_gpu_module_paths.py: its rows, how one row is run, and the recorder that writes what a
given csrc computes for every row to tests/golden/module_paths.json.

Each row is one blockDiagonalize (retries=1) on a fresh Context(seed, eig_driver, flags): instance x seed x one flag, through the
module-compression driver (eig_driver = 6; the automatic selection for the order-1024 instance).  One more row per instance
that does not fail runs sdpsr_jordan_reduce from partition_as_sdp(L, seed=1): the path that leaves the driver without a host wait.
A row records the status (or the error code and its message), the block sizes in the order returned, the ctx's draw position
after the call, the host waits of the call and a CRC32 of the Q_hat bytes and of all blks bytes.

    python tools/record_module_paths.py --csrc-commit <commit whose csrc is built> [--out tests/golden/module_paths.json]

The file is recorded ONCE, from the csrc before a change to the driver, and then compared against (never regenerated from
the code under test).  A row whose CRCs did not reproduce between two recordings of that csrc carries its integer fields only."""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "module_paths.json")
SEEDS = (3, 4, 5)
FLAGS = ("0", "SMALL_EIGEN_ON_DEVICE", "ALWAYS_REORTHOGONALIZE", "SPMM_ONE_BY_ONE", "FRESH_IRREDUCIBLE_ELEMENT")
# name -> eig_driver (6: module compression forced, 0: the automatic selection, n >= 512)
INSTANCES = {"circ256": 6, "er7k8": 6, "K2": 6, "sym8k24": 6, "K17": 6, "nonsym24": 6, "jordan1024": 0}
FAILING = ("K17", "nonsym24")  # forced compression rejects K17: the fallback is an error under eig_driver = 6
INT_FIELDS = ("status", "sizes", "draws", "host_waits")


def instances(pr, golden):
    """name -> (labels uint32 n x n, dim): circ256 (commutative, the class sums are the module), er7k8 (n = 456, growth rounds,
    the small-host tail), K2 (n = 200, w = 6), sym8k24 (n = 192, w = 72 > 64: the device tail), K17 (n = 68, the module
    exceeds wmax: driver fallback), nonsym24 (not symmetric: the verdict behind the first Gram read-back), jordan1024."""
    nonsym = np.random.default_rng(11).integers(1, 4, size=(24, 24))  # test_nonsymmetric_partition_rejected_by_both_drivers
    inst = {"circ256": (golden["circ256_P"], int(golden["circ256_P"].max())),
            "er7k8": pr.kron_with_complete(golden["er7_P"], 8, seed=5),
            "K2": pr.known_blocks_instance("K2")[:2],
            "sym8k24": pr.kron_with_complete(pr.sym_full_labels(8), 24, seed=8),
            "K17": pr.known_blocks_instance("K17")[:2],
            "nonsym24": (nonsym, 3),
            "jordan1024": pr.synthetic_jordan_partition(1024, seed=4)}
    return {k: (np.asarray(L).astype(np.uint32), int(d)) for k, (L, d) in inst.items()}


def rows():
    """(id, instance, seed, flag, entry) of every row; entry: "bd" (blockDiagonalize) or "jr" (sdpsr_jordan_reduce)."""
    out = [(f"{name}-s{seed}-{flag}", name, seed, flag, "bd") for name in INSTANCES for seed in SEEDS for flag in FLAGS]
    out += [(f"{name}-s{SEEDS[0]}-0-jordan_reduce", name, SEEDS[0], "0", "jr") for name in INSTANCES if name not in FAILING]
    return out


def _crc(mats):
    crc = 0
    for m in mats:
        crc = zlib.crc32(np.asarray(m).tobytes(order="F"), crc)
    return crc


def _block_diagonalize(pkg, ctx, L, d):
    bd = pkg.blockDiagonalize(pkg.Partition(d, L), ctx=ctx, retries=1)
    return [int(s) for s in bd.blkSizes], _crc(bd.Q_hat), _crc(b for row in bd.blks for b in row)


def _jordan_reduce(pkg, ctx, L, d):
    """One raw sdpsr_jordan_reduce with room for the images (sum s_k^2 <= 2 dim(P)) and for Q_hat (sum s_k <= n)."""
    setup = pkg.admissible_setup(*pkg.problems.partition_as_sdp(L.astype(np.int64), seed=1))
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    if setup.hint:
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    P, blks, qh = np.zeros(n * n, dtype=np.uint32), np.zeros(2 * d * d), np.zeros(n * n)
    dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rtol = pkg.api.RTOL_DEFAULT
    ctx.check(ctx._lib.sdpsr_jordan_reduce(ctx._h, n, vp(CL), vp(X0L), vp(Uf), U.shape[1], rtol, rtol, vp(P), C.byref(dd), C.byref(it),
                                           C.byref(nb), C.byref(ssq), C.byref(ss), vp(blks), blks.size, vp(qh), qh.size, None,
                                           pkg._lib.MEM_HOST))
    assert dd.value == d and dd.value * ssq.value <= blks.size and n * ss.value <= qh.size
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, vp(sizes)))
    return [int(s) for s in sizes], _crc([qh[:n * ss.value]]), _crc([blks[:dd.value * ssq.value]])


def run_row(pkg, inst, row):
    """What the library computes for one row: a call that fails is a row too (its code and message)."""
    _, name, seed, flag, entry = row
    lib, prof = pkg._lib, pkg._lib.load_prof_library()
    L, d = inst[name]
    flags = 0 if flag == "0" else getattr(lib, "FLAG_" + flag)
    with pkg.Context(seed=seed, eig_driver=INSTANCES[name], flags=flags) as ctx:
        w0, w1, cnt = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 4)()
        ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w0)))
        try:
            sizes, crc_q, crc_b = (_block_diagonalize if entry == "bd" else _jordan_reduce)(pkg, ctx, L, d)
            rec = {"status": 0, "sizes": sizes, "crc32_qhat": crc_q, "crc32_blks": crc_b}
        except pkg.api.SdpsrError as e:
            rec = {"status": e.status, "message": str(e), "sizes": None}
        ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w1)))
        ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, cnt))
        rec.update(draws=int(cnt[0]), host_waits=int(w1.value - w0.value))
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
