"""The loop-path table of tests/test_gpu_loop_contract.py: its rows, how one row is run, and the recorder that writes what a
given csrc computes for every row to tests/golden/loop_paths.json.

Each row is one seeded sdpsr_admissible_subspace call from host arrays on a fresh ctx: instance x square mode x one flag x
hint (the setup's own, or 0: the full-matrix initial partition and the probe pass) x channels (int8 only).  Two more rows
run behind a closed call on the same ctx: the confirmed and the wrong speculation.  A row records dim, iterations, the
dimension trajectory, the loop's draws / squares / speculative squares, its host waits and a CRC32 of the label bytes.

    python tools/record_loop_paths.py --csrc-commit <commit whose csrc is built> [--out tests/golden/loop_paths.json]

The file is recorded ONCE, from the csrc before a change to the loop, and then compared against (never regenerated from
the code under test)."""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_paths.json")
SEED, PRIME_SEED = 7, 100
INSTANCES = ("closed", "open", "other")
MODES = ("i8", "f32", "f64")
I8_FLAGS = ("0", "SEPARATE_REFINEMENTS", "UNPACK_EVERY_STEP", "NO_VERIFY_SHORTCUT", "ALWAYS_PROJECT", "WAIT_FOR_EVERY_VERDICT")
FLOAT_FLAGS = ("0", "SEPARATE_REFINEMENTS")
I8_CHANNELS = (0, 1, 3)  # 3: the int8 path that does not keep the labels packed


def instances(pkg, golden):
    """closed (N = 256), open (N = 256, trajectory 6, 10, 18, 18), other (N = 57: ld = 128 with a ragged tile)."""
    pr = pkg.problems
    closed = pkg.admissible_setup(*pr.partition_as_sdp(golden["circ256_P"].astype(np.int64), seed=1))
    Cv, A, b = pr.theta_prime_product_problem(pr.cycle_adjacency(16), pr.symmetric_circulant_labels(16), 16, seed=1)[:3]
    other = pkg.admissible_setup(*pr.partition_as_sdp(golden["er7_P"].astype(np.int64), seed=1))
    return {"closed": closed, "open": pkg.admissible_setup(Cv, A, b), "other": other}


def rows():
    """(id, instance, mode, flag, own_hint, channels, primed) of every row; primed: a closed call runs first on the ctx."""
    out = []
    for name in INSTANCES:
        for mode in MODES:
            for flag in (I8_FLAGS if mode == "i8" else FLOAT_FLAGS):
                for own_hint in (True, False):
                    for ch in (I8_CHANNELS if mode == "i8" else (0,)):
                        out.append((f"{name}-{mode}-{flag}-{'own' if own_hint else 'nohint'}-ch{ch}", name, mode, flag, own_hint, ch, False))
    for name in ("closed", "open"):
        out.append((f"{name}-i8-0-own-ch0-after_closed", name, "i8", "0", True, 0, True))
    return out


def _call(pkg, ctx, setup, hint, seed):
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    prof = pkg._lib.load_prof_library()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ctx.set_seed(seed)
    if hint:
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, hint)
    c0, c1, w0, w1 = (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), C.c_uint64(0), C.c_uint64(0)
    ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, c0))
    ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w0)))
    P = np.zeros(n * n, dtype=np.uint32)
    d, it = C.c_int64(0), C.c_int32(0)
    ctx.check(ctx._lib.sdpsr_admissible_subspace(ctx._h, n, vp(CL), vp(X0L), vp(Uf), U.shape[1], pkg.api.RTOL_DEFAULT, vp(P),
                                                 C.byref(d), C.byref(it), None, pkg._lib.MEM_HOST))
    ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w1)))
    ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, c1))
    return {"dim": d.value, "iterations": it.value, "traj": ctx.dimension_trajectory(), "draws": int(c1[0]),
            "squares": int(c1[1] - c0[1]), "spec": int(c1[2] - c0[2]), "host_waits": int(w1.value - w0.value),
            "crc32": zlib.crc32(P.tobytes())}


def run_row(pkg, inst, row):
    """What the library computes for one row, or None if it rejects the combination."""
    _, name, mode, flag, own_hint, ch, primed = row
    lib = pkg._lib
    flags = 0 if flag == "0" else getattr(lib, "FLAG_" + flag)
    try:
        with pkg.Context(seed=1, square_mode=getattr(lib, "SQUARE_" + mode.upper()), channels=ch, flags=flags) as ctx:
            if primed:
                _call(pkg, ctx, inst["closed"], inst["closed"].hint, PRIME_SEED)
            return _call(pkg, ctx, inst[name], inst[name].hint if own_hint else 0, SEED)
    except pkg.api.SdpsrError:
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--csrc-commit", required=True, help="the commit whose csrc the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    inst = instances(pkg, np.load(os.path.join(ROOT, "tests", "golden", "golden_partitions.npz")))
    table = {}
    for row in rows():
        rec = run_row(pkg, inst, row)
        if rec is not None:
            table[row[0]] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"csrc_commit": args.csrc_commit, "seed": SEED, "rows": table}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} of {len(rows())} rows recorded to {args.out}")


if __name__ == "__main__":
    main()
