"""blockDiagonalize of a guessed reduction reads the record's copy of the labels (include/sdpsr.h: SDPSR_FLAG_LABELS_BEFORE_BLOCKDIAG).

A reduction of sdpsr_jordan_reduce that guesses its input closed refines nothing: its labels are the recorded initial partition of the
ctx's last closed input.  With device outputs at label width 32 and no phase timers the ctx keeps a full n x n copy of those labels
("adm_lfull_rec", made by the unguessed call that makes the record); blockDiagonalize of the guessed reduction starts on that copy, and
the square check's class constants and its pass -- the launches that write the caller's P_out -- are enqueued with the other check
segments inside blockDiagonalize.  Same kernels, keys and stream: everything a caller sees is equal bit for bit to the old order, which
the flag keeps; only sdpsr_profile_recorded_labels (the ten words of sdpsr_profile_deferred_checks and an eleventh: reductions whose
blockDiagonalize ran on the copy) tells the two apart.

Instances (raw sdpsr_jordan_reduce on device arrays; module compression forced, eig_driver = 6, so that the segments ride, unless a
test says otherwise):
  closed  partition_as_sdp(synthetic_jordan_partition(n)) at n = 256 (whole 64-tiles of the check), 312 (ragged last tile), 64 (one tile)
  other   the closed instance of the same order under one fixed simultaneous permutation of rows and columns: closed again, another partition
  open    theta' of C_m [] K_k at n = 256 and 312, as in test_gpu_deferred_checks.py

Counter sequence of consecutive closed calls on one ctx: 0, 1, 1, 1.  The first call takes no guess, finds its input closed and makes
the record -- with its copy, since that call already runs under the conditions of the new route -- so the second call, the first
that guesses, is also the first whose blockDiagonalize reads the copy."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = {256: (16, 16), 312: (8, 39), 64: None}  # n -> (m, k) of the open instance C_m [] K_k
SEED0 = 71


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def inst(pkg, problems):
    pr = problems
    out = {}
    for n, mk in ORDERS.items():
        La, da = pr.synthetic_jordan_partition(n, seed=3)
        p = np.roll(np.arange(n), 5)[::-1].copy()  # one fixed permutation of rows and columns
        Lb, db = pr.canonical_labels(La[np.ix_(p, p)])
        assert da == db and not np.array_equal(La, Lb)
        I = {"closed": pkg.admissible_setup(*pr.partition_as_sdp(La, seed=1)), "L": La, "d": da,
             "other": pkg.admissible_setup(*pr.partition_as_sdp(Lb, seed=1)), "Lother": Lb}
        if mk is not None:
            Cv, A, b, Lo, do = pr.theta_prime_product_problem(pr.cycle_adjacency(mk[0]), pr.symmetric_circulant_labels(mk[0]), mk[1], seed=1)
            I["open"], I["Lopen"], I["dopen"] = pkg.admissible_setup(Cv, A, b), Lo, do
        for k in ("closed", "other", "open"):
            assert k not in I or (I[k][0] == n and I[k].hint == 3 and I[k][3].shape[1] >= 1)
        out[n] = I
    return out


def _vp(a):
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _counts(pkg, ctx, restart=0):
    prof = pkg._lib.load_prof_library()
    lc = (C.c_uint64 * 4)()
    ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, restart, lc))
    dc = (C.c_uint64 * 11)()
    ctx.check(prof.sdpsr_profile_recorded_labels(ctx._h, restart, dc))
    return {"draws": int(lc[0]), "registered": int(dc[0]), "in_ride": int(dc[1]), "outside": int(dc[2]), "on_record": int(dc[10]),
            "voided": (int(dc[7]), int(dc[8]), int(dc[9]))}


_DEV = {}


def _on_device(setup):
    """the setup's arrays as device tensors (made once per setup, never written)"""
    torch = _torch()
    key = id(setup)
    if key not in _DEV:
        n, CL, X0L, U = setup
        _DEV[key] = (setup, [torch.from_numpy(np.ascontiguousarray(np.asfortranarray(a).ravel(order="F"))).cuda() for a in (CL, X0L, U)])
        torch.cuda.synchronize()
    return _DEV[key][1]


def _reduce(pkg, ctx, setup, seed, host=False, timed=False, width=32, fill=False, keep=None):
    """One sdpsr_jordan_reduce with labels, images and Q_hat delivered, reseeded.  Device arrays unless host.  fill: P_out holds
    0xFF bytes when the call starts; keep: a list that receives the label buffer, so that the next call gets another address."""
    torch = _torch()
    n, CL, X0L, U = setup
    r = U.shape[1]
    ctx.set_seed(seed)
    ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    c0 = _counts(pkg, ctx)
    cap = n * n
    np_lab = {32: np.uint32, 16: np.uint16}[width]
    if host:
        ins = [np.ascontiguousarray(np.asfortranarray(a).ravel(order="F")) for a in (CL, X0L, U)]
        P = np.full(n * n, np.iinfo(np_lab).max if fill else 0, dtype=np_lab)
        blks, Q = np.full(cap, np.nan), np.full(cap, np.nan)
    else:
        ins = _on_device(setup)
        P = torch.full((n * n,), -1 if fill else 0, dtype={32: torch.int32, 16: torch.int16}[width], device="cuda")
        blks = torch.full((cap,), float("nan"), dtype=torch.float64, device="cuda")
        Q = torch.full((cap,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    if keep is not None:
        keep.append(P)
    dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    pm = np.zeros(pkg._lib.T_COUNT) if timed else None
    rtol = pkg.api.RTOL_DEFAULT
    ctx.check(ctx._lib.sdpsr_jordan_reduce(ctx._h, n, _vp(ins[0]), _vp(ins[1]), _vp(ins[2]), r, rtol, rtol, _vp(P), C.byref(dd), C.byref(it),
                                           C.byref(nb), C.byref(ssq), C.byref(ss), _vp(blks), cap, _vp(Q), cap, _vp(pm),
                                           pkg._lib.MEM_HOST if host else pkg._lib.MEM_DEVICE))
    c1 = _counts(pkg, ctx)
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
    used, qused = dd.value * ssq.value, n * ss.value
    assert 0 < used <= cap and 0 < qused <= cap
    if not host:
        P, blks, Q = P.cpu().numpy().view(np_lab), blks.cpu().numpy(), Q.cpu().numpy()
    assert not np.isnan(blks[:used]).any() and not np.isnan(Q[:qused]).any()  # images and Q_hat were delivered
    out = {"P": P.astype(np.uint32).reshape(n, n, order="F"), "dim": dd.value, "iterations": it.value, "sizes": [int(x) for x in sizes],
           "blks": blks[:used].copy(), "Q": Q[:qused].copy(), "draws": c1["draws"], "voided": c1["voided"]}
    out.update({k: c1[k] - c0[k] for k in ("registered", "in_ride", "outside", "on_record")})
    return out


def _same(a, b):
    assert np.array_equal(a["P"], b["P"]) and a["dim"] == b["dim"] and a["iterations"] == b["iterations"]
    assert a["sizes"] == b["sizes"]
    assert np.array_equal(a["blks"], b["blks"]) and np.array_equal(a["Q"], b["Q"])  # same draws, same kernels, fixed summation orders
    assert a["draws"] == b["draws"]


def _segments(x):
    return x["registered"], x["in_ride"], x["outside"]


def _run(pkg, setup, seeds, flags=0, driver=6, **kw):
    with pkg.Context(seed=12, flags=flags, eig_driver=driver, label_width=kw.get("width", 32)) as ctx:
        return [_reduce(pkg, ctx, setup, seed=s, **kw) for s in seeds]


@pytest.fixture(scope="module")
def base(pkg, inst):
    """four consecutive closed reductions on one ctx at every order: by default and in the old order (the flag)"""
    out = {}
    for n, I in inst.items():
        seeds = [SEED0 + k for k in range(4)]
        out[n] = {"default": _run(pkg, I["closed"], seeds), "flag": _run(pkg, I["closed"], seeds, flags=pkg._lib.FLAG_LABELS_BEFORE_BLOCKDIAG)}
    return out


@pytest.mark.parametrize("n", list(ORDERS))
def test_same_bits_as_the_old_order(inst, base, n):
    I, B = inst[n], base[n]
    for x, y in zip(B["default"], B["flag"]):
        assert np.array_equal(x["P"], I["L"]) and x["dim"] == I["d"] and x["iterations"] == 1
        _same(x, y)
        assert _segments(x) == _segments(y) and y["on_record"] == 0
    assert [x["on_record"] for x in B["default"]] == [0, 1, 1, 1]  # (the module docstring explains the second call's 1)
    assert _segments(B["default"][0]) == (0, 0, 0)
    for x in B["default"][1:]:
        assert _segments(x) == (2, 2, 0), _segments(x)


@pytest.mark.parametrize("n", list(ORDERS))
def test_blockdiag_does_not_read_the_callers_buffer_and_the_pass_fills_it(pkg, inst, base, n):
    I, keep = inst[n], []
    with pkg.Context(seed=12, eig_driver=6) as ctx:
        got = [_reduce(pkg, ctx, I["closed"], seed=SEED0 + k, fill=k >= 1, keep=keep) for k in range(4)]
    assert len({_vp(p).value for p in keep}) == 4  # a different buffer on every call
    for x, ref in zip(got, base[n]["default"]):
        assert np.array_equal(x["P"], I["L"])  # complete: no 0xFFFFFFFF left, equal to the generator's closure
        _same(x, ref)
        assert x["on_record"] == ref["on_record"]


@pytest.mark.parametrize("n", list(ORDERS))
def test_another_closed_input_of_the_same_order_voids_the_guess(pkg, inst, n):
    """closed A, A, then B (A under a fixed permutation), B, B on one ctx.  The first B guesses A's partition and starts
    blockDiagonalize on A's labels: the pair word reads violated (the projection compare and the square check see A's labels, which
    are closed, with the same basis: their words stay 0), the reduction is voided and repeated and equals a fresh ctx's; the repeat
    records, the two calls after it guess again.  Checked
    once by hand while this was written: with the repeat disabled in reduce.cpp this test fails on the labels and the images."""
    I = inst[n]
    ref = _run(pkg, I["other"], [33, 34, 35], flags=pkg._lib.FLAG_LABELS_BEFORE_BLOCKDIAG)
    with pkg.Context(seed=12, eig_driver=6) as ctx:
        a = [_reduce(pkg, ctx, I["closed"], seed=31 + k) for k in range(2)]
        b = [_reduce(pkg, ctx, I["other"], seed=33 + k, fill=True) for k in range(3)]
    assert [x["on_record"] for x in a] == [0, 1]
    for x, y in zip(b, ref):
        assert np.array_equal(x["P"], I["Lother"]) and x["dim"] == I["d"]
        _same(x, y)
    assert b[0]["on_record"] == 1 and _segments(b[0])[0] == 2 and b[0]["in_ride"] + b[0]["outside"] == 2  # the voided run; its repeat adds nothing
    assert b[0]["voided"] == (0, 0, 1), b[0]["voided"]
    # The repeat is itself an unguessed closed reduction of B: it makes B's record and the copy of B's labels, so both later calls
    # guess, on B's labels (a stale copy of A's would fail the comparison with the fresh ctx above).
    for x in b[1:]:
        assert (x["on_record"], _segments(x)) == (1, (2, 2, 0)), (x["on_record"], _segments(x))


@pytest.mark.parametrize("n", [256, 312])
def test_open_input_after_a_record(pkg, inst, n):
    I = inst[n]
    ref = _run(pkg, I["open"], [43])[0]
    assert np.array_equal(ref["P"], I["Lopen"]) and ref["dim"] == I["dopen"] and ref["iterations"] > 1 and ref["on_record"] == 0
    with pkg.Context(seed=12, eig_driver=6) as ctx:
        a = [_reduce(pkg, ctx, I["closed"], seed=41 + k) for k in range(2)]
        o = _reduce(pkg, ctx, I["open"], seed=43, fill=True)
        c = _reduce(pkg, ctx, I["closed"], seed=44)
    assert [x["on_record"] for x in a] == [0, 1]
    _same(o, ref)
    assert o["on_record"] == 1 and o["registered"] == 2 and o["in_ride"] + o["outside"] == 2
    assert o["voided"] == (1, 0, 1), o["voided"]  # as in test_gpu_deferred_checks.py: the pair word and the projection compare
    assert (c["on_record"], _segments(c)) == (0, (0, 0, 0)) and np.array_equal(c["P"], I["L"])  # the record and its copy are gone


@pytest.mark.parametrize("route", ["phase_ms", "host", "width16", "labels_before_blockdiag", "checks_in_loop", "square_every_verdict",
                                   "wait_for_every_verdict"])
def test_routes_that_keep_the_old_order(pkg, inst, base, route):
    n = 312
    I, F = inst[n], pkg._lib
    flags = {"labels_before_blockdiag": F.FLAG_LABELS_BEFORE_BLOCKDIAG, "checks_in_loop": F.FLAG_CHECKS_IN_LOOP,
             "square_every_verdict": F.FLAG_SQUARE_EVERY_VERDICT, "wait_for_every_verdict": F.FLAG_WAIT_FOR_EVERY_VERDICT}.get(route, 0)
    kw = {"phase_ms": {"timed": True}, "host": {"host": True}, "width16": {"width": 16}}.get(route, {})
    got = _run(pkg, I["closed"], [SEED0 + k for k in range(3)], flags=flags, **kw)
    for x, ref in zip(got, base[n]["default"]):
        _same(x, ref)
        assert x["on_record"] == 0


def test_record_dropped_by_a_buffer_change(pkg, inst):
    """256, 256, 312, 312, 256, 256 on one ctx: the larger order replaces the ctx's label buffers and with them the record; every
    first call of an order takes no guess, every second one guesses and reads a copy made at its own order."""
    seq = [256, 256, 312, 312, 256, 256]
    seeds = [51 + k for k in range(len(seq))]
    with pkg.Context(seed=12, eig_driver=6) as ctx:
        got = [_reduce(pkg, ctx, inst[n]["closed"], seed=s, fill=True) for n, s in zip(seq, seeds)]
    with pkg.Context(seed=12, eig_driver=6, flags=pkg._lib.FLAG_LABELS_BEFORE_BLOCKDIAG) as ctx:
        ref = [_reduce(pkg, ctx, inst[n]["closed"], seed=s) for n, s in zip(seq, seeds)]
    for n, x, y in zip(seq, got, ref):
        assert np.array_equal(x["P"], inst[n]["L"]) and x["dim"] == inst[n]["d"]
        _same(x, y)
        assert _segments(x) == _segments(y)
    assert [x["on_record"] for x in got] == [0, 1, 0, 1, 0, 1]
    assert [x["registered"] for x in got] == [0, 2, 0, 2, 0, 2]


def test_batch_restarts_read_their_own_record(pkg, inst):
    torch = _torch()
    n, R = 256, 2
    I = inst[n]
    setup = I["closed"]
    ins = _on_device(setup)
    r = setup[3].shape[1]
    rtol = pkg.api.RTOL_DEFAULT
    cap = n * n
    seeds = [[61, 62], [63, 64], [65, 66]]
    got, recs = [], []
    with pkg.Context(seed=5, eig_driver=6) as ctx:
        for k, sd_ in enumerate(seeds):
            sd = (C.c_uint64 * R)(*sd_)
            Ps = [torch.full((n * n,), -1, dtype=torch.int32, device="cuda") for _ in range(R)]
            Bs = [torch.full((cap,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(R)]
            torch.cuda.synchronize()
            pP = (C.c_void_p * R)(*[t.data_ptr() for t in Ps])
            pb = (C.c_void_p * R)(*[t.data_ptr() for t in Bs])
            caps = (C.c_int64 * R)(*[cap] * R)
            dd, it, nb = (C.c_int64 * R)(), (C.c_int32 * R)(), (C.c_int32 * R)()
            ssq, ss, st = (C.c_int64 * R)(), (C.c_int64 * R)(), (C.c_int32 * R)()
            before = [_counts(pkg, ctx, i) if k else None for i in range(R)]
            ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
            ctx.check(ctx._lib.sdpsr_jordan_reduce_batch(ctx._h, R, C.cast(sd, C.c_void_p), n, _vp(ins[0]), _vp(ins[1]), _vp(ins[2]), r, rtol, rtol,
                                                         C.cast(pP, C.c_void_p), dd, it, nb, ssq, ss, C.cast(pb, C.c_void_p), caps, st,
                                                         pkg._lib.MEM_DEVICE))
            for i in range(R):
                assert st[i] == 0, (sd_, i, st[i])
                after = _counts(pkg, ctx, i)
                recs.append(after["on_record"] - (before[i]["on_record"] if k else 0))
                got.append({"seed": sd_[i], "P": Ps[i].cpu().numpy().view(np.uint32).reshape(n, n, order="F"), "dim": dd[i], "iterations": it[i],
                            "nblocks": nb[i], "blks": Bs[i].cpu().numpy()[:dd[i] * ssq[i]].copy()})
    assert recs == [0, 0, 1, 1, 1, 1], recs  # per restart as on a single ctx: 0, 1, 1
    with pkg.Context(seed=6, eig_driver=6) as single:
        for g in got:
            s = _reduce(pkg, single, setup, seed=g["seed"])
            assert np.array_equal(g["P"], s["P"]) and np.array_equal(g["P"], I["L"])
            assert g["dim"] == s["dim"] and g["iterations"] == s["iterations"] and g["nblocks"] == len(s["sizes"])
            assert np.array_equal(g["blks"], s["blks"]), g["seed"]


def test_dense_driver_enqueues_before_its_first_launch(pkg, inst):
    """eig_driver = 4 at n = 256: no ride; the pass and the checks are enqueued in front of the dense driver's first launch, which
    reads the record's copy (blockDiagonalize's label bookkeeping launches nothing on this route)."""
    I = inst[256]
    seeds = [81, 82, 83]
    d = _run(pkg, I["closed"], seeds, driver=4, fill=True)
    f = _run(pkg, I["closed"], seeds, driver=4, flags=pkg._lib.FLAG_LABELS_BEFORE_BLOCKDIAG)
    for x, y in zip(d, f):
        assert np.array_equal(x["P"], I["L"]) and x["dim"] == I["d"]
        _same(x, y)
        assert _segments(x) == _segments(y) and y["on_record"] == 0
    assert [x["on_record"] for x in d] == [0, 1, 1]
    for x in d[1:]:
        assert _segments(x) == (2, 0, 2), _segments(x)
