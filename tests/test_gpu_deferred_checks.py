"""The check segments of sdpsr_jordan_reduce's guessed-closed path (csrc/sdpsr_internal.h: DeferredSegment, DEFERRED_CHECK).

On a ctx whose previous input of this order was closed, the launches whose only product is a verdict word -- the pair check of the
guessed initial partition; the projection's dot products, the projection compare and the square check's verdict kernels -- are
registered on the ctx and enqueued inside blockDiagonalize: one segment behind each of the two Gram products of the module growth
whose read-backs the host waits for (a ride), or all of them in front of the first launch of every route without such a wait.
SDPSR_FLAG_CHECKS_IN_LOOP launches them in the loop.  Same kernels, keys and stream either way: everything a caller sees must be
equal bit for bit, host waits included; only sdpsr_profile_deferred_checks tells the two apart.

Instances (raw sdpsr_jordan_reduce from host arrays, no phase timers unless a test says so; r = 1 with the symmetric-basis hint, so
the projection compare is live):
  512   synthetic_jordan_partition(512) wrapped as an SDP: module compression, both rides
  256   the golden circulant partition of order 256: the dense driver, no ride
  312   synthetic_jordan_partition(312), Z_8 (x) K_39: not a multiple of 64 -- the square check's pass and its rows kernel have a
        ragged last tile -- with module compression forced (eig_driver = 6), so that it rides as well
  open  theta' of C_m [] K_k at each order: not closed, and its initial partition is another one
  split the closed instance with another basis matrix, diag(3, 1, .., 1) normalised: the same initial partition, closed under
        squaring, but the projection splits the diagonal class

The case "same initial partition, not closed under squaring" is dropped: it cannot be built.  The record a guess starts from IS the
initial partition of an input found closed, and squaring depends on the partition alone; more than that, a guessed reduction checks
X^2 on the RECORDED labels whatever the new input is, so no input at all makes a deferred square-check word 1 (the open instance
leaves the speculative round's word 0 as well: measured, and asserted below).  The words that can be violated are violated, each
alone where that is possible, and every word a voided reduction read is checked not to be the "never ran" mark."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 1 << 20  # doubles per block-image buffer: dim(P) * sum_sq of every instance here is far below


def _split_setup(pkg, setup):
    """The closed setup with U = vec(diag(3, 1, .., 1)) normalised: C_L and X0_L (and so the initial partition) as they were."""
    n, CL, X0L, U = setup
    D = np.eye(n)
    D[0, 0] = 3.0
    U2 = np.asfortranarray((D / np.linalg.norm(D)).reshape(n * n, 1, order="F"))
    return pkg.api.Setup((n, CL, X0L, U2), True, True)


@pytest.fixture(scope="module")
def inst(pkg, problems, golden):
    pr = problems
    out = {}
    for n, (m, k) in {512: (16, 32), 256: (16, 16), 312: (8, 39)}.items():
        if n == 256:
            Lc = golden["circ256_P"].astype(np.int64)
            dc = int(Lc.max())
        else:
            Lc, dc = pr.synthetic_jordan_partition(n, seed=3)
        closed = pkg.admissible_setup(*pr.partition_as_sdp(Lc, seed=1))
        Cv, A, b, Lo, do = pr.theta_prime_product_problem(pr.cycle_adjacency(m), pr.symmetric_circulant_labels(m), k, seed=1)
        opened = pkg.admissible_setup(Cv, A, b)
        assert closed[0] == opened[0] == n and closed[3].shape[1] >= 1 and closed.hint == 3 and opened.hint == 3
        out[n] = {"closed": closed, "open": opened, "split": _split_setup(pkg, closed), "Lclosed": Lc, "dclosed": dc, "Lopen": Lo, "dopen": do,
                  "driver": 6 if n == 312 else 0, "rides": n != 256}
    # Z_78 (x) K_4: n = 312 (ld = 384 != n), 80 classes -- beyond the class-sum kernel's tables at this order: a growth without a class-sum round
    # (class values pairwise distinct by construction: 80 random values out of partition_as_sdp's 1000 collide more often than not, and an
    # initial partition that merges two classes is not closed)
    Lw, dw = pr.kron_with_complete(pr.symmetric_circulant_labels(78), 4, seed=5)
    cw = np.concatenate([[0.0], 3.0 + 7.0 * np.arange(dw)])
    wide = pkg.admissible_setup(cw[Lw].ravel(order="F"), np.eye(312).ravel(order="F")[None, :], np.array([1.0]))
    assert wide[0] == 312 and wide.hint == 3
    assert len(np.unique(np.stack([wide[1], wide[2]]), axis=1).T) == dw  # the initial partition is the whole partition
    out["wide312"] = {"closed": wide, "Lclosed": Lw, "dclosed": dw}
    return out


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _counts(pkg, ctx, restart=0):
    prof = pkg._lib.load_prof_library()
    lc = (C.c_uint64 * 4)()
    ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, restart, lc))
    w = C.c_uint64(0)
    ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w)))
    dc = (C.c_uint64 * 10)()
    ctx.check(prof.sdpsr_profile_deferred_checks(ctx._h, restart, dc))
    return {"draws": int(lc[0]), "squares": int(lc[1]), "spec": int(lc[2]), "waits": int(w.value), "registered": int(dc[0]), "in_ride": int(dc[1]),
            "outside": int(dc[2])}


def _voided_words(pkg, ctx):
    """(first round's, speculative round's, initial partition's) deferred word as the last voided reduction read them"""
    dc = (C.c_uint64 * 10)()
    ctx.check(pkg._lib.load_prof_library().sdpsr_profile_deferred_checks(ctx._h, 0, dc))
    return int(dc[7]), int(dc[8]), int(dc[9])


def _reduce(pkg, ctx, setup, seed, timed=False):
    """sdpsr_jordan_reduce from host arrays with block images, reseeded; the counters are differences around the call (draws: absolute)."""
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    ctx.set_seed(seed)
    if setup.hint:
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    c0 = _counts(pkg, ctx)
    P = np.zeros(n * n, dtype=np.uint32)
    blks = np.full(CAP, np.nan)
    dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    pm = np.zeros(pkg._lib.T_COUNT) if timed else None
    rtol = pkg.api.RTOL_DEFAULT
    ctx.check(ctx._lib.sdpsr_jordan_reduce(ctx._h, n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], rtol, rtol, _vp(P), C.byref(dd), C.byref(it), C.byref(nb),
                                           C.byref(ssq), C.byref(ss), _vp(blks), CAP, None, 0, _vp(pm) if timed else None, pkg._lib.MEM_HOST))
    c1 = _counts(pkg, ctx)
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
    used = dd.value * ssq.value
    assert 0 < used <= CAP and not np.isnan(blks[:used]).any()  # the images were delivered
    out = {"P": P.reshape(n, n, order="F"), "dim": dd.value, "iterations": it.value, "sizes": [int(x) for x in sizes], "blks": blks[:used].copy()}
    out.update({k: (c1[k] if k == "draws" else c1[k] - c0[k]) for k in c1})
    return out


def _same(a, b, waits=True):
    assert np.array_equal(a["P"], b["P"]) and a["dim"] == b["dim"] and a["iterations"] == b["iterations"]
    assert a["sizes"] == b["sizes"]
    assert np.array_equal(a["blks"], b["blks"])  # same draws, same kernels, fixed summation orders: bit for bit
    assert a["draws"] == b["draws"]
    if waits:
        assert a["waits"] == b["waits"], (a["waits"], b["waits"])


@pytest.mark.parametrize("n", [512, 256, 312])
def test_default_equals_checks_in_loop(pkg, inst, n):
    """closed, closed, closed on one ctx, by default and under SDPSR_FLAG_CHECKS_IN_LOOP: labels, dim, iterations, block sizes, images,
    draws, squares and host waits are equal; from the second reduction on the default run registers two check segments and enqueues
    both in rides (module compression) or both outside one (the dense driver); the flag run registers none."""
    I = inst[n]
    res = {}
    for name, flags in (("default", 0), ("flag", pkg._lib.FLAG_CHECKS_IN_LOOP)):
        with pkg.Context(seed=12, flags=flags, eig_driver=I["driver"]) as ctx:
            res[name] = [_reduce(pkg, ctx, I["closed"], seed=21 + k) for k in range(3)]
    for x, y in zip(res["default"], res["flag"]):
        assert np.array_equal(x["P"], I["Lclosed"]) and x["dim"] == I["dclosed"] and x["iterations"] == 1
        _same(x, y)
        assert x["squares"] == y["squares"] == 2 and x["spec"] == y["spec"]
        assert (y["registered"], y["in_ride"], y["outside"]) == (0, 0, 0)
    a = res["default"]
    assert (a[0]["registered"], a[0]["in_ride"], a[0]["outside"]) == (0, 0, 0) and a[0]["spec"] == 0
    for x in a[1:]:
        assert x["spec"] == 1
        assert (x["registered"], x["in_ride"], x["outside"]) == ((2, 2, 0) if I["rides"] else (2, 0, 2)), (x["registered"], x["in_ride"], x["outside"])


@pytest.mark.parametrize("case", ["open", "split"])
@pytest.mark.parametrize("n", [512, 256, 312])
def test_each_violated_verdict_voids_the_reduction(pkg, inst, n, case):
    """closed, closed, then an input of the same order that violates a deferred verdict, then closed again, on one ctx.  open: the
    initial partition is another one (the pair word; the projection compare with its basis fails on the guessed labels as well).
    split: the same initial partition, but the projection splits a class (the projection compare alone).  The verdicts read at the
    end are those of segments that ran: the reduction is voided (its two checked rounds stay counted) and repeated, and equals a
    fresh ctx's reduction of that input in labels, sizes, images and draws.  The closed input afterwards takes no guess and defers
    nothing, as before this change."""
    I = inst[n]
    prof = pkg._lib.load_prof_library()
    with pkg.Context(seed=11, eig_driver=I["driver"]) as fresh:
        ref = _reduce(pkg, fresh, I[case], seed=33)
    assert ref["spec"] == 0 and ref["registered"] == 0
    if case == "open":
        assert np.array_equal(ref["P"], I["Lopen"]) and ref["dim"] == I["dopen"] and ref["iterations"] > 1
    else:
        assert ref["dim"] > I["dclosed"]  # the projection refined the closed partition
    with pkg.Context(seed=12, eig_driver=I["driver"]) as ctx:
        c1 = _reduce(pkg, ctx, I["closed"], seed=31)
        c2 = _reduce(pkg, ctx, I["closed"], seed=32)
        assert c2["spec"] == 1 and c2["registered"] == 2
        g0 = (C.c_uint64 * 2)()
        ctx.check(prof.sdpsr_profile_initial_guess(ctx._h, 0, g0))
        r = _reduce(pkg, ctx, I[case], seed=33)
        g1 = (C.c_uint64 * 2)()
        ctx.check(prof.sdpsr_profile_initial_guess(ctx._h, 0, g1))
        # the voided run guessed, registered both segments, and every one of them was enqueued before its word was read
        assert g1[0] - g0[0] == 1 and g1[1] - g0[1] == (1 if case == "open" else 0)
        assert r["registered"] == 2 and r["in_ride"] + r["outside"] == 2
        # ... and every word the voided run read is a 1 stored by a kernel that ran or a 0 the host stored in front of its segment,
        # never the "never ran" mark.  open: the pair word, and the first round's word from the projection compare (the open input's
        # basis on the guessed labels).  The speculative round's word is the square check's alone and stays 0 here too: a guessed
        # reduction runs on the RECORDED labels, which were found closed under squaring, whatever the new input is -- no reachable
        # input makes a deferred square-check word 1.  split: the projection compare alone.
        assert _voided_words(pkg, ctx) == ((1, 0, 1) if case == "open" else (1, 0, 0)), _voided_words(pkg, ctx)
        assert r["spec"] == 1 and r["squares"] == ref["squares"] + 2, (r["squares"], ref["squares"])
        _same(r, ref, waits=False)
        c4 = _reduce(pkg, ctx, I["closed"], seed=32)  # the ctx has unlearnt the guess; same seed as c2: the same outputs without one
        assert c4["spec"] == 0 and c4["registered"] == 0
        _same(c4, c2, waits=False)
        assert np.array_equal(c1["P"], I["Lclosed"]) and np.array_equal(c4["P"], I["Lclosed"])


@pytest.mark.parametrize("route", ["dense512", "wide312"])
def test_routes_without_a_ride_enqueue_before_their_first_launch(pkg, inst, route):
    """The dense driver forced (eig_driver = 4) at N = 512, and a module growth that has no class-sum round (N = 312, 80 classes):
    both segments are registered and both are enqueued outside a ride; the results equal the flag run's."""
    I, driver = (inst[512], 4) if route == "dense512" else (inst["wide312"], 6)
    res = {}
    for name, flags in (("default", 0), ("flag", pkg._lib.FLAG_CHECKS_IN_LOOP)):
        with pkg.Context(seed=12, flags=flags, eig_driver=driver) as ctx:
            res[name] = [_reduce(pkg, ctx, I["closed"], seed=41 + k) for k in range(2)]
    for x, y in zip(res["default"], res["flag"]):
        assert np.array_equal(x["P"], I["Lclosed"]) and x["dim"] == I["dclosed"]
        _same(x, y)
        assert y["registered"] == 0
    x = res["default"][1]
    assert x["spec"] == 1 and (x["registered"], x["in_ride"], x["outside"]) == (2, 0, 2), (x["registered"], x["in_ride"], x["outside"])


def test_phase_timers_register_nothing(pkg, inst):
    """A timed call (phase_ms given) launches everything in the loop: nothing is registered, and the results equal the untimed call's
    (whose segments ride) and the flag run's."""
    I = inst[512]
    with pkg.Context(seed=12) as ctx:
        a = [_reduce(pkg, ctx, I["closed"], seed=51 + k, timed=True) for k in range(2)]
    with pkg.Context(seed=12) as ctx:
        b = [_reduce(pkg, ctx, I["closed"], seed=51 + k) for k in range(2)]
    with pkg.Context(seed=12, flags=pkg._lib.FLAG_CHECKS_IN_LOOP) as ctx:
        f = [_reduce(pkg, ctx, I["closed"], seed=51 + k, timed=True) for k in range(2)]
    for x, y, z in zip(a, b, f):
        assert (x["registered"], x["in_ride"], x["outside"]) == (0, 0, 0)
        _same(x, y, waits=False)  # (a timed call waits for its events as well)
        _same(x, z)
    assert a[1]["spec"] == 1 and b[1]["registered"] == 2 and b[1]["in_ride"] == 2


def test_batch_restarts_defer_on_their_own_ctx(pkg, inst):
    """sdpsr_jordan_reduce_batch with 3 restarts, twice: in the second batch every restart guesses, registers its two segments on its
    own ctx and enqueues them in its own rides (the report waits yield to the other restarts' fibers).  Every restart's outputs equal
    those of a single call with its seed."""
    I, R, n = inst[512], 3, 512
    _, CL, X0L, U = I["closed"]
    Uf = np.asfortranarray(U)
    rtol = pkg.api.RTOL_DEFAULT
    seeds = [[61, 62, 63], [64, 65, 66]]
    got = []
    with pkg.Context(seed=5) as ctx:
        for sd_ in seeds:
            sd = (C.c_uint64 * R)(*sd_)
            Ps = [np.zeros(n * n, dtype=np.uint32) for _ in range(R)]
            Bs = [np.full(CAP, np.nan) for _ in range(R)]
            pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
            pb = (C.c_void_p * R)(*[a.ctypes.data for a in Bs])
            caps = (C.c_int64 * R)(*[CAP] * R)
            dd, it, nb = (C.c_int64 * R)(), (C.c_int32 * R)(), (C.c_int32 * R)()
            ssq, ss, st = (C.c_int64 * R)(), (C.c_int64 * R)(), (C.c_int32 * R)()
            before = [_counts(pkg, ctx, i) if got else None for i in range(R)]
            ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, I["closed"].hint)
            ctx.check(ctx._lib.sdpsr_jordan_reduce_batch(ctx._h, R, C.cast(sd, C.c_void_p), n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], rtol, rtol,
                                                         C.cast(pP, C.c_void_p), dd, it, nb, ssq, ss, C.cast(pb, C.c_void_p), caps, st, pkg._lib.MEM_HOST))
            for i in range(R):
                assert st[i] == 0, (sd_, i, st[i])
                if before[i] is not None:  # the second batch: every restart deferred on its own ctx
                    after = _counts(pkg, ctx, i)
                    assert (after["registered"] - before[i]["registered"], after["in_ride"] - before[i]["in_ride"],
                            after["outside"] - before[i]["outside"]) == (2, 2, 0), (i, before[i], after)
                got.append({"seed": sd_[i], "P": Ps[i].reshape(n, n, order="F"), "dim": dd[i], "iterations": it[i], "nblocks": nb[i],
                            "blks": Bs[i][:dd[i] * ssq[i]].copy()})
    with pkg.Context(seed=6) as single:
        for g in got:
            s = _reduce(pkg, single, I["closed"], seed=g["seed"])
            assert np.array_equal(g["P"], s["P"]) and np.array_equal(g["P"], I["Lclosed"])
            assert g["dim"] == s["dim"] and g["iterations"] == s["iterations"] and g["nblocks"] == len(s["sizes"])
            assert np.array_equal(g["blks"], s["blks"]), g["seed"]
