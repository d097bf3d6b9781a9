"""The deferred tail of sdpsr_jordan_reduce's guessed-closed path (csrc/sdpsr_internal.h: DeferredTail).

On a ctx whose previous input of this order was closed the loop launches its two gathers only; the two squares and their verify
passes are registered on the ctx and enqueued inside blockDiagonalize -- one behind each of the two Gram products of the module
growth whose read-backs the host waits for (N >= 512: module compression), or all at once in front of every other route (N = 256:
the dense driver).  Same stream, same kernels, same keys: every result must be what the control flow without deferral
(SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT) and a fresh ctx give, bit for bit, and the verdicts read at the end must be real ones.

Instances: closed512 = synthetic_jordan_partition(512) wrapped as an SDP (commutative, closed; N = 512 is the smallest order at
which the module compression is eligible), open512 = theta' of C_16 [] K_32 (N = 512, not closed: a wrong guess sends
blockDiagonalize over labels that are not closed), and the N = 256 pair of test_gpu_loop_contract.py for the dense route."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 1 << 16  # doubles per block-image buffer: dim(P) * sum_sq of every instance here is far below


@pytest.fixture(scope="module")
def inst(pkg, problems, golden):
    L512, d512 = problems.synthetic_jordan_partition(512, seed=3)
    closed512 = pkg.admissible_setup(*problems.partition_as_sdp(L512, seed=1))
    Cv, A, b, Lo512, do512 = problems.theta_prime_product_problem(problems.cycle_adjacency(16), problems.symmetric_circulant_labels(16), 32, seed=1)
    open512 = pkg.admissible_setup(Cv, A, b)
    Lc = golden["circ256_P"].astype(np.int64)
    closed256 = pkg.admissible_setup(*problems.partition_as_sdp(Lc, seed=1))
    Cv, A, b, Lo256, do256 = problems.theta_prime_product_problem(problems.cycle_adjacency(16), problems.symmetric_circulant_labels(16), 16, seed=1)
    open256 = pkg.admissible_setup(Cv, A, b)
    assert closed512[0] == open512[0] == 512 and closed256[0] == open256[0] == 256
    return {512: {"closed": closed512, "open": open512, "Lclosed": L512, "dclosed": d512, "Lopen": Lo512, "dopen": do512},
            256: {"closed": closed256, "open": open256, "Lclosed": Lc, "dclosed": int(Lc.max()), "Lopen": Lo256, "dopen": do256}}


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _counts(pkg, ctx):
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint64 * 4)()
    ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, out))
    w = C.c_uint64(0)
    ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w)))
    return tuple(int(x) for x in out) + (int(w.value),)


def _reduce(pkg, ctx, setup, seed):
    """sdpsr_jordan_reduce from host arrays with block images and WITHOUT phase timers (a timed call defers nothing), reseeded."""
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    ctx.set_seed(seed)
    if setup.hint:
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    c0 = _counts(pkg, ctx)
    P = np.zeros(n * n, dtype=np.uint32)
    blks = np.full(CAP, np.nan)
    dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rtol = pkg.api.RTOL_DEFAULT
    ctx.check(ctx._lib.sdpsr_jordan_reduce(ctx._h, n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], rtol, rtol, _vp(P), C.byref(dd), C.byref(it), C.byref(nb),
                                           C.byref(ssq), C.byref(ss), _vp(blks), CAP, None, 0, None, pkg._lib.MEM_HOST))
    c1 = _counts(pkg, ctx)
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
    used = dd.value * ssq.value
    assert 0 < used <= CAP and not np.isnan(blks[:used]).any()  # the images were delivered
    return {"P": P.reshape(n, n, order="F"), "dim": dd.value, "iterations": it.value, "sizes": [int(x) for x in sizes], "blks": blks[:used].copy(),
            "draws": c1[0], "squares": c1[1] - c0[1], "spec": c1[2] - c0[2], "waits": c1[4] - c0[4]}


def _same(a, b):
    assert np.array_equal(a["P"], b["P"]) and a["dim"] == b["dim"] and a["iterations"] == b["iterations"]
    assert a["sizes"] == b["sizes"]
    assert np.array_equal(a["blks"], b["blks"])  # same draws, same kernels, fixed summation orders: bit for bit
    assert a["draws"] == b["draws"]


@pytest.mark.parametrize("n", [512, 256], ids=["compressed512", "dense256"])
def test_deferred_tail_equals_the_control_flow_without_it(pkg, inst, n):
    """Two reductions of a closed input on one ctx (the second guesses and defers its squares into blockDiagonalize's host waits)
    against the same two calls under SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT: labels, block sizes, block images (bit for bit), draws,
    iterations and squares are equal; the deferring call speculates exactly one square and needs strictly fewer host waits.
    (Squares, not squares - spec: a confirmed speculative square IS the call's confirm round, so a closed input looks at two
    squares on either ctx -- test_confirm_rounds_are_honoured_on_every_call pins that -- of which the deferring ctx counts one as
    speculative and the flagged ctx none: 2 - 1 against 2 - 0, before this change as after it.  squares - spec is the invariant of a
    WRONG guess, whose speculative square is discarded: the next test.)"""
    I = inst[n]
    with pkg.Context(seed=12) as ctx:
        a = [_reduce(pkg, ctx, I["closed"], seed=21 + k) for k in range(2)]
    with pkg.Context(seed=12, flags=pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT) as ctx:
        b = [_reduce(pkg, ctx, I["closed"], seed=21 + k) for k in range(2)]
    for x, y in zip(a, b):
        assert np.array_equal(x["P"], I["Lclosed"]) and x["dim"] == I["dclosed"] and x["iterations"] == 1
        _same(x, y)
        assert x["squares"] == y["squares"] == 2
    assert a[0]["spec"] == 0 and a[1]["spec"] == 1 and b[0]["spec"] == b[1]["spec"] == 0
    assert a[1]["waits"] < b[1]["waits"], (a[1]["waits"], b[1]["waits"])


@pytest.mark.parametrize("n", [512, 256], ids=["compressed512", "dense256"])
def test_wrong_guess_reads_real_verdicts(pkg, inst, n, capfd, monkeypatch):
    """closed, closed, then an input of the same order that is NOT closed: the guess is wrong, blockDiagonalize runs over labels
    that are not closed (and may fail in any way), and the verdicts read at the end are those of the segments that ran -- not the
    "never ran" mark, not the zeros of the call before: the reduction is repeated and equals a fresh ctx's, at the price of the two
    voided squares.  The closed input afterwards is right again."""
    I = inst[n]
    with pkg.Context(seed=11) as fresh:
        ref = _reduce(pkg, fresh, I["open"], seed=33)
    assert np.array_equal(ref["P"], I["Lopen"]) and ref["dim"] == I["dopen"] and ref["iterations"] > 1 and ref["spec"] == 0
    with pkg.Context(seed=12) as ctx:
        c1 = _reduce(pkg, ctx, I["closed"], seed=31)
        c2 = _reduce(pkg, ctx, I["closed"], seed=32)
        assert c2["spec"] == 1
        monkeypatch.setenv("SDPSR_DEBUG", "1")  # (read by the library at every trace point)
        capfd.readouterr()
        r = _reduce(pkg, ctx, I["open"], seed=33)
        monkeypatch.delenv("SDPSR_DEBUG")
        assert "not closed after all" in capfd.readouterr().err
        assert r["spec"] == 1 and r["squares"] == ref["squares"] + 2, (r["squares"], ref["squares"])  # (the voided run: both its squares)
        _same(r, ref)
        c4 = _reduce(pkg, ctx, I["closed"], seed=32)  # the ctx has unlearnt the guess; same seed as c2: the same outputs without one
        assert c4["spec"] == 0
        _same(c4, c2)
        assert np.array_equal(c1["P"], I["Lclosed"]) and np.array_equal(c4["P"], I["Lclosed"])


@pytest.mark.parametrize("confirm", [2, 3])
@pytest.mark.parametrize("n", [512, 256], ids=["compressed512", "dense256"])
def test_more_confirm_rounds_keep_every_square_in_the_loop(pkg, inst, n, confirm):
    """confirm_rounds >= 2: behind a confirmed guess the loop still has rounds to launch -- their gathers reuse the first square's
    buffer, and behind a violated verdict a refinement rewrites the labels and representatives the verify passes read -- so such
    a call registers no tail: every square runs in the loop, in stream order.  Untimed sdpsr_jordan_reduce on a primed ctx, closed
    then NOT closed, against SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT and a fresh ctx: a closed input looks at confirm_rounds + 1 squares of
    which one is speculative, a wrong guess costs at least its two voided squares, and labels, block sizes, block images (bit for bit),
    iterations and draws are those of the control flow that takes no guess."""
    I = inst[n]
    with pkg.Context(seed=11, confirm_rounds=confirm) as fresh:
        ref_open = _reduce(pkg, fresh, I["open"], seed=53)
    assert np.array_equal(ref_open["P"], I["Lopen"]) and ref_open["spec"] == 0
    with pkg.Context(seed=12, confirm_rounds=confirm) as ctx:
        a = [_reduce(pkg, ctx, I["closed"], seed=51 + k) for k in range(2)]
        r = _reduce(pkg, ctx, I["open"], seed=53)
        a4 = _reduce(pkg, ctx, I["closed"], seed=52)
    with pkg.Context(seed=12, confirm_rounds=confirm, flags=pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT) as ctx:
        b = [_reduce(pkg, ctx, I["closed"], seed=51 + k) for k in range(2)]
        rb = _reduce(pkg, ctx, I["open"], seed=53)
    for x, y in zip(a, b):
        assert np.array_equal(x["P"], I["Lclosed"]) and x["iterations"] == 1
        assert x["squares"] == y["squares"] == confirm + 1, (x["squares"], y["squares"])
        _same(x, y)
    assert a[0]["spec"] == 0 and a[1]["spec"] == 1 and b[1]["spec"] == 0
    # (the voided run: its first and its speculative square at least -- its further confirm round sees the violation at once and the
    # loop refines on before the deferred verdicts void it all, as before this change)
    assert r["spec"] == 1 and r["squares"] >= ref_open["squares"] + 2, (r["squares"], ref_open["squares"])
    assert rb["spec"] == 0 and rb["squares"] == ref_open["squares"]
    _same(r, ref_open)
    _same(rb, ref_open)
    assert a4["spec"] == 0
    _same(a4, a[1])


def test_batch_restarts_defer_independently(pkg, inst):
    """sdpsr_problem_reduce_batch with two restarts, twice: in the second batch both restarts guess and defer, each on its own ctx
    and fiber (the report waits yield to the other restart).  Every restart's outputs equal those of a single call with its seed."""
    I, R = inst[512], 2
    n = 512
    rtol = pkg.api.RTOL_DEFAULT
    seeds = [[41, 42], [43, 44]]
    with pkg.Context(seed=5) as ctx, pkg.Problem(setup=I["closed"], ctx=ctx) as prob:
        got = []
        for sd_ in seeds:
            sd = (C.c_uint64 * R)(*sd_)
            Ps = [np.zeros(n * n, dtype=np.uint32) for _ in range(R)]
            Bs = [np.full(CAP, np.nan) for _ in range(R)]
            pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
            pb = (C.c_void_p * R)(*[a.ctypes.data for a in Bs])
            caps = (C.c_int64 * R)(*[CAP] * R)
            dd, it, nb = (C.c_int64 * R)(), (C.c_int32 * R)(), (C.c_int32 * R)()
            ssq, ss, st = (C.c_int64 * R)(), (C.c_int64 * R)(), (C.c_int32 * R)()
            ctx.check(ctx._lib.sdpsr_problem_reduce_batch(ctx._h, prob._h, R, C.cast(sd, C.c_void_p), rtol, rtol, C.cast(pP, C.c_void_p), dd, it, nb, ssq, ss,
                                                          C.cast(pb, C.c_void_p), caps, st, pkg._lib.MEM_HOST))
            for i in range(R):
                assert st[i] == 0, (sd_, i, st[i])
                got.append({"seed": sd_[i], "P": Ps[i].reshape(n, n, order="F"), "dim": dd[i], "iterations": it[i], "nblocks": nb[i], "sum_sq": ssq[i],
                            "blks": Bs[i][:dd[i] * ssq[i]].copy()})
        prof = pkg._lib.load_prof_library()
        for i in range(R):  # the second batch guessed on both restarts
            out = (C.c_uint64 * 4)()
            assert prof.sdpsr_profile_loop_counts(ctx._h, i, out) == 0
            assert int(out[2]) == 1, (i, int(out[2]))
    with pkg.Context(seed=6) as single:
        for g in got:
            s = _reduce(pkg, single, I["closed"], seed=g["seed"])
            assert np.array_equal(g["P"], s["P"]) and np.array_equal(g["P"], I["Lclosed"])
            assert g["dim"] == s["dim"] and g["iterations"] == s["iterations"] and g["nblocks"] == len(s["sizes"])
            assert np.array_equal(g["blks"], s["blks"]), g["seed"]
