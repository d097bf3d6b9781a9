"""The guessed initial partition of sdpsr_jordan_reduce (csrc/loop.cpp: Loop::initial_partition).

On a ctx whose last loop call found its input closed, the packed labels and class representatives of that call's INITIAL partition
are still in place; the next reduction of that order checks them against its own C_L, X0_L with one streaming pass
(launch_verify_pair) instead of rebuilding them, and reads the verdict with the loop's two deferred ones behind its last host
wait.  A wrong guess repeats the reduction without guesses.  Results alone cannot show that the path ran:
sdpsr_profile_initial_guess counts the guesses taken and the guesses violated.

Raw sdpsr_jordan_reduce from host arrays, no phase timers; the instances of test_gpu_deferred_tail.py (closed512 / open512 through
the module compression, the N = 256 pair through the dense driver)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 1 << 16  # doubles per block-image buffer


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
    for s in (closed512, open512, closed256, open256):
        assert s.hint == 3  # the packed initial partition and the joint iteration: where the guess applies
    return {512: {"closed": closed512, "open": open512, "Lclosed": L512, "dclosed": d512, "Lopen": Lo512, "dopen": do512},
            256: {"closed": closed256, "open": open256, "Lclosed": Lc, "dclosed": int(Lc.max()), "Lopen": Lo256, "dopen": do256}}


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _counts(pkg, ctx, restart=0):
    """(draws, squares, speculative squares, host waits, guesses taken, guesses violated)"""
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint64 * 4)()
    ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, restart, out))
    w = C.c_uint64(0)
    ctx.check(prof.sdpsr_profile_host_waits(ctx._h, C.byref(w)))
    g = (C.c_uint64 * 2)()
    ctx.check(prof.sdpsr_profile_initial_guess(ctx._h, restart, g))
    return int(out[0]), int(out[1]), int(out[2]), int(w.value), int(g[0]), int(g[1])


def _reduce(pkg, ctx, setup, seed):
    """One untimed sdpsr_jordan_reduce with block images; an error status is an outcome like any other (key "status")."""
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
    st = ctx._lib.sdpsr_jordan_reduce(ctx._h, n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], rtol, rtol, _vp(P), C.byref(dd), C.byref(it), C.byref(nb),
                                      C.byref(ssq), C.byref(ss), _vp(blks), CAP, None, 0, None, pkg._lib.MEM_HOST)
    c1 = _counts(pkg, ctx)
    out = {"status": st, "draws": c1[0], "squares": c1[1] - c0[1], "spec": c1[2] - c0[2], "waits": c1[3] - c0[3], "taken": c1[4] - c0[4],
           "violated": c1[5] - c0[5]}
    if st != 0:
        return out
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
    used = dd.value * ssq.value
    delivered = 0 < used <= CAP  # (more than the buffer holds: the call delivers labels and sizes only)
    assert not delivered or not np.isnan(blks[:used]).any()
    out.update({"P": P.reshape(n, n, order="F"), "dim": dd.value, "iterations": it.value, "sizes": [int(x) for x in sizes],
                "blks": blks[:used].copy() if delivered else None})
    return out


def _same(a, b):
    assert a["status"] == b["status"]
    if a["status"] != 0:
        return
    assert np.array_equal(a["P"], b["P"]) and a["dim"] == b["dim"] and a["iterations"] == b["iterations"]
    assert a["sizes"] == b["sizes"]
    assert (a["blks"] is None) == (b["blks"] is None)
    assert a["blks"] is None or np.array_equal(a["blks"], b["blks"])  # same draws, same kernels, fixed summation orders: bit for bit
    assert a["draws"] == b["draws"]


@pytest.mark.parametrize("n", [512, 256], ids=["compressed512", "dense256"])
def test_guessed_initial_partition_equals_the_rebuilt_one(pkg, inst, n):
    """(a) closed, closed, closed on one ctx against the same calls under SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT (which guesses nothing)."""
    I = inst[n]
    with pkg.Context(seed=12) as ctx:
        a = [_reduce(pkg, ctx, I["closed"], seed=61 + k) for k in range(3)]
    with pkg.Context(seed=12, flags=pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT) as ctx:
        b = [_reduce(pkg, ctx, I["closed"], seed=61 + k) for k in range(3)]
    for x, y in zip(a, b):
        assert x["status"] == 0 and np.array_equal(x["P"], I["Lclosed"]) and x["dim"] == I["dclosed"] and x["iterations"] == 1
        assert x["blks"] is not None
        _same(x, y)
        assert x["squares"] == y["squares"]
    assert [x["taken"] for x in a] == [0, 1, 1] and [x["violated"] for x in a] == [0, 0, 0]  # running totals 0, 1, 2
    assert [y["taken"] for y in b] == [0, 0, 0]
    for k in (1, 2):
        assert a[k]["waits"] < b[k]["waits"], (k, a[k]["waits"], b[k]["waits"])


@pytest.mark.parametrize("n", [512, 256], ids=["compressed512", "dense256"])
def test_a_wrong_initial_guess_repeats_the_reduction(pkg, inst, n):
    """(b) closed, closed, then the open input of the same order: the recorded partition is not this input's."""
    I = inst[n]
    with pkg.Context(seed=11) as fresh:
        ref = _reduce(pkg, fresh, I["open"], seed=73)
    assert ref["status"] == 0 and np.array_equal(ref["P"], I["Lopen"]) and ref["dim"] == I["dopen"] and ref["taken"] == 0
    with pkg.Context(seed=12, flags=pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT) as plain:
        unguessed = _reduce(pkg, plain, I["closed"], seed=72)
    with pkg.Context(seed=12) as ctx:
        _reduce(pkg, ctx, I["closed"], seed=71)
        c2 = _reduce(pkg, ctx, I["closed"], seed=72)
        assert c2["taken"] == 1 and c2["violated"] == 0
        r = _reduce(pkg, ctx, I["open"], seed=73)
        assert r["taken"] == 1 and r["violated"] == 1
        _same(r, ref)
        c4 = _reduce(pkg, ctx, I["closed"], seed=72)  # the ctx has unlearnt both guesses
        assert c4["taken"] == 0 and c4["violated"] == 0 and c4["spec"] == 0
        _same(c4, unguessed)
        _same(c4, c2)


def _with_needle(pkg, setup):
    """The setup with C_L changed at one symmetric off-diagonal pair."""
    n, CL, X0L, U = setup
    CLn = CL.copy()
    i, j = n - 2, 5
    CLn[i + j * n] += 1.0
    CLn[j + i * n] += 1.0
    return pkg.api.Setup((n, CLn, X0L, U), setup.basis_symmetric, setup.inputs_symmetric)


def test_one_changed_pair_of_entries_is_found(pkg, inst):
    """(c) closed, closed, then the closed input with C_L changed at one symmetric off-diagonal pair: every output is a fresh ctx's."""
    I = inst[256]
    needle = _with_needle(pkg, I["closed"])
    with pkg.Context(seed=11) as fresh:
        ref = _reduce(pkg, fresh, needle, seed=83)
    with pkg.Context(seed=12) as ctx:
        _reduce(pkg, ctx, I["closed"], seed=81)
        assert _reduce(pkg, ctx, I["closed"], seed=82)["taken"] == 1
        r = _reduce(pkg, ctx, needle, seed=83)
    assert r["taken"] == 1 and r["violated"] == 1
    if ref["status"] == 0:
        assert not np.array_equal(ref["P"], I["Lclosed"])  # (the needle changes the partition)
    _same(r, ref)


def test_admissible_subspace_in_between_drops_the_record(pkg, inst):
    """(d) closed, closed, sdpsr_admissible_subspace of the open input on the same ctx, closed: no guess on that call."""
    I = inst[256]
    with pkg.Context(seed=12, flags=pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT) as plain:
        unguessed = _reduce(pkg, plain, I["closed"], seed=93)
    with pkg.Context(seed=12) as ctx:
        _reduce(pkg, ctx, I["closed"], seed=91)
        assert _reduce(pkg, ctx, I["closed"], seed=92)["taken"] == 1
        n, CL, X0L, U = I["open"]
        Uf = np.asfortranarray(U)
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, I["open"].hint)
        P = np.zeros(n * n, dtype=np.uint32)
        d, it = C.c_int64(0), C.c_int32(0)
        ctx.check(ctx._lib.sdpsr_admissible_subspace(ctx._h, n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], pkg.api.RTOL_DEFAULT, _vp(P),
                                                     C.byref(d), C.byref(it), None, pkg._lib.MEM_HOST))
        assert np.array_equal(P.reshape(n, n, order="F"), I["Lopen"]) and d.value == I["dopen"]
        r = _reduce(pkg, ctx, I["closed"], seed=93)
    assert r["taken"] == 0 and r["violated"] == 0
    assert np.array_equal(r["P"], I["Lclosed"])
    _same(r, unguessed)


def test_batch_restarts_guess_independently(pkg, inst):
    """(e) a 2-restart batch, twice: in the second batch each restart checks the record of ITS ctx; outputs are single calls'."""
    I, R = inst[512], 2
    n = 512
    rtol = pkg.api.RTOL_DEFAULT
    seeds = [[141, 142], [143, 144]]
    with pkg.Context(seed=5) as ctx, pkg.Problem(setup=I["closed"], ctx=ctx) as prob:
        got = []
        for k, sd_ in enumerate(seeds):
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
                got.append({"seed": sd_[i], "P": Ps[i].reshape(n, n, order="F"), "dim": dd[i], "iterations": it[i], "nblocks": nb[i],
                            "blks": Bs[i][:dd[i] * ssq[i]].copy()})
                assert _counts(pkg, ctx, i)[4:] == (k, 0), (k, i)  # each restart: no guess in the first batch, its own in the second
    with pkg.Context(seed=6, flags=pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT) as single:
        for g in got:
            s = _reduce(pkg, single, I["closed"], seed=g["seed"])
            assert s["taken"] == 0
            assert np.array_equal(g["P"], s["P"]) and np.array_equal(g["P"], I["Lclosed"])
            assert g["dim"] == s["dim"] and g["iterations"] == s["iterations"] and g["nblocks"] == len(s["sizes"])
            assert np.array_equal(g["blks"], s["blks"]), g["seed"]
