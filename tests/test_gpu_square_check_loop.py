"""The loop's guessed-closed first iteration judged by the square check (csrc/loop.cpp: check_round) against the same library
forming both squares (SDPSR_FLAG_SQUARE_EVERY_VERDICT) and against a fresh ctx, on the instances of tests/test_gpu_deferred_tail.py
(N = 512: module compression, N = 256: the dense driver; closed and not closed).  Everything a caller sees -- labels, dimension,
iterations, block sizes, block images bit for bit, random draws, the squares and speculative squares counted -- must be equal; only
sdpsr_profile_square_checks tells the two apart."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 1 << 16


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
    return {512: {"closed": closed512, "open": open512, "Lclosed": L512, "dclosed": d512, "Lopen": Lo512, "dopen": do512},
            256: {"closed": closed256, "open": open256, "Lclosed": Lc, "dclosed": int(Lc.max()), "Lopen": Lo256, "dopen": do256}}


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _counts(pkg, ctx):
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint64 * 4)()
    ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, out))
    chk = (C.c_uint64 * 2)()
    ctx.check(prof.sdpsr_profile_square_checks(ctx._h, 0, chk))
    return {"draws": int(out[0]), "squares": int(out[1]), "spec": int(out[2]), "checks": int(chk[0]), "fallbacks": int(chk[1])}


def _delta(c0, c1):
    return {k: (c1[k] if k == "draws" else c1[k] - c0[k]) for k in c1}


def _reduce(pkg, ctx, setup, seed):
    """sdpsr_jordan_reduce from host arrays with block images, untimed, reseeded."""
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
    sizes = np.zeros(nb.value, dtype=np.int32)
    ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
    used = dd.value * ssq.value
    assert 0 < used <= CAP and not np.isnan(blks[:used]).any()
    out = {"P": P.reshape(n, n, order="F"), "dim": dd.value, "iterations": it.value, "sizes": [int(x) for x in sizes], "blks": blks[:used].copy()}
    out.update(_delta(c0, _counts(pkg, ctx)))
    return out


def _adm(pkg, ctx, setup, seed):
    """sdpsr_admissible_subspace alone: every verdict is read inside the loop."""
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    ctx.set_seed(seed)
    if setup.hint:
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    c0 = _counts(pkg, ctx)
    P = np.zeros(n * n, dtype=np.uint32)
    dd, it = C.c_int64(0), C.c_int32(0)
    ctx.check(ctx._lib.sdpsr_admissible_subspace(ctx._h, n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], pkg.api.RTOL_DEFAULT, _vp(P), C.byref(dd), C.byref(it),
                                                 None, pkg._lib.MEM_HOST))
    out = {"P": P.reshape(n, n, order="F"), "dim": dd.value, "iterations": it.value}
    out.update(_delta(c0, _counts(pkg, ctx)))
    return out


def _same(a, b):
    assert np.array_equal(a["P"], b["P"]) and a["dim"] == b["dim"] and a["iterations"] == b["iterations"]
    assert a["draws"] == b["draws"]
    if "blks" in a:
        assert a["sizes"] == b["sizes"]
        assert np.array_equal(a["blks"], b["blks"])  # bit for bit


@pytest.mark.parametrize("n", [512, 256], ids=["compressed512", "dense256"])
def test_checked_rounds_equal_squared_rounds(pkg, inst, n):
    """closed, closed, NOT closed, closed on one ctx, default against SDPSR_FLAG_SQUARE_EVERY_VERDICT; the wrong guess is voided and
    repeated either way and equals a fresh ctx's reduction."""
    I = inst[n]
    seq = [("closed", 31), ("closed", 32), ("open", 33), ("closed", 32)]
    with pkg.Context(seed=12) as ctx:
        a = [_reduce(pkg, ctx, I[k], seed=s) for k, s in seq]
    with pkg.Context(seed=12, flags=pkg._lib.FLAG_SQUARE_EVERY_VERDICT) as ctx:
        b = [_reduce(pkg, ctx, I[k], seed=s) for k, s in seq]
    with pkg.Context(seed=11) as fresh:
        ref_open = _reduce(pkg, fresh, I["open"], seed=33)
    for x, y in zip(a, b):
        _same(x, y)
        assert x["squares"] == y["squares"] and x["spec"] == y["spec"], (x["squares"], y["squares"], x["spec"], y["spec"])
        assert y["checks"] == 0 and y["fallbacks"] == 0  # the flag: never a check
    for k in (0, 1, 3):
        assert np.array_equal(a[k]["P"], I["Lclosed"]) and a[k]["dim"] == I["dclosed"] and a[k]["iterations"] == 1 and a[k]["squares"] == 2
    # the second call guesses and checks; so does the third, wrongly; the fourth has unlearnt the guess
    assert [x["checks"] for x in a] == [0, 1, 1, 0] and [x["spec"] for x in a] == [0, 1, 1, 0]
    assert all(x["fallbacks"] == 0 for x in a)  # deferred verdicts: a violated one repeats the reduction, no square behind the check
    assert np.array_equal(a[2]["P"], I["Lopen"]) and a[2]["dim"] == I["dopen"] and a[2]["squares"] == ref_open["squares"] + 2
    _same(a[2], ref_open)
    _same(a[3], a[1])


@pytest.mark.parametrize("n", [512, 256], ids=["n512", "n256"])
def test_violated_check_read_in_the_loop_forms_the_square(pkg, inst, n):
    """sdpsr_admissible_subspace alone on a primed ctx: the verdicts are read in the loop.  Closed input: both rounds confirmed by
    the check.  NOT closed: the first verdict is violated, the real square of the same key is formed for the refinement (a
    fallback, not counted as another square), the speculative key is handed back, and the call ends on the fresh ctx's labels
    with the fresh ctx's draws."""
    I = inst[n]
    with pkg.Context(seed=11) as fresh:
        ref_open = _adm(pkg, fresh, I["open"], seed=43)
    res = {}
    for name, flags in (("check", 0), ("square", pkg._lib.FLAG_SQUARE_EVERY_VERDICT)):
        with pkg.Context(seed=12, flags=flags) as ctx:
            res[name] = [_adm(pkg, ctx, I["closed"], seed=41), _adm(pkg, ctx, I["closed"], seed=42), _adm(pkg, ctx, I["open"], seed=43)]
    for x, y in zip(res["check"], res["square"]):
        _same(x, y)
        assert x["squares"] == y["squares"] and x["spec"] == y["spec"]
        assert y["checks"] == 0 and y["fallbacks"] == 0
    a = res["check"]
    assert np.array_equal(a[1]["P"], I["Lclosed"]) and a[1]["iterations"] == 1
    assert (a[0]["checks"], a[1]["checks"], a[2]["checks"]) == (0, 1, 1)
    assert (a[0]["fallbacks"], a[1]["fallbacks"], a[2]["fallbacks"]) == (0, 0, 1)
    assert a[1]["spec"] == 1 and a[2]["spec"] == 1
    assert np.array_equal(a[2]["P"], I["Lopen"]) and a[2]["dim"] == I["dopen"]
    _same(a[2], ref_open)
