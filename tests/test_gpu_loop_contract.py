"""The loop's stopping rule and the reproducibility of a call's random draws, whatever ran on the ctx before.

The loop guesses from its history: when the previous admissible_subspace call on a ctx found its input closed, the next call of
the same order speculates the confirm round, and inside sdpsr_jordan_reduce it even defers both verdicts to the reduction's later
waits (dev. 12).  The result is a canonical partition either way, so comparing results alone cannot see a call
that stopped after fewer squares than confirm_rounds demands, or one whose draws depend on the calls before it.  These tests
count through sdpsr_profile_loop_counts (include/sdpsr_prof.h): the ctx's stream position (draws), the squares the loop
launched and of those the speculative ones, and the symmetric-basis hint its last run used.

Instances, all N = 256: closed = circ256 wrapped as an SDP (the loop's first square finds nothing to split), open = theta' of
C_16 [] K_16 (dimension trajectory 6, 10, 18, 18 in the oracle), and er7 wrapped as an SDP (closed, another order)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 7  # the seed of every measured call
R = 3


@pytest.fixture(scope="module")
def inst(pkg, problems, golden):
    Lc = golden["circ256_P"].astype(np.int64)
    closed = pkg.admissible_setup(*problems.partition_as_sdp(Lc, seed=1))
    Cv, A, b, Le, dopen = problems.theta_prime_product_problem(problems.cycle_adjacency(16), problems.symmetric_circulant_labels(16), 16, seed=1)
    open_ = pkg.admissible_setup(Cv, A, b)
    other = pkg.admissible_setup(*problems.partition_as_sdp(golden["er7_P"].astype(np.int64), seed=1))
    assert closed[0] == open_[0] == 256 and other[0] == 57
    return {"closed": closed, "open": open_, "other": other, "Lc": Lc, "Le": Le, "dopen": dopen,
            "open_sdp": (Cv, A, b), "closed_blk": sorted(int(x) for x in golden["circ256_blk"])}


def _counts(pkg, ctx, restart=0):
    """(draws, squares, speculative squares, hint bits) of ctx or of a batch restart; zeros for a restart not created yet."""
    prof = pkg._lib.load_prof_library()
    out = (C.c_uint64 * 4)()
    if restart > 0 and prof.sdpsr_profile_loop_counts(ctx._h, restart, out) != 0:
        return (0, 0, 0, 0)
    if restart == 0:
        ctx.check(prof.sdpsr_profile_loop_counts(ctx._h, 0, out))
    return tuple(int(x) for x in out)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _adm(pkg, ctx, setup, seed=SEED):
    """sdpsr_admissible_subspace from host arrays, reseeded, with the setup's hint."""
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    ctx.set_seed(seed)
    if setup.hint:
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    c0 = _counts(pkg, ctx)
    P = np.zeros(n * n, dtype=np.uint32)
    d, it = C.c_int64(0), C.c_int32(0)
    ctx.check(ctx._lib.sdpsr_admissible_subspace(ctx._h, n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], pkg.api.RTOL_DEFAULT, _vp(P),
                                                 C.byref(d), C.byref(it), None, pkg._lib.MEM_HOST))
    c1 = _counts(pkg, ctx)
    return {"P": P.reshape(n, n, order="F"), "dim": d.value, "iterations": it.value, "traj": ctx.dimension_trajectory(),
            "draws": c1[0], "squares": c1[1] - c0[1], "spec": c1[2] - c0[2], "hint": c1[3]}


def _reduce(pkg, ctx, setup, seed=SEED):
    """sdpsr_jordan_reduce from host arrays, reseeded, with the setup's hint; + the bytes it uploaded."""
    n, CL, X0L, U = setup
    Uf = np.asfortranarray(U)
    ctx.set_seed(seed)
    if setup.hint:
        ctx._lib.sdpsr_hint_symmetric_basis(ctx._h, setup.hint)
    c0 = _counts(pkg, ctx)
    h0, _ = ctx.transfer_bytes()
    P = np.zeros(n * n, dtype=np.uint32)
    dd, it, nb, ssq, ss = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    ms = (C.c_double * pkg._lib.T_COUNT)()
    rtol = pkg.api.RTOL_DEFAULT
    st = ctx._lib.sdpsr_jordan_reduce(ctx._h, n, _vp(CL), _vp(X0L), _vp(Uf), U.shape[1], rtol, rtol, _vp(P), C.byref(dd), C.byref(it), C.byref(nb),
                                      C.byref(ssq), C.byref(ss), None, 0, None, 0, C.cast(ms, C.c_void_p), pkg._lib.MEM_HOST)
    assert st in (0, 2, 3), st  # (a randomized failure of blockDiagonalize is a result like any other here)
    h1, _ = ctx.transfer_bytes()
    c1 = _counts(pkg, ctx)
    sizes = np.zeros(max(nb.value, 1), dtype=np.int32)
    if st == 0:
        ctx.check(ctx._lib.sdpsr_block_sizes(ctx._h, sizes.ctypes.data_as(C.c_void_p)))
    return {"P": P.reshape(n, n, order="F"), "dim": dd.value, "iterations": it.value, "status": st, "nblocks": nb.value, "sum_sq": ssq.value,
            "sum_s": ss.value, "sizes": sorted(int(x) for x in sizes[:nb.value]) if st == 0 else None, "draws": c1[0], "squares": c1[1] - c0[1],
            "spec": c1[2] - c0[2], "hint": c1[3], "h2d": h1 - h0, "total_ms": ms[pkg._lib.T_TOTAL]}


# (channels, confirm_rounds) -> confirm rounds in effect: channels = 0 is the default pair, 2 channels + at least 1 confirm round
GRID = [(0, 0), (1, 1), (2, 2), (1, 3), (4, 0)]


def _confirm_eff(channels, confirm):
    return max(confirm, 1) if channels == 0 else confirm


@pytest.mark.parametrize("channels,confirm", GRID)
def test_confirm_rounds_are_honoured_on_every_call(pkg, inst, channels, confirm):
    """sdpsr_opts.channels: "a false stop needs confirm_rounds + 1 consecutive squares".  A closed input looks at exactly
    confirm_rounds + 1 squares before it stops -- on the ctx's first call and on the later ones that speculate the confirm round
    (a confirmed speculation is ONE of the confirm rounds, not all of them) -- through both entry points."""
    eff = _confirm_eff(channels, confirm)
    guessing = channels in (0, 2, 4) and eff >= 1  # the joint int8 iteration (2 or 4 channels) is where the guess is taken
    for call in (_adm, _reduce):
        with pkg.Context(seed=1, channels=channels, confirm_rounds=confirm) as ctx:
            for k in range(3):
                r = call(pkg, ctx, inst["closed"], seed=SEED + k)
                assert r["squares"] == eff + 1, (call.__name__, k, r["squares"], eff)
                assert r["iterations"] == 1 and r["dim"] == inst["Lc"].max()
                assert np.array_equal(r["P"], inst["Lc"]), (call.__name__, k)
                if call is _adm:
                    assert r["traj"] == [r["dim"], r["dim"]]
                if k == 0:
                    assert r["spec"] == 0  # nothing to guess from yet
                elif guessing:
                    assert 0 < r["spec"] < r["squares"], (call.__name__, k, r["spec"], r["squares"])  # the guess really ran
                if call is _reduce:
                    assert r["status"] in (0, 2, 3)
                    if r["status"] == 0:
                        assert r["sizes"] == inst["closed_blk"]


HISTORIES = {
    "none": [],
    "closed_same_order": ["closed"],   # the previous call found a closed input of this order: the guess, a wrong one
    "closed_other_order": ["other"],
    "open_itself": ["open"],
}


def _same_loop_result(a, b):
    assert np.array_equal(a["P"], b["P"])
    assert a["dim"] == b["dim"] and a["iterations"] == b["iterations"]


@pytest.mark.parametrize("wait_every", [False, True], ids=["default", "wait_for_every_verdict"])
def test_loop_draws_do_not_depend_on_history(pkg, inst, wait_every):
    """A seeded sdpsr_admissible_subspace on the open input makes the draws of the same call on a fresh ctx, whatever ran on
    the ctx before: a wrong guess gives back the key of its discarded square.  Same squares but for that one discarded
    speculative square, same trajectory, iterations and partition.  SDPSR_FLAG_WAIT_FOR_EVERY_VERDICT takes no guess."""
    flags = pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT if wait_every else 0
    with pkg.Context(seed=1, flags=flags) as fresh:
        ref = _adm(pkg, fresh, inst["open"])
    assert ref["spec"] == 0 and np.array_equal(ref["P"], inst["Le"]) and ref["dim"] == inst["dopen"] and ref["iterations"] > 1
    for name, hist in HISTORIES.items():
        with pkg.Context(seed=1, flags=flags) as ctx:
            for j, h in enumerate(hist):
                _adm(pkg, ctx, inst[h], seed=100 + j)
            r = _adm(pkg, ctx, inst["open"])
        wrong_guess = name == "closed_same_order" and not wait_every
        assert r["spec"] == (1 if wrong_guess else 0), (name, r["spec"])
        assert r["draws"] == ref["draws"], (name, r["draws"], ref["draws"])
        assert r["squares"] - r["spec"] == ref["squares"], (name, r["squares"], r["spec"], ref["squares"])
        assert r["traj"] == ref["traj"], (name, r["traj"], ref["traj"])
        _same_loop_result(r, ref)


@pytest.mark.parametrize("wait_every", [False, True], ids=["default", "wait_for_every_verdict"])
def test_jordan_reduce_draws_do_not_depend_on_history(pkg, inst, wait_every, capfd, monkeypatch):
    """The same for sdpsr_jordan_reduce, where a wrong guess is found out only behind the reduction's later waits and the whole
    reduction is repeated: the repeat starts from the seed position and the hint of the call's entry and reads the inputs the
    first run uploaded.  Draws, partition, iterations, status and block structure equal a fresh ctx's; the voided run costs
    exactly its two squares (the first verify square and the speculative one) and uploads nothing more."""
    flags = pkg._lib.FLAG_WAIT_FOR_EVERY_VERDICT if wait_every else 0
    n, _, _, U = inst["open"]
    inputs = 8 * n * n * (2 + U.shape[1])
    with pkg.Context(seed=1, flags=flags) as fresh:
        ref = _reduce(pkg, fresh, inst["open"])
    assert ref["spec"] == 0 and np.array_equal(ref["P"], inst["Le"]) and ref["dim"] == inst["dopen"] and ref["iterations"] > 1
    assert ref["hint"] == inst["open"].hint
    assert inputs <= ref["h2d"] < inputs + inputs // 4, (ref["h2d"], inputs)
    hists = dict(HISTORIES, closed_closed=["closed", "closed"])  # the second closed call already defers its verdicts
    for name, hist in hists.items():
        with pkg.Context(seed=1, flags=flags) as ctx:
            for j, h in enumerate(hist):
                _reduce(pkg, ctx, inst[h], seed=100 + j)
            monkeypatch.setenv("SDPSR_DEBUG", "1")  # (read by the library at every trace point)
            capfd.readouterr()
            r = _reduce(pkg, ctx, inst["open"])
            monkeypatch.delenv("SDPSR_DEBUG")
            err = capfd.readouterr().err
        wrong_guess = hist[-1:] == ["closed"] and not wait_every
        assert ("not closed after all" in err) == wrong_guess, name  # the repeat path ran exactly when the guess was wrong
        assert r["spec"] == (1 if wrong_guess else 0), (name, r["spec"])
        assert r["squares"] == ref["squares"] + (2 if wrong_guess else 0), (name, r["squares"], ref["squares"])
        assert r["draws"] == ref["draws"], (name, r["draws"], ref["draws"])
        assert r["hint"] == inst["open"].hint, (name, r["hint"])  # the repeat ran with the caller's hint
        assert inputs <= r["h2d"] < inputs + inputs // 4, (name, r["h2d"], inputs)  # C_L, X0_L, U uploaded once
        assert r["total_ms"] > 0
        _same_loop_result(r, ref)
        for key in ("status", "nblocks", "sum_sq", "sum_s", "sizes"):
            assert r[key] == ref[key], (name, key, r[key], ref[key])


def _batch(pkg, ctx, prob, seeds, blk_arrays=None):
    """One raw sdpsr_problem_reduce_batch; per restart its outputs and the counters' deltas."""
    lib, n = ctx._lib, prob.n
    before = [_counts(pkg, ctx, i) for i in range(R)]
    sd = (C.c_uint64 * R)(*seeds)
    Ps = [np.zeros(n * n, dtype=np.uint32) for _ in range(R)]
    pP = (C.c_void_p * R)(*[a.ctypes.data for a in Ps])
    dd, it, nb = (C.c_int64 * R)(), (C.c_int32 * R)(), (C.c_int32 * R)()
    ssq, ss, st = (C.c_int64 * R)(), (C.c_int64 * R)(), (C.c_int32 * R)()
    pb = caps = None
    if blk_arrays is not None:
        pb = (C.c_void_p * R)(*[a.ctypes.data for a in blk_arrays])
        caps = (C.c_int64 * R)(*[a.size for a in blk_arrays])
    rtol = pkg.api.RTOL_DEFAULT
    lib.sdpsr_problem_reduce_batch(ctx._h, prob._h, R, C.cast(sd, C.c_void_p), rtol, rtol, C.cast(pP, C.c_void_p), dd, it, nb, ssq, ss,
                                   C.cast(pb, C.c_void_p) if pb is not None else None, caps, st, pkg._lib.MEM_HOST)
    out = []
    for i in range(R):
        c1 = _counts(pkg, ctx, i)
        assert st[i] in (0, 2, 3), (i, st[i])
        out.append({"status": st[i], "dim": dd[i], "iterations": it[i], "nblocks": nb[i], "sum_sq": ssq[i], "sum_s": ss[i], "P": Ps[i],
                    "draws": c1[0], "squares": c1[1] - before[i][1], "spec": c1[2] - before[i][2]})
    return out


def _check_images(P, blks, sizes):
    """Block images without Q_hat: every image Q_k' 1[P==i] Q_k is symmetric, and the images of the classes on the diagonal
    (they partition the identity: I lies in the span of a Jordan partition) sum to Q_k'Q_k = I in every block."""
    d = blks.shape[0]
    diag = np.unique(np.diag(P))
    off = P[~np.eye(P.shape[0], dtype=bool)]
    assert not np.isin(off, diag).any()  # the diagonal classes hold diagonal entries only
    off_k = 0
    for s in sizes:
        acc = np.zeros((s, s))
        for i in range(d):
            B = blks[i, off_k:off_k + s * s].reshape(s, s, order="F")
            assert np.allclose(B, B.T, atol=1e-9), (i, s)
            if i + 1 in diag:
                acc += B
        assert np.allclose(acc, np.eye(s), atol=1e-9), (s, acc)
        off_k += s * s
    assert off_k == blks.shape[1]


@pytest.mark.parametrize("primed", ["none", "closed_same_order", "same_problem"])
def test_batch_sizes_pass_equals_images_pass(pkg, inst, primed):
    """Problem.reduce_batch runs the restarts twice with the same seeds -- sizes, then images into buffers of those sizes -- and
    relies on both passes running the same reductions.  Restart ctxs keep their history between calls (the guess); with the
    history that makes the sizes pass guess wrong, both passes still make the same draws and end with the same status and block
    structure, and every restart with status 0 delivers images of the right shape that pass the identity check."""
    seeds = [31, 32, 33]
    n = inst["open"][0]
    for via_api in (False, True):
        with pkg.Context(seed=5) as ctx, pkg.Problem(setup=inst["open"], ctx=ctx) as prob, pkg.Problem(setup=inst["closed"], ctx=ctx) as closed:
            if primed != "none":
                _batch(pkg, ctx, closed if primed == "closed_same_order" else prob, [71, 72, 73])
            if not via_api:
                a = _batch(pkg, ctx, prob, seeds)
                b = _batch(pkg, ctx, prob, seeds, [np.zeros(max(1, x["dim"] * x["sum_sq"])) for x in a])
                for i, (x, y) in enumerate(zip(a, b)):
                    assert y["spec"] == 0
                    assert x["spec"] == (1 if primed == "closed_same_order" else 0), (i, x["spec"])
                    assert x["squares"] - 2 * x["spec"] == y["squares"], (i, x["squares"], y["squares"])  # (the voided run: 2 squares)
                    # the images pass draws once more, AFTER the reduction: the random vector of basis_image
                    assert y["draws"] == x["draws"] + (1 if y["status"] == 0 else 0), (primed, i, x["draws"], y["draws"])
                    for key in ("status", "dim", "iterations", "nblocks", "sum_sq", "sum_s"):
                        assert x[key] == y[key], (primed, i, key, x[key], y[key])
                    assert np.array_equal(x["P"].reshape(n, n, order="F"), inst["Le"]) and np.array_equal(y["P"], x["P"])
            else:
                res = prob.reduce_batch(R, seeds=seeds)
                assert any(x["status"] == 0 for x in res), [x["status"] for x in res]
                for i, x in enumerate(res):
                    assert x["P"].nparts == inst["dopen"] and np.array_equal(np.asarray(x["P"].matrix), inst["Le"])
                    if x["status"] != 0:
                        assert x["blks"] is None
                        continue
                    assert x["blks"].shape == (x["P"].nparts, x["sum_sq"])
                    sizes = np.zeros(x["nblocks"], dtype=np.int32)
                    ctx.check(ctx._lib.sdpsr_batch_block_sizes(ctx._h, i, sizes.ctypes.data_as(C.c_void_p)))
                    assert int((sizes.astype(np.int64) ** 2).sum()) == x["sum_sq"] and int(sizes.sum()) == x["sum_s"]
                    _check_images(np.asarray(x["P"].matrix), x["blks"], [int(s) for s in sizes])


def test_restored_confirm_rounds_keep_the_oracle_trajectory(pkg, oracle, inst):
    """confirm_rounds = 3 on a ctx primed with the closed input of the same order: the closed input again looks at four squares,
    and the open input walks through the oracle's dimension sequence (as test_dimension_trajectory_default_mode checks for the
    default pair) -- the restored confirm rounds change the work done, not the result."""
    n, CL, X0L, U = inst["open"]
    Cv, A, b = inst["open_sdp"]
    trace = []
    ref = oracle.admissible_subspace(Cv, A, b, rng=np.random.default_rng(0), trace=trace,
                                     setup=(n, U, CL.reshape(n, n, order="F"), X0L.reshape(n, n, order="F")))
    assert np.array_equal(ref.matrix, inst["Le"])
    with pkg.Context(seed=1, confirm_rounds=3) as fresh:
        f = _adm(pkg, fresh, inst["open"])
    with pkg.Context(seed=1, confirm_rounds=3) as ctx:
        c1 = _adm(pkg, ctx, inst["closed"], seed=100)
        c2 = _adm(pkg, ctx, inst["closed"], seed=101)
        assert c1["squares"] == c2["squares"] == 4 and c2["spec"] > 0
        r = _adm(pkg, ctx, inst["open"])
    dims = r["traj"]
    assert np.array_equal(r["P"], inst["Le"]) and r["dim"] == ref.nparts
    assert len(dims) == r["iterations"] + 1 and dims[-1] == r["dim"]
    assert dims[1:] == trace, (dims, trace)
    assert r["draws"] == f["draws"] and r["squares"] - r["spec"] == f["squares"] and dims == f["traj"]


def _loop_paths_tool():
    """tools/record_loop_paths.py: the table's rows and the one way a row is run, shared with the recorder."""
    import importlib.util
    import pathlib
    path = pathlib.Path(__file__).resolve().parents[1] / "tools" / "record_loop_paths.py"
    spec = importlib.util.spec_from_file_location("record_loop_paths", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_loop_path_matches_the_recorded_table(pkg, inst):
    """Every path of the loop at once: instance x square mode x one flag x hint x channels, plus the confirmed and the wrong
    speculation (tools/record_loop_paths.py).  Each row -- dim, iterations, dimension trajectory, draws, squares, speculative
    squares, host waits, CRC32 of the labels -- equals tests/golden/loop_paths.json, recorded once from the csrc of the commit
    the file names; a combination the library rejects has no row there and is rejected here too."""
    import json
    tool = _loop_paths_tool()
    with open(tool.GOLDEN) as f:
        recorded = json.load(f)
    assert recorded["seed"] == tool.SEED == SEED
    rows = tool.rows()
    assert set(recorded["rows"]) <= {row[0] for row in rows}
    assert len(recorded["rows"]) >= 100  # (the table really is there: 134 rows less the rejected combinations)
    bad = []
    for row in rows:
        got, want = tool.run_row(pkg, inst, row), recorded["rows"].get(row[0])
        if got != want:
            bad.append((row[0], got, want))
    assert not bad, bad
