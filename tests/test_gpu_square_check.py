"""The kernels of the square check (csrc/kernels_square_check.hip) on made-up inputs through libsdpsr_prof.so
(sdpsr_profile_square_check), against the integer reference of tests/square_check_ref.py with ==: the class constants c, every
tile's share of X v and C v (part), y, w, the (round, channel) equality bits, the verdict words and the full label matrix, at both
label widths, T = 2 and 4 channels, one and two rounds.  The workspace goes up filled with 0xFF and comes back whole: the 64 bytes
in front of every array and behind the last, and the guard behind the full labels, must come back as they went.
tests/test_square_check_ref_cpu.py shows, without a GPU, that on these inputs and keys the check's answer is the exact one."""
import ctypes as C

import numpy as np
import pytest

import square_check_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
GAP = 64


@pytest.fixture(scope="module")
def cases(problems, golden):
    return {c["name"]: c for c in R.build_cases(problems, golden)}


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _run(pkg, ctx, case, width, T, G, write_full):
    prof = pkg._lib.load_prof_library()
    L, first = case["L"], case["first"]
    n, d = L.shape[0], len(first)
    Lp = R.pack(L)
    keys = np.array(R.KEYS[:G], dtype=np.uint64)
    layout = np.zeros(8, dtype=np.uint64)
    ctx.check(prof.sdpsr_profile_square_check(ctx._h, n, d, G, T, None, width, 0, None, None, None, _vp(layout), None, None, 0))
    ws = np.full(int(layout[7]), 0xFF, dtype=np.uint8)
    Lw = np.full(n * n + GUARD, 0xFFFFFFFF, dtype=np.uint32)
    verdicts = np.full(2, 7, dtype=np.uint32)
    ctx.check(prof.sdpsr_profile_square_check(ctx._h, n, d, G, T, _vp(keys), width, int(write_full), _vp(Lp), _vp(first), _vp(ws), _vp(layout),
                                              _vp(verdicts), _vp(Lw) if write_full else None, GUARD))
    return ws, [int(x) for x in layout], verdicts, Lw


def _check(case, T, G, write_full, ws, layout, verdicts, Lw):
    L, first = case["L"], case["first"]
    n, d = L.shape[0], len(first)
    nb = (n + 63) // 64
    npad = 64 * nb
    GT = G * T
    sizes = [GT * d * 4, GT * nb * npad * 4, GT * nb * npad * 8, GT * npad * 8, GT * npad * 8, GT * nb * 16, GT * 4]
    # nobody wrote outside the arrays
    mask = np.ones(len(ws), dtype=bool)
    for off, sz in zip(layout[:7], sizes):
        assert off >= GAP and off % 16 == 0
        mask[off:off + sz] = False
    assert layout[7] >= layout[6] + sizes[6] + GAP and mask[:GAP].all() and mask[-GAP:].all()
    assert (ws[mask] == 0xFF).all()

    def arr(k, dtype, shape):
        return ws[layout[k]:layout[k] + sizes[k]].view(dtype).reshape(shape)

    c, px, pc = arr(0, np.int32, (GT, d)), arr(1, np.int32, (GT, nb, npad)), arr(2, np.int64, (GT, nb, npad))
    y, w, bits = arr(3, np.int64, (GT, npad)), arr(4, np.int64, (GT, npad)), arr(6, np.uint32, (GT,))
    for g in range(G):
        ref = R.reference_of(case, g)
        tab = R.class_tables(R.KEYS[g], d, T)
        v = np.zeros(npad, dtype=np.int64)
        v[:n] = R.vector(R.KEYS[g], n)
        for t in range(T):
            a = g * T + t
            assert np.array_equal(c[a], ref["c"][t]), (g, t)
            X = np.zeros((npad, npad), dtype=np.int64)
            Cm = np.zeros((npad, npad), dtype=np.int64)
            X[:n, :n] = tab[t][L]
            Cm[:n, :n] = np.concatenate([[0], ref["c"][t]])[L]
            # part[b][i] = the share of column block b in row i; padding rows hold zeros, every slot is written
            assert np.array_equal(px[a], (X * v[None, :]).reshape(npad, nb, 64).sum(axis=2).T), (g, t)
            assert np.array_equal(pc[a], (Cm * v[None, :]).reshape(npad, nb, 64).sum(axis=2).T), (g, t)
            assert np.array_equal(y[a, :n], ref["y"][t]) and not y[a, n:].any(), (g, t)
            assert np.array_equal(w[a, :n], ref["w"][t]) and not w[a, n:].any(), (g, t)
            assert int(bits[a]) == int(ref["equal"][t]), (g, t, ref["q1"][t], ref["q2"][t])
        assert int(verdicts[g]) == int(not all(ref["equal"][:T])), (g, verdicts)
        if case["closed"] is not None:
            assert int(verdicts[g]) == int(not case["closed"])
    if G == 1:
        assert int(verdicts[1]) == 0  # cleared by the host, nobody's to set
    if write_full:
        assert np.array_equal(Lw[:n * n], L.ravel(order="F").astype(np.uint32))
        assert (Lw[n * n:] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("name", R.NAMES)
def test_square_check_stores_the_reference_values(pkg, gpu_ctx, cases, name):
    case = cases[name]
    for width in (8, 32):
        for T in (2, 4):
            for G in (1, 2):
                write_full = G == 2 or width == 32
                got = _run(pkg, gpu_ctx, case, width, T, G, write_full)
                try:
                    _check(case, T, G, write_full, *got)
                except AssertionError as e:
                    raise AssertionError("width %d, T %d, G %d: %s" % (width, T, G, e)) from e


def test_square_check_refuses_what_it_cannot_hold(pkg, gpu_ctx, cases):
    """More than 255 classes, other channel counts, three rounds: SDPSR_BAD_ARGUMENT, nothing launched."""
    prof = pkg._lib.load_prof_library()
    layout = np.zeros(8, dtype=np.uint64)
    for n, d, G, T in ((64, 256, 2, 2), (64, 3, 3, 2), (64, 3, 2, 3), (64, 0, 1, 2), (0, 1, 1, 2)):
        assert prof.sdpsr_profile_square_check(gpu_ctx._h, n, d, G, T, None, 32, 0, None, None, None, _vp(layout), None, None, 0) == 5
